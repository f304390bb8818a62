# The text of a kernel file for a model WITHOUT state-triggered events: its SMC_USER_ROOTS blocks left out, the #else side kept.
# csrc/Makefile runs it in front of strip_events.awk, so a SMC_USER_ROOTS block may stand inside a SMC_USER_EVENTS block and
# may hold SMC_USER_EVENTS markers on its #else side; the markers are whole lines, exactly these three.
/^#ifdef SMC_USER_ROOTS$/        { skip = 1; next }
/^#else  \/\/ SMC_USER_ROOTS$/   { skip = 0; next }
/^#endif  \/\/ SMC_USER_ROOTS$/  { skip = 0; next }
!skip
