# The text of a kernel file for a model WITHOUT count observations: its SMC_USER_COUNT blocks left out, the #else side kept.
# csrc/Makefile embeds both texts; the markers are whole lines, exactly these three.
/^#ifdef SMC_USER_COUNT$/        { skip = 1; next }
/^#else  \/\/ SMC_USER_COUNT$/   { skip = 0; next }
/^#endif  \/\/ SMC_USER_COUNT$/  { skip = 0; next }
!skip
