# The text of a kernel file for a model WITHOUT censored observations: its SMC_USER_CENSOR blocks left out, the #else side kept.
# csrc/Makefile embeds both texts; the markers are whole lines, exactly these three.
/^#ifdef SMC_USER_CENSOR$/        { skip = 1; next }
/^#else  \/\/ SMC_USER_CENSOR$/   { skip = 0; next }
/^#endif  \/\/ SMC_USER_CENSOR$/  { skip = 0; next }
!skip
