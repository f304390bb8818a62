"""Example sources for HipEngine.set_model_user (include/smc_hip.h: smc_set_model_user) - what a user of the
reference writes instead of a new Micmem_likelihood.py (README.md:4, "modify for your problem")."""

# Micmem_likelihood.py:14-33 as a user model: theta = (Vmax, Km, sigma), cond = (S0,), one state S, observed P = S0 - S
MICHAELIS_MENTEN_PLAIN = r"""
__device__ void smc_user_y0(const double *theta, const double *cond, double *y) { y[0] = cond[0]; }
__device__ void smc_user_rhs(double t, const double *y, const double *theta, const double *cond, double *dydt) {
    dydt[0] = smc_div((-theta[0]) * y[0], theta[1] + y[0]);     // a / b, faster (include/smc_hip.h)
}
__device__ double smc_user_obs(double t, const double *y, const double *theta, const double *cond) { return cond[0] - y[0]; }
"""
# ... with the optional cost hint (include/smc_hip.h): explicit RK45 runs on its stability limit for about 3.7 Vmax / Km step
# attempts, so the sweeps hand those solves out first and run the longest one per wave - results are the same either way
MICHAELIS_MENTEN = MICHAELIS_MENTEN_PLAIN + r"""
__device__ double smc_user_cost(const double *theta) { return theta[1] > 0.0 ? 3.7 * theta[0] / theta[1] : 0.0; }
"""

# two states: A -> B -> C with rate constants theta = (k1, k2, sigma), cond = (A0,), the intermediate B is observed
CONSECUTIVE_REACTIONS = r"""
__device__ void smc_user_y0(const double *theta, const double *cond, double *y) { y[0] = cond[0]; y[1] = 0.0; }
__device__ void smc_user_rhs(double t, const double *y, const double *theta, const double *cond, double *dydt) {
    dydt[0] = -theta[0] * y[0];
    dydt[1] = theta[0] * y[0] - theta[1] * y[1];
}
__device__ double smc_user_obs(double t, const double *y, const double *theta, const double *cond) { return y[1]; }
"""

# Robertson's stiff kinetics (A -> B, B + B -> C + B, B + C -> A + C) for method="BDF" (include/smc_hip.h): the rate constants
# k1 = theta[0] and k3 = theta[1] are estimated, k2 = 3e7 is fixed; theta = (k1, k3, sigma), cond = (A0,), the product C is
# observed.  With the classic k1 = 0.04, k3 = 1e4 explicit RK45 runs on its stability limit (tens of thousands of attempts).
ROBERTSON_NUMJAC = r"""
__device__ void smc_user_y0(const double *theta, const double *cond, double *y) { y[0] = cond[0]; y[1] = 0.0; y[2] = 0.0; }
__device__ void smc_user_rhs(double t, const double *y, const double *theta, const double *cond, double *dydt) {
    const double k1 = theta[0], k2 = 3e7, k3 = theta[1];
    dydt[0] = -k1 * y[0] + k3 * y[1] * y[2];
    dydt[1] = k1 * y[0] - k3 * y[1] * y[2] - k2 * y[1] * y[1];
    dydt[2] = k2 * y[1] * y[1];
}
__device__ double smc_user_obs(double t, const double *y, const double *theta, const double *cond) { return y[2]; }
"""
# ... with the analytic Jacobian (row-major J[i * 3 + j] = d dydt[i] / d y[j])
ROBERTSON = ROBERTSON_NUMJAC + r"""
__device__ void smc_user_jac(double t, const double *y, const double *theta, const double *cond, double *J) {
    const double k1 = theta[0], k2 = 3e7, k3 = theta[1];
    J[0] = -k1; J[1] = k3 * y[2];                    J[2] = k3 * y[1];
    J[3] = k1;  J[4] = -k3 * y[2] - 2.0 * k2 * y[1]; J[5] = -k3 * y[1];
    J[6] = 0.0; J[7] = 2.0 * k2 * y[1];              J[8] = 0.0;
}
"""
