// count_floor.h -- the floor of a Poisson term (user_count.h; include/smc_hip.h: COUNT OBSERVATIONS), host code: a data constant that
// the library sums per experiment (C_e) and tabulates per cell for the pointwise kernels.  A header of its own so that
// tests/hostcheck/likelihood_terms_hostcheck.cpp holds the very text the library compiles to 60-digit values.
#pragma once
#include <cmath>

namespace smc_cnt_host {
// c(y) = lgamma(y + 1) - y log y + y, minus the log-probability of the saturated Poisson model at the count y (user_count.h;
// user_models.count_floor is the same in NumPy): as written up to y = 32, where nothing cancels yet, and from there on by its
// Stirling series 1/2 log(2 pi y) + 1/(12 y) - 1/(360 y^3) + 1/(1260 y^5) - 1/(1680 y^7), whose next term is below 1e-16 - the
// three terms of the definition reach 1e7 at y = 1e6 and would leave c(y), a number below 10, with an error of 1e-9.
inline double count_floor(double y) {
    if (y < 32.0) return y > 0.0 ? (std::lgamma(y + 1.0) - y * std::log(y)) + y : 0.0;
    const double r = 1.0 / y, r2 = r * r;
    return 0.5 * std::log(6.283185307179586 * y) + r * (1.0 / 12.0 - r2 * (1.0 / 360.0 - r2 * (1.0 / 1260.0 - r2 * (1.0 / 1680.0))));
}
}  // namespace smc_cnt_host
