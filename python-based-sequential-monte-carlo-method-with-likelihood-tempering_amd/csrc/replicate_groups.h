// replicate_groups.h -- host code: which experiments of a Michaelis-Menten data set are REPLICATES of each other, i.e. integrate
// the same initial value problem, and how a sweep groups them into solves (mm_kernels.hip: ShareArgs).
//
// Two experiments are replicates when their S0 and all their n_t data times are equal BIT FOR BIT (memcmp, not ==: -0.0 and 0.0
// do not merge, and a NaN needs no thought).  The trajectory of a (particle, experiment) item depends on (Vmax, Km, S0, the time
// row, rtol, atol) and on nothing else, so the solves of two replicates perform the same attempts and produce the same dense
// outputs; only the observations differ.
//
// Solve groups, in order of first appearance: a primary experiment (the lowest index) and at most ONE partner.  A condition
// that appears three or more times becomes pairs and, if their number is odd, a single: indices a, b, c, d, e of one condition
// give (a, b), (c, d), (e).
#pragma once
#include <string.h>

namespace smc {

// primary[g], partner[g] (-1: none) for g < the return value, the number of solve groups; both arrays have room for n_ex entries
inline int group_replicates(const double *t, const double *S0, int n_ex, int n_t, int *primary, int *partner) {
    int n_solve = 0;
    for (int e = 0; e < n_ex; ++e) {
        int g = 0;
        for (; g < n_solve; ++g) {      // an earlier group of the same condition that still lacks its partner
            const int q = primary[g];
            if (partner[g] < 0 && memcmp(S0 + q, S0 + e, sizeof(double)) == 0 &&
                memcmp(t + (size_t)q * n_t, t + (size_t)e * n_t, (size_t)n_t * sizeof(double)) == 0)
                break;
        }
        if (g < n_solve) {
            partner[g] = e;
        } else {
            primary[n_solve] = e;
            partner[n_solve] = -1;
            ++n_solve;
        }
    }
    for (int g = n_solve; g < n_ex; ++g) primary[g] = partner[g] = -1;
    return n_solve;
}

}  // namespace smc
