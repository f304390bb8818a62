// tools/fp64_chain_probe.hip -- what ONE wave with ONE live lane pays per FP64 instruction on THIS device: the pacing of the
// lone stiff chain (csrc/mm_rk45.h: mm_fast_uniform_attempts), whose ~130 instructions per attempt run alone on their SIMD.
// Each case is an inline-asm body of UNROLL groups inside a counted loop, stamped with s_memtime (shader cycles) and
// s_memrealtime (100 MHz) around the whole loop; the lone wave's clock is the quotient of the two.  Cases:
//   dep_fma / dep_add_mul   one dependent chain
//   ilp2 / ilp3 / ilp8      2, 3, 8 interleaved independent v_fma_f64 chains (cost per instruction against ILP; ilp8 = issue cost)
//   dep_rcp8                a dependent chain of 7 v_fma_f64 + 1 v_rcp_f64 (+ the s_nop its hazard needs) per group
//   div6                    the six-operation division of the block (rcp, 2 Newton FMAs, q, residual, correction), dependent
//   pow_f32                 the block's v_cvt_f32_f64 / v_log_f32 / v_mul_f32 / v_exp_f32 / v_cvt_f64_f32 chain with its two s_nop
//   br_adjacent             producer, v_cmp_f64, s_cbranch_vccnz (never taken), 8 independent v_fma_f64
//   br_cmp_far              producer, 8 independent, v_cmp_f64, s_cbranch_vccnz
//   br_far                  producer, v_cmp_f64, 8 independent, s_cbranch_vccnz
//   br_none                 producer, 8 independent (the same group without the pair)
//   rcp_use / rcp_shadow3   v_rcp_f64, then its first use after an s_nop / after 3 independent v_fma_f64: is the rest of
//                           the reciprocal's time a latency that independent work fills, or issue time?
//   scc_taken / scc_not_taken  producer, s_cmp + s_cbranch_scc1 (taken to the next instruction / never taken), 8 independent
//   mask_or                 producer, two v_cmp_f64 into scalar pairs, 8 independent, s_or_b64 vcc + s_cbranch_vccnz
//   salu8                   producer, 8 dependent s_add_u32 (the cost of a scalar instruction in a lone wave's stream)
// Prints one JSON line.  Build: hipcc -O3 --offload-arch=gfx950 -o fp64_chain_probe fp64_chain_probe.hip
#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstdlib>

#define STR_(x) #x
#define STR(x) STR_(x)
#define UNROLL 16

enum Case { kDepFma, kDepAddMul, kIlp2, kIlp3, kIlp8, kDepRcp8, kDiv6, kPowF32, kBrAdjacent, kBrCmpFar, kBrFar, kBrNone, kRcpUse, kRcpShadow3, kSccTaken, kSccNotTaken, kMaskOr, kSalu8, kCases };
struct CaseInfo { const char *name; int per_group; };   // instructions per group, s_nop included
static const CaseInfo kInfo[kCases] = {{"dep_fma", 8},     {"dep_add_mul", 8}, {"ilp2", 8},        {"ilp3", 9},
                                       {"ilp8", 8},        {"dep_rcp8", 9},    {"div6", 7},        {"pow_f32", 7},
                                       {"br_adjacent", 11}, {"br_cmp_far", 11}, {"br_far", 11},     {"br_none", 9},
                                       {"rcp_use", 3},     {"rcp_shadow3", 5}, {"scc_taken", 11},  {"scc_not_taken", 11},
                                       {"mask_or", 12},    {"salu8", 9}};

#define FMA(x) "v_fma_f64 " x ", " x ", %[a], %[b]\n"
#define INDEP8 FMA("%[y0]") FMA("%[y1]") FMA("%[y2]") FMA("%[y3]") FMA("%[y4]") FMA("%[y5]") FMA("%[y6]") FMA("%[y7]")
#define BODY(text)                                                                                                          \
    asm volatile(".rept " STR(UNROLL) "\n" text ".endr\n.Lprobe_out_%=:\n"                                                  \
                 : [x0] "+v"(x0), [x1] "+v"(x1), [x2] "+v"(x2), [y0] "+v"(y[0]), [y1] "+v"(y[1]), [y2] "+v"(y[2]),         \
                   [y3] "+v"(y[3]), [y4] "+v"(y[4]), [y5] "+v"(y[5]), [y6] "+v"(y[6]), [y7] "+v"(y[7]), [r] "=&v"(r),      \
                   [e] "=&v"(e), [q] "=&v"(q), [w] "=&v"(w), [m0] "=&s"(m0), [m1] "=&s"(m1), [c0] "+s"(c0)                  \
                 : [a] "v"(a), [b] "v"(b), [big] "v"(big), [zero] "s"(zero)                                                 \
                 : "vcc", "scc")

template <int CASE>
__global__ void __launch_bounds__(64) probe_kernel(unsigned long long *out, int iters, double a, double b, double big) {
    double x0 = 2.0, x1 = 1.5, x2 = 1.25, y[8], r, e, q;
    float w;
    unsigned long long m0, m1;
    unsigned c0 = 0;
    const int zero = __builtin_amdgcn_readfirstlane(iters < 0);   // 0, in a scalar register
    for (int i = 0; i < 8; ++i) y[i] = 1.0 + 0.125 * i;
    const unsigned long long r0 = __builtin_amdgcn_s_memrealtime();
    const unsigned long long t0 = __builtin_amdgcn_s_memtime();
    for (int it = 0; it < iters; ++it) {
        if (CASE == kDepFma) BODY(FMA("%[x0]") FMA("%[x0]") FMA("%[x0]") FMA("%[x0]") FMA("%[x0]") FMA("%[x0]") FMA("%[x0]") FMA("%[x0]"));
        if (CASE == kDepAddMul)
            BODY("v_add_f64 %[x0], %[x0], %[b]\n v_mul_f64 %[x0], %[x0], %[a]\n v_add_f64 %[x0], %[x0], %[b]\n v_mul_f64 %[x0], %[x0], %[a]\n"
                 "v_add_f64 %[x0], %[x0], %[b]\n v_mul_f64 %[x0], %[x0], %[a]\n v_add_f64 %[x0], %[x0], %[b]\n v_mul_f64 %[x0], %[x0], %[a]\n");
        if (CASE == kIlp2) BODY(FMA("%[x0]") FMA("%[x1]") FMA("%[x0]") FMA("%[x1]") FMA("%[x0]") FMA("%[x1]") FMA("%[x0]") FMA("%[x1]"));
        if (CASE == kIlp3) BODY(FMA("%[x0]") FMA("%[x1]") FMA("%[x2]") FMA("%[x0]") FMA("%[x1]") FMA("%[x2]") FMA("%[x0]") FMA("%[x1]") FMA("%[x2]"));
        if (CASE == kIlp8) BODY(INDEP8);
        if (CASE == kDepRcp8)
            BODY(FMA("%[x0]") FMA("%[x0]") FMA("%[x0]") FMA("%[x0]") FMA("%[x0]") FMA("%[x0]") FMA("%[x0]")
                 "v_rcp_f64 %[x0], %[x0]\n s_nop 0\n");
        if (CASE == kDiv6)   // x0 = b / x0 by the block's division, each group's denominator the previous quotient
            BODY("v_rcp_f64 %[r], %[x0]\n s_nop 0\n v_fma_f64 %[e], -%[x0], %[r], 1.0\n v_fma_f64 %[r], %[r], %[e], %[r]\n"
                 "v_mul_f64 %[q], %[b], %[r]\n v_fma_f64 %[e], -%[x0], %[q], %[b]\n v_fma_f64 %[x0], %[e], %[r], %[q]\n");
        if (CASE == kPowF32)
            BODY("v_cvt_f32_f64 %[w], |%[x0]|\n v_log_f32 %[w], %[w]\n s_nop 0\n v_mul_f32 %[w], 0xbe4ccccd, %[w]\n v_exp_f32 %[w], %[w]\n"
                 "s_nop 0\n v_cvt_f64_f32 %[x0], %[w]\n");
        if (CASE == kBrAdjacent) BODY(FMA("%[x0]") "v_cmp_gt_f64 vcc, %[x0], %[big]\n s_cbranch_vccnz .Lprobe_out_%=\n" INDEP8);
        if (CASE == kBrCmpFar) BODY(FMA("%[x0]") INDEP8 "v_cmp_gt_f64 vcc, %[x0], %[big]\n s_cbranch_vccnz .Lprobe_out_%=\n");
        if (CASE == kBrFar) BODY(FMA("%[x0]") "v_cmp_gt_f64 vcc, %[x0], %[big]\n" INDEP8 "s_cbranch_vccnz .Lprobe_out_%=\n");
        if (CASE == kBrNone) BODY(FMA("%[x0]") INDEP8);
        if (CASE == kRcpUse) BODY("v_rcp_f64 %[r], %[x0]\n s_nop 0\n v_fma_f64 %[x0], %[r], %[a], %[b]\n");
        if (CASE == kRcpShadow3) BODY("v_rcp_f64 %[r], %[x0]\n" FMA("%[y0]") FMA("%[y1]") FMA("%[y2]") "v_fma_f64 %[x0], %[r], %[a], %[b]\n");
        if (CASE == kSccTaken) BODY(FMA("%[x0]") "s_cmp_eq_u32 %[zero], 0\n s_cbranch_scc1 1f\n 1:\n" INDEP8);
        if (CASE == kSccNotTaken) BODY(FMA("%[x0]") "s_cmp_lg_u32 %[zero], 0\n s_cbranch_scc1 .Lprobe_out_%=\n" INDEP8);
        if (CASE == kMaskOr)   // two compares into scalar pairs, combined and branched on 8 instructions later
            BODY(FMA("%[x0]") "v_cmp_gt_f64 %[m0], %[x0], %[big]\n v_cmp_gt_f64 %[m1], %[y0], %[big]\n" INDEP8
                 "s_or_b64 vcc, %[m0], %[m1]\n s_cbranch_vccnz .Lprobe_out_%=\n");
        if (CASE == kSalu8)
            BODY(FMA("%[x0]") "s_add_u32 %[c0], %[c0], 1\n s_add_u32 %[c0], %[c0], 1\n s_add_u32 %[c0], %[c0], 1\n s_add_u32 %[c0], %[c0], 1\n"
                 "s_add_u32 %[c0], %[c0], 1\n s_add_u32 %[c0], %[c0], 1\n s_add_u32 %[c0], %[c0], 1\n s_add_u32 %[c0], %[c0], 1\n");
    }
    const unsigned long long t1 = __builtin_amdgcn_s_memtime();
    const unsigned long long r1 = __builtin_amdgcn_s_memrealtime();
    double s = x0 + x1 + x2;
    for (int i = 0; i < 8; ++i) s += y[i];
    out[0] = t1 - t0;
    out[1] = r1 - r0;
    out[2] = (unsigned long long)__double_as_longlong(s) + c0;   // keeps every chain alive
}

#define CK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { fprintf(stderr, "%s: %s\n", #x, hipGetErrorString(e_)); return 1; } } while (0)

typedef void (*Kernel)(unsigned long long *, int, double, double, double);

int main() {
    hipDeviceProp_t p;
    CK(hipGetDeviceProperties(&p, 0));
    unsigned long long *out, host[3];
    CK(hipMalloc(&out, sizeof(host)));
    const Kernel kernels[kCases] = {probe_kernel<kDepFma>,   probe_kernel<kDepAddMul>,  probe_kernel<kIlp2>,     probe_kernel<kIlp3>,
                                    probe_kernel<kIlp8>,     probe_kernel<kDepRcp8>,    probe_kernel<kDiv6>,     probe_kernel<kPowF32>,
                                    probe_kernel<kBrAdjacent>, probe_kernel<kBrCmpFar>, probe_kernel<kBrFar>,    probe_kernel<kBrNone>,
                                    probe_kernel<kRcpUse>,   probe_kernel<kRcpShadow3>, probe_kernel<kSccTaken>, probe_kernel<kSccNotTaken>,
                                    probe_kernel<kMaskOr>,   probe_kernel<kSalu8>};
    const int iters = 20000, reps = 5;
    // x -> 0.5 x + 1 settles at 2 (no overflow, no denormal whatever the case does to x in between); `big` is never exceeded
    const double a = 0.5, b = 1.0, big = 1e300;
    double cyc[kCases], ns[kCases], clock_mhz[kCases], wall_clock_mhz = 0.0;
    for (int c = 0; c < kCases; ++c) {
        hipLaunchKernelGGL(kernels[c], dim3(1), dim3(1), 0, 0, out, 100, a, b, big);   // warm-up: code object, clocks
        CK(hipDeviceSynchronize());
        double best_ticks = 1e300, best_real = 0.0, best_wall = 0.0;
        for (int rep = 0; rep < reps; ++rep) {
            const auto w0 = std::chrono::steady_clock::now();
            hipLaunchKernelGGL(kernels[c], dim3(1), dim3(1), 0, 0, out, iters, a, b, big);
            CK(hipDeviceSynchronize());
            const double wall = std::chrono::duration<double>(std::chrono::steady_clock::now() - w0).count();
            CK(hipMemcpy(host, out, sizeof(host), hipMemcpyDeviceToHost));
            if ((double)host[0] < best_ticks) { best_ticks = (double)host[0]; best_real = (double)host[1]; best_wall = wall; }
        }
        const double n = (double)iters * UNROLL * kInfo[c].per_group;
        cyc[c] = best_ticks / n;
        ns[c] = best_real * 10.0 / n;                       // s_memrealtime ticks at 100 MHz
        clock_mhz[c] = best_ticks / best_real * 100.0;
        if (c == kDepFma) wall_clock_mhz = best_ticks / best_wall * 1e-6;   // launch and sync included: a lower bound
    }
    printf("{\"probe\": \"fp64_lone_chain\", \"device\": \"%s\", \"arch\": \"%s\", \"reported_clock_MHz\": %d, \"live_lanes\": 1, "
           "\"iters\": %d, \"groups_per_iter\": %d, \"lone_wave_clock_MHz\": %.0f, \"lone_wave_clock_MHz_against_host_wall\": %.0f, \"cases\": {",
           p.name[0] ? p.name : "(no name reported by the runtime)", p.gcnArchName, p.clockRate / 1000, iters, UNROLL, clock_mhz[kDepFma], wall_clock_mhz);
    for (int c = 0; c < kCases; ++c)
        printf("%s\"%s\": {\"instructions_per_group\": %d, \"cycles_per_instruction\": %.3f, \"ns_per_instruction\": %.3f, \"clock_MHz\": %.0f}",
               c ? ", " : "", kInfo[c].name, kInfo[c].per_group, cyc[c], ns[c], clock_mhz[c]);
    printf("}}\n");
    return 0;
}
