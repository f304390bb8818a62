// user_event.h -- scheduled events of a user model (include/smc_hip.h: smc_set_model_user6): at known times the state jumps
// (a dose, a feed addition, a reset) and the integrator stops there.  Device code only, handed to hiprtc as an in-memory header
// and included by the generated source ONLY for a model with events (user_model.hip: build_source defines SMC_USER_EVENTS,
// SMC_USER_EVAT, SMC_USER_NEV and SMC_USER_NVAL in front of the #include); a model without events never sees this file, and the
// kernel files reach it stripped of their SMC_USER_EVENTS blocks (csrc/Makefile), the text they had before events existed.
//
// The table lies BEHIND each experiment's cond row in global memory, after the input table of user_input.h if there is one
// (DESIGN.md 4.11).  In doubles, with A = SMC_USER_EVAT, E = SMC_USER_NEV (the event capacity), V = SMC_USER_NVAL:
//   [A, A + E]                    the row's m <= E event times, strictly increasing, then +inf: E + 1 words, so that the index
//                                 of the next event, which never exceeds E, always reads a time
//   [A + E + 1, .. + E V)         the values, event-major: value k of event j at A + E + 1 + j V + k
// The next event time is read once per segment (item start, event), never per attempt, so it is not part of the LDS image.
#pragma once
#ifndef __HIPCC_RTC__
#include <hip/hip_runtime.h>
#endif

namespace smc_ev {

constexpr int kAt = SMC_USER_EVAT, kEvents = SMC_USER_NEV, kValues = SMC_USER_NVAL;
static_assert(kAt >= 0 && kEvents >= 1 && kEvents <= 256 && kValues >= 0 && kValues <= 8,
              "SMC_USER_NEV in 1 .. 256 (SMC_USER_MAX_EVENTS), SMC_USER_NVAL in 0 .. 8 (SMC_USER_MAX_EVENT_VALUES)");
constexpr int kValueAt = kAt + kEvents + 1;
constexpr int kRowWords = kEvents + 1 + kEvents * kValues;      // what the table adds to a cond row

// what a source calls: value k of event j of the experiment `cond` belongs to
__device__ __forceinline__ double smc_event_value(const double *cond, int j, int k) { return cond[kValueAt + j * kValues + k]; }

// The bound of the segment in front of event i_ev of a row that ends at t_end: the event's time if it fires, else the row's
// end.  An event fires only strictly inside the row (tau < t_end; tau > t0 is a data rule): one at or beyond t_end, and the
// +inf behind the row's last event, gives t_end.
__device__ __forceinline__ double segment_bound(const double *cond, int i_ev, double t_end) {
    const double tau = cond[kAt + i_ev];
    return (tau < t_end) ? tau : t_end;
}

}  // namespace smc_ev
