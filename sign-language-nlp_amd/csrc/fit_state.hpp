// fit_state.hpp -- the device-resident state of the queued fits (fit_temperature, fit_bias_temperature, fit_priors; DESIGN.md
// section 4): 8 doubles, then 8 int64 (include/slnlp.h documents them).  A fit queues a fixed sequence of launches and never waits
// for the host; ONE thread takes the stop decision and writes the reason, every later launch reads it as a flag, so every block of
// every launch sees the same decision.  Here: the slots the fits share, the flag's read, the reset, and the result's writer.  A
// fit's own slots (doubles 4 .. 7, words 4 .. 7; fit_priors: doubles 0 and 1 too) stay an enum in its file.
#pragma once
#include "common.hpp"

namespace slnlp {

enum { FIT_BETA = 0, FIT_T = 1, FIT_F_BEFORE = 2, FIT_F_AFTER = 3 };        // doubles: the two calibrations
enum { FIT_REASON = 0, FIT_ITERATIONS = 1, FIT_ROWS = 2, FIT_BAD = 3 };     // words: every fit (BAD: labels out of range, or NaN rows)

__device__ __forceinline__ int64_t* fit_words(double* state) { return (int64_t*)(state + 8); }
__device__ __forceinline__ const int64_t* fit_words(const double* state) { return (const int64_t*)(state + 8); }

// whether the stop decision has been taken (every thread reads the same flag: a block returns as one)
__device__ __forceinline__ bool fit_settled(const double* state) { return fit_words(state)[FIT_REASON] != 0; }
// whether evaluation `eval` of the sequence has nothing left to do: `first` initialises the state and `final` always runs, at the
// result -- neither reads the flag
__device__ __forceinline__ bool fit_settled(const double* state, int eval, int first, int final) {
    return eval != first && eval != final && fit_settled(state);
}

// the first evaluation's thread 0: all 16 words zero, then the rows that count and those that do not
__device__ __forceinline__ void fit_state_reset(double* state, long rows, long bad) {
    int64_t* q = fit_words(state);
    for (int k = 0; k < 8; ++k) state[k] = 0.0;
    for (int k = 0; k < 8; ++k) q[k] = 0;
    q[FIT_ROWS] = rows;
    q[FIT_BAD] = bad;
}

// entry i of the result (beta, b_0, b_1, ..): beta and T = 1 / beta go into the state, a bias into `bias`
__device__ __forceinline__ void fit_result(double* state, double* bias, int i, double v) {
    if (i == 0) {
        state[FIT_BETA] = v;
        state[FIT_T] = 1.0 / v;
    } else {
        bias[i - 1] = v;
    }
}

}  // namespace slnlp
