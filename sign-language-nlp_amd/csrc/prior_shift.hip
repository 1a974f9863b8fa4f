// prior_shift.hip -- label-shift adaptation on the device: the class priors of a set of UNLABELLED rows re-estimated by EM, and
// the log-probs re-weighted by them (slnlp.PriorShift, slnlp/prior_shift.py; include/slnlp.h states the
// algorithm, tests/prior_shift_ref.py is its numpy restatement, line by line).
//
// A classifier trained under the class priors pi_s and used under pi_t is corrected exactly by p_t(c | x) ~ p_s(c | x) pi_t(c) /
// pi_s(c).  pi_t is the fixed point of  pi_c <- mean_i softmax_c(beta z_i + ln pi - ln pi_s)  (Saerens, Latinne and Decaestecker
// 2002: the EM of the mixture whose component posteriors the classifier supplies; every iteration raises the rows' likelihood).
// With z float32 log-probs [N, ld] (V columns used), beta the inverse temperature, ls = ln pi_s and lw the current log-ratio,
// iteration t is
//   a_ic = beta z_ic + lw_c      lse_i = max_c a_ic + log sum_c exp(a_ic - max)      S_c = sum_i exp(a_ic - lse_i)      pi_c = S_c / M
// over the M rows that hold no NaN and have a finite maximum.  Everything but z itself is fp64.
//
// HOW IT RUNS.  The call queues a FIXED sequence of 3 (max_iter + 1) + 2 launches and never waits for the host.  Iteration t:
//   prior_rows     one wave per row, four rows per block, rows over a grid-stride loop (wave_rows, common.hpp): lanes stride the
//                  columns; the maximum of a and the sum of exp(a - max) are wave reductions in a fixed order; lane 0 writes lse_i
//                  (NaN for an excluded row) into scratch.  Iteration 0 runs at lw = 0 and keeps its lse_i for the gain.
//   prior_classes  one block of 256 threads per class c (ranking.hip's grid): thread t adds exp(a_ic - lse_i) over rows t, t + 256,
//                  ... in increasing order, then a fixed binary tree over the 256 partial sums in LDS -- an order that depends
//                  on N alone -- and thread 0 writes S_c into scratch.
//   prior_update   ONE block: pi_c = S_c / M into table row 1 (iteration 0: row 0 too), lw_c = ln max(pi_c, 2^-1022) - ls_c into
//                  row 2, d = max_c |pi_c - previous pi_c| (a maximum: it does not depend on the order), and thread 0 takes the
//                  stop decision and writes `state`.
// then prior_rows once more at the result's lw and prior_gain, one block that sums lse_i(lw) - lse_i(0) like prior_classes does.
// The stop decision is taken by one thread and read by every later launch as a flag in `state`, so every block of every launch
// sees the same decision; once it is set the iteration launches return at once, the two final launches always run.  No
// atomics, nothing depends on the grid or on timing: the result is a pure function of the arguments.
//
// COST.  One fp64 exp per (row, column) in prior_rows and another in prior_classes, per iteration; prior_classes reads the
// matrix by columns (a 4-byte load per row and thread), out of L2 for the [4000, 202] sets this project judges.  What is
// measured (tools/time_prior_shift.py, profiles/prior_shift_timing.json) is the whole queued sequence against one forward pass.
//
// slnlp_shift_logp writes out[i, c] = a_ic - lse_i for a given lw, as (a - max) - log1p(sum e - 1) with the columns AT the
// maximum counted and not summed (scale_logp's form: the value at the maximum of a confident row keeps its digits), rounded
// once to float32.  IN PLACE (out == logp, ld_out == ld) is allowed under scale_logp's rule: a lane RE-READS each of its columns
// right before it stores that column, no other lane or wave touches it, and the row's reductions -- data-dependent on every
// load of the row -- are complete before the first store.
#include <limits.h>
#include <math.h>

#include "block_reduce.hpp"
#include "common.hpp"
#include "fit_state.hpp"
#include "launch.hpp"
#include "logp_row.hpp"
#include "spans.hpp"

// a_ic = beta z_ic + lw_c is rounded after the product and after the sum, as the restatement's numpy expression is: no fused
// multiply-add in this file's own arithmetic
#pragma clang fp contract(off)

namespace slnlp {

constexpr double PRIOR_FLOOR = 2.2250738585072014e-308;  // 2^-1022: ln of it is finite, so is every lw
// state (fit_state.hpp): this fit's own doubles; FIT_BAD counts the rows that hold a NaN or have no finite maximum
enum { PRIOR_GAIN = 0, PRIOR_D = 1 };
// the evaluation a launch belongs to: 0 .. max_iter are the iterations, PRIOR_FINAL the one at the result
constexpr int PRIOR_FINAL = -1;

// lse_i at lw (null: lw = 0) for every row, NaN for an excluded one
__device__ __forceinline__ void prior_rows_body(const float* __restrict__ logp, long ld, int N, int V, const double* __restrict__ beta_dev,
                                                const double* __restrict__ lw, const double* __restrict__ state,
                                                double* __restrict__ lse, int eval) {
    if (fit_settled(state, eval, 0, PRIOR_FINAL)) return;
    const double beta = beta_dev ? beta_dev[0] : 1.0;
    wave_rows(N, [&](long r, int lane) {
        const float* row = logp + r * ld;
        const LogpRowMax m = logp_row_argmax(row, V, lane);
        double amax = -INFINITY;
        for (int j = lane; j < V; j += 64) amax = fmax(amax, beta * (double)row[j] + (lw ? lw[j] : 0.0));
        amax = wave_max_d(amax);
        double s = 0.0;
        for (int j = lane; j < V; j += 64) s += exp((beta * (double)row[j] + (lw ? lw[j] : 0.0)) - amax);
        s = wave_sum_d(s);
        if (lane == 0) lse[r] = m.finite ? amax + log(s) : NAN;
    });
}
SLNLP_ZKERNEL(prior_rows_kernel, 256, prior_rows_body)

// S_c = sum_i exp(a_ic - lse_i) over the rows that count: block c
__device__ __forceinline__ void prior_classes_body(const float* __restrict__ logp, long ld, int N, const double* __restrict__ beta_dev,
                                                   const double* __restrict__ lw, const double* __restrict__ state,
                                                   const double* __restrict__ lse, double* __restrict__ S, int eval) {
    if (fit_settled(state, eval, 0, PRIOR_FINAL)) return;              // (every thread reads the same flag: the block returns as one)
    __shared__ double red[256];
    const double beta = beta_dev ? beta_dev[0] : 1.0;
    const int tid = threadIdx.x;
    const long c = blockIdx.x;
    const double lwc = lw ? lw[c] : 0.0;
    block_sum_rows<1>(&red, tid, N, [&](long r, double* s) {
        const double l = lse[r];
        if (l == l) s[0] += exp((beta * (double)logp[r * ld + c] + lwc) - l);
    });
    if (tid == 0) S[c] = red[0];
}
SLNLP_ZKERNEL(prior_classes_kernel, 256, prior_classes_body)

// pi = S / M, lw, d and the stop decision of iteration `eval`; table = (pi^1, pi, lw), each [V]
__device__ __forceinline__ void prior_update_body(const double* __restrict__ S, const double* __restrict__ lse0,
                                                  const double* __restrict__ log_source, int N, int V, int max_iter, double tol,
                                                  double* __restrict__ table, double* __restrict__ state, int eval) {
    if (fit_settled(state, eval, 0, PRIOR_FINAL)) return;
    __shared__ double red[256];
    __shared__ int bad_red[256];
    int64_t* q = fit_words(state);
    const int tid = threadIdx.x;
    long M = q[FIT_ROWS];
    if (eval == 0) {                                     // count the rows prior_rows excluded
        block_sum_rows<1>(&bad_red, tid, N, [&](long r, int* bad) { bad[0] += lse0[r] != lse0[r] ? 1 : 0; });
        M = (long)N - bad_red[0];
    }
    double* mean = table;
    double* pi = table + V;
    double* lw = table + 2 * (long)V;
    double d = 0.0;
    for (long c = tid; c < V; c += 256) {
        const double before = eval == 0 ? exp(log_source[c]) : pi[c];
        const double now = M > 0 ? S[c] / (double)M : before;      // no rows: pi stays the source's, lw = 0
        const double diff = fabs(now - before);
        d = diff > d || diff != diff ? diff : d;         // (a NaN, from arguments out of contract, is kept: d <= tol then fails)
        pi[c] = now;
        if (eval == 0) mean[c] = now;
        lw[c] = M > 0 ? log(fmax(now, PRIOR_FLOOR)) - log_source[c] : 0.0;
    }
    red[tid] = d;
    block_tree<1>(&red, tid, [](double m, double o) { return o > m || o != o ? o : m; });   // the larger, or a NaN, wins
    if (tid != 0) return;
    if (eval == 0) {
        fit_state_reset(state, M, (long)N - M);
        if (M == 0) {
            q[FIT_REASON] = SLNLP_PRIOR_EMPTY;
            return;
        }
    }
    d = red[0];
    state[PRIOR_D] = d;
    q[FIT_ITERATIONS] = eval + 1;
    if (d <= tol) q[FIT_REASON] = SLNLP_PRIOR_TOL;
    else if (eval == max_iter) q[FIT_REASON] = SLNLP_PRIOR_CAP;
}
SLNLP_ZKERNEL(prior_update_kernel, 256, prior_update_body)

// gain = (1 / M) sum_i (lse_i(lw) - lse_i(0)) over the rows that count
__device__ __forceinline__ void prior_gain_body(const double* __restrict__ lse, const double* __restrict__ lse0, int N,
                                                double* __restrict__ state) {
    __shared__ double red[256];
    const int tid = threadIdx.x;
    block_sum_rows<1>(&red, tid, N, [&](long r, double* s) {
        const double l0 = lse0[r];
        if (l0 == l0) s[0] += lse[r] - l0;
    });
    if (tid != 0) return;
    const int64_t M = fit_words(state)[FIT_ROWS];
    state[PRIOR_GAIN] = M > 0 ? red[0] / (double)M : 0.0;
}
SLNLP_ZKERNEL(prior_gain_kernel, 256, prior_gain_body)

// (no __restrict__ on logp / out: out may be logp itself)
__device__ __forceinline__ void shift_logp_body(const float* logp, long ld, int N, int V, const double* __restrict__ beta_dev,
                                                const double* __restrict__ lw, float* out, long ld_out) {
    const double beta = beta_dev ? beta_dev[0] : 1.0;
    wave_rows(N, [&](long r, int lane) {
        const float* row = logp + r * ld;
        float* dst = out + r * ld_out;
        const LogpRowMax m = logp_row_argmax(row, V, lane);
        double amax = -INFINITY;
        for (int j = lane; j < V; j += 64) amax = fmax(amax, beta * (double)row[j] + lw[j]);
        amax = wave_max_d(amax);
        double rest = 0.0, at_max = 0.0;                 // sum e - 1 without the 1 ever entering a sum
        for (int j = lane; j < V; j += 64) {
            const double a = beta * (double)row[j] + lw[j];
            if (a == amax) at_max += 1.0; else rest += exp(a - amax);
        }
        // lse - amax; it depends on every load of the row: none is outstanding past here
        const double l = log1p(wave_sum_d(rest) + (wave_sum_d(at_max) - 1.0));
        const bool ok = m.finite && fabs(amax) < INFINITY;           // a row without a softmax: NaN in every column
        for (int j = lane; j < V; j += 64)                           // re-read, then stored, by its own lane
            dst[j] = ok ? (float)(((beta * (double)row[j] + lw[j]) - amax) - l) : NAN;
    });
}
SLNLP_ZKERNEL(shift_logp_kernel, 256, shift_logp_body)

static size_t prior_scratch_bytes(int64_t N, int64_t V) { return (2 * (size_t)N + (size_t)V) * 8; }   // lse(0), lse, S

int64_t fit_priors_scratch_bytes(int64_t N, int64_t V) {
    if (N < 1 || N > INT_MAX || V < 1 || V > INT_MAX) {
        set_error("fit_priors_scratch_bytes: N=%ld or V=%ld outside 1..%d", (long)N, (long)V, INT_MAX);
        return -1;
    }
    return (int64_t)prior_scratch_bytes(N, V);
}

int fit_priors(const float* logp, int64_t ld, int64_t N, int64_t V, const double* beta_dev, const double* log_source, int max_iter,
               double tol, double* table, void* state, void* scratch, int64_t scratch_bytes, hipStream_t st) {
    SLNLP_CHECK_ARG(logp && log_source && table && state && scratch, "fit_priors: null pointer");
    Span z;
    SLNLP_TRY(check_logp_matrix("fit_priors", logp, N, INT_MAX, V, INT_MAX, ld, &z));
    SLNLP_CHECK_ARG(max_iter >= 0 && max_iter <= SLNLP_PRIOR_MAX_ITER, "fit_priors: max_iter=%d outside 0..%d", max_iter, SLNLP_PRIOR_MAX_ITER);
    SLNLP_CHECK_ARG(tol >= 0.0 && tol < INFINITY, "fit_priors: tol=%g is not a finite number >= 0", tol);
    const size_t need = prior_scratch_bytes(N, V);
    SLNLP_TRY(check_scratch("fit_priors", scratch, scratch_bytes, need, N, V, 0));
    SLNLP_CHECK_ARG(((uintptr_t)logp & 3) == 0, "fit_priors: misaligned pointer (logp: 4 bytes)");
    SLNLP_CHECK_ARG((((uintptr_t)beta_dev | (uintptr_t)log_source | (uintptr_t)table | (uintptr_t)state | (uintptr_t)scratch) & 7) == 0,
                    "fit_priors: misaligned pointer (beta, log_source, table, state, scratch: 8 bytes)");
    const Span out[3] = {{table, 3 * (size_t)V * 8, "table"}, {state, SLNLP_PRIOR_STATE_BYTES, "state"}, {scratch, need, "scratch"}};
    const Span in[3] = {z, {beta_dev, 8, "beta"}, {log_source, (size_t)V * 8, "log_source"}};
    SLNLP_TRY(check_no_overlap("fit_priors", out, in));
    double* lse0 = (double*)scratch;
    double* lse = lse0 + N;
    double* S = lse + N;
    const double* lw = table + 2 * V;
    const int blocks = wave_rows_grid(N);
    for (int t = 0; t <= max_iter; ++t) {
        SLNLP_TRY(zlaunch(prior_rows_kernel, dim3(blocks), 256, 0, st, "fit_priors_rows", logp, (long)ld, (int)N, (int)V, beta_dev,
                          t == 0 ? (const double*)nullptr : lw, (const double*)state, t == 0 ? lse0 : lse, t));
        SLNLP_TRY(zlaunch(prior_classes_kernel, dim3((unsigned)V), 256, 0, st, "fit_priors_classes", logp, (long)ld, (int)N, beta_dev,
                          t == 0 ? (const double*)nullptr : lw, (const double*)state, (const double*)(t == 0 ? lse0 : lse), S, t));
        SLNLP_TRY(zlaunch(prior_update_kernel, dim3(1), 256, 0, st, "fit_priors_update", (const double*)S, (const double*)lse0, log_source,
                          (int)N, (int)V, max_iter, tol, table, (double*)state, t));
    }
    SLNLP_TRY(zlaunch(prior_rows_kernel, dim3(blocks), 256, 0, st, "fit_priors_rows", logp, (long)ld, (int)N, (int)V, beta_dev, lw,
                      (const double*)state, lse, PRIOR_FINAL));
    return zlaunch(prior_gain_kernel, dim3(1), 256, 0, st, "fit_priors_gain", (const double*)lse, (const double*)lse0, (int)N, (double*)state);
}

int shift_logp(const float* logp, int64_t ld, int64_t N, int64_t V, const double* beta_dev, const double* log_w, float* out,
               int64_t ld_out, hipStream_t st) {
    SLNLP_CHECK_ARG(logp && log_w && out, "shift_logp: null pointer");
    Span z, o;
    SLNLP_TRY(check_logp_matrix("shift_logp", logp, N, INT_MAX, V, INT_MAX, ld, &z));
    SLNLP_TRY(check_out_matrix("shift_logp", out, N, "N", V, ld_out, &o));
    SLNLP_CHECK_ARG((((uintptr_t)logp | (uintptr_t)out) & 3) == 0 && (((uintptr_t)beta_dev | (uintptr_t)log_w) & 7) == 0,
                    "shift_logp: misaligned pointer (logp, out: 4 bytes; beta, log_w: 8 bytes)");
    SLNLP_TRY(check_in_place("shift_logp", o, ld_out, z, ld));
    SLNLP_CHECK_ARG(!spans_overlap(o, Span{beta_dev, 8, "beta"}) && !spans_overlap(o, Span{log_w, (size_t)V * 8, "log_w"}),
                    "shift_logp: out overlaps beta or log_w");
    const int blocks = wave_rows_grid(N);
    return zlaunch(shift_logp_kernel, dim3(blocks), 256, 0, st, "shift_logp", logp, (long)ld, (int)N, (int)V, beta_dev, log_w, out, (long)ld_out);
}

}  // namespace slnlp

extern "C" int64_t slnlp_fit_priors_scratch_bytes(int64_t N, int64_t V) { return slnlp::fit_priors_scratch_bytes(N, V); }

extern "C" int slnlp_fit_priors(const float* logp, int64_t ld, int64_t N, int64_t V, const double* beta_dev, const double* log_source,
                                int max_iter, double tol, double* table, void* state, void* scratch, int64_t scratch_bytes, void* stream) {
    return slnlp::fit_priors(logp, ld, N, V, beta_dev, log_source, max_iter, tol, table, (double*)state, scratch, scratch_bytes,
                             (hipStream_t)stream);
}

extern "C" int slnlp_shift_logp(const float* logp, int64_t ld, int64_t N, int64_t V, const double* beta_dev, const double* log_w, float* out,
                                int64_t ld_out, void* stream) {
    return slnlp::shift_logp(logp, ld, N, V, beta_dev, log_w, out, ld_out, (hipStream_t)stream);
}
