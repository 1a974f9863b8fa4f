// calibration.hip -- temperature calibration fitted and applied on the device (the estimator's `calibration` option; DESIGN.md
// section 4; slnlp/net.py, slnlp/lockstep.py).
//
// One scalar T, fitted after training on the fit's held-out valid split, applied as softmax(z / T) at prediction time: the
// arg-max never moves, the log-loss does.  With beta = 1 / T, z float32 log-probs [N, ld] (V columns used), y int64 [N], and
// p = softmax(beta z_i), the objective is the mean over the M rows whose label lies in [0, V) of
//   f_i = logsumexp_c(beta z_ic) - beta z_iy        g_i = sum_c p_c z_ic - z_iy        (df / dbeta)
//   h_i = sum_c p_c z_ic^2 - (sum_c p_c z_ic)^2     (d2f / dbeta2 >= 0)                s_i = |sum_c p_c z_ic| + |z_iy|
// f is convex in beta; s is the scale the gradient test is relative to.  slnlp_fit_temperature minimises f over beta in
// [2^-6, 2^6] by the fixed algorithm include/slnlp.h states (tests/calibration_ref.py is its numpy restatement, line by line):
// end-point tests, then a safeguarded Newton iteration in u = ln beta, where the step -g / (g + beta h) is scale free and beta
// stays positive.  Everything but z itself is fp64.
//
// HOW IT RUNS.  The call queues a FIXED sequence of 36 evaluations and never waits for the host:
//   0: beta = 1 (nll_before, the flat test's second half)   1: beta = 2^-6   2: beta = 2^6   3 .. 34: the 32 iterations
//   35: the result (nll_after)
// One evaluation is two launches.  fit_rows: one wave per row, four rows per block, rows over a grid-stride loop (wave_rows,
// common.hpp); lanes stride the columns, the row maximum and the sums sum e - 1, sum e z, sum e z^2 (e = exp(beta z - max)) are wave
// reductions in a fixed order (DPP inside 16 lanes, v_readlane across the four rows), and lane 0 writes (f_i, g_i, h_i, s_i)
// into scratch [N, 4].  fit_update: ONE block of 256 threads sums the row terms -- thread t rows t, t + 256, ... in increasing
// order, then a fixed binary tree over the 256 partial sums in LDS: an order that depends on N alone -- and thread 0 applies
// the update rule and writes `state`.  The row terms go through scratch, not per-block partial sums, so the result is a pure
// function of the arguments: nothing depends on the grid, the block count or timing.  Once the reason is set, evaluations
// 1 .. 34 read the flag and return; evaluation 35 always runs, at the result.
//
// COST.  fp64 exp / log are software sequences on the device (tens of instructions each), one exp per (row, column) and
// evaluation.  N V is at most about 10^6 here and a fit calibrates once, so that cost does not matter; what is measured
// (tools/time_calibration.py, profiles/calibration_timing.json) is the whole 72-launch sequence and one slnlp_scale_logp call
// against one valid pass over the same rows -- the only yardstick the fitting cost answers to.
//
// slnlp_scale_logp writes the calibrated log-probs out[i, c] = beta z_ic - logsumexp_c'(beta z_ic'), beta read from device
// memory (state's first double), per row in fp64 with the maximum subtracted -- (beta z - max) - log1p(sum e - 1), so the value at
// the maximum, which is tiny for a confident row, keeps its digits -- rounded once to float32.  Same wave-per-row
// shape.  IN PLACE (out == logp, ld_out == ld) is allowed: a lane RE-READS each of its columns right before it stores that
// column, no other lane or wave touches it, and the row's logsumexp -- a wave reduction, data-dependent on every load of the
// row -- is complete before the first store.  Any other overlap of the two matrices is rejected.
#include <limits.h>
#include <math.h>

#include "common.hpp"
#include "fit_state.hpp"
#include "launch.hpp"
#include "scale_row.hpp"
#include "spans.hpp"

namespace slnlp {

constexpr int CAL_ITERS = 32;          // the iteration cap
constexpr int CAL_EVALS = CAL_ITERS + 4;   // beta = 1, the two bounds, the iterations, the result
// state (fit_state.hpp): the iteration's own doubles and word
enum { CAL_LO = 4, CAL_HI = 5, CAL_NEXT = 6 };
enum { CAL_FLAT_AT_ONE = 4 };
constexpr double CAL_BETA_MIN = 0.015625, CAL_BETA_MAX = 64.0;                    // 2^-6, 2^6
constexpr double CAL_GRAD_TOL = 5.6843418860808015e-14;                           // 2^-44
constexpr double CAL_STEP_TOL = 9.094947017729282e-13;                            // 2^-40

// (the fp64 wave reductions dpp_mov_d / lane_bcast_d / wave_sum_d: common.hpp, shared with reliability.hip)

__device__ __forceinline__ void fit_rows_body(const float* __restrict__ logp, long ld, const int64_t* __restrict__ y, int N, int V,
                                              const double* __restrict__ state, double* __restrict__ terms, int eval) {
    if (fit_settled(state, eval, 0, CAL_EVALS - 1)) return;
    const double beta = eval == 0 ? 1.0 : state[CAL_NEXT];
    wave_rows(N, [&](long r, int lane) {
        const float* row = logp + r * ld;
        const int64_t label = y[r];
        const bool ok = label >= 0 && label < V;         // a label outside the columns is never used as an index
        float zmax = -INFINITY;
        for (int j = lane; j < V; j += 64) zmax = fmaxf(zmax, row[j]);
        zmax = wave_max(zmax);
        const double a = beta * (double)zmax;            // beta > 0: the maximum of beta z
        // the columns AT the maximum have e = 1 exactly: they are counted, the others summed, so that sum e - 1 -- what log1p
        // takes -- loses nothing to the 1 (a confident row's f_i is tiny against a)
        double rest = 0.0, at_max = 0.0, s1 = 0.0, s2 = 0.0;
        for (int j = lane; j < V; j += 64) {
            const float zf = row[j];
            const double z = (double)zf;
            const double e = exp(beta * z - a);
            if (zf == zmax) at_max += 1.0; else rest += e;
            s1 += e * z;
            s2 += e * z * z;
        }
        rest = wave_sum_d(rest) + (wave_sum_d(at_max) - 1.0);    // sum e - 1 (at_max >= 1: whole numbers, summed exactly)
        const double s0 = 1.0 + rest;
        s1 = wave_sum_d(s1);
        s2 = wave_sum_d(s2);
        if (lane == 0) {
            double4 t = {0.0, 0.0, 0.0, 0.0};            // an excluded row adds nothing to any sum
            if (ok) {
                const double zy = (double)row[label], mean = s1 / s0;
                t.x = log1p(rest) - (beta * zy - a);
                t.y = mean - zy;
                t.z = s2 / s0 - mean * mean;
                t.w = fabs(mean) + fabs(zy);
            }
            *(double4*)(terms + 4 * r) = t;
        }
    });
}
SLNLP_ZKERNEL(fit_rows_kernel, 256, fit_rows_body)

// the end of the search: the result, why, and after how many iterations; evaluation 35 then runs at the result
__device__ __forceinline__ void cal_finish(double* state, int64_t* q, double beta, int reason, int iterations) {
    fit_result(state, nullptr, 0, beta);
    state[CAL_NEXT] = beta;
    q[FIT_ITERATIONS] = iterations;
    q[FIT_REASON] = reason;
}

__device__ __forceinline__ void fit_update_body(const double* __restrict__ terms, const int64_t* __restrict__ y, int N, int V,
                                                double* __restrict__ state, int eval) {
    if (fit_settled(state, eval, 0, CAL_EVALS - 1)) return;
    int64_t* q = fit_words(state);
    __shared__ double red[4][256];
    __shared__ int bad_red[256];
    const int tid = threadIdx.x;
    double f = 0.0, g = 0.0, h = 0.0, s = 0.0;
    int bad = 0;
    for (long r = tid; r < N; r += 256) {
        const double4 t = *(const double4*)(terms + 4 * r);
        f += t.x; g += t.y; h += t.z; s += t.w;
        const int64_t label = y[r];
        bad += (label < 0 || label >= V) ? 1 : 0;
    }
    red[0][tid] = f; red[1][tid] = g; red[2][tid] = h; red[3][tid] = s;
    bad_red[tid] = bad;
    __syncthreads();
    for (int w = 128; w >= 1; w >>= 1) {                 // block_reduce.hpp's tree over the four doubles AND the int: one pass of
        if (tid < w) {                                   // nine barriers where two block_tree calls make two, 36 times a fit
#pragma unroll
            for (int k = 0; k < 4; ++k) red[k][tid] += red[k][tid + w];
            bad_red[tid] += bad_red[tid + w];
        }
        __syncthreads();
    }
    if (tid != 0) return;
    const long n_bad = bad_red[0], M = (long)N - n_bad;
    if (eval == 0) {
        fit_state_reset(state, M, n_bad);
        if (M == 0) {                                    // nothing to fit on: T = 1 (the caller reads bad_labels)
            cal_finish(state, q, 1.0, SLNLP_CAL_FLAT, 0);
            return;
        }
    }
    const double inv = M > 0 ? 1.0 / (double)M : 0.0;    // (no rows: evaluation 35 records f = 0)
    f = red[0][0] * inv; g = red[1][0] * inv; h = red[2][0] * inv; s = red[3][0] * inv;
    const bool flat = fabs(g) <= CAL_GRAD_TOL * s;
    if (eval == 0) {                                     // beta = 1
        state[FIT_F_BEFORE] = f;
        q[CAL_FLAT_AT_ONE] = flat ? 1 : 0;
        state[CAL_NEXT] = CAL_BETA_MIN;
    } else if (eval == 1) {                              // beta = 2^-6
        if (flat && q[CAL_FLAT_AT_ONE]) cal_finish(state, q, 1.0, SLNLP_CAL_FLAT, 0);
        else if (g >= 0.0) cal_finish(state, q, CAL_BETA_MIN, SLNLP_CAL_BOUND, 0);
        else state[CAL_NEXT] = CAL_BETA_MAX;
    } else if (eval == 2) {                              // beta = 2^6
        if (g <= 0.0) {
            cal_finish(state, q, CAL_BETA_MAX, SLNLP_CAL_BOUND, 0);
        } else {                                         // g changes sign: the root is bracketed
            state[CAL_LO] = CAL_BETA_MIN;
            state[CAL_HI] = CAL_BETA_MAX;
            state[CAL_NEXT] = 1.0;
        }
    } else if (eval < CAL_EVALS - 1) {                   // iteration eval - 2 of 32
        const int it = eval - 2;
        const double beta = state[CAL_NEXT];
        if (flat) {
            cal_finish(state, q, beta, SLNLP_CAL_GRADIENT, it);
            return;
        }
        double lo = state[CAL_LO], hi = state[CAL_HI];
        if (g < 0.0) lo = beta; else hi = beta;          // g increases with beta (h >= 0): the root lies where g changes sign
        state[CAL_LO] = lo;
        state[CAL_HI] = hi;
        const double den = g + beta * h;                 // the Newton step in u = ln beta: du = -g / (g + beta h)
        double next = den > 0.0 ? beta * exp(-g / den) : 0.0;
        if (!(next > lo && next < hi)) next = sqrt(lo * hi);
        if (fabs(log(next / beta)) <= CAL_STEP_TOL) cal_finish(state, q, next, SLNLP_CAL_STEP, it);
        else if (it == CAL_ITERS) cal_finish(state, q, next, SLNLP_CAL_CAP, it);
        else state[CAL_NEXT] = next;
    } else {                                             // the result
        state[FIT_F_AFTER] = f;
    }
}
SLNLP_ZKERNEL(fit_update_kernel, 256, fit_update_body)

// (no __restrict__: out may be logp itself); the row itself is scale_row.hpp's, which scatter_logp (label_audit.hip) shares
__device__ __forceinline__ void scale_logp_body(const float* logp, long ld, int N, int V, const double* __restrict__ beta_dev, float* out,
                                                long ld_out) {
    const double beta = beta_dev[0];
    wave_rows(N, [&](long r, int lane) { scale_logp_row(logp + r * ld, out + r * ld_out, V, lane, beta); });
}
SLNLP_ZKERNEL(scale_logp_kernel, 256, scale_logp_body)

int64_t fit_temperature_scratch_bytes(int64_t N) {
    if (N < 1 || N > INT_MAX) {
        set_error("fit_temperature_scratch_bytes: N=%ld outside 1..%d", (long)N, INT_MAX);
        return -1;
    }
    return N * 32;                                       // (f_i, g_i, h_i, s_i) per row
}

int fit_temperature(const float* logp, int64_t ld, const int64_t* y, int64_t N, int64_t V, void* state, void* scratch,
                    int64_t scratch_bytes, hipStream_t st) {
    SLNLP_CHECK_ARG(logp && y && state && scratch, "fit_temperature: null pointer");
    Span z;
    SLNLP_TRY(check_logp_matrix("fit_temperature", logp, N, INT_MAX, V, INT_MAX, ld, &z));
    SLNLP_TRY(check_scratch("fit_temperature", scratch, scratch_bytes, (size_t)N * 32, N, 0, 32));
    SLNLP_CHECK_ARG(((uintptr_t)logp & 3) == 0 && (((uintptr_t)y | (uintptr_t)state) & 7) == 0, "fit_temperature: misaligned pointer");
    const Span labels = {y, (size_t)N * 8, "y"}, s = {state, SLNLP_CAL_STATE_BYTES, "state"}, t = {scratch, (size_t)N * 32, "scratch"};
    SLNLP_CHECK_ARG(!spans_overlap(s, z) && !spans_overlap(s, labels) && !spans_overlap(t, z) && !spans_overlap(t, labels) && !spans_overlap(t, s),
                    "fit_temperature: state or scratch overlaps an input or each other");
    const int blocks = wave_rows_grid(N);
    for (int eval = 0; eval < CAL_EVALS; ++eval) {
        SLNLP_TRY(zlaunch(fit_rows_kernel, dim3(blocks), 256, 0, st, "fit_temperature_rows", logp, (long)ld, y, (int)N, (int)V,
                          (const double*)state, (double*)scratch, eval));
        SLNLP_TRY(zlaunch(fit_update_kernel, dim3(1), 256, 0, st, "fit_temperature_update", (const double*)scratch, y, (int)N, (int)V,
                          (double*)state, eval));
    }
    return 0;
}

int scale_logp(const float* logp, int64_t ld, int64_t N, int64_t V, const double* beta_dev, float* out, int64_t ld_out, hipStream_t st) {
    SLNLP_CHECK_ARG(logp && beta_dev && out, "scale_logp: null pointer");
    SLNLP_TRY(check_logp_dims("scale_logp", N, INT_MAX, V, INT_MAX));
    SLNLP_CHECK_ARG(ld >= V && ld_out >= V, "scale_logp: ld=%ld or ld_out=%ld is less than V=%ld", (long)ld, (long)ld_out, (long)V);
    SLNLP_CHECK_ARG(ld <= INT64_MAX / 8 / N && ld_out <= INT64_MAX / 8 / N, "scale_logp: ld=%ld / ld_out=%ld times N=%ld is no addressable matrix",
                    (long)ld, (long)ld_out, (long)N);
    SLNLP_CHECK_ARG((((uintptr_t)logp | (uintptr_t)out) & 3) == 0 && ((uintptr_t)beta_dev & 7) == 0, "scale_logp: misaligned pointer");
    const Span z = {logp, matrix_bytes(N, ld, V), "logp"}, o = {out, matrix_bytes(N, ld_out, V), "out"};
    SLNLP_TRY(check_in_place("scale_logp", o, ld_out, z, ld));
    SLNLP_CHECK_ARG(!spans_overlap(o, Span{beta_dev, 8, "beta"}), "scale_logp: out overlaps beta");
    const int blocks = wave_rows_grid(N);
    return zlaunch(scale_logp_kernel, dim3(blocks), 256, 0, st, "scale_logp", logp, (long)ld, (int)N, (int)V, beta_dev, out, (long)ld_out);
}

}  // namespace slnlp

extern "C" int64_t slnlp_fit_temperature_scratch_bytes(int64_t N) { return slnlp::fit_temperature_scratch_bytes(N); }

extern "C" int slnlp_fit_temperature(const float* logp, int64_t ld, const int64_t* y, int64_t N, int64_t V, void* state, void* scratch,
                                     int64_t scratch_bytes, void* stream) {
    return slnlp::fit_temperature(logp, ld, y, N, V, state, scratch, scratch_bytes, (hipStream_t)stream);
}

extern "C" int slnlp_scale_logp(const float* logp, int64_t ld, int64_t N, int64_t V, const double* beta_dev, float* out, int64_t ld_out,
                                void* stream) {
    return slnlp::scale_logp(logp, ld, N, V, beta_dev, out, ld_out, (hipStream_t)stream);
}
