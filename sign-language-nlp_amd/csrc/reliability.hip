// reliability.hip -- reliability diagnostics of a set of log-probs on the device: per-row confidence, Brier and log-loss terms and
// the equal-width reliability table that ECE and MCE are functions of (slnlp/metrics.py's neg_ece / neg_mce /
// neg_brier, NeuralNetClassifier.reliability).
//
// z float32 log-probs [N, ld] (V columns used), y int64 [N], B bins, beta = beta_dev ? beta_dev[0] : 1 (a calibration state's
// first double), p = softmax(beta z_i) -- never materialised.  Per row, all in fp64 but z itself, from the row head of
// logp_row.hpp: pred / zmax, a = beta zmax, e_c = exp(beta z_c - a), the k columns at the maximum, rest = sum e - 1, s0 = 1 + rest.
//   pred    the first maximum in score_beats' order on the float32 values       correct = (pred == y_i)
//   conf    1 / s0: the probability of the arg-max class
//   brier   sum_c (p_c - 1[c = y_i])^2 = (k + sum_{c not at max} e_c^2) / s0^2 - 2 exp(beta z_y - a) / s0 + 1
//   nll     log1p(rest) - (beta z_y - a): fit_rows' f_i
//   bin     clamp(ceil(conf B) - 1, 0, B - 1): equal-width, right-closed bins (b / B, (b + 1) / B] (Guo et al. 2017), taken from
//           the conf that is stored -- a saturated row (conf 1 or one ulp below) lands in the top bin either way
// rows[i] = (conf, brier, nll, code): code = 2 bin + correct for a scored row; -1 for a label outside [0, V) (never used as an
// index; the three terms are 0; the label is looked at first); -2 for a row that holds a NaN or whose maximum is not finite (the
// three terms are NaN).  table [B + 1, 4]: row b < B = (count, sum conf, sum correct, 0) over the scored rows of bin b; row B =
// (sum brier, sum nll, n_bad_label, n_nan) -- the two sums over the scored rows only.  tests/reliability_ref.py restates both.
//
// HOW IT RUNS.  Two launches, no atomics, nothing that depends on the grid.  reliability_rows: wave_rows' shape (common.hpp) -- one
// wave per row, four rows per block, rows over a grid-stride loop, lanes stride the columns; the arg-max and the three sums are
// wave reductions in the fixed DPP / v_readlane order (common.hpp); lane 0 stores the row's four doubles; no LDS.
// reliability_table: B + 1 blocks of 256 threads, block b reduces bin b and block B the totals: thread t adds rows t, t + 256, ...
// in increasing order (only those that belong to its block), then fit_update's fixed binary tree over the 256 partial sums in
// LDS.  The result is a pure function of the arguments, so a lockstep fit's numbers equal its solo fit's bit for bit.
#include <limits.h>
#include <math.h>

#include "common.hpp"
#include "launch.hpp"
#include "logp_row.hpp"
#include "spans.hpp"

namespace slnlp {

__device__ __forceinline__ void reliability_rows_body(const float* __restrict__ logp, long ld, const int64_t* __restrict__ y, int N, int V,
                                                      int bins, const double* __restrict__ beta_dev, double* __restrict__ rows) {
    const double beta = beta_dev ? beta_dev[0] : 1.0;
    // (wave_rows' loop, written out: through the helper two of six figures timed above the parent's spread, twice, with no cause
    // in the instruction stream -- profiles/judging_shell_ab.json)
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane((int)(blockIdx.x * 4 + (threadIdx.x >> 6)));
    const int nwaves = gridDim.x * 4;
    const double qnan = __builtin_bit_cast(double, 0x7ff8000000000000ull);
    for (long r = wave; r < N; r += nwaves) {            // r: the same in every lane, so every lane reaches the reductions
        const float* row = logp + r * ld;
        const int64_t label = y[r];
        const bool ok = label >= 0 && label < V;         // a label outside the columns is never used as an index
        const LogpRowMax top = logp_row_argmax(row, V, lane);
        double sq = 0.0;                                 // sum e^2 over the columns not at the maximum
        const LogpRowSums h = logp_row_sums(row, V, lane, beta, top.zmax, [&](double e) { sq += e * e; });
        sq = wave_sum_d(sq);
        if (lane == 0) {
            double4 t = {0.0, 0.0, 0.0, -1.0};           // a label out of range: nothing to score
            if (ok && !top.finite) {
                t = {qnan, qnan, qnan, -2.0};
            } else if (ok) {
                const double s0 = h.s0;
                const double by = beta * (double)row[label] - h.a;
                t.x = 1.0 / s0;
                t.y = (h.n_max + sq) / (s0 * s0) - 2.0 * exp(by) / s0 + 1.0;
                t.z = log1p(h.rest) - by;
                const double bin = fmin(fmax(ceil(t.x * (double)bins) - 1.0, 0.0), (double)(bins - 1));
                t.w = 2.0 * bin + (top.pred == label ? 1.0 : 0.0);
            }
            *(double4*)(rows + 4 * r) = t;
        }
    }
}
SLNLP_ZKERNEL(reliability_rows_kernel, 256, reliability_rows_body)

__device__ __forceinline__ void reliability_table_body(const double* __restrict__ rows, int N, int bins, double* __restrict__ table) {
    __shared__ double red[4][256];
    const int tid = threadIdx.x, b = blockIdx.x;         // b < bins: that bin; b == bins: the totals
    double s0 = 0.0, s1 = 0.0, s2 = 0.0, s3 = 0.0;
    for (long r = tid; r < N; r += 256) {
        const double4 t = *(const double4*)(rows + 4 * r);
        const int code = (int)t.w;                       // exact: -2, -1 or 2 bin + correct < 128
        if (b < bins) {
            if (code >= 0 && (code >> 1) == b) { s0 += 1.0; s1 += t.x; s2 += (double)(code & 1); }
        } else if (code >= 0) {
            s0 += t.y; s1 += t.z;
        } else if (code == -1) {
            s2 += 1.0;
        } else {
            s3 += 1.0;
        }
    }
    red[0][tid] = s0; red[1][tid] = s1; red[2][tid] = s2; red[3][tid] = s3;
    __syncthreads();
    for (int w = 128; w >= 1; w >>= 1) {
        if (tid < w) {
#pragma unroll
            for (int k = 0; k < 4; ++k) red[k][tid] += red[k][tid + w];
        }
        __syncthreads();
    }
    if (tid == 0) *(double4*)(table + 4 * b) = double4{red[0][0], red[1][0], red[2][0], red[3][0]};
}
SLNLP_ZKERNEL(reliability_table_kernel, 256, reliability_table_body)

int reliability_rows(const float* logp, int64_t ld, const int64_t* y, int64_t N, int64_t V, int bins, const double* beta_dev, double* rows,
                     double* table, hipStream_t st) {
    SLNLP_CHECK_ARG(logp && y && rows && table, "reliability_rows: null pointer");
    Span z;
    SLNLP_TRY(check_logp_matrix("reliability_rows", logp, N, INT_MAX, V, INT_MAX, ld, &z));
    SLNLP_CHECK_ARG(bins >= 1 && bins <= SLNLP_REL_MAX_BINS, "reliability_rows: bins=%d outside 1..%d", bins, SLNLP_REL_MAX_BINS);
    SLNLP_CHECK_ARG(((uintptr_t)logp & 3) == 0 && (((uintptr_t)y | (uintptr_t)beta_dev) & 7) == 0, "reliability_rows: misaligned pointer");
    SLNLP_CHECK_ARG((((uintptr_t)rows | (uintptr_t)table) & 31) == 0, "reliability_rows: rows or table is not 32-byte aligned");
    const size_t n = (size_t)N;
    const Span in[3] = {z, {y, n * 8, "y"}, {beta_dev, 8, "beta"}};
    const Span out[2] = {{rows, n * 32, "rows"}, {table, ((size_t)bins + 1) * 32, "table"}};
    SLNLP_TRY(check_no_overlap("reliability_rows", out, in));
    const int blocks = wave_rows_grid(N);
    SLNLP_TRY(zlaunch(reliability_rows_kernel, dim3(blocks), 256, 0, st, "reliability_rows", logp, (long)ld, y, (int)N, (int)V, bins, beta_dev,
                      rows));
    return zlaunch(reliability_table_kernel, dim3(bins + 1), 256, 0, st, "reliability_table", (const double*)rows, (int)N, bins, table);
}

}  // namespace slnlp

extern "C" int slnlp_reliability_rows(const float* logp, int64_t ld, const int64_t* y, int64_t N, int64_t V, int bins,
                                      const double* beta_dev, double* rows, double* table, void* stream) {
    return slnlp::reliability_rows(logp, ld, y, N, V, bins, beta_dev, rows, table, (hipStream_t)stream);
}
