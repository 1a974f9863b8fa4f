// confusion.hip -- error analysis of a set of log-probs on the device: the top-k classes of every row with their probabilities, the
// confusion matrix of (label, arg-max) and its most-confused pairs (NeuralNetClassifier.predict_topk /
// error_analysis).  include/slnlp.h states the three definitions; tests/confusion_ref.py restates them in numpy.
//
// topk_rows: z float32 log-probs [N, ld] (V columns used), beta = beta_dev ? beta_dev[0] : 1.  Per row the first k columns in
// score_beats' total order on the float32 values (common.hpp: a NaN first, then larger values, equal values by ascending index) and
// prob = exp(beta z_c - a) / s0 with a and s0 from the row head of logp_row.hpp, which reliability_rows shares: prob[i, 0] = 1 / s0
// is that kernel's conf bit for bit.  Then k - 1 rounds: a wave arg-max over the elements that come strictly AFTER the previous winner
// in the order; nothing is stored in between (a row stays in L2), lane m keeps winner m and the k results leave in one store.
// One wave per row, four rows per block, rows over a grid-stride loop, lanes stride the columns; no LDS.
//
// confusion_matrix: counts[y_i V + pred_i] += 1 over the rows whose label and prediction both lie in [0, V); any other row is counted
// in counts[V V] and never used as an index.  One thread per row; integer atomics: the sums do not depend on the order of arrival.
//
// confusion_pairs: the M largest off-diagonal cells with a count above 0, by (count descending, flat index ascending).  A cell is ONE
// 64-bit key, count << 32 | ~flat: the order is "larger key first" and a key of 0 means "no cell".  Stage 1: the V V cells are cut
// into contiguous slices, one block each; a block extracts its slice's first M keys by M rounds of a block-wide maximum over the keys
// BELOW the previous winner (a round that finds none ends the block: the rest of its list is 0).  Stage 2: one block does the same
// over the slices' lists and writes the pairs.  The order is total, so the result is the same however the cells are sliced.
#include <limits.h>
#include <math.h>

#include <algorithm>

#include "common.hpp"
#include "launch.hpp"
#include "logp_row.hpp"
#include "spans.hpp"

namespace slnlp {

constexpr int CONF_MAX_BLOCKS = 2048;      // x 256 entries (zero / count): larger inputs wrap the stride loops
constexpr int PAIRS_SLICE_CELLS = 4096;    // a stage-1 block takes at least this many cells (16 per thread) ...
constexpr int PAIRS_MAX_SLICES = 1024;     // ... and there are at most this many blocks: 16384 cells each at V = 4096

// ------------------------------------------------------------------------------------------------------ top-k rows ----
__device__ __forceinline__ void topk_rows_body(const float* __restrict__ logp, long ld, int N, int V, int k, const double* __restrict__ beta_dev,
                                               int* __restrict__ idx, double* __restrict__ prob) {
    const double beta = beta_dev ? beta_dev[0] : 1.0;
    // (wave_rows' loop, written out: through the helper this kernel's register counts change -- profiles/judging_shell_isa.txt)
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane((int)(blockIdx.x * 4 + (threadIdx.x >> 6)));
    const int nwaves = gridDim.x * 4;
    const double qnan = __builtin_bit_cast(double, 0x7ff8000000000000ull);
    for (long r = wave; r < N; r += nwaves) {            // r: the same in every lane, so every lane reaches the reductions
        const float* row = logp + r * ld;
        const LogpRowMax top = logp_row_argmax(row, V, lane);
        const float zmax = top.zmax;
        const LogpRowSums h = logp_row_sums(row, V, lane, beta, zmax);
        const double a = h.a, s0 = h.s0;
        float pv = zmax, mine_v = zmax;                  // (pv, pi): the previous winner; lane m keeps winner m (k <= 64)
        int pi = top.pred, mine_i = top.pred;
        for (int m = 1; m < k; ++m) {                    // k <= V: every round has an element left
            float bv = -INFINITY;
            int bi = INT_MAX;
            for (int j = lane; j < V; j += 64) {
                const float x = row[j];
                if (score_beats(pv, pi, x, j) && score_beats(x, j, bv, bi)) { bv = x; bi = j; }
            }
            wave_best(bv, bi);
            if (lane == m) { mine_v = bv; mine_i = bi; }
            pv = bv; pi = bi;
        }
        if (lane < k) {
            idx[r * k + lane] = mine_i;
            double p = qnan;                             // a row that holds a NaN or whose maximum is not finite
            if (top.finite) p = mine_v == zmax ? 1.0 / s0 : exp(beta * (double)mine_v - a) / s0;
            prob[r * k + lane] = p;
        }
    }
}
SLNLP_ZKERNEL(topk_rows_kernel, 256, topk_rows_body)

// ------------------------------------------------------------------------------------------------ confusion matrix ----
__device__ __forceinline__ void confusion_zero_body(int* __restrict__ counts, long n) {
    for (long i = blockIdx.x * 256L + threadIdx.x; i < n; i += gridDim.x * 256L) counts[i] = 0;
}
SLNLP_ZKERNEL(confusion_zero_kernel, 256, confusion_zero_body)

__device__ __forceinline__ void confusion_count_body(const int* __restrict__ pred, const int64_t* __restrict__ y, int N, int V,
                                                     int* __restrict__ counts) {
    for (long i = blockIdx.x * 256L + threadIdx.x; i < N; i += gridDim.x * 256L) {
        const int64_t label = y[i];
        const int p = pred[i];
        const bool ok = label >= 0 && label < V && p >= 0 && p < V;     // a value outside the classes is never used as an index
        atomicAdd(&counts[ok ? (long)label * V + p : (long)V * V], 1);
    }
}
SLNLP_ZKERNEL(confusion_count_kernel, 256, confusion_count_body)

// ------------------------------------------------------------------------------------------------ most-confused pairs ----
typedef unsigned long long pair_key;                     // count << 32 | ~flat index; 0: no cell

template <int CTRL>
__device__ __forceinline__ pair_key dpp_max_key(pair_key v) {
    const unsigned lo = (unsigned)__builtin_amdgcn_update_dpp(0, (int)(unsigned)v, CTRL, 0xF, 0xF, true);
    const unsigned hi = (unsigned)__builtin_amdgcn_update_dpp(0, (int)(unsigned)(v >> 32), CTRL, 0xF, 0xF, true);
    const pair_key o = ((pair_key)hi << 32) | lo;
    return o > v ? o : v;
}
__device__ __forceinline__ pair_key lane_key(pair_key v, int lane) {
    const unsigned lo = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)v, lane);
    const unsigned hi = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)(v >> 32), lane);
    return ((pair_key)hi << 32) | lo;
}
// the largest key of the block's 256 threads, in every thread (all of them call it): DPP / readlane inside a wave, four LDS words across
__device__ __forceinline__ pair_key block_max_key(pair_key v, pair_key* across) {
    v = dpp_max_key<DPP_XOR1>(v);
    v = dpp_max_key<DPP_XOR2>(v);
    v = dpp_max_key<DPP_HALF_MIRROR>(v);
    v = dpp_max_key<DPP_MIRROR>(v);
    const pair_key a = lane_key(v, 0), b = lane_key(v, 16), c = lane_key(v, 32), d = lane_key(v, 48);
    v = std::max(std::max(a, b), std::max(c, d));
    __syncthreads();                                     // the previous round's reads of `across` are over
    if ((threadIdx.x & 63) == 0) across[threadIdx.x >> 6] = v;
    __syncthreads();
    return std::max(std::max(across[0], across[1]), std::max(across[2], across[3]));
}

// the key of cell `flat` of a V x V matrix: 0 on the diagonal and for a count that is not positive
__device__ __forceinline__ pair_key cell_key(int count, long flat, int V) {
    if (count <= 0 || flat / V == flat % V) return 0;
    return ((pair_key)(unsigned)count << 32) | (0xFFFFFFFFu - (unsigned)flat);
}

// stage 1: block b's slice of the cells -> lists[b M .. b M + M), its first M keys in descending order, then zeros
__device__ __forceinline__ void pairs_slice_body(const int* __restrict__ counts, int V, int M, long slice, pair_key* __restrict__ lists) {
    __shared__ pair_key across[4];
    const long cells = (long)V * V;
    const long begin = blockIdx.x * slice, end = std::min(begin + slice, cells);
    pair_key* out = lists + (long)blockIdx.x * M;
    pair_key below = ~0ull;                              // the previous winner: every key is below this start
    int m = 0;
    for (; m < M; ++m) {
        pair_key best = 0;
        for (long f = begin + threadIdx.x; f < end; f += 256) {
            const int c = counts[f];
            if (c > 0 && (unsigned)c >= (unsigned)(best >> 32)) {        // (the division only for a cell that could win)
                const pair_key key = cell_key(c, f, V);
                if (key < below && key > best) best = key;
            }
        }
        best = block_max_key(best, across);
        if (best == 0) break;                            // block-uniform: the slice holds no further cell
        if (threadIdx.x == 0) out[m] = best;
        below = best;
    }
    for (int q = m + threadIdx.x; q < M; q += 256) out[q] = 0;
}
SLNLP_ZKERNEL(pairs_slice_kernel, 256, pairs_slice_body)

// stage 2: the first M keys of the n listed ones -> pairs [M, 3] = (true, predicted, count), then (-1, -1, 0)
__device__ __forceinline__ void pairs_merge_body(const pair_key* __restrict__ lists, int n, int V, int M, int* __restrict__ pairs) {
    __shared__ pair_key across[4];
    pair_key below = ~0ull;
    int m = 0;
    for (; m < M; ++m) {
        pair_key best = 0;
        for (int i = threadIdx.x; i < n; i += 256) {
            const pair_key key = lists[i];
            if (key < below && key > best) best = key;
        }
        best = block_max_key(best, across);
        if (best == 0) break;
        if (threadIdx.x == 0) {
            const unsigned flat = 0xFFFFFFFFu - (unsigned)best;
            pairs[3 * m] = (int)(flat / (unsigned)V);
            pairs[3 * m + 1] = (int)(flat % (unsigned)V);
            pairs[3 * m + 2] = (int)(best >> 32);
        }
        below = best;
    }
    for (int q = m + threadIdx.x; q < M; q += 256) {
        pairs[3 * q] = -1;
        pairs[3 * q + 1] = -1;
        pairs[3 * q + 2] = 0;
    }
}
SLNLP_ZKERNEL(pairs_merge_kernel, 256, pairs_merge_body)

// ------------------------------------------------------------------------------------------------------ host side ----
int topk_rows(const float* logp, int64_t ld, int64_t N, int64_t V, int k, const double* beta_dev, int32_t* idx, double* prob, hipStream_t st) {
    SLNLP_CHECK_ARG(logp && idx && prob, "topk_rows: null pointer");
    Span z;
    SLNLP_TRY(check_logp_matrix("topk_rows", logp, N, INT_MAX, V, INT_MAX, ld, &z));
    const int k_max = (int)std::min<int64_t>(V, SLNLP_TOPK_MAX);
    SLNLP_CHECK_ARG(k >= 1 && k <= k_max, "topk_rows: k=%d outside 1..%d", k, k_max);
    SLNLP_CHECK_ARG((((uintptr_t)logp | (uintptr_t)idx) & 3) == 0 && (((uintptr_t)prob | (uintptr_t)beta_dev) & 7) == 0,
                    "topk_rows: misaligned pointer");
    const size_t n = (size_t)N;
    const Span in[2] = {z, {beta_dev, 8, "beta"}};
    const Span out[2] = {{idx, n * k * 4, "idx"}, {prob, n * k * 8, "prob"}};
    SLNLP_TRY(check_no_overlap("topk_rows", out, in));
    return zlaunch(topk_rows_kernel, dim3(wave_rows_grid(N)), 256, 0, st, "topk_rows", logp, (long)ld, (int)N, (int)V, k, beta_dev, idx, prob);
}

int confusion_matrix(const int32_t* pred, const int64_t* y, int64_t N, int64_t V, int32_t* counts, hipStream_t st) {
    SLNLP_CHECK_ARG(pred && y && counts, "confusion_matrix: null pointer");
    SLNLP_CHECK_ARG(N >= 1 && N <= INT_MAX, "confusion_matrix: N=%ld outside 1..%d", (long)N, INT_MAX);
    SLNLP_CHECK_ARG(V >= 1 && V <= SLNLP_CONFUSION_MAX_V, "confusion_matrix: V=%ld outside 1..%d", (long)V, SLNLP_CONFUSION_MAX_V);
    SLNLP_CHECK_ARG((((uintptr_t)pred | (uintptr_t)counts) & 3) == 0 && ((uintptr_t)y & 7) == 0, "confusion_matrix: misaligned pointer");
    const size_t n = (size_t)N, n_counts = (size_t)V * (size_t)V + 1;
    const Span in[2] = {{pred, n * 4, "pred"}, {y, n * 8, "y"}}, out[1] = {{counts, n_counts * 4, "counts"}};
    SLNLP_TRY(check_no_overlap("confusion_matrix", out, in));
    const int zero_blocks = (int)std::min<size_t>((n_counts + 255) / 256, CONF_MAX_BLOCKS);
    SLNLP_TRY(zlaunch(confusion_zero_kernel, dim3(zero_blocks), 256, 0, st, "confusion_zero", counts, (long)n_counts));
    const int blocks = (int)std::min<int64_t>((N + 255) / 256, CONF_MAX_BLOCKS);
    return zlaunch(confusion_count_kernel, dim3(blocks), 256, 0, st, "confusion_count", pred, y, (int)N, (int)V, counts);
}

// the stage-1 grid of a V x V matrix: a function of V alone
static int pairs_slices(int64_t V) { return (int)std::min<int64_t>((V * V + PAIRS_SLICE_CELLS - 1) / PAIRS_SLICE_CELLS, PAIRS_MAX_SLICES); }

static int pairs_check_sizes(const char* what, int64_t V, int M) {
    SLNLP_CHECK_ARG(V >= 1 && V <= SLNLP_CONFUSION_MAX_V, "%s: V=%ld outside 1..%d", what, (long)V, SLNLP_CONFUSION_MAX_V);
    SLNLP_CHECK_ARG(M >= 1 && M <= SLNLP_PAIRS_MAX, "%s: M=%d outside 1..%d", what, M, SLNLP_PAIRS_MAX);
    return 0;
}

int64_t confusion_pairs_workspace_bytes(int64_t V, int M) {
    if (pairs_check_sizes("confusion_pairs_workspace_bytes", V, M) != 0) return -1;
    return (int64_t)pairs_slices(V) * M * (int64_t)sizeof(pair_key);
}

int confusion_pairs(const int32_t* counts, int64_t V, int M, int32_t* pairs, void* work, int64_t work_bytes, hipStream_t st) {
    SLNLP_CHECK_ARG(counts && pairs && work, "confusion_pairs: null pointer");
    SLNLP_TRY(pairs_check_sizes("confusion_pairs", V, M));
    const int64_t need = confusion_pairs_workspace_bytes(V, M);
    SLNLP_CHECK_ARG(work_bytes >= need, "confusion_pairs: work_bytes=%ld is too small, V=%ld and M=%d need %ld", (long)work_bytes, (long)V, M,
                    (long)need);
    SLNLP_CHECK_ARG((((uintptr_t)counts | (uintptr_t)pairs) & 3) == 0 && ((uintptr_t)work & 7) == 0, "confusion_pairs: misaligned pointer");
    const Span in[1] = {{counts, (size_t)V * (size_t)V * 4, "counts"}};
    const Span out[2] = {{pairs, (size_t)M * 12, "pairs"}, {work, (size_t)need, "work"}};
    SLNLP_TRY(check_no_overlap("confusion_pairs", out, in));
    const int slices = pairs_slices(V);
    const long slice = (long)((V * V + slices - 1) / slices);
    SLNLP_TRY(zlaunch(pairs_slice_kernel, dim3(slices), 256, 0, st, "confusion_pairs_slice", counts, (int)V, M, slice, (pair_key*)work));
    return zlaunch(pairs_merge_kernel, dim3(1), 256, 0, st, "confusion_pairs_merge", (const pair_key*)work, slices * M, (int)V, M, pairs);
}

}  // namespace slnlp

extern "C" int slnlp_topk_rows(const float* logp, int64_t ld, int64_t N, int64_t V, int k, const double* beta_dev, int32_t* idx, double* prob,
                               void* stream) {
    return slnlp::topk_rows(logp, ld, N, V, k, beta_dev, idx, prob, (hipStream_t)stream);
}
extern "C" int slnlp_confusion_matrix(const int32_t* pred, const int64_t* y, int64_t N, int64_t V, int32_t* counts, void* stream) {
    return slnlp::confusion_matrix(pred, y, N, V, counts, (hipStream_t)stream);
}
extern "C" int64_t slnlp_confusion_pairs_workspace_bytes(int64_t V, int M) { return slnlp::confusion_pairs_workspace_bytes(V, M); }
extern "C" int slnlp_confusion_pairs(const int32_t* counts, int64_t V, int M, int32_t* pairs, void* work, int64_t work_bytes, void* stream) {
    return slnlp::confusion_pairs(counts, V, M, pairs, work, work_bytes, (hipStream_t)stream);
}
