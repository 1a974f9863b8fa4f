// selective.hip -- selective prediction on a set of log-probs on the device: per row a confidence kappa and whether the arg-max is
// wrong, per included row the exact number of rows (and of wrong rows) at least as confident, and from those the risk-coverage
// curve's area (AURC), coverage at a given risk and risk at a given coverage (NeuralNetClassifier.risk_coverage /
// fit_rejection / predict_selective).  include/slnlp.h states the definitions; tests/selective_ref.py restates them in numpy.
//
// selective_rows: z float32 log-probs [N, ld] (V columns used), beta = beta_dev ? beta_dev[0] : 1.  One wave per row, one row per
// 64-thread block (rows over a grid-stride loop), on the row head of logp_row.hpp: pred is logp_row_argmax's, s0, rest and n_max are
// logp_row_sums', so kappa = 1 / s0 (max_prob) is topk_rows' prob[i, 0] and reliability_rows' conf bit for bit.  The margin takes the
// largest e beside the maximum from the same pass (each()); the negative entropy makes one more pass over the row for sum e_c t_c.
// No LDS, no atomics.
//
// selective_counts: kappa float64 [N] and rows int32 [N, 4] as selective_rows wrote them (or as a caller made them: ties are ties of
// the fp64 values).  A row is INCLUDED when its code is 0 and its kappa is no NaN.  Three launches on the stream:
//   init    one block: the level cells of the table take the neutral element of their reduction (0 for a maximum, ~0 for a minimum);
//   chunks  ceil(N / SEL_CHUNK) blocks of 256 threads, ranking_rows' scheme with a block per chunk of included rows -- written out
//           here and NOT on rank_chunk.hpp's helpers: on them every output bit was the same, but selective_counts at N = 4000
//           measured 0.4 % above this body's spread in each of three runs, so this body stays.  Block b
//     1. scans rows in tiles of 256 and compacts the included rows with ordinal in [b C, (b + 1) C) -- row index and an order-
//        preserving uint64 key of kappa -- into LDS in ascending row order: a ballot per wave and a prefix over the four wave totals
//        give every included row its ordinal, so a chunk's membership does not depend on timing; the scan also yields n;
//     2. sorts the chunk by key with one bitonic network in LDS (equal keys give equal counts: their order is immaterial);
//     3. streams all N rows: per included row one binary search in the sorted keys (ub: the first position whose key is larger)
//        and integer LDS atomics on two histograms (all rows, wrong rows) at ub.  Integer adds commute;
//     4. strict suffix sums turn them into (ge, ge_wrong) of the row at sorted position p; they go to counts by original row index;
//     5. forms the chunk's sum of ge_wrong / ge: a thread adds its 8 positions in ascending order, a fixed binary tree adds the 256
//        threads; the sum goes to the chunk's own slot of the table;
//     6. reduces the levels: a thread keeps the best (ge << 32 | ge_wrong) of its positions per level and hands it to the level's
//        cell with ONE 64-bit integer atomic max (coverage at risk) or min (risk at coverage); both commute;
//   final   one block: counts n, E and the excluded rows again, adds the chunk sums in ascending chunk order, writes the table's
//           head and turns the level cells into doubles in place.
// No host wait, no float atomics, no "last block done" counter: the result is a function of the arguments alone.  Every block
// scans all N rows twice, so the work is O(N^2 / C log C): right for an epoch's few thousand rows, correct beyond.
#include <limits.h>
#include <math.h>

#include <algorithm>

#include "block_reduce.hpp"
#include "common.hpp"
#include "launch.hpp"
#include "logp_row.hpp"
#include "spans.hpp"

namespace slnlp {

constexpr int SEL_CHUNK = SLNLP_SEL_CHUNK;               // included rows per LDS chunk: a power of two, 8 per thread
constexpr int SEL_PER_THREAD = SEL_CHUNK / 256;
static_assert(SEL_PER_THREAD * 256 == SEL_CHUNK && (SEL_CHUNK & (SEL_CHUNK - 1)) == 0, "SLNLP_SEL_CHUNK: a power of two, a multiple of 256");
constexpr int SEL_LEVELS = SLNLP_SEL_MAX_LEVELS;
constexpr int SEL_HEAD = 8;                              // table: 8 head doubles, then 2 per risk level, 2 per coverage level, then the chunk sums
constexpr int SEL_AT_RISK = SEL_HEAD, SEL_AT_COV = SEL_HEAD + 2 * SEL_LEVELS, SEL_AT_CHUNKS = SEL_HEAD + 4 * SEL_LEVELS;
static_assert(SEL_AT_CHUNKS == SLNLP_SEL_TABLE_HEAD, "SLNLP_SEL_TABLE_HEAD: 8 + 4 levels");
constexpr int SEL_MAX_BLOCKS = 16384;                    // selective_rows: x 1 row; more rows wrap the stride loop
constexpr unsigned long long SEL_KEY_PAD = ~0ull;        // the sort's padding: behind every real key (+inf is 0xFFF0000000000000)

struct SelLevels {
    double risk[SEL_LEVELS], coverage[SEL_LEVELS];
    int nr, nc;
};

// ------------------------------------------------------------------------------------------------------------ rows ----
__device__ __forceinline__ void selective_rows_body(const float* __restrict__ logp, long ld, const int64_t* __restrict__ y, int N, int V,
                                                    int score, const double* __restrict__ beta_dev, const double* __restrict__ tau_dev,
                                                    double* __restrict__ kappa, int* __restrict__ rows) {
    const double beta = beta_dev ? beta_dev[0] : 1.0;
    const bool have_tau = tau_dev != nullptr;
    const double tau = have_tau ? tau_dev[0] : 0.0;
    const int lane = threadIdx.x;                        // 64 threads: one wave
    const double qnan = __builtin_bit_cast(double, 0x7ff8000000000000ull);
    for (long r = blockIdx.x; r < N; r += gridDim.x) {   // r: the same in every lane, so every lane reaches the reductions
        const float* row = logp + r * ld;
        int64_t label = -1;
        if (y) label = y[r];
        const bool label_ok = !y || (label >= 0 && label < V);   // a label outside the columns is never used as an index
        const LogpRowMax top = logp_row_argmax(row, V, lane);
        const float zmax = top.zmax;
        if (!top.finite) {                               // wave-uniform: the row has no softmax
            if (lane == 0) {
                kappa[r] = qnan;
                *(int4*)(rows + 4 * r) = int4{top.pred, 0, 0, -2};
            }
            continue;
        }
        double e2 = 0.0;                                 // the largest e over the columns not at the maximum (none: 0)
        const LogpRowSums h = logp_row_sums(row, V, lane, beta, zmax, [&](double e) { e2 = fmax(e2, e); });
        const double s0 = h.s0;
        double k;
        if (score == SLNLP_SEL_MAX_PROB) {
            k = 1.0 / s0;
        } else if (score == SLNLP_SEL_MARGIN) {
            e2 = wave_max_d(e2);                         // (e >= 0: no NaN)
            k = h.n_max >= 2.0 ? 0.0 : (1.0 - e2) / s0;
        } else {                                         // sum p ln p = (sum e_c t_c) / s0 - log1p(rest); t = 0 at the maximum
            double et = 0.0;
            for (int j = lane; j < V; j += 64) {
                const float zf = row[j];
                if (zf == zmax) continue;
                const double t = beta * (double)zf - h.a;
                const double e = exp(t);
                if (e != 0.0) et += e * t;               // e == 0 (t = -inf included) counts as 0
            }
            k = wave_sum_d(et) / s0 - log1p(h.rest);
        }
        if (lane == 0) {
            kappa[r] = k;
            const int wrong = (y && label_ok && (int64_t)top.pred != label) ? 1 : 0;
            *(int4*)(rows + 4 * r) = int4{top.pred, wrong, (have_tau && k >= tau) ? 1 : 0, label_ok ? 0 : -1};
        }
    }
}
SLNLP_ZKERNEL(selective_rows_kernel, 64, selective_rows_body)

// ---------------------------------------------------------------------------------------------------------- counts ----
// double -> uint64 with the doubles' order; ties are ties of the fp64 values, so -0.0 takes +0.0's key.  No NaN comes here.
__device__ __forceinline__ unsigned long long sel_key(double k) {
    if (k == 0.0) k = 0.0;
    return order_key_d(k);
}
__device__ __forceinline__ bool sel_included(int code, double k) { return code == 0 && k == k; }

__device__ __forceinline__ void selective_init_body(unsigned long long* __restrict__ cells) {
    const int t = threadIdx.x;                           // 64 threads
    if (t < 2 * SEL_LEVELS) {
        cells[SEL_AT_RISK + t] = 0ull;                                           // a maximum over keys > 0 (ge >= 1)
        cells[SEL_AT_COV + t] = (t & 1) ? 0ull : ~0ull;                          // a minimum; the odd slots are the final launch's
    }
}
SLNLP_ZKERNEL(selective_init_kernel, 64, selective_init_body)

__device__ __forceinline__ void selective_chunks_body(const double* __restrict__ kappa, const int* __restrict__ rows, int N, SelLevels lv,
                                                      int* __restrict__ counts, double* __restrict__ table) {
    __shared__ unsigned long long keys[SEL_CHUNK];
    __shared__ int idx[SEL_CHUNK];
    __shared__ int hist[2][SEL_CHUNK + 1];               // all rows / wrong rows, at ub
    __shared__ int part[2][256];
    __shared__ double red[256];
    __shared__ int wtot[4];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int b = blockIdx.x;
    const long first = (long)b * SEL_CHUNK;              // the ordinal of the chunk's first included row
    // 1. the included rows of this chunk, in ascending row order
    long base = 0;
    for (long r0 = 0; r0 < N; r0 += 256) {               // every thread makes every round: ballots and barriers inside
        const long r = r0 + tid;
        double k = 0.0;
        bool in = false;
        if (r < N) {
            k = kappa[r];
            in = sel_included(rows[4 * r + 3], k);
        }
        const unsigned long long bm = __ballot(in);
        if (lane == 0) wtot[wave] = __popcll(bm);
        __syncthreads();
        int before = 0, all = 0;
#pragma unroll
        for (int w = 0; w < 4; ++w) {
            const int t = wtot[w];
            if (w < wave) before += t;
            all += t;
        }
        const long ord = base + before + __popcll(bm & ((1ull << lane) - 1ull));
        if (in && ord >= first && ord - first < SEL_CHUNK) {
            keys[ord - first] = sel_key(k);
            idx[ord - first] = (int)r;
        }
        if (b == 0 && r < N && !in) *(int2*)(counts + 2 * r) = int2{0, 0};
        base += all;
        __syncthreads();                                 // wtot is rewritten by the next round
    }
    const long n_all = base;                             // the included rows
    if (first >= n_all) {                                // block-uniform: no chunk here (n = 0: block 0 too)
        if (tid == 0) table[SEL_AT_CHUNKS + b] = 0.0;
        return;
    }
    const int n = (int)min(n_all - first, (long)SEL_CHUNK);
    int m = 1;
    while (m < n) m <<= 1;                               // <= SEL_CHUNK
    for (int i = n + tid; i < m; i += 256) { keys[i] = SEL_KEY_PAD; idx[i] = -1; }
    for (int i = tid; i <= SEL_CHUNK; i += 256) { hist[0][i] = 0; hist[1][i] = 0; }
    __syncthreads();
    // 2. bitonic sort of keys[0, m) (idx follows)
    for (int k = 2; k <= m; k <<= 1) {
        for (int j = k >> 1; j >= 1; j >>= 1) {
            for (int i = tid; i < m; i += 256) {
                const int l = i ^ j;
                if (l > i) {
                    const unsigned long long a = keys[i], c = keys[l];
                    if ((a > c) == ((i & k) == 0)) {
                        keys[i] = c; keys[l] = a;
                        const int t = idx[i]; idx[i] = idx[l]; idx[l] = t;
                    }
                }
            }
            __syncthreads();
        }
    }
    // 3. every included row against the sorted keys
    for (long r = tid; r < N; r += 256) {
        const int4 t = *(const int4*)(rows + 4 * r);     // (pred, wrong, accepted, code)
        const double k = kappa[r];
        if (!sel_included(t.w, k)) continue;
        const unsigned long long key = sel_key(k);
        int ub = 0, hi = n;
        while (ub < hi) {                                // the first position whose key is > key: in 0..n
            const int mid = (ub + hi) >> 1;
            if (keys[mid] <= key) ub = mid + 1; else hi = mid;
        }
        atomicAdd(&hist[0][ub], 1);
        if (t.y != 0) atomicAdd(&hist[1][ub], 1);
    }
    __syncthreads();
    // 4. strict suffix sums: S[p] = sum of hist over the positions p + 1 .. SEL_CHUNK
    const int p0 = tid * SEL_PER_THREAD;
    int tot[2];
#pragma unroll
    for (int h = 0; h < 2; ++h) {
        int s = tid == 255 ? hist[h][SEL_CHUNK] : 0;
#pragma unroll
        for (int q = 0; q < SEL_PER_THREAD; ++q) s += hist[h][p0 + q];
        tot[h] = s;
        part[h][tid] = s;
    }
    __syncthreads();
    for (int d = 1; d < 256; d <<= 1) {                  // inclusive suffix scan over the threads' totals
        int add[2];
#pragma unroll
        for (int h = 0; h < 2; ++h) add[h] = tid + d < 256 ? part[h][tid + d] : 0;
        __syncthreads();
#pragma unroll
        for (int h = 0; h < 2; ++h) part[h][tid] += add[h];
        __syncthreads();
    }
    int run[2];
#pragma unroll
    for (int h = 0; h < 2; ++h) run[h] = part[h][tid] - tot[h] + (tid == 255 ? hist[h][SEL_CHUNK] : 0);
    // the thread's positions from the last to the first; the terms are kept to be added in ascending order
    double term[SEL_PER_THREAD];
    unsigned long long best_r[SEL_LEVELS], best_c[SEL_LEVELS];
    double need[SEL_LEVELS];                             // ceil(c n): the least number of accepted rows of a coverage level
#pragma unroll
    for (int l = 0; l < SEL_LEVELS; ++l) {
        best_r[l] = 0ull;
        best_c[l] = ~0ull;
        need[l] = ceil(lv.coverage[l] * (double)n_all);
    }
#pragma unroll
    for (int q = SEL_PER_THREAD - 1; q >= 0; --q) {
        const int p = p0 + q;
        term[q] = 0.0;
        if (p < n) {
            const int ge = run[0], gw = run[1];          // ge >= 1: the row itself
            term[q] = (double)gw / (double)ge;
            *(int2*)(counts + 2 * (long)idx[p]) = int2{ge, gw};
            const unsigned long long cell = ((unsigned long long)(unsigned)ge << 32) | (unsigned)gw;
#pragma unroll
            for (int l = 0; l < SEL_LEVELS; ++l) {
                if (l < lv.nr && (double)gw <= lv.risk[l] * (double)ge) best_r[l] = max(best_r[l], cell);
                if (l < lv.nc && (double)ge >= need[l]) best_c[l] = min(best_c[l], cell);
            }
        }
#pragma unroll
        for (int h = 0; h < 2; ++h) run[h] += hist[h][p];
    }
    // 5. the chunk's sum
    double s = 0.0;
#pragma unroll
    for (int q = 0; q < SEL_PER_THREAD; ++q) s += term[q];
    red[tid] = s;
    __syncthreads();
    for (int w = 128; w >= 1; w >>= 1) {
        if (tid < w) red[tid] += red[tid + w];
        __syncthreads();
    }
    if (tid == 0) table[SEL_AT_CHUNKS + b] = red[0];
    // 6. the levels: integer maxima and minima commute
    unsigned long long* cells = (unsigned long long*)table;
#pragma unroll
    for (int l = 0; l < SEL_LEVELS; ++l) {
        if (best_r[l] != 0ull) atomicMax(&cells[SEL_AT_RISK + 2 * l], best_r[l]);
        if (best_c[l] != ~0ull) atomicMin(&cells[SEL_AT_COV + 2 * l], best_c[l]);
    }
}
SLNLP_ZKERNEL(selective_chunks_kernel, 256, selective_chunks_body)

__device__ __forceinline__ void selective_final_body(const double* __restrict__ kappa, const int* __restrict__ rows, int N,
                                                     double* __restrict__ table) {
    __shared__ int part[4][256];
    const int tid = threadIdx.x;
    int c[4] = {0, 0, 0, 0};                             // included, wrong among them, code -1, everything else
    for (long r = tid; r < N; r += 256) {
        const int4 t = *(const int4*)(rows + 4 * r);
        if (sel_included(t.w, kappa[r])) { ++c[0]; c[1] += t.y != 0 ? 1 : 0; }
        else if (t.w == -1) ++c[2];
        else ++c[3];
    }
#pragma unroll
    for (int h = 0; h < 4; ++h) part[h][tid] = c[h];
    block_tree<4>(part, tid, TreeSum{});
    const int n = part[0][0];
    if (tid == 0) {
        const int chunks = (n + SEL_CHUNK - 1) / SEL_CHUNK;
        double sum = 0.0;
        for (int b = 0; b < chunks; ++b) sum += table[SEL_AT_CHUNKS + b];        // ascending chunk order
        *(double4*)table = double4{(double)n, (double)part[1][0], (double)part[2][0], (double)part[3][0]};
        *(double4*)(table + 4) = double4{sum, sum / (double)n, 0.0, 0.0};        // n = 0: AURC is a NaN
    }
    if (tid < 2 * SEL_LEVELS) {                          // thread t owns cell t: (ge << 32 | ge_wrong) -> two doubles in its own two slots
        const int at = SEL_AT_RISK + 2 * tid;            // the coverage cells follow the risk cells
        unsigned long long cell = ((const unsigned long long*)table)[at];
        if (cell == ~0ull) cell = 0ull;                  // a minimum over nothing (n = 0)
        *(double2*)(table + at) = double2{(double)(unsigned)(cell >> 32), (double)(unsigned)cell};
    }
}
SLNLP_ZKERNEL(selective_final_kernel, 256, selective_final_body)

// ------------------------------------------------------------------------------------------------------- host side ----
int selective_rows(const float* logp, int64_t ld, const int64_t* y, int64_t N, int64_t V, int score, const double* beta_dev,
                   const double* tau_dev, double* kappa, int32_t* rows, hipStream_t st) {
    SLNLP_CHECK_ARG(logp && kappa && rows, "selective_rows: null pointer");
    Span z;
    SLNLP_TRY(check_logp_matrix("selective_rows", logp, N, SLNLP_SEL_MAX_ROWS, V, INT_MAX - 1, ld, &z));
    SLNLP_CHECK_ARG(score == SLNLP_SEL_MAX_PROB || score == SLNLP_SEL_MARGIN || score == SLNLP_SEL_NEG_ENTROPY,
                    "selective_rows: score=%d, expected %d (max_prob), %d (margin) or %d (neg_entropy)", score, SLNLP_SEL_MAX_PROB,
                    SLNLP_SEL_MARGIN, SLNLP_SEL_NEG_ENTROPY);
    SLNLP_CHECK_ARG(((uintptr_t)logp & 3) == 0 && (((uintptr_t)y | (uintptr_t)beta_dev | (uintptr_t)tau_dev | (uintptr_t)kappa) & 7) == 0,
                    "selective_rows: misaligned pointer");
    SLNLP_CHECK_ARG(((uintptr_t)rows & 15) == 0, "selective_rows: rows is not 16-byte aligned");
    const size_t n = (size_t)N;
    const Span in[4] = {z, {y, n * 8, "y"}, {beta_dev, 8, "beta"}, {tau_dev, 8, "tau"}};
    const Span out[2] = {{kappa, n * 8, "kappa"}, {rows, n * 16, "rows"}};
    SLNLP_TRY(check_no_overlap("selective_rows", out, in));
    const int blocks = (int)std::min<int64_t>(N, SEL_MAX_BLOCKS);
    return zlaunch(selective_rows_kernel, dim3(blocks), 64, 0, st, "selective_rows", logp, (long)ld, y, (int)N, (int)V, score, beta_dev, tau_dev,
                   kappa, (int*)rows);
}

int selective_counts(const double* kappa, const int32_t* rows, int64_t N, const double* risks, int nr, const double* coverages, int nc,
                     int32_t* counts, double* table, hipStream_t st) {
    SLNLP_CHECK_ARG(kappa && rows && counts && table, "selective_counts: null pointer");
    SLNLP_CHECK_ARG(N >= 1 && N <= SLNLP_SEL_MAX_ROWS, "selective_counts: N=%ld outside 1..%d", (long)N, SLNLP_SEL_MAX_ROWS);
    SLNLP_CHECK_ARG(nr >= 0 && nr <= SEL_LEVELS, "selective_counts: nr=%d outside 0..%d", nr, SEL_LEVELS);
    SLNLP_CHECK_ARG(nc >= 0 && nc <= SEL_LEVELS, "selective_counts: nc=%d outside 0..%d", nc, SEL_LEVELS);
    SLNLP_CHECK_ARG((nr == 0 || risks) && (nc == 0 || coverages), "selective_counts: null pointer");
    SelLevels lv{};
    lv.nr = nr;
    lv.nc = nc;
    for (int l = 0; l < nr; ++l) {                       // host memory: checked and copied before anything is launched
        SLNLP_CHECK_ARG(risks[l] >= 0.0 && risks[l] <= 1.0, "selective_counts: risks[%d]=%g outside [0, 1]", l, risks[l]);
        lv.risk[l] = risks[l];
    }
    for (int l = 0; l < nc; ++l) {
        SLNLP_CHECK_ARG(coverages[l] >= 0.0 && coverages[l] <= 1.0, "selective_counts: coverages[%d]=%g outside [0, 1]", l, coverages[l]);
        lv.coverage[l] = coverages[l];
    }
    SLNLP_CHECK_ARG(((uintptr_t)kappa & 7) == 0 && ((uintptr_t)counts & 7) == 0, "selective_counts: misaligned pointer");
    SLNLP_CHECK_ARG(((uintptr_t)rows & 15) == 0, "selective_counts: rows is not 16-byte aligned");
    SLNLP_CHECK_ARG(((uintptr_t)table & 31) == 0, "selective_counts: table is not 32-byte aligned");
    const size_t n = (size_t)N;
    const int chunks = (int)((N + SEL_CHUNK - 1) / SEL_CHUNK);
    const Span in[2] = {{kappa, n * 8, "kappa"}, {rows, n * 16, "rows"}};
    const Span out[2] = {{counts, n * 8, "counts"}, {table, ((size_t)SEL_AT_CHUNKS + (size_t)chunks) * 8, "table"}};
    SLNLP_TRY(check_no_overlap("selective_counts", out, in));
    SLNLP_TRY(zlaunch(selective_init_kernel, dim3(1), 64, 0, st, "selective_init", (unsigned long long*)table));
    SLNLP_TRY(zlaunch(selective_chunks_kernel, dim3(chunks), 256, 0, st, "selective_chunks", kappa, (const int*)rows, (int)N, lv, (int*)counts,
                      table));
    return zlaunch(selective_final_kernel, dim3(1), 256, 0, st, "selective_final", kappa, (const int*)rows, (int)N, table);
}

}  // namespace slnlp

extern "C" int slnlp_selective_rows(const float* logp, int64_t ld, const int64_t* y, int64_t N, int64_t V, int score, const double* beta_dev,
                                    const double* tau_dev, double* kappa, int32_t* rows, void* stream) {
    return slnlp::selective_rows(logp, ld, y, N, V, score, beta_dev, tau_dev, kappa, rows, (hipStream_t)stream);
}
extern "C" int slnlp_selective_counts(const double* kappa, const int32_t* rows, int64_t N, const double* risks, int nr, const double* coverages,
                                      int nc, int32_t* counts, double* table, void* stream) {
    return slnlp::selective_counts(kappa, rows, N, risks, nr, coverages, nc, counts, table, (hipStream_t)stream);
}
