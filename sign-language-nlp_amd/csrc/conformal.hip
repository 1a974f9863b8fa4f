// conformal.hip -- split conformal prediction sets of a set of log-probs on the device: per-row scores (LAC / APS / RAPS), the
// threshold as an exact order statistic of the calibration scores, the sets as bit masks and their coverage / size summary
// (NeuralNetClassifier.conformalize / predict_set / coverage).  include/slnlp.h states the definitions;
// tests/conformal_ref.py restates them in numpy.
//
// conformal_rows: z float32 log-probs [N, ld] (V columns used), beta = beta_dev ? beta_dev[0] : 1, p_c = exp(beta z_c - a) / s0 with
// a and s0 from the row head of logp_row.hpp, which topk_rows shares (p of the arg-max is that kernel's prob[i, 0] bit for bit).
// One wave per row, one row per 64-thread block (rows over a grid-stride loop), so every barrier is the wave's own:
//   1. the row goes to LDS as 64-bit keys, ~rank_key(value) << 32 | column -- ascending keys are score_beats' order, equal values
//      by ascending column for free; the padding up to M, the next power of two >= max(V, 64), is ~0 and sorts last; one bitonic
//      network over M, every lane taking M / 128 compare-exchanges per step;
//   2. lane l owns the sorted positions [l R, (l + 1) R), R = M / 64: it decodes the value from the key, forms p and adds its run in
//      ascending order; the 64 lane totals go through LDS and lane l adds those of lanes 0 .. l - 1 in ascending order: before(c);
//   3. per position the score, the membership s <= qhat (one ballot per step gives the set's size) and an integer OR into the row's
//      LDS mask; the lane that meets column y_i keeps score, rank and covered and stores the row's int4 and score;
//   4. lanes 0 .. W - 1 store the W mask words.
// A row with a NaN or a maximum that is not finite leaves before the sort (code -2).  No global atomics.
//
// conformal_quantile: one block of 256 threads; the k-th smallest of the code-0 scores by radix select over order-preserving
// uint64 keys: 8 passes from the top byte down, each a 256-bin integer histogram in LDS over the scores that share the prefix
// found so far.  conformal_summary: a zero launch and one thread per row with 64-bit integer atomics, as confusion_count does.
#include <limits.h>
#include <math.h>

#include <algorithm>

#include "block_reduce.hpp"
#include "common.hpp"
#include "launch.hpp"
#include "logp_row.hpp"
#include "spans.hpp"

namespace slnlp {

constexpr int CONFORMAL_MAX_V = SLNLP_CONFORMAL_MAX_V;       // a power of two: the largest sort
constexpr int CONFORMAL_MAX_BLOCKS = 16384;                  // x 1 row (conformal_rows), x 256 entries (zero / summary): larger inputs wrap the stride loops
static_assert((CONFORMAL_MAX_V & (CONFORMAL_MAX_V - 1)) == 0 && CONFORMAL_MAX_V >= 64, "SLNLP_CONFORMAL_MAX_V: a power of two, at least a wave");

// ------------------------------------------------------------------------------------------------------------ rows ----
__device__ __forceinline__ void conformal_rows_body(const float* __restrict__ logp, long ld, const int64_t* __restrict__ y, int N, int V,
                                                    const double* __restrict__ beta_dev, int method, double lam, int k_reg, int randomized,
                                                    unsigned long long seed, unsigned draw, const double* __restrict__ qhat_dev,
                                                    double* __restrict__ score, int* __restrict__ rows, unsigned* __restrict__ sets) {
    __shared__ unsigned long long keys[CONFORMAL_MAX_V];
    __shared__ double prob[CONFORMAL_MAX_V];             // p by sorted position: written and read by the position's owner only
    __shared__ double tot[64];
    __shared__ unsigned mask[CONFORMAL_MAX_V / 32];
    const double beta = beta_dev ? beta_dev[0] : 1.0;
    const bool have_q = qhat_dev != nullptr;
    const double qhat = have_q ? qhat_dev[0] : 0.0;
    const int lane = threadIdx.x;                        // 64 threads: one wave
    const int W = (V + 31) >> 5;
    int M = 64;
    while (M < V) M <<= 1;                               // <= CONFORMAL_MAX_V
    const int R = M >> 6;
    const SeedKey K = seed_key(seed, draw);
    const double qnan = __builtin_bit_cast(double, 0x7ff8000000000000ull);
    for (long r = blockIdx.x; r < N; r += gridDim.x) {   // r: the same in every lane, so every lane reaches the reductions and barriers
        const float* row = logp + r * ld;
        int64_t label = -1;
        if (y) label = y[r];
        const bool label_ok = label >= 0 && label < V;   // a label outside the columns is never used as an index
        const LogpRowMax top = logp_row_argmax(row, V, lane);
        const float zmax = top.zmax;
        if (!top.finite) {                                   // wave-uniform: no set can be formed
            if (lane == 0) {
                if (score) score[r] = qnan;
                if (rows) *(int4*)(rows + 4 * r) = int4{0, 0, 0, -2};
            }
            if (sets && lane < W) sets[r * W + lane] = 0u;
            continue;
        }
        const LogpRowSums h = logp_row_sums(row, V, lane, beta, zmax);
        const double a = h.a, s0 = h.s0;
        // 1. the keys and their sort
        for (int j = lane; j < M; j += 64)
            keys[j] = j < V ? ((unsigned long long)(~rank_key(row[j])) << 32) | (unsigned)j : ~0ull;
        if (lane < CONFORMAL_MAX_V / 32) mask[lane] = 0u;
        __syncthreads();
        for (int k = 2; k <= M; k <<= 1) {
            for (int j = k >> 1; j >= 1; j >>= 1) {
                for (int t = lane; t < (M >> 1); t += 64) {
                    const int i = ((t & ~(j - 1)) << 1) | (t & (j - 1)), l = i | j;      // the t-th pair of this step: bit j of i clear
                    const unsigned long long ka = keys[i], kb = keys[l];
                    if ((ka > kb) == ((i & k) == 0)) { keys[i] = kb; keys[l] = ka; }
                }
                __syncthreads();
            }
        }
        // 2. p of the lane's run and the mass in front of it
        const int p0 = lane * R;
        double run = 0.0;
        for (int q = 0; q < R; ++q) {
            const int pos = p0 + q;
            double p = 0.0;                              // the padding: positions V .. M - 1
            if (pos < V) {
                const float x = rank_key_inv(~(unsigned)(keys[pos] >> 32));
                p = x == zmax ? 1.0 / s0 : exp(beta * (double)x - a) / s0;
            }
            prob[pos] = p;
            run += p;
        }
        tot[lane] = run;
        __syncthreads();
        double before = 0.0;
        for (int l = 0; l < 63; ++l) {
            const double t = tot[l];
            if (l < lane) before += t;
        }
        // 3. scores, membership, the label's own entry
        double u = 1.0;
        if (randomized) u = ((double)seed_words((unsigned)r, SLNLP_CONFORMAL_STAGE, K).x + 0.5) * 0x1p-32;
        int size = 0, my_rank = 0, my_cov = 0;
        double my_score = qnan;
        bool mine = false;
        for (int q = 0; q < R; ++q) {                    // R is wave-uniform: every lane reaches every ballot
            const int pos = p0 + q, rank = pos + 1;
            const bool real = pos < V;
            const unsigned col = (unsigned)keys[pos];
            const double p = prob[pos];
            double s;
            if (method == SLNLP_CONFORMAL_LAC) s = 1.0 - p;
            else s = before + u * p + lam * (double)max(0, rank - k_reg);
            const bool member = real && have_q && s <= qhat;
            if (member) atomicOr(&mask[col >> 5], 1u << (col & 31u));
            size += __popcll(__ballot(member));
            if (real && label_ok && (int64_t)col == label) { mine = true; my_rank = rank; my_cov = member ? 1 : 0; my_score = s; }
            before += p;
        }
        if (label_ok ? mine : lane == 0) {               // exactly one lane: a valid label is one of the row's V columns
            if (score) score[r] = my_score;
            if (rows) *(int4*)(rows + 4 * r) = int4{size, my_rank, my_cov, (y && !label_ok) ? -1 : 0};
        }
        __syncthreads();                                 // the mask is complete
        // 4. the words
        if (sets && lane < W) sets[r * W + lane] = mask[lane];
        __syncthreads();                                 // the next row rewrites keys, tot and mask
    }
}
SLNLP_ZKERNEL(conformal_rows_kernel, 64, conformal_rows_body)

// -------------------------------------------------------------------------------------------------------- quantile ----
// (the keys are order_key_d's of the scores as stored, -0.0 apart from +0.0: the answer is decoded from the winning key)
__device__ __forceinline__ void conformal_quantile_body(const double* __restrict__ score, const int* __restrict__ rows, int N, double alpha,
                                                        double* __restrict__ state) {
    __shared__ int hist[256];
    __shared__ unsigned long long found_prefix;
    __shared__ long found_k;
    const int tid = threadIdx.x;
    int mine = 0;
    for (long i = tid; i < N; i += 256) mine += rows[4 * i + 3] == 0 ? 1 : 0;
    hist[tid] = mine;
    block_tree<1>(&hist, tid, TreeSum{});
    const int n = hist[0];
    __syncthreads();                                     // hist is rewritten below
    const double kd = ceil((double)((long)n + 1) * (1.0 - alpha));
    if (kd > (double)n) {                                // block-uniform: too few rows for this alpha (n = 0 included)
        if (tid == 0) *(double4*)state = double4{INFINITY, (double)n, kd, (double)(N - n)};
        return;
    }
    unsigned long long prefix = 0;                       // the top bytes of the answer's key found so far
    long k = (long)kd;                                   // the answer is the k-th smallest among the keys that share the prefix
    for (int pass = 0; pass < 8; ++pass) {
        const int shift = 56 - 8 * pass;
        hist[tid] = 0;
        __syncthreads();
        for (long i = tid; i < N; i += 256) {
            if (rows[4 * i + 3] != 0) continue;
            const unsigned long long key = order_key_d(score[i]);
            if (pass == 0 || (key >> (shift + 8)) == prefix) atomicAdd(&hist[(int)((key >> shift) & 255ull)], 1);
        }
        __syncthreads();
        if (tid == 0) {
            long below = 0;
            int b = 0;
            for (; b < 255; ++b) {                       // the counts sum to at least k: bin 255 takes what is left
                const int h = hist[b];
                if (below + h >= k) break;
                below += h;
            }
            found_prefix = (prefix << 8) | (unsigned long long)b;
            found_k = k - below;
        }
        __syncthreads();
        prefix = found_prefix;
        k = found_k;
        __syncthreads();                                 // found_* and hist are rewritten by the next pass
    }
    if (tid == 0) *(double4*)state = double4{order_key_d_inv(prefix), (double)n, kd, (double)(N - n)};
}
SLNLP_ZKERNEL(conformal_quantile_kernel, 256, conformal_quantile_body)

// --------------------------------------------------------------------------------------------------------- summary ----
__device__ __forceinline__ void conformal_zero_body(unsigned long long* __restrict__ table, long n) {
    for (long i = blockIdx.x * 256L + threadIdx.x; i < n; i += gridDim.x * 256L) table[i] = 0ull;
}
SLNLP_ZKERNEL(conformal_zero_kernel, 256, conformal_zero_body)

__device__ __forceinline__ void conformal_count_body(const int* __restrict__ rows, const int64_t* __restrict__ y, int N, int V,
                                                     unsigned long long* __restrict__ table) {
    for (long i = blockIdx.x * 256L + threadIdx.x; i < N; i += gridDim.x * 256L) {
        const int4 t = *(const int4*)(rows + 4 * i);     // (size, rank, covered, code)
        const int64_t label = y[i];
        const bool ok = t.w == 0 && label >= 0 && label < V && t.x >= 0 && t.x <= V;     // a value outside its range is never used as an index
        if (!ok) {
            atomicAdd(&table[4 * (long)V], 1ull);
            continue;
        }
        atomicAdd(&table[4 * label], 1ull);
        if (t.z != 0) atomicAdd(&table[4 * label + 1], 1ull);
        atomicAdd(&table[4 * label + 2], (unsigned long long)t.x);
        atomicAdd(&table[4 * (long)t.x + 3], 1ull);
    }
}
SLNLP_ZKERNEL(conformal_count_kernel, 256, conformal_count_body)

// ------------------------------------------------------------------------------------------------------- host side ----
int conformal_rows(const float* logp, int64_t ld, const int64_t* y, int64_t N, int64_t V, const double* beta_dev, int method, double lam,
                   int k_reg, int randomized, uint64_t seed, uint32_t draw, const double* qhat_dev, double* score, int32_t* rows,
                   uint32_t* sets, hipStream_t st) {
    SLNLP_CHECK_ARG(logp, "conformal_rows: null pointer");
    Span z;
    SLNLP_TRY(check_logp_matrix("conformal_rows", logp, N, INT_MAX, V, SLNLP_CONFORMAL_MAX_V, ld, &z));
    SLNLP_CHECK_ARG(method == SLNLP_CONFORMAL_LAC || method == SLNLP_CONFORMAL_APS, "conformal_rows: method=%d, expected %d (LAC) or %d (APS)",
                    method, SLNLP_CONFORMAL_LAC, SLNLP_CONFORMAL_APS);
    SLNLP_CHECK_ARG(lam >= 0.0 && lam < (double)INFINITY, "conformal_rows: lam=%g, expected a finite number >= 0", lam);
    SLNLP_CHECK_ARG(k_reg >= 0, "conformal_rows: k_reg=%d is negative", k_reg);
    SLNLP_CHECK_ARG(!score || y, "conformal_rows: score needs y");
    SLNLP_CHECK_ARG(!sets || qhat_dev, "conformal_rows: sets needs qhat_dev");
    SLNLP_CHECK_ARG((((uintptr_t)logp | (uintptr_t)sets) & 3) == 0 &&
                        (((uintptr_t)y | (uintptr_t)beta_dev | (uintptr_t)qhat_dev | (uintptr_t)score) & 7) == 0,
                    "conformal_rows: misaligned pointer");
    SLNLP_CHECK_ARG(((uintptr_t)rows & 15) == 0, "conformal_rows: rows is not 16-byte aligned");
    const size_t n = (size_t)N, W = ((size_t)V + 31) / 32;
    const Span in[4] = {z, {y, n * 8, "y"}, {beta_dev, 8, "beta"}, {qhat_dev, 8, "qhat"}};
    const Span out[3] = {{score, n * 8, "score"}, {rows, n * 16, "rows"}, {sets, n * W * 4, "sets"}};
    SLNLP_TRY(check_no_overlap("conformal_rows", out, in));
    const int blocks = (int)std::min<int64_t>(N, CONFORMAL_MAX_BLOCKS);
    return zlaunch(conformal_rows_kernel, dim3(blocks), 64, 0, st, "conformal_rows", logp, (long)ld, y, (int)N, (int)V, beta_dev, method, lam,
                   k_reg, randomized ? 1 : 0, (unsigned long long)seed, (unsigned)draw, qhat_dev, score, (int*)rows, (unsigned*)sets);
}

int conformal_quantile(const double* score, const int32_t* rows, int64_t N, double alpha, double* state, hipStream_t st) {
    SLNLP_CHECK_ARG(score && rows && state, "conformal_quantile: null pointer");
    SLNLP_CHECK_ARG(N >= 1 && N <= INT_MAX, "conformal_quantile: N=%ld outside 1..%d", (long)N, INT_MAX);
    SLNLP_CHECK_ARG(alpha > 0.0 && alpha < 1.0, "conformal_quantile: alpha=%g outside (0, 1)", alpha);
    SLNLP_CHECK_ARG(((uintptr_t)score & 7) == 0, "conformal_quantile: misaligned pointer");
    SLNLP_CHECK_ARG(((uintptr_t)rows & 15) == 0, "conformal_quantile: rows is not 16-byte aligned");
    SLNLP_CHECK_ARG(((uintptr_t)state & 31) == 0, "conformal_quantile: state is not 32-byte aligned");
    const size_t n = (size_t)N;
    const Span in[2] = {{score, n * 8, "score"}, {rows, n * 16, "rows"}}, out[1] = {{state, SLNLP_CONFORMAL_STATE_BYTES, "state"}};
    SLNLP_TRY(check_no_overlap("conformal_quantile", out, in));
    return zlaunch(conformal_quantile_kernel, dim3(1), 256, 0, st, "conformal_quantile", score, (const int*)rows, (int)N, alpha, state);
}

int conformal_summary(const int32_t* rows, const int64_t* y, int64_t N, int64_t V, int64_t* table, hipStream_t st) {
    SLNLP_CHECK_ARG(rows && y && table, "conformal_summary: null pointer");
    SLNLP_CHECK_ARG(N >= 1 && N <= INT_MAX, "conformal_summary: N=%ld outside 1..%d", (long)N, INT_MAX);
    SLNLP_CHECK_ARG(V >= 1 && V <= SLNLP_CONFORMAL_MAX_V, "conformal_summary: V=%ld outside 1..%d", (long)V, SLNLP_CONFORMAL_MAX_V);
    SLNLP_CHECK_ARG(((uintptr_t)y & 7) == 0, "conformal_summary: misaligned pointer");
    SLNLP_CHECK_ARG(((uintptr_t)rows & 15) == 0, "conformal_summary: rows is not 16-byte aligned");
    SLNLP_CHECK_ARG(((uintptr_t)table & 31) == 0, "conformal_summary: table is not 32-byte aligned");
    const size_t n = (size_t)N, cells = ((size_t)V + 1) * 4;
    const Span in[2] = {{rows, n * 16, "rows"}, {y, n * 8, "y"}}, out[1] = {{table, cells * 8, "table"}};
    SLNLP_TRY(check_no_overlap("conformal_summary", out, in));
    const int zero_blocks = (int)std::min<size_t>((cells + 255) / 256, CONFORMAL_MAX_BLOCKS);
    SLNLP_TRY(zlaunch(conformal_zero_kernel, dim3(zero_blocks), 256, 0, st, "conformal_zero", (unsigned long long*)table, (long)cells));
    const int blocks = (int)std::min<int64_t>((N + 255) / 256, CONFORMAL_MAX_BLOCKS);
    return zlaunch(conformal_count_kernel, dim3(blocks), 256, 0, st, "conformal_count", (const int*)rows, y, (int)N, (int)V,
                   (unsigned long long*)table);
}

}  // namespace slnlp

extern "C" int slnlp_conformal_rows(const float* logp, int64_t ld, const int64_t* y, int64_t N, int64_t V, const double* beta_dev, int method,
                                    double lam, int k_reg, int randomized, uint64_t seed, uint32_t draw, const double* qhat_dev, double* score,
                                    int32_t* rows, uint32_t* sets, void* stream) {
    return slnlp::conformal_rows(logp, ld, y, N, V, beta_dev, method, lam, k_reg, randomized, seed, draw, qhat_dev, score, rows, sets,
                                 (hipStream_t)stream);
}
extern "C" int slnlp_conformal_quantile(const double* score, const int32_t* rows, int64_t N, double alpha, double* state, void* stream) {
    return slnlp::conformal_quantile(score, rows, N, alpha, state, (hipStream_t)stream);
}
extern "C" int slnlp_conformal_summary(const int32_t* rows, const int64_t* y, int64_t N, int64_t V, int64_t* table, void* stream) {
    return slnlp::conformal_summary(rows, y, N, V, table, (hipStream_t)stream);
}
