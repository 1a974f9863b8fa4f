// bootstrap.hip -- B bootstrap replicates of the scoring metrics of one set of predictions, on the device (DESIGN.md section 4;
// slnlp/metrics.py's bootstrap_intervals / bootstrap_difference, NeuralNetClassifier.score_interval / compare).  include/slnlp.h
// states the definition; tests/bootstrap_ref.py restates it in numpy on metrics.scores_from_rows.
//
// Inputs are what the earlier calls left on the device: y int64 [N], score_rows' pred and rank int32 [N], and Q fp64 value columns
// [N, ldv] (reliability_rows' rows: conf, brier, nll).  Replicate b draws N rows with replacement -- draw j: Threefry words at
// counter (j >> 2, b, SEED_STAGE_BOOTSTRAP, 0) under key (seed, 0, 0), word j & 3, row = mulhi32(word, N) -- a function of
// (seed, b, j, N) alone, so two calls with one seed see the same resamples whatever they score, and replicate b does not depend on B.
// Over the drawn rows it counts true_sum / pred_sum / tp_sum per class, n_bad and the top-k hits (a value outside [0, V) is never
// used as an index: score_rows' rule) and sums the value columns; stats[b] = accuracy, precision / recall / f1 macro and weighted,
// balanced accuracy, top-k accuracy and the column means, with metrics._scores' rules: the macro and weighted families run over the
// classes PRESENT IN THE REPLICATE (true_sum + pred_sum > 0; zero_division = 0), balanced accuracy over those with true_sum > 0.
//
// HOW IT RUNS.  One launch, one block of 256 threads per replicate.  The 3 V class counts live in LDS (dynamic, 12 V bytes) and
// are accumulated with integer LDS atomics: sums of integers, the same whatever the order of arrival.  Every fp64 sum has a fixed
// order: thread t adds its draws j = t, t + 256, ... (its classes c = t, t + 256, ...) in increasing order, then the 256 partial
// sums meet in a fixed binary tree -- wave_sum_d's DPP / v_readlane order inside a wave, (w0 + w1) + (w2 + w3) across the four
// waves through LDS.  No global atomics; the result is a function of the arguments alone.  The gathers into y, pred, rank and
// values are random but touch a few hundred KiB at most: they are left to L2.
// A Threefry call yields four draws, j = 4 q .. 4 q + 3, which belong to the four threads of a quad (256 is a multiple of 4: in
// every round of the draw loop a quad shares one call and thread t takes word t & 3).  So that the quad does not compute the same
// call four times, the rounds go four at a time: quad lane l computes the call of round i0 + l, and in round i0 + s every lane
// fetches the four words of lane s by DPP quad broadcasts and keeps its own -- one call per four draws, as the definition reads.
#include <limits.h>
#include <math.h>

#include <algorithm>

#include "common.hpp"
#include "launch.hpp"
#include "spans.hpp"

namespace slnlp {

enum { BT_HITS = 0, BT_BAD = 1, BT_CORRECT = 2, BT_PRESENT = 3, BT_SEEN = 4, BT_TALLIES = 5 };      // the block's integer tallies
enum { BS_P = 0, BS_R = 1, BS_F = 2, BS_WP = 3, BS_WR = 4, BS_WF = 5, BS_BAL = 6, BS_SUMS = 7 };      // its fp64 sums over the classes

// word w (0..3) of a Threefry call; a 64-bit shift, not a select chain over the vector's elements (common.hpp: pick_lot)
__device__ __forceinline__ unsigned boot_word(const uint4& v, unsigned w) {
    const unsigned long long lo = (unsigned long long)v.x | ((unsigned long long)v.y << 32);
    const unsigned long long hi = (unsigned long long)v.z | ((unsigned long long)v.w << 32);
    return (unsigned)(((w & 2u) ? hi : lo) >> (32u * (w & 1u)));
}

// the Threefry words of quad lane S (0..3), in every lane of the quad (all lanes active)
template <int S>
__device__ __forceinline__ uint4 quad_words(const uint4& v) {
    return make_uint4((unsigned)dpp_mov_i<S * 0x55>((int)v.x), (unsigned)dpp_mov_i<S * 0x55>((int)v.y), (unsigned)dpp_mov_i<S * 0x55>((int)v.z),
                      (unsigned)dpp_mov_i<S * 0x55>((int)v.w));          // quad_perm [S, S, S, S]
}

__device__ __forceinline__ double boot_ratio(double num, int den) { return den == 0 ? 0.0 : num / (double)den; }      // zero_division = 0

__device__ __forceinline__ void bootstrap_body(const int64_t* __restrict__ y, const int* __restrict__ pred, const int* __restrict__ rank,
                                               const double* __restrict__ values, long ldv, int Q, int N, int V, int top_k,
                                               unsigned long long seed, double* __restrict__ stats, int* __restrict__ counts) {
    extern __shared__ int cls[];                         // true_sum [V] | pred_sum [V] | tp_sum [V]
    __shared__ double across[4][BS_SUMS + SLNLP_BOOT_MAX_VALUES];
    __shared__ int tally[BT_TALLIES];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const unsigned b = blockIdx.x;
    for (int i = tid; i < 3 * V; i += 256) cls[i] = 0;
    if (tid < BT_TALLIES) tally[tid] = 0;
    __syncthreads();

    // ---- the draws: thread t takes j = t, t + 256, ... in increasing order; its word of every call is w = t & 3
    const SeedKey K = seed_key(seed, b);
    const unsigned w = (unsigned)tid & 3u;
    int hits = 0, bad = 0, correct = 0;
    double vs[SLNLP_BOOT_MAX_VALUES];
#pragma unroll
    for (int c = 0; c < SLNLP_BOOT_MAX_VALUES; ++c) vs[c] = 0.0;
    auto take = [&](long j, unsigned x) {
        if (j >= N) return;
        const long r = (long)(((unsigned long long)x * (unsigned)N) >> 32);      // mulhi32: in [0, N)
        const int64_t label = y[r];
        const int p = pred[r];
        const bool ok = label >= 0 && label < V, pok = p >= 0 && p < V;          // a value outside the classes is never used as an index
        if (ok) atomicAdd(&cls[label], 1); else ++bad;
        if (pok) atomicAdd(&cls[V + p], 1);
        if (ok && (int64_t)p == label) { atomicAdd(&cls[2 * V + p], 1); ++correct; }
        if (top_k > 0 && ok && rank[r] < top_k) ++hits;
        const double* row = values + r * ldv;            // (not read when Q == 0)
#pragma unroll
        for (int c = 0; c < SLNLP_BOOT_MAX_VALUES; ++c)
            if (c < Q) vs[c] += row[c];
    };
    const int rounds = (N + 255) >> 8;                   // the same in every thread: every lane reaches the quad broadcasts
    for (int i0 = 0; i0 < rounds; i0 += 4) {
        // round i: j = t + 256 i, call q = j >> 2 = (t >> 2) + 64 i; this lane computes the quad's call of round i0 + w (a call
        // past the last round is computed and not used)
        const uint4 mine = seed_words((unsigned)(tid >> 2) + 64u * ((unsigned)i0 + w), SEED_STAGE_BOOTSTRAP, K);
        const long j = tid + 256L * i0;
        take(j, boot_word(quad_words<0>(mine), w));
        take(j + 256, boot_word(quad_words<1>(mine), w));
        take(j + 512, boot_word(quad_words<2>(mine), w));
        take(j + 768, boot_word(quad_words<3>(mine), w));
    }
    if (hits) atomicAdd(&tally[BT_HITS], hits);
    if (bad) atomicAdd(&tally[BT_BAD], bad);
    if (correct) atomicAdd(&tally[BT_CORRECT], correct);
    __syncthreads();

    // ---- the classes: thread t takes c = t, t + 256, ...
    if (counts) {
        int* out = counts + (long)b * (3L * V + 1);
        for (int i = tid; i < 3 * V; i += 256) out[i] = cls[i];
        if (tid == 0) out[3 * V] = tally[BT_BAD];
    }
    double s[BS_SUMS];
#pragma unroll
    for (int k = 0; k < BS_SUMS; ++k) s[k] = 0.0;
    int present = 0, seen = 0;
    for (int c = tid; c < V; c += 256) {
        const int ts = cls[c], ps = cls[V + c];
        if (ts + ps == 0) continue;                      // the class does not occur in this replicate
        const double tp = (double)cls[2 * V + c];
        const double pr = boot_ratio(tp, ps), rc = boot_ratio(tp, ts), f1 = (2.0 * tp) / (double)(ts + ps);
        ++present;
        s[BS_P] += pr; s[BS_R] += rc; s[BS_F] += f1;
        s[BS_WP] += pr * (double)ts; s[BS_WR] += rc * (double)ts; s[BS_WF] += f1 * (double)ts;
        if (ts > 0) { ++seen; s[BS_BAL] += rc; }
    }
    if (present) atomicAdd(&tally[BT_PRESENT], present);
    if (seen) atomicAdd(&tally[BT_SEEN], seen);

    // ---- the fixed tree: inside the waves (every lane takes part), then thread 0 over the four waves
#pragma unroll
    for (int k = 0; k < BS_SUMS; ++k) {
        const double t = wave_sum_d(s[k]);
        if (lane == 0) across[wave][k] = t;
    }
#pragma unroll
    for (int c = 0; c < SLNLP_BOOT_MAX_VALUES; ++c) {
        if (c < Q) {                                     // Q: the same in every thread
            const double t = wave_sum_d(vs[c]);
            if (lane == 0) across[wave][BS_SUMS + c] = t;
        }
    }
    __syncthreads();
    if (tid != 0) return;
    double tot[BS_SUMS];
#pragma unroll
    for (int k = 0; k < BS_SUMS; ++k) tot[k] = (across[0][k] + across[1][k]) + (across[2][k] + across[3][k]);
    const double n = (double)N, n_present = (double)tally[BT_PRESENT], n_true = (double)(N - tally[BT_BAD]);
    double* out = stats + (long)b * (SLNLP_BOOT_FIXED + Q);
    out[0] = (double)tally[BT_CORRECT] / n;
    out[1] = tot[BS_P] / n_present;                      // (no class present: 0 / 0, the mean of nothing)
    out[2] = tot[BS_R] / n_present;
    out[3] = tot[BS_F] / n_present;
    const bool any_true = tally[BT_BAD] < N;
    out[4] = any_true ? tot[BS_WP] / n_true : 0.0;
    out[5] = any_true ? tot[BS_WR] / n_true : 0.0;
    out[6] = any_true ? tot[BS_WF] / n_true : 0.0;
    out[7] = tot[BS_BAL] / (double)tally[BT_SEEN];
    out[8] = top_k > 0 ? (double)tally[BT_HITS] / n : __builtin_bit_cast(double, 0x7ff8000000000000ull);
    for (int c = 0; c < Q; ++c) out[SLNLP_BOOT_FIXED + c] = ((across[0][BS_SUMS + c] + across[1][BS_SUMS + c]) +
                                                             (across[2][BS_SUMS + c] + across[3][BS_SUMS + c])) / n;
}
SLNLP_ZKERNEL(bootstrap_kernel, 256, bootstrap_body)

int bootstrap_scores(const int64_t* y, const int32_t* pred, const int32_t* rank, const double* values, int64_t ldv, int Q, int64_t N, int V,
                     int top_k, int B, uint64_t seed, double* stats, int32_t* counts, hipStream_t st) {
    SLNLP_CHECK_ARG(Q >= 0 && Q <= SLNLP_BOOT_MAX_VALUES, "bootstrap_scores: Q=%d outside 0..%d", Q, SLNLP_BOOT_MAX_VALUES);
    SLNLP_CHECK_ARG(y && pred && stats && (rank || top_k == 0) && (values || Q == 0), "bootstrap_scores: null pointer");
    SLNLP_CHECK_ARG(N >= 1 && N <= INT_MAX, "bootstrap_scores: N=%ld outside 1..%d", (long)N, INT_MAX);
    SLNLP_CHECK_ARG(V >= 1 && V <= SLNLP_CONFUSION_MAX_V, "bootstrap_scores: V=%d outside 1..%d", V, SLNLP_CONFUSION_MAX_V);
    SLNLP_CHECK_ARG(B >= 1 && B <= SLNLP_BOOT_MAX_REPLICATES, "bootstrap_scores: B=%d outside 1..%d", B, SLNLP_BOOT_MAX_REPLICATES);
    SLNLP_CHECK_ARG(Q == 0 || ldv >= Q, "bootstrap_scores: ldv=%ld is less than Q=%d", (long)ldv, Q);
    SLNLP_CHECK_ARG(Q == 0 || ldv <= INT64_MAX / 8 / N, "bootstrap_scores: ldv=%ld times N=%ld is no addressable matrix", (long)ldv, (long)N);
    SLNLP_CHECK_ARG(top_k == 0 || (top_k >= 1 && top_k < V), "bootstrap_scores: top_k=%d outside [1, %d) and not 0", top_k, V);
    SLNLP_CHECK_ARG((((uintptr_t)pred | (uintptr_t)rank | (uintptr_t)counts) & 3) == 0 &&
                        (((uintptr_t)y | (uintptr_t)values | (uintptr_t)stats) & 7) == 0,
                    "bootstrap_scores: misaligned pointer");
    const size_t n = (size_t)N, b = (size_t)B;
    const Span in[4] = {{y, n * 8, "y"}, {pred, n * 4, "pred"}, {top_k ? rank : nullptr, n * 4, "rank"},
                            {Q ? values : nullptr, Q ? ((n - 1) * (size_t)ldv + (size_t)Q) * 8 : 0, "values"}};
    const Span out[2] = {{stats, b * (size_t)(SLNLP_BOOT_FIXED + Q) * 8, "stats"}, {counts, b * (3 * (size_t)V + 1) * 4, "counts"}};
    SLNLP_TRY(check_no_overlap("bootstrap_scores", out, in));
    return zlaunch(bootstrap_kernel, dim3(B), 256, 3 * (size_t)V * sizeof(int), st, "bootstrap_scores", y, pred, top_k ? rank : nullptr,
                   Q ? values : nullptr, (long)(Q ? ldv : 0), Q, (int)N, V, top_k, (unsigned long long)seed, stats, counts);
}

}  // namespace slnlp

extern "C" int slnlp_bootstrap_scores(const int64_t* y, const int32_t* pred, const int32_t* rank, const double* values, int64_t ldv, int Q,
                                      int64_t N, int V, int top_k, int B, uint64_t seed, double* stats, int32_t* counts, void* stream) {
    return slnlp::bootstrap_scores(y, pred, rank, values, ldv, Q, N, V, top_k, B, seed, stats, counts, (hipStream_t)stream);
}
