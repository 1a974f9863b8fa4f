// rank_chunk.hpp -- the chunked rank count of ranking.hip (selective.hip's chunks kernel is the same scheme,
// still written out there, with uint64 keys and two histograms: the templates are ready for it): for every member of a set, exact
// integer counts of the rows whose key lies above (or at) its own, with no global atomics and no dependence on timing.  One block of
// 256 threads takes one chunk of CHUNK members (a power of two, a multiple of 256: 8 positions per thread) in LDS arrays that the
// caller declares; the caller also states who is a member, what a row's key is and which histogram a row adds to.  In the order a
// body calls them: chunk_ordinal, chunk_pad_and_clear, chunk_bitonic_sort, chunk_lower_bound / chunk_upper_bound (the caller adds 1
// to a histogram cell there with an integer LDS atomic: integer adds commute), chunk_suffix and chunk_step.
// Every helper that holds a barrier says so: all 256 threads must reach it, from block-uniform control flow only.
#pragma once
#include <hip/hip_runtime.h>

namespace slnlp {

// One tile of 256 rows, thread tid holding row tile + tid: flag[0] says whether the row is a member.  Returns the number of members
// in front of this row within the tile (its ordinal is the caller's running base plus this, so which members form a chunk is a
// function of the arguments) and in total[f] the tile's count of flag[f]: further flags (ranking.hip: the valid rows) ride through
// the same round for no more barriers.  A ballot per wave, the four wave totals through wtot.  TWO BARRIERS INSIDE: behind the
// store to wtot and behind its reads, so the next call may rewrite it.
template <int F>
__device__ __forceinline__ int chunk_ordinal(const bool (&flag)[F], int (&wtot)[F][4], int tid, int (&total)[F]) {
    const int lane = tid & 63, wave = tid >> 6;
    unsigned long long b[F];
#pragma unroll
    for (int f = 0; f < F; ++f) b[f] = __ballot(flag[f]);
    if (lane == 0) {
#pragma unroll
        for (int f = 0; f < F; ++f) wtot[f][wave] = __popcll(b[f]);
    }
    __syncthreads();
    int before = 0;
#pragma unroll
    for (int f = 0; f < F; ++f) total[f] = 0;
#pragma unroll
    for (int w = 0; w < 4; ++w) {
        const int t = wtot[0][w];
        if (w < wave) before += t;
        total[0] += t;
#pragma unroll
        for (int f = 1; f < F; ++f) total[f] += wtot[f][w];
    }
    __syncthreads();
    return before + __popcll(b[0] & ((1ull << lane) - 1ull));
}

// keys[n, m) = pad and idx[n, m) = -1 with m the power of two >= max(n, 1) (<= CHUNK), every histogram cell = 0; returns m.
// ENDS WITH A BARRIER: the compaction's stores to keys and idx are complete behind it too.
template <class Key, int H, int CELLS>
__device__ __forceinline__ int chunk_pad_and_clear(Key* keys, int* idx, int (&hist)[H][CELLS], int n, Key pad, int tid) {
    int m = 1;
    while (m < n) m <<= 1;
    for (int i = n + tid; i < m; i += 256) { keys[i] = pad; idx[i] = -1; }
    for (int i = tid; i < CELLS; i += 256) {
#pragma unroll
        for (int h = 0; h < H; ++h) hist[h][i] = 0;
    }
    __syncthreads();
    return m;
}

// bitonic network over keys[0, m), m a power of two; idx follows its key.  A BARRIER BEHIND EVERY STEP.
template <class Key>
__device__ __forceinline__ void chunk_bitonic_sort(Key* keys, int* idx, int m, int tid) {
    for (int k = 2; k <= m; k <<= 1) {
        for (int j = k >> 1; j >= 1; j >>= 1) {
            for (int i = tid; i < m; i += 256) {
                const int l = i ^ j;
                if (l > i) {
                    const Key a = keys[i], b = keys[l];
                    if ((a > b) == ((i & k) == 0)) {
                        keys[i] = b; keys[l] = a;
                        const int t = idx[i]; idx[i] = idx[l]; idx[l] = t;
                    }
                }
            }
            __syncthreads();
        }
    }
}

// the first position in [from, n) of the sorted keys whose key is >= key (lower) or > key (upper), n if there is none
template <class Key>
__device__ __forceinline__ int chunk_lower_bound(const Key* keys, int n, Key key) {
    int lb = 0, hi = n;
    while (lb < hi) {
        const int mid = (lb + hi) >> 1;
        if (keys[mid] < key) lb = mid + 1; else hi = mid;
    }
    return lb;
}
template <class Key>
__device__ __forceinline__ int chunk_upper_bound(const Key* keys, int n, Key key, int from = 0) {
    int ub = from, hi = n;
    while (ub < hi) {
        const int mid = (ub + hi) >> 1;
        if (keys[mid] <= key) ub = mid + 1; else hi = mid;
    }
    return ub;
}

// Strict suffix sums S_h[p] = the sum of hist[h] over the cells p + 1 .. CHUNK.  Thread tid owns the positions tid * 8 .. tid * 8 + 7:
// it totals its cells (thread 255 the last cell, CHUNK, too), a 256-thread inclusive suffix scan over the totals runs through part,
// and run[h] comes back as S_h of the thread's LAST position; walking down, chunk_step(run, hist, p) turns S_h[p] into S_h[p - 1].
// The histograms must be complete (a barrier of the caller's in front); BARRIERS INSIDE (17).
template <int H, int CELLS>
__device__ __forceinline__ void chunk_suffix(const int (&hist)[H][CELLS], int (&part)[H][256], int tid, int (&run)[H]) {
    constexpr int CHUNK = CELLS - 1, PER_THREAD = CHUNK / 256;
    static_assert(PER_THREAD * 256 == CHUNK, "the histograms have CHUNK + 1 cells, CHUNK a multiple of 256");
    const int p0 = tid * PER_THREAD;
    int tot[H];
#pragma unroll
    for (int h = 0; h < H; ++h) {
        int s = tid == 255 ? hist[h][CHUNK] : 0;
#pragma unroll
        for (int q = 0; q < PER_THREAD; ++q) s += hist[h][p0 + q];
        tot[h] = s;
        part[h][tid] = s;
    }
    __syncthreads();
    for (int d = 1; d < 256; d <<= 1) {                  // inclusive suffix scan over the threads' totals
        int add[H];
#pragma unroll
        for (int h = 0; h < H; ++h) add[h] = tid + d < 256 ? part[h][tid + d] : 0;
        __syncthreads();
#pragma unroll
        for (int h = 0; h < H; ++h) part[h][tid] += add[h];
        __syncthreads();
    }
#pragma unroll
    for (int h = 0; h < H; ++h) run[h] = part[h][tid] - tot[h] + (tid == 255 ? hist[h][CHUNK] : 0);
}
template <int H, int CELLS>
__device__ __forceinline__ void chunk_step(int (&run)[H], const int (&hist)[H][CELLS], int p) {
#pragma unroll
    for (int h = 0; h < H; ++h) run[h] += hist[h][p];
}

}  // namespace slnlp
