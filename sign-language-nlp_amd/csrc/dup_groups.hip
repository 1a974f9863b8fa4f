// dup_groups.hip -- near-duplicate GROUPS of the rows of one data set, on the device (slnlp.duplicate_groups): the
// connected components of the graph whose edges are the pairs {i, j}, i != j, with d(i, j) <= radius, every row labelled with the
// LOWEST row index of its component.  The distances are the matrices the three *_distances entry points write (uint8 with the
// sentinel 255, uint16 with 65535); the N x N matrix is never resident: the host forms it one chunk of query rows at a time and
// every chunk is linked into ONE device-resident forest, parent int32 [N].  include/slnlp.h states the definitions;
// tests/dup_groups_ref.py restates them in numpy (a plain union-find).  Integers only, integer atomics only.
//
//   dup_begin    parent[i] = i, degree[i] = 0, the head zeroed.
//   dup_link     a wave per query row i = q0 + qi over its row of the chunk: 16-byte loads (a peeled head and tail where the row does
//                not begin or end on 16 bytes), per element one compare; the hits are sparse.  degree[i] = #{j != i : d <= radius},
//                and every hit with j < i is a union(i, j) -- the matrix is symmetric, so j < i sees every edge once.
//   dup_finish   two launches: one thread sets the head's group count to 0 and the pairs to the degree sum halved; then a thread per
//                row walks to its root (group[i]) and the roots are counted (a ballot per wave, one integer atomic per wave).
//
// THE FOREST.  union(a, b): find both roots, then hook the LARGER root under the SMALLER with a 32-bit atomicCAS(parent + big, big,
// small).  Invariants, by induction over the successful CASes (the only stores to parent behind dup_begin):
//   (1) parent[x] <= x always, and parent[x] < x once x is no root: a CAS only ever writes a smaller index over x's own.
//   (2) a row that was ever a non-root stays one: the CAS expects parent[x] == x, so it never succeeds on a non-root.
//   (3) an old value of parent[x] is x itself or the one parent x ever gets (by (2) a word changes at most once), so a walk over
//       values of any age moves along true ancestors or stands still, and strictly downwards in index when it moves.
// Hence a tree's root is its minimum, and by the kernel boundary in front of dup_finish every link is visible: the labelling is the
// unique lowest-index one, a pure function of the arguments, although the intermediate trees depend on the order of the hooks.
//
// VISIBILITY.  Per-XCD L2s and per-CU L1s are not coherent for plain loads, so `find` reads parent with RELAXED AGENT-SCOPE ATOMIC
// LOADS (global_load sc1: past L1, where the agent-scope CAS is performed).  That is for progress, not for correctness: by (3)
// a stale value is still an ancestor or the row itself.  What a stale read can do is name a row a root that no longer is one -- then
// the CAS on it fails, RETURNS THE TRUE VALUE, and the walk goes on from there.  Only the CAS must be atomic.  There are no
// path-compression stores: link's hits are sparse, and finish resolves the roots.  dup_finish reads parent with plain loads: nothing
// stores to it in those launches, and a launch begins with clean L1s.
//
// NO LOOP HERE CAN RUN FOREVER.  A walk descends strictly (1), so it ends within N steps; a failed CAS means that another thread
// completed a hook on that root, and at most N - 1 hooks exist.  All the same, every walk and every retry loop counts its rounds to
// N + 1 and gives up: the thread sets DUP_HEAD_CODE in the head and leaves, and the host wrapper raises.  It is no spin-wait:
// no thread waits for another's store.
//
// head int64 [8]: groups | pairs (the degree sum halved) | unusable rows | code (0: fine) | the degree sum | 0 0 0.
#include <limits.h>

#include "common.hpp"
#include "edit_shared.hpp"
#include "launch.hpp"
#include "spans.hpp"

namespace slnlp {

enum { DUP_HEAD_GROUPS = 0, DUP_HEAD_PAIRS = 1, DUP_HEAD_FLAGGED = 2, DUP_HEAD_CODE = 3, DUP_HEAD_DEGREES = 4 };
static_assert(SLNLP_DUP_HEAD_BYTES == 64, "the head is int64 [8]");

__device__ __forceinline__ void dup_head_add(int64_t* head, int at, long long v) {
    atomicAdd(reinterpret_cast<unsigned long long*>(head + at), (unsigned long long)v);
}
__device__ __forceinline__ void dup_give_up(int64_t* head) { atomicOr(reinterpret_cast<unsigned long long*>(head + DUP_HEAD_CODE), 1ull); }

__device__ __forceinline__ int dup_parent(const int* parent, int x) {
    return __hip_atomic_load(parent + x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
// the root above x as far as this thread can see, or -1 after N + 1 steps (which (1) rules out)
__device__ __forceinline__ int dup_find(const int* parent, int x, int N) {
    for (int r = 0; r <= N; ++r) {
        const int p = dup_parent(parent, x);
        if (p == x) return x;
        x = p;
    }
    return -1;
}
// false: gave up
__device__ __forceinline__ bool dup_union(int* parent, int i, int j, int N) {
    int a = dup_find(parent, i, N), b = dup_find(parent, j, N);
    for (int r = 0; r <= N; ++r) {
        if (a < 0 || b < 0) return false;
        if (a == b) return true;
        const int big = a > b ? a : b, small = a > b ? b : a;
        const int seen = atomicCAS(parent + big, big, small);
        if (seen == big) return true;
        a = dup_find(parent, seen, N);                       // big got a parent meanwhile: the true one, a smaller index
        b = dup_find(parent, small, N);
    }
    return false;
}

__device__ __forceinline__ void dup_begin_body(int* __restrict__ parent, int* __restrict__ degree, int N, int64_t* __restrict__ head) {
    const long stride = (long)gridDim.x * 256;
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < N; i += stride) {
        parent[i] = (int)i;
        degree[i] = 0;
    }
    if (blockIdx.x == 0 && threadIdx.x < 8) head[threadIdx.x] = 0;
}
SLNLP_ZKERNEL(dup_begin_kernel, 256, dup_begin_body)

// one element of row i: *deg counts it, a lower index is linked
__device__ __forceinline__ void dup_hit(int* parent, int i, long j, int d, int radius, int N, int* deg, bool* ok) {
    if (d > radius || j == i) return;
    *deg += 1;
    if (j < i && !dup_union(parent, i, (int)j, N)) *ok = false;
}

template <class T, int NONE>
__device__ __forceinline__ void dup_link_generic(const T* __restrict__ dist, int nq, int N, int q0, int radius, int* parent,
                                                 int* __restrict__ degree, int64_t* head) {
    constexpr int PER = 16 / (int)sizeof(T);                 // elements of a 16-byte load
    wave_rows<int>(nq, [&](int qi, int lane) {               // qi, i and usable: the same in every lane
        const int i = q0 + qi;
        const T* row = dist + (long)qi * N;
        const bool usable = row[i] != NONE;
        int deg = 0;
        bool ok = true;
        if (usable) {
            // [0, lead) one element a lane, [lead, lead + PER * nvec) in 16-byte loads, the rest one element a lane again
            const long mis = (long)(((uintptr_t)row & 15) / sizeof(T));
            long lead = mis ? PER - mis : 0;
            if (lead > N) lead = N;
            const long nvec = (N - lead) / PER;
            const long tail = lead + nvec * PER;
            if (lane < lead) dup_hit(parent, i, lane, row[lane], radius, N, &deg, &ok);
            const uint4* vec = reinterpret_cast<const uint4*>(row + lead);
            for (long v = lane; v < nvec; v += 64) {
                const uint4 w = vec[v];
                const unsigned word[4] = {w.x, w.y, w.z, w.w};
                const long j0 = lead + v * PER;
#pragma unroll
                for (int e = 0; e < PER; ++e) {
                    const int d = (int)((word[e * (int)sizeof(T) / 4] >> (8 * ((e * (int)sizeof(T)) & 3))) & (unsigned)NONE);
                    dup_hit(parent, i, j0 + e, d, radius, N, &deg, &ok);
                }
            }
            if (tail + lane < N) dup_hit(parent, i, tail + lane, row[tail + lane], radius, N, &deg, &ok);
        }
        const int total = wave_sum_i(deg);
        const bool fine = __all(ok);
        if (lane == 0) {
            degree[i] = total;
            if (!usable) dup_head_add(head, DUP_HEAD_FLAGGED, 1);
            if (total) dup_head_add(head, DUP_HEAD_DEGREES, total);
            if (!fine) dup_give_up(head);
        }
    });
}
__device__ __forceinline__ void dup_link8_body(const unsigned char* __restrict__ dist, int nq, int N, int q0, int radius, int* parent,
                                               int* __restrict__ degree, int64_t* head) {
    dup_link_generic<unsigned char, 255>(dist, nq, N, q0, radius, parent, degree, head);
}
__device__ __forceinline__ void dup_link16_body(const unsigned short* __restrict__ dist, int nq, int N, int q0, int radius, int* parent,
                                                int* __restrict__ degree, int64_t* head) {
    dup_link_generic<unsigned short, 65535>(dist, nq, N, q0, radius, parent, degree, head);
}
SLNLP_ZKERNEL(dup_link8_kernel, 256, dup_link8_body)
SLNLP_ZKERNEL(dup_link16_kernel, 256, dup_link16_body)

__device__ __forceinline__ void dup_head_body(int64_t* __restrict__ head) {
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        head[DUP_HEAD_GROUPS] = 0;
        head[DUP_HEAD_PAIRS] = head[DUP_HEAD_DEGREES] / 2;
    }
}
SLNLP_ZKERNEL(dup_head_kernel, 64, dup_head_body)

__device__ __forceinline__ void dup_finish_body(const int* __restrict__ parent, int N, int* __restrict__ group, int64_t* head) {
    const long stride = (long)gridDim.x * 256;
    const long rounds = ((long)N + stride - 1) / stride;      // the same in every thread: whole waves reach the ballot
    for (long t = 0; t < rounds; ++t) {
        const long i = t * stride + (long)blockIdx.x * 256 + threadIdx.x;
        bool root = false, lost = false;
        if (i < N) {
            int x = (int)i, r = 0;
            for (; r <= N; ++r) {
                const int p = parent[x];
                if (p == x) break;
                x = p;
            }
            lost = r > N;
            group[i] = x;
            root = x == (int)i;
        }
        const unsigned long long roots = __ballot(root);
        const bool any_lost = __any(lost);
        if ((threadIdx.x & 63) == 0) {
            if (roots) dup_head_add(head, DUP_HEAD_GROUPS, __popcll(roots));
            if (any_lost) dup_give_up(head);
        }
    }
}
SLNLP_ZKERNEL(dup_finish_kernel, 256, dup_finish_body)

static inline int dup_check_rows(const char* what, const char* name, int64_t n) {
    SLNLP_CHECK_ARG(n >= 1 && n <= SLNLP_EDIT_MAX_ROWS, "%s: %s=%ld outside 1..%d", what, name, (long)n, SLNLP_EDIT_MAX_ROWS);
    return 0;
}
static inline int dup_row_blocks(int64_t N) { return (int)((N + 255) / 256 < WAVE_ROWS_MAX_BLOCKS ? (N + 255) / 256 : WAVE_ROWS_MAX_BLOCKS); }

}  // namespace slnlp

extern "C" int slnlp_dup_groups_begin(int32_t* parent, int32_t* degree, int64_t N, int64_t* head, void* stream) {
    using namespace slnlp;
    const char* what = "dup_groups_begin";
    SLNLP_CHECK_ARG(parent && degree && head, "%s: null pointer", what);
    SLNLP_TRY(dup_check_rows(what, "N", N));
    SLNLP_CHECK_ARG((((uintptr_t)parent | (uintptr_t)degree) & 3) == 0 && ((uintptr_t)head & 7) == 0,
                    "%s: misaligned pointer (parent, degree: 4 bytes; head: 8 bytes)", what);
    const Span out[3] = {{parent, (size_t)N * 4, "parent"}, {degree, (size_t)N * 4, "degree"}, {head, SLNLP_DUP_HEAD_BYTES, "head"}};
    const Span in[1] = {Span{nullptr, 0, ""}};
    SLNLP_TRY(check_no_overlap(what, out, in));
    return zlaunch(dup_begin_kernel, dim3(dup_row_blocks(N)), 256, 0, (hipStream_t)stream, what, (int*)parent, (int*)degree, (int)N, head);
}

extern "C" int slnlp_dup_groups_link(const void* dist, int width, int64_t nq, int64_t N, int64_t q0, int64_t radius, int32_t* parent,
                                     int32_t* degree, int64_t* head, void* stream) {
    using namespace slnlp;
    const char* what = "dup_groups_link";
    const hipStream_t st = (hipStream_t)stream;
    SLNLP_CHECK_ARG(dist && parent && degree && head, "%s: null pointer", what);
    SLNLP_CHECK_ARG(width == 1 || width == 2, "%s: width=%d, expected 1 (uint8 distances) or 2 (uint16 distances)", what, width);
    SLNLP_TRY(dup_check_rows(what, "N", N));
    SLNLP_TRY(dup_check_rows(what, "nq", nq));
    SLNLP_CHECK_ARG(q0 >= 0 && q0 <= N - nq, "%s: the query rows q0=%ld .. q0 + nq=%ld lie outside the %ld rows", what, (long)q0, (long)(q0 + nq),
                    (long)N);
    SLNLP_TRY(edit_check_pairs(what, nq, N, width));
    const int64_t top = width == 1 ? 254 : 65534;
    SLNLP_CHECK_ARG(radius >= 0 && radius <= top, "%s: radius=%ld outside 0..%ld (%s distances)", what, (long)radius, (long)top,
                    width == 1 ? "uint8" : "uint16");
    SLNLP_CHECK_ARG(((uintptr_t)dist & (uintptr_t)(width - 1)) == 0 && (((uintptr_t)parent | (uintptr_t)degree) & 3) == 0 && ((uintptr_t)head & 7) == 0,
                    "%s: misaligned pointer (dist: %d bytes; parent, degree: 4 bytes; head: 8 bytes)", what, width);
    const Span in[1] = {{dist, (size_t)nq * (size_t)N * (size_t)width, "dist"}};
    const Span out[3] = {{parent, (size_t)N * 4, "parent"}, {degree, (size_t)N * 4, "degree"}, {head, SLNLP_DUP_HEAD_BYTES, "head"}};
    SLNLP_TRY(check_no_overlap(what, out, in));
    const dim3 grid(wave_rows_grid(nq));
    if (width == 1)
        return zlaunch(dup_link8_kernel, grid, 256, 0, st, what, (const unsigned char*)dist, (int)nq, (int)N, (int)q0, (int)radius, (int*)parent,
                       (int*)degree, head);
    return zlaunch(dup_link16_kernel, grid, 256, 0, st, what, (const unsigned short*)dist, (int)nq, (int)N, (int)q0, (int)radius, (int*)parent,
                   (int*)degree, head);
}

extern "C" int slnlp_dup_groups_finish(const int32_t* parent, int64_t N, int32_t* group, int64_t* head, void* stream) {
    using namespace slnlp;
    const char* what = "dup_groups_finish";
    const hipStream_t st = (hipStream_t)stream;
    SLNLP_CHECK_ARG(parent && group && head, "%s: null pointer", what);
    SLNLP_TRY(dup_check_rows(what, "N", N));
    SLNLP_CHECK_ARG((((uintptr_t)parent | (uintptr_t)group) & 3) == 0 && ((uintptr_t)head & 7) == 0,
                    "%s: misaligned pointer (parent, group: 4 bytes; head: 8 bytes)", what);
    const Span in[1] = {{parent, (size_t)N * 4, "parent"}};
    const Span out[2] = {{group, (size_t)N * 4, "group"}, {head, SLNLP_DUP_HEAD_BYTES, "head"}};
    SLNLP_TRY(check_no_overlap(what, out, in));
    SLNLP_TRY(zlaunch(dup_head_kernel, dim3(1), 64, 0, st, "dup_groups_finish_head", head));
    return zlaunch(dup_finish_kernel, dim3(dup_row_blocks(N)), 256, 0, st, what, (const int*)parent, (int)N, (int*)group, head);
}
