// gloss_structure.hip -- the structure of the LABELS of one data set under an edit distance, on the device (slnlp.gloss_structure;
// DESIGN.md section 4): per row the summed distance to its own gloss and to the nearest other gloss (the two integers of a
// silhouette), per gloss its medoid, and the C x C table of summed distances between glosses.  The distances are the matrices the
// three *_distances entry points write (uint8 with the sentinel 255, uint16 with 65535); the N x N matrix is never resident: the
// host forms it one chunk of query rows at a time, as slnlp.duplicate_groups does, and every chunk is read ONCE, while it still
// lies in cache behind the distance launch.  include/slnlp.h states the definitions; tests/gloss_structure_ref.py restates them in
// numpy.  Integers only, integer atomics only: sums and minima of integers do not depend on the order they are taken in, so the
// result is a pure function of the arguments.
//
//   gs_init     count = 0, class_sum = 0, med_sum = UINT64_MAX, medoid = INT_MAX ("none"), the head zeroed.
//   gs_count    a thread per row: count[label[i]] += 1; the head gets the labelled rows and the rows left out (a ballot per wave).
//               A label outside -1..C-1 sets GS_CODE_LABEL and is treated as -1 by EVERY kernel here: no index is formed from it.
//   gs_rows     a wave per query row i = q0 + qi.  The wave owns a table of C uint32 sums in LDS (four waves a block: 16 C bytes, at
//               most 16 KiB) and adds every element d(i, j), j != i, label[j] >= 0, into table[label[j]] with an LDS integer add --
//               dup_link_generic's loads: 16 bytes a lane, a peeled head and tail where the row does not begin or end on 16 bytes.
//               Then the lanes stride over the classes: own = table[label[i]]; other = the class c != label[i], n_c > 0, of smallest
//               table[c] / n_c, compared EXACTLY as table[a] n_b < table[b] n_a in 64 bits (a sum is below 2^32 -- begin refuses
//               max_distance N >= 2^32 -- and a count at most 2^30), ties to the lower class: a total order on (ratio, class), so
//               the wave reduction has one winner whatever its shape.  class_sum[label[i], c] += table[c] (64-bit atomic add),
//               med_sum[label[i]] = min(own) (64-bit atomic min).
//   gs_medoid   a thread per row: own[i] == med_sum[label[i]] takes a 32-bit atomic min of i into medoid[label[i]].
//   gs_head     one wave: medoid "none" -> -1; head[1] = the classes that have a medoid = the non-empty ones.
//
// THE LDS TABLE is private to its wave: no other wave reads or writes it, so there is no block barrier anywhere (the waves of a
// block run different numbers of rows).  Within the wave the order zero -> adds -> reads is program order on one LDS queue; a
// wavefront-scope fence and a wave barrier at the two seams keep the compiler from moving accesses across them.
// Contention: every lane of a wave may add to ONE address (a data set of one gloss); the LDS serialises the adds of an instruction
// that meet in one bank, it loses none.
//
// head int64 [8]: labelled rows | non-empty classes | rows left out | code (0: fine) | the sum of own | 0 0 0.
#include <limits.h>

#include "common.hpp"
#include "edit_shared.hpp"
#include "launch.hpp"
#include "spans.hpp"

namespace slnlp {

enum { GS_HEAD_LABELLED = 0, GS_HEAD_CLASSES = 1, GS_HEAD_LEFT_OUT = 2, GS_HEAD_CODE = 3, GS_HEAD_OWN = 4 };
enum { GS_CODE_SENTINEL = 1, GS_CODE_LABEL = 2 };
static_assert(SLNLP_GLOSS_HEAD_BYTES == 64, "the head is int64 [8]");
constexpr int GS_NONE = INT_MAX;                              // medoid: no row yet

typedef unsigned long long gs_u64;

__device__ __forceinline__ void gs_head_add(int64_t* head, int at, long long v) { atomicAdd(reinterpret_cast<gs_u64*>(head + at), (gs_u64)v); }
__device__ __forceinline__ void gs_head_code(int64_t* head, int code) { atomicOr(reinterpret_cast<gs_u64*>(head + GS_HEAD_CODE), (gs_u64)code); }
// the class of a row, or -1: left out, or a label the count kernel has reported
__device__ __forceinline__ int gs_class(const int* __restrict__ label, long i, int C) {
    const int c = label[i];
    return (unsigned)c < (unsigned)C ? c : -1;
}

__device__ __forceinline__ void gs_init_body(int C, int* __restrict__ count, int64_t* __restrict__ class_sum, int64_t* __restrict__ med_sum,
                                             int* __restrict__ medoid, int64_t* __restrict__ head) {
    const long stride = (long)gridDim.x * 256, cells = (long)C * C;
    const long t = (long)blockIdx.x * 256 + threadIdx.x;
    for (long k = t; k < cells; k += stride) class_sum[k] = 0;
    for (long c = t; c < C; c += stride) {
        count[c] = 0;
        med_sum[c] = -1;                                     // UINT64_MAX
        medoid[c] = GS_NONE;
    }
    if (t < 8) head[t] = 0;
}
SLNLP_ZKERNEL(gs_init_kernel, 256, gs_init_body)

__device__ __forceinline__ void gs_count_body(const int* __restrict__ label, int N, int C, int* count, int64_t* head) {
    const long stride = (long)gridDim.x * 256;
    const long rounds = ((long)N + stride - 1) / stride;      // the same in every thread: whole waves reach the ballots
    for (long t = 0; t < rounds; ++t) {
        const long i = t * stride + (long)blockIdx.x * 256 + threadIdx.x;
        bool in = false, out = false, bad = false;
        if (i < N) {
            const int c = label[i];
            in = (unsigned)c < (unsigned)C;
            bad = !in && c != -1;
            out = !in;
            if (in) atomicAdd(count + c, 1);
        }
        const gs_u64 ins = __ballot(in), outs = __ballot(out);
        const bool any_bad = __any(bad);
        if ((threadIdx.x & 63) == 0) {
            if (ins) gs_head_add(head, GS_HEAD_LABELLED, __popcll(ins));
            if (outs) gs_head_add(head, GS_HEAD_LEFT_OUT, __popcll(outs));
            if (any_bad) gs_head_code(head, GS_CODE_LABEL);
        }
    }
}
SLNLP_ZKERNEL(gs_count_kernel, 256, gs_count_body)

// one element of row i into the wave's table
__device__ __forceinline__ void gs_add(unsigned* table, const int* __restrict__ label, int C, int i, long j, unsigned d, unsigned none, bool* bad) {
    if (j == i) return;
    const int c = gs_class(label, j, C);
    if (c < 0) return;
    if (d == none) { *bad = true; return; }
    atomicAdd(table + c, d);                                 // ds_add_u32, no return value
}

// the seams of a wave's private LDS table (see above)
__device__ __forceinline__ void gs_wave_seam() {
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
}

// whether (ta / na, a) comes before (tb / nb, b): the smaller mean, then the lower class; a class of -1 is no candidate
__device__ __forceinline__ bool gs_before(unsigned ta, int na, int a, unsigned tb, int nb, int b) {
    if (a < 0 || b < 0) return b < 0 && a >= 0;
    const gs_u64 l = (gs_u64)ta * (gs_u64)(unsigned)nb, r = (gs_u64)tb * (gs_u64)(unsigned)na;
    return l < r || (l == r && a < b);
}
template <int CTRL>
__device__ __forceinline__ void gs_best_step(unsigned& t, int& n, int& c) {
    const unsigned ot = (unsigned)dpp_mov_i<CTRL>((int)t);
    const int on = dpp_mov_i<CTRL>(n), oc = dpp_mov_i<CTRL>(c);
    if (gs_before(ot, on, oc, t, n, c)) { t = ot; n = on; c = oc; }
}
// over the whole wave (all 64 lanes active); every lane gets the winner
__device__ __forceinline__ void gs_wave_best(unsigned& t, int& n, int& c) {
    gs_best_step<DPP_XOR1>(t, n, c);
    gs_best_step<DPP_XOR2>(t, n, c);
    gs_best_step<DPP_HALF_MIRROR>(t, n, c);
    gs_best_step<DPP_MIRROR>(t, n, c);
    unsigned rt = (unsigned)__builtin_amdgcn_readlane((int)t, 0);
    int rn = __builtin_amdgcn_readlane(n, 0), rc = __builtin_amdgcn_readlane(c, 0);
#pragma unroll
    for (int l = 16; l < 64; l += 16) {
        const unsigned ot = (unsigned)__builtin_amdgcn_readlane((int)t, l);
        const int on = __builtin_amdgcn_readlane(n, l), oc = __builtin_amdgcn_readlane(c, l);
        if (gs_before(ot, on, oc, rt, rn, rc)) { rt = ot; rn = on; rc = oc; }
    }
    t = rt; n = rn; c = rc;
}

template <class T, int NONE>
__device__ __forceinline__ void gs_rows_generic(const T* __restrict__ dist, int nq, int N, int q0, const int* __restrict__ label, int C,
                                                const int* __restrict__ count, unsigned* __restrict__ own, unsigned* __restrict__ other,
                                                int* __restrict__ other_class, int64_t* class_sum, int64_t* med_sum, int64_t* head) {
    extern __shared__ unsigned gs_tables[];                  // [4][C]
    constexpr int PER = 16 / (int)sizeof(T);                 // elements of a 16-byte load
    unsigned* table = gs_tables + (size_t)(threadIdx.x >> 6) * C;
    wave_rows<int>(nq, [&](int qi, int lane) {               // qi, i and li: the same in every lane
        const int i = q0 + qi;
        const int li = gs_class(label, i, C);
        if (li < 0) {
            if (lane == 0) { own[i] = 0; other[i] = 0; other_class[i] = -1; }
            return;
        }
        for (int c = lane; c < C; c += 64) table[c] = 0;
        gs_wave_seam();
        const T* row = dist + (long)qi * N;
        bool bad = false;
        // [0, lead) one element a lane, [lead, lead + PER * nvec) in 16-byte loads, the rest one element a lane again
        const long mis = (long)(((uintptr_t)row & 15) / sizeof(T));
        long lead = mis ? PER - mis : 0;
        if (lead > N) lead = N;
        const long nvec = (N - lead) / PER;
        const long tail = lead + nvec * PER;
        if (lane < lead) gs_add(table, label, C, i, lane, row[lane], NONE, &bad);
        const uint4* vec = reinterpret_cast<const uint4*>(row + lead);
        for (long v = lane; v < nvec; v += 64) {
            const uint4 w = vec[v];
            const unsigned word[4] = {w.x, w.y, w.z, w.w};
            const long j0 = lead + v * PER;
#pragma unroll
            for (int e = 0; e < PER; ++e) {
                const unsigned d = (word[e * (int)sizeof(T) / 4] >> (8 * ((e * (int)sizeof(T)) & 3))) & (unsigned)NONE;
                gs_add(table, label, C, i, j0 + e, d, NONE, &bad);
            }
        }
        if (tail + lane < N) gs_add(table, label, C, i, tail + lane, row[tail + lane], NONE, &bad);
        gs_wave_seam();
        unsigned bt = 0;
        int bn = 0, bc = -1;
        int64_t* sums = class_sum + (long)li * C;
        for (int c = lane; c < C; c += 64) {
            const unsigned t = table[c];
            const int n = count[c];
            if (t) atomicAdd(reinterpret_cast<gs_u64*>(sums + c), (gs_u64)t);
            if (c != li && n > 0 && gs_before(t, n, c, bt, bn, bc)) { bt = t; bn = n; bc = c; }
        }
        gs_wave_best(bt, bn, bc);
        const unsigned mine = table[li];
        const bool any_bad = __any(bad);
        gs_wave_seam();                                      // the reads above, before the next row's zeroes
        if (lane == 0) {
            own[i] = mine;
            other[i] = bc < 0 ? 0u : bt;
            other_class[i] = bc;
            atomicMin(reinterpret_cast<gs_u64*>(med_sum + li), (gs_u64)mine);
            if (mine) gs_head_add(head, GS_HEAD_OWN, mine);
            if (any_bad) gs_head_code(head, GS_CODE_SENTINEL);
        }
    });
}
__device__ __forceinline__ void gs_rows8_body(const unsigned char* __restrict__ dist, int nq, int N, int q0, const int* __restrict__ label, int C,
                                              const int* __restrict__ count, unsigned* __restrict__ own, unsigned* __restrict__ other,
                                              int* __restrict__ other_class, int64_t* class_sum, int64_t* med_sum, int64_t* head) {
    gs_rows_generic<unsigned char, 255>(dist, nq, N, q0, label, C, count, own, other, other_class, class_sum, med_sum, head);
}
__device__ __forceinline__ void gs_rows16_body(const unsigned short* __restrict__ dist, int nq, int N, int q0, const int* __restrict__ label, int C,
                                               const int* __restrict__ count, unsigned* __restrict__ own, unsigned* __restrict__ other,
                                               int* __restrict__ other_class, int64_t* class_sum, int64_t* med_sum, int64_t* head) {
    gs_rows_generic<unsigned short, 65535>(dist, nq, N, q0, label, C, count, own, other, other_class, class_sum, med_sum, head);
}
SLNLP_ZKERNEL(gs_rows8_kernel, 256, gs_rows8_body)
SLNLP_ZKERNEL(gs_rows16_kernel, 256, gs_rows16_body)

__device__ __forceinline__ void gs_medoid_body(const int* __restrict__ label, const unsigned* __restrict__ own, const int64_t* __restrict__ med_sum,
                                               int N, int C, int* medoid) {
    const long stride = (long)gridDim.x * 256;
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < N; i += stride) {
        const int c = gs_class(label, i, C);
        if (c >= 0 && (gs_u64)own[i] == (gs_u64)med_sum[c]) atomicMin(medoid + c, (int)i);
    }
}
SLNLP_ZKERNEL(gs_medoid_kernel, 256, gs_medoid_body)

__device__ __forceinline__ void gs_head_body(int C, int* __restrict__ medoid, int64_t* __restrict__ head) {
    if (blockIdx.x != 0) return;
    const int lane = threadIdx.x;                            // one wave
    int found = 0;
    for (int c = lane; c < C; c += 64) {
        const int m = medoid[c];
        if (m == GS_NONE || m < 0) medoid[c] = -1;           // m < 0: finish called again
        else found += 1;
    }
    found = wave_sum_i(found);
    if (lane == 0) head[GS_HEAD_CLASSES] = found;
}
SLNLP_ZKERNEL(gs_head_kernel, 64, gs_head_body)

static inline int gs_check_rows(const char* what, const char* name, int64_t n) {
    SLNLP_CHECK_ARG(n >= 1 && n <= SLNLP_EDIT_MAX_ROWS, "%s: %s=%ld outside 1..%d", what, name, (long)n, SLNLP_EDIT_MAX_ROWS);
    return 0;
}
static inline int gs_check_classes(const char* what, int64_t C) {
    SLNLP_CHECK_ARG(C >= 1 && C <= SLNLP_GLOSS_MAX_CLASSES, "%s: C=%ld outside 1..%d", what, (long)C, SLNLP_GLOSS_MAX_CLASSES);
    return 0;
}
static inline int gs_row_blocks(int64_t n) { return (int)((n + 255) / 256 < WAVE_ROWS_MAX_BLOCKS ? (n + 255) / 256 : WAVE_ROWS_MAX_BLOCKS); }
static inline bool gs_misaligned(const void* a, const void* b, const void* c, unsigned mask) {
    return (((uintptr_t)a | (uintptr_t)b | (uintptr_t)c) & mask) != 0;
}

}  // namespace slnlp

extern "C" int slnlp_gloss_structure_begin(const int32_t* label, int64_t N, int64_t C, int64_t max_distance, int32_t* count, int64_t* class_sum,
                                           int64_t* med_sum, int32_t* medoid, int64_t* head, void* stream) {
    using namespace slnlp;
    const char* what = "gloss_structure_begin";
    const hipStream_t st = (hipStream_t)stream;
    SLNLP_CHECK_ARG(label && count && class_sum && med_sum && medoid && head, "%s: null pointer", what);
    SLNLP_TRY(gs_check_rows(what, "N", N));
    SLNLP_TRY(gs_check_classes(what, C));
    SLNLP_CHECK_ARG(max_distance >= 1 && max_distance <= 65534, "%s: max_distance=%ld outside 1..65534", what, (long)max_distance);
    SLNLP_CHECK_ARG(max_distance * N < ((int64_t)1 << 32), "%s: max_distance=%ld times N=%ld reaches 2^32: a row's sum over one class must fit 32 bits",
                    what, (long)max_distance, (long)N);
    SLNLP_CHECK_ARG(!gs_misaligned(label, count, medoid, 3) && !gs_misaligned(class_sum, med_sum, head, 7),
                    "%s: misaligned pointer (label, count, medoid: 4 bytes; class_sum, med_sum, head: 8 bytes)", what);
    const Span in[1] = {{label, (size_t)N * 4, "label"}};
    const Span out[5] = {{count, (size_t)C * 4, "count"}, {class_sum, (size_t)C * (size_t)C * 8, "class_sum"}, {med_sum, (size_t)C * 8, "med_sum"},
                         {medoid, (size_t)C * 4, "medoid"}, {head, SLNLP_GLOSS_HEAD_BYTES, "head"}};
    SLNLP_TRY(check_no_overlap(what, out, in));
    SLNLP_TRY(zlaunch(gs_init_kernel, dim3(gs_row_blocks(C * C)), 256, 0, st, "gloss_structure_begin_init", (int)C, (int*)count, class_sum, med_sum,
                      (int*)medoid, head));
    return zlaunch(gs_count_kernel, dim3(gs_row_blocks(N)), 256, 0, st, what, (const int*)label, (int)N, (int)C, (int*)count, head);
}

extern "C" int slnlp_gloss_structure_rows(const void* dist, int width, int64_t nq, int64_t N, int64_t q0, const int32_t* label, int64_t C,
                                          const int32_t* count, uint32_t* own, uint32_t* other, int32_t* other_class, int64_t* class_sum,
                                          int64_t* med_sum, int64_t* head, void* stream) {
    using namespace slnlp;
    const char* what = "gloss_structure_rows";
    const hipStream_t st = (hipStream_t)stream;
    SLNLP_CHECK_ARG(dist && label && count && own && other && other_class && class_sum && med_sum && head, "%s: null pointer", what);
    SLNLP_CHECK_ARG(width == 1 || width == 2, "%s: width=%d, expected 1 (uint8 distances) or 2 (uint16 distances)", what, width);
    SLNLP_TRY(gs_check_rows(what, "N", N));
    SLNLP_TRY(gs_check_rows(what, "nq", nq));
    SLNLP_TRY(gs_check_classes(what, C));
    SLNLP_CHECK_ARG(q0 >= 0 && q0 <= N - nq, "%s: the query rows q0=%ld .. q0 + nq=%ld lie outside the %ld rows", what, (long)q0, (long)(q0 + nq),
                    (long)N);
    SLNLP_TRY(edit_check_pairs(what, nq, N, width));
    SLNLP_CHECK_ARG(((uintptr_t)dist & (uintptr_t)(width - 1)) == 0 && !gs_misaligned(label, count, own, 3) && !gs_misaligned(other, other_class, own, 3) &&
                        !gs_misaligned(class_sum, med_sum, head, 7),
                    "%s: misaligned pointer (dist: %d bytes; label, count, own, other, other_class: 4 bytes; class_sum, med_sum, head: 8 bytes)", what,
                    width);
    const Span in[3] = {{dist, (size_t)nq * (size_t)N * (size_t)width, "dist"}, {label, (size_t)N * 4, "label"}, {count, (size_t)C * 4, "count"}};
    const Span out[6] = {{own, (size_t)N * 4, "own"}, {other, (size_t)N * 4, "other"}, {other_class, (size_t)N * 4, "other_class"},
                         {class_sum, (size_t)C * (size_t)C * 8, "class_sum"}, {med_sum, (size_t)C * 8, "med_sum"}, {head, SLNLP_GLOSS_HEAD_BYTES, "head"}};
    SLNLP_TRY(check_no_overlap(what, out, in));
    const dim3 grid(wave_rows_grid(nq));
    const size_t lds = (size_t)4 * (size_t)C * sizeof(unsigned);
    if (width == 1)
        return zlaunch(gs_rows8_kernel, grid, 256, lds, st, what, (const unsigned char*)dist, (int)nq, (int)N, (int)q0, (const int*)label, (int)C,
                       (const int*)count, (unsigned*)own, (unsigned*)other, (int*)other_class, class_sum, med_sum, head);
    return zlaunch(gs_rows16_kernel, grid, 256, lds, st, what, (const unsigned short*)dist, (int)nq, (int)N, (int)q0, (const int*)label, (int)C,
                   (const int*)count, (unsigned*)own, (unsigned*)other, (int*)other_class, class_sum, med_sum, head);
}

extern "C" int slnlp_gloss_structure_finish(const int32_t* label, const uint32_t* own, const int64_t* med_sum, int64_t N, int64_t C, int32_t* medoid,
                                            int64_t* head, void* stream) {
    using namespace slnlp;
    const char* what = "gloss_structure_finish";
    const hipStream_t st = (hipStream_t)stream;
    SLNLP_CHECK_ARG(label && own && med_sum && medoid && head, "%s: null pointer", what);
    SLNLP_TRY(gs_check_rows(what, "N", N));
    SLNLP_TRY(gs_check_classes(what, C));
    SLNLP_CHECK_ARG(!gs_misaligned(label, own, medoid, 3) && !gs_misaligned(med_sum, head, head, 7),
                    "%s: misaligned pointer (label, own, medoid: 4 bytes; med_sum, head: 8 bytes)", what);
    const Span in[3] = {{label, (size_t)N * 4, "label"}, {own, (size_t)N * 4, "own"}, {med_sum, (size_t)C * 8, "med_sum"}};
    const Span out[2] = {{medoid, (size_t)C * 4, "medoid"}, {head, SLNLP_GLOSS_HEAD_BYTES, "head"}};
    SLNLP_TRY(check_no_overlap(what, out, in));
    SLNLP_TRY(zlaunch(gs_medoid_kernel, dim3(gs_row_blocks(N)), 256, 0, st, what, (const int*)label, (const unsigned*)own, med_sum, (int)N, (int)C,
                      (int*)medoid));
    return zlaunch(gs_head_kernel, dim3(1), 64, 0, st, "gloss_structure_finish_head", (int)C, (int*)medoid, head);
}
