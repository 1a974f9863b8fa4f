// edit_knn.hip -- all-pairs Levenshtein distances between two sets of token rows and the k nearest references of every query, on the
// device (slnlp.EditKNN, slnlp.split_audit): the non-neural baseline of a sign data set -- "look up the most
// similar training sign" -- and the audit of a split -- "does this held-out row have a twin in train".  include/slnlp.h states the
// definitions and the buffers; tests/edit_knn_ref.py restates them in numpy, line by line.  This file owns the 64-frame search's
// kernels and entry points, and the head, vote and bad-label kernels that all three searches launch (edit_launch_head /
// edit_launch_logp); the checks and the launch order of a search are edit_shared.hpp's shell.
//
// Xq int64 [nq, .] with row stride ldq, Lq int64 [nq]; Xr / Lr the references.  A row is USABLE when its length lies in
// 0 .. min(64, its row stride): only the first L tokens of a usable row are read, nothing of an unusable one is, tokens are compared
// as full int64 values.  EVERYTHING IS INTEGER until the votes and there are no floating-point atomics: each result is a pure
// function of the arguments, whatever the grid, the stream or the kernels beside it.
//
//   edit_dist     edit_dist.hpp's body -- written once for this search and edit_long.hip's -- for queries of up to 64 frames: a block
//                 per query (queries over a grid-stride loop; with few queries the references in tiles over grid.y), the query's
//                 match masks in ONE 64-bit word per position behind a 128-slot open hash in LDS (1536 bytes a block), and per
//                 reference token one lookup and one column step of Myers' recurrence (edit_myers_multi.hpp at one word, which is
//                 edit_myers.hpp's step; the bit-63 note is there).  uint8 [nq, nr]; 255 where either row is unusable.
//   edit_select   (the body is edit_shared.hpp's, shared with field_knn.hip; here over uint8 with its 65 bins a compile-time constant)
//                 a wave per query over its row of the distance matrix: a 65-bin count in LDS (integer atomics) gives the cut-off
//                 distance T, the count below it and how many rows AT T are still wanted; a second sweep in ascending reference
//                 index keeps the rows below T and the first wanted ones at T by ordered ballot compaction (lanes_below, as
//                 augment.hip and attribution.hip close rows up) -- ties at the k-th distance go to the lower index; the <= 64
//                 kept pairs are ranked by (distance, index) by counting.  The sweep stops once the list is full.
//   edit_head     one block: the unusable queries and references, summed over the fixed tree.
//   edit_logp     a wave per query: the neighbours' weights in fp64 and per class their sum IN LIST ORDER.  The distance bound and
//                 the unit are arguments (64 and 1 here; 64 F and F for field_knn.hip, which launches these kernels too).
//   edit_bad      one block: the neighbours whose reference label lies outside the classes.
#include <limits.h>
#include <math.h>

#include "block_reduce.hpp"
#include "common.hpp"
#include "edit_dist.hpp"
#include "edit_shared.hpp"
#include "launch.hpp"
#include "spans.hpp"

// the vote's arithmetic is rounded operation by operation, as the restatement's numpy expressions are
#pragma clang fp contract(off)

namespace slnlp {

// ------------------------------------------------------------------------------------------------------- distances ----
// the shared body (edit_dist.hpp) for queries of up to 64 frames over the uint8 matrix: one mask word, a 128-slot hash, 1536 bytes of LDS
__device__ __forceinline__ void edit_dist_body(const int64_t* __restrict__ Xq, long ldq, const int64_t* __restrict__ Lq, int nq,
                                               const int64_t* __restrict__ Xr, long ldr, const int64_t* __restrict__ Lr, int nr, int max_q,
                                               int max_r, int tile, unsigned char* __restrict__ dist) {
    edit_dist_generic<SLNLP_EDIT_MAX_LEN, unsigned char, EDIT_NONE>(Xq, ldq, Lq, nq, Xr, ldr, Lr, nr, max_q, max_r, tile, dist);
}
SLNLP_ZKERNEL(edit_dist_kernel, 256, edit_dist_body)

// ------------------------------------------------------------------------------------------------------- selection ----
// the shared body (edit_shared.hpp) over the uint8 matrix, its 65 bins a compile-time constant
__device__ __forceinline__ void edit_select_body(const unsigned char* __restrict__ dist, const int64_t* __restrict__ Lq,
                                                 const int64_t* __restrict__ exclude, int nq, int nr, int max_q, int k, int radius,
                                                 int* __restrict__ rows, int* __restrict__ nbr) {
    edit_select_generic<unsigned char, EDIT_NONE, EDIT_BINS, true>(dist, Lq, exclude, nq, nr, max_q, k, radius, EDIT_BINS, rows, nbr);
}
SLNLP_ZKERNEL(edit_select_kernel, 256, edit_select_body)

__device__ __forceinline__ void edit_head_body(const int64_t* __restrict__ Lq, int nq, int max_q, const int64_t* __restrict__ Lr, int nr,
                                               int max_r, int64_t* __restrict__ head) {
    __shared__ int part[2][256];
    const int tid = threadIdx.x;
    const long n = nq > nr ? nq : nr;
    block_sum_rows<2>(part, tid, n, [&](long i, int* acc) {
        if (i < nq) acc[0] += (Lq[i] < 0 || Lq[i] > max_q) ? 1 : 0;
        if (i < nr) acc[1] += (Lr[i] < 0 || Lr[i] > max_r) ? 1 : 0;
    });
    if (tid < 8) head[tid] = tid < 2 ? (int64_t)part[tid][0] : 0;
}
SLNLP_ZKERNEL(edit_head_kernel, 256, edit_head_body)

// ----------------------------------------------------------------------------------------------------------- votes ----
// the reference label of neighbour j of query q, or -1: outside the list, an index or a distance no selection writes (never used
// as an address), a label outside the classes.  *d and *idx: the pair.  bound: the largest distance of the metric (64, or 64 F)
__device__ __forceinline__ int edit_neighbour_label(const int* __restrict__ nbr, const int64_t* __restrict__ yr, long q, int j, int k, int nr, int V,
                                                    int bound, int* d, int* idx, bool* listed) {
    *d = nbr[(q * k + j) * 2];
    *idx = nbr[(q * k + j) * 2 + 1];
    *listed = *idx >= 0 && *idx < nr && *d >= 0 && *d <= bound;
    if (!*listed) return -1;
    const int64_t y = yr[*idx];
    return (y >= 0 && y < V) ? (int)y : -1;
}
__device__ __forceinline__ int edit_found(const int* __restrict__ rows, long q, int k) {
    const int f = rows[4 * q];
    return f < 0 ? 0 : (f > k ? k : f);
}

__device__ __forceinline__ void edit_logp_body(const int* __restrict__ nbr, const int* __restrict__ rows, const int64_t* __restrict__ Lq,
                                               const int64_t* __restrict__ Lr, const int64_t* __restrict__ yr, int nq, int nr, int k, int V,
                                               int weights, double tau, int normalize, double lam, const double* __restrict__ prior,
                                               float* __restrict__ logp, long ld, int bound, int unit) {
    __shared__ double wj[4][64];
    __shared__ int lab[4][64];
    const int w = threadIdx.x >> 6;
    wave_rows<int>(nq, [&](int q, int lane) {
        float* out = logp + (long)q * ld;
        if (rows[4 * (long)q + 3] & SLNLP_EDIT_CODE_QUERY) {     // wave-uniform: reported, not patched
            for (int c = lane; c < V; c += 64) out[c] = __builtin_nanf("");
            return;
        }
        const int found = edit_found(rows, q, k);
        double wt = 0.0;
        int y = -1;
        if (lane < found) {
            int d, idx;
            bool listed;
            y = edit_neighbour_label(nbr, yr, q, lane, k, nr, V, bound, &d, &idx, &listed);
            if (y >= 0) {
                wt = 1.0;
                if (weights == SLNLP_EDIT_DISTANCE) {
                    int64_t frames = 1;                      // n = unit * frames: tau is in frames in both metrics (unit 1: n as ever)
                    if (normalize) {
                        const int64_t a = Lq[q], b = Lr[idx];
                        const int64_t mx = a > b ? a : b;
                        frames = mx > 1 ? mx : 1;
                    }
                    const double n = (double)(frames * unit);
                    wt = exp(-(double)d / (tau * n));
                }
            }
        }
        wj[w][lane] = wt;
        lab[w][lane] = y;
        wave_lds_sync();
        double W = 0.0;
        for (int j = 0; j < found; ++j) {
            if (lab[w][j] >= 0) W += wj[w][j];
        }
        const double den = W + lam;
        for (int c = lane; c < V; c += 64) {
            double s = 0.0;
            for (int j = 0; j < found; ++j) {
                if (lab[w][j] == c) s += wj[w][j];
            }
            const double p = (s + lam * prior[c]) / den;
            out[c] = (float)log(p);
        }
        wave_lds_sync();
    });
}
SLNLP_ZKERNEL(edit_logp_kernel, 256, edit_logp_body)

__device__ __forceinline__ void edit_bad_body(const int* __restrict__ nbr, const int* __restrict__ rows, const int64_t* __restrict__ yr, int nq,
                                              int nr, int k, int V, int bound, int64_t* __restrict__ head) {
    __shared__ long long part[256];
    const int tid = threadIdx.x;
    block_sum_rows<1>(&part, tid, (long)nq * k, [&](long g, long long* acc) {
        const long q = g / k;
        const int j = (int)(g - q * k);
        if ((rows[4 * q + 3] & SLNLP_EDIT_CODE_QUERY) || j >= edit_found(rows, q, k)) return;
        int d, idx;
        bool listed;
        const int y = edit_neighbour_label(nbr, yr, q, j, k, nr, V, bound, &d, &idx, &listed);
        acc[0] += (listed && y < 0) ? 1 : 0;
    });
    if (tid == 0) head[EDIT_HEAD_BAD_LABELS] = (int64_t)part[0];
}
SLNLP_ZKERNEL(edit_bad_kernel, 256, edit_bad_body)

// ------------------------------------------------------------------------------------------------------- host side ----
int edit_launch_head(const char* what, const int64_t* Lq, int64_t nq, int max_q, const int64_t* Lr, int64_t nr, int max_r, int64_t* head, hipStream_t st) {
    return zlaunch(edit_head_kernel, dim3(1), 256, 0, st, what, Lq, (int)nq, max_q, Lr, (int)nr, max_r, head);
}

// what this search states: a uint8 matrix, the distances 0 .. 64
static EditSearch edit_search(const char* what) {
    return EditSearch{what, "edit_knn_distances", "edit_knn_select", "edit_knn_head", 1, SLNLP_EDIT_MAX_LEN, "64", Span{}};
}

int edit_launch_logp(const char* what, const char* what_head, int bound, int unit, const int32_t* nbr, const int32_t* rows, const int64_t* Lq,
                     const int64_t* Lr, const int64_t* yr, int64_t nq, int64_t nr, int64_t k, int64_t V, int weights, double tau, int normalize,
                     double lam, const double* prior, float* logp, int64_t ld, int64_t* head, hipStream_t st) {
    SLNLP_CHECK_ARG(nbr && rows && Lq && Lr && yr && prior && logp && head, "%s: null pointer", what);
    SLNLP_CHECK_ARG(nq >= 1 && nq <= SLNLP_EDIT_MAX_ROWS, "%s: nq=%ld outside 1..%d", what, (long)nq, SLNLP_EDIT_MAX_ROWS);
    SLNLP_CHECK_ARG(nr >= 1 && nr <= SLNLP_EDIT_MAX_ROWS, "%s: nr=%ld outside 1..%d", what, (long)nr, SLNLP_EDIT_MAX_ROWS);
    SLNLP_CHECK_ARG(k >= 1 && k <= SLNLP_EDIT_MAX_K, "%s: k=%ld outside 1..%d", what, (long)k, SLNLP_EDIT_MAX_K);
    SLNLP_CHECK_ARG(V >= 1 && V <= INT_MAX, "%s: V=%ld outside 1..%d", what, (long)V, INT_MAX);
    SLNLP_CHECK_ARG(weights == SLNLP_EDIT_UNIFORM || weights == SLNLP_EDIT_DISTANCE, "%s: weights=%d, expected 0 (uniform) or 1 (distance)", what, weights);
    SLNLP_CHECK_ARG(normalize == 0 || normalize == 1, "%s: normalize=%d, expected 0 or 1", what, normalize);
    SLNLP_CHECK_ARG(tau > 0.0 && tau < (double)INFINITY, "%s: tau=%g, expected a finite number > 0", what, tau);
    SLNLP_CHECK_ARG(lam > 0.0 && lam < (double)INFINITY, "%s: lam=%g, expected a finite number > 0", what, lam);
    Span z;
    SLNLP_TRY(check_out_matrix(what, logp, nq, "nq", V, ld, &z));
    z.name = "logp";
    SLNLP_CHECK_ARG((((uintptr_t)nbr | (uintptr_t)rows | (uintptr_t)logp) & 3) == 0 &&
                    (((uintptr_t)Lq | (uintptr_t)Lr | (uintptr_t)yr | (uintptr_t)prior | (uintptr_t)head) & 7) == 0,
                    "%s: misaligned pointer (nbr, rows, logp: 4 bytes; Lq, Lr, yr, prior, head: 8 bytes)", what);
    const Span in[6] = {{nbr, (size_t)nq * (size_t)k * 8, "nbr"}, {rows, (size_t)nq * 16, "rows"}, {Lq, (size_t)nq * 8, "Lq"},
                        {Lr, (size_t)nr * 8, "Lr"}, {yr, (size_t)nr * 8, "yr"}, {prior, (size_t)V * 8, "prior"}};
    const Span out[2] = {z, {head, SLNLP_EDIT_HEAD_BYTES, "head"}};
    SLNLP_TRY(check_no_overlap(what, out, in));
    SLNLP_TRY(zlaunch(edit_logp_kernel, dim3(wave_rows_grid(nq)), 256, 0, st, what, (const int*)nbr, (const int*)rows, Lq, Lr, yr, (int)nq, (int)nr, (int)k,
                      (int)V, weights, tau, normalize, lam, prior, logp, (long)ld, bound, unit));
    return zlaunch(edit_bad_kernel, dim3(1), 256, 0, st, what_head, (const int*)nbr, (const int*)rows, yr, (int)nq, (int)nr, (int)k, (int)V, bound, head);
}

}  // namespace slnlp

extern "C" int slnlp_edit_distances(const int64_t* Xq, int64_t ldq, const int64_t* Lq, int64_t nq, const int64_t* Xr, int64_t ldr, const int64_t* Lr,
                                    int64_t nr, uint8_t* dist, void* stream) {
    using namespace slnlp;
    const hipStream_t st = (hipStream_t)stream;
    const EditSearch s = edit_search("edit_distances");
    EditSide Q, R;
    SLNLP_TRY(edit_check_side(s.what, "query", Xq, ldq, Lq, nq, SLNLP_EDIT_MAX_LEN, &Q));
    SLNLP_TRY(edit_check_side(s.what, "reference", Xr, ldr, Lr, nr, SLNLP_EDIT_MAX_LEN, &R));
    return edit_search_distances(s, Q, R, dist,
                                 [&](const char* what, void* d) { return edit_launch_dist(edit_dist_kernel, what, Q, R, (unsigned char*)d, st); });
}
extern "C" int64_t slnlp_edit_knn_scratch_bytes(int64_t nq, int64_t nr) { return slnlp::edit_scratch_bytes("edit_knn_scratch_bytes", nq, nr, 1); }
extern "C" int slnlp_edit_knn_rows(const int64_t* Xq, int64_t ldq, const int64_t* Lq, int64_t nq, const int64_t* Xr, int64_t ldr, const int64_t* Lr,
                                   int64_t nr, const int64_t* exclude, int64_t k, int64_t radius, void* scratch, int64_t scratch_bytes, int64_t* head,
                                   int32_t* rows, int32_t* nbr, void* stream) {
    using namespace slnlp;
    const hipStream_t st = (hipStream_t)stream;
    const EditSearch s = edit_search("edit_knn_rows");
    EditSide Q, R;
    SLNLP_TRY(edit_check_side(s.what, "query", Xq, ldq, Lq, nq, SLNLP_EDIT_MAX_LEN, &Q));
    SLNLP_TRY(edit_check_side(s.what, "reference", Xr, ldr, Lr, nr, SLNLP_EDIT_MAX_LEN, &R));
    return edit_search_rows(
        s, Q, R, exclude, k, radius, scratch, scratch_bytes, head, rows, nbr, st,
        [&](const char* what, void* d) { return edit_launch_dist(edit_dist_kernel, what, Q, R, (unsigned char*)d, st); },
        [&](const char* what, void* d) {
            return zlaunch(edit_select_kernel, dim3(wave_rows_grid(nq)), 256, 0, st, what, (const unsigned char*)d, Lq, exclude, (int)nq, (int)nr,
                           Q.max_len, (int)k, (int)radius, (int*)rows, (int*)nbr);
        });
}
extern "C" int slnlp_edit_knn_logp(const int32_t* nbr, const int32_t* rows, const int64_t* Lq, const int64_t* Lr, const int64_t* yr, int64_t nq, int64_t nr,
                                   int64_t k, int64_t V, int weights, double tau, int normalize, double lam, const double* prior, float* logp, int64_t ld,
                                   int64_t* head, void* stream) {
    return slnlp::edit_launch_logp("edit_knn_logp", "edit_knn_logp_head", SLNLP_EDIT_MAX_LEN, 1, nbr, rows, Lq, Lr, yr, nq, nr, k, V, weights, tau,
                                   normalize, lam, prior, logp, ld, head, (hipStream_t)stream);
}
