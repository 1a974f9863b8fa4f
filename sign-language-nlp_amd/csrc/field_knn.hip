// field_knn.hip -- the phonology-weighted edit distance between two sets of token rows and the k nearest references of every query,
// on the device (slnlp.PhonoKNN, slnlp.split_audit(field_codes=...)).  A token of this data is a composition
// of F phonological fields; substituting one frame for another costs the number of fields in which they differ, inserting or
// deleting a frame costs gap.  include/slnlp.h states the definitions; tests/field_knn_ref.py restates them in numpy.
//
// Rows, usability and the buffers are those of edit_knn.hip; codes int32 [Vt, F] holds the per-field value ids of token id v in row
// v.  EVERYTHING IS INTEGER until the votes and there are no atomics on global memory: each result is a pure function of the
// arguments, whatever the grid, the stream or the kernels beside it.
//
//   field_dist    a block per query (queries over a grid-stride loop; with few queries the references in tiles over grid.y, as
//                 edit_dist).  The query's tokens, their "outside the table" flags and their code vectors -- padded with zeros to 16
//                 entries -- go to LDS once per block and query.  Thread t then runs the weighted recurrence (field_edit.hpp) over
//                 the references t, t + 256, ...: per reference token its code vector into 4 G registers (fixed indices: the kernel
//                 is built for G = (F + 3) / 4 = 1, 2, 3 and 4 groups of four fields, so a cell is straight-line code and its
//                 LDS reads are all in flight before the first compare) and one column step.  THE COLUMN lives transposed in LDS,
//                 col[word][thread] with two uint16 positions per dword: 32 x 256 dwords = 32 KiB, 37.6 KiB a block with the query.
//                 A wave's 64 lanes read and write 64 consecutive dwords (every bank once: no conflict), the query's entries are
//                 read at one address by all lanes (a broadcast).  uint16 [nq, nr]; 65535 where either row is unusable.
//   field_dist_w  the same body under PER-FIELD WEIGHTS (slnlp_field_distances_w / _knn_rows_w): field f counts w[f] (0..16, their
//                 sum W in 1..16), a token outside the table costs W, gap lies in 1..W, d <= 64 W.  The weights travel BY VALUE among
//                 the kernel's arguments (FieldWeights, 16 ints): uniform values in scalar registers, no table read for them.  The
//                 unweighted kernels are not routed through it: the cost policy is a template argument of the one body.
//   field_select  edit_shared.hpp's selection body over the uint16 matrix with 64 F + 1 <= 1025 bins.
//   the head and the votes are edit_knn.hip's kernels with the bound 64 F and the unit F.
// Host side: this file checks the table and the weights (field_check_metric) and states the search (its names, two bytes a pair, the
// bound 64 F or 64 W, the table as one more input); every other check and the launch order are edit_shared.hpp's shell.
#include <limits.h>
#include <stdio.h>

#include "common.hpp"
#include "edit_shared.hpp"
#include "field_edit.hpp"
#include "launch.hpp"
#include "spans.hpp"

namespace slnlp {

constexpr int FIELD_NONE = 65535;                                            // the matrix entry of a pair with an unusable row
constexpr int FIELD_BINS_CAP = SLNLP_EDIT_MAX_LEN * SLNLP_FIELD_MAX_FIELDS + 1;   // the distances 0 .. 1024
static_assert(FIELD_MAX == SLNLP_FIELD_MAX_FIELDS && FIELD_WORDS * 2 == SLNLP_EDIT_MAX_LEN, "field_edit.hpp and slnlp.h disagree");

// a thread's column: word p of thread t at col[p][t]
struct FieldLdsColumn {
    unsigned* base;
    __device__ __forceinline__ unsigned load(int p) const { return base[p * 256]; }
    __device__ __forceinline__ void store(int p, unsigned w) const { base[p * 256] = w; }
};

// ------------------------------------------------------------------------------------------------------- distances ----
// what a substitution between two tokens of the table costs, and what a token outside it costs: the unit metric counts the
// differing fields (F outside), the weighted one adds their weights (W outside).  The body below is written once over the two.
struct FieldUnitCost {
    int F;
    template <int G, class A, class B>
    __device__ __forceinline__ int differ(const A& a, const B& b) const { return field_differ_groups<G>(a, b); }
    __device__ __forceinline__ int outside() const { return F; }
};
struct FieldWeightedCost {
    FieldWeights fw;
    int W;
    template <int G, class A, class B>
    __device__ __forceinline__ int differ(const A& a, const B& b) const { return field_weigh_groups<G>(a, b, fw); }
    __device__ __forceinline__ int outside() const { return W; }
};

template <int G, class Cost>
__device__ __forceinline__ void field_dist_impl(const int64_t* __restrict__ Xq, long ldq, const int64_t* __restrict__ Lq, int nq,
                                                const int64_t* __restrict__ Xr, long ldr, const int64_t* __restrict__ Lr, int nr, int max_q,
                                                int max_r, int tile, const int* __restrict__ codes, int F, int Vt, int gap,
                                                unsigned short* __restrict__ dist, const Cost cost) { // (F + 3) / 4 == G
    __shared__ int64_t qtok[SLNLP_EDIT_MAX_LEN];
    __shared__ int qout[SLNLP_EDIT_MAX_LEN];
    __shared__ __attribute__((aligned(16))) int qcode[SLNLP_EDIT_MAX_LEN][FIELD_MAX];
    __shared__ unsigned col[FIELD_WORDS][256];
    const int tid = threadIdx.x;
    const FieldLdsColumn column{&col[0][tid]};
    const long j_begin = (long)blockIdx.y * tile;
    const int j_end = (int)(j_begin + tile < nr ? j_begin + tile : nr);
    for (int q = blockIdx.x; q < nq; q += gridDim.x) {       // q, lq, m: the same in every thread, so is every branch on them
        const int64_t lq = Lq[q];
        unsigned short* out = dist + (long)q * nr;
        if (lq < 0 || lq > max_q) {                          // reads nothing more
            for (int j = (int)j_begin + tid; j < j_end; j += 256) out[j] = (unsigned short)FIELD_NONE;
            continue;
        }
        const int m = (int)lq;
        const int words = (m + 1) >> 1;
        __syncthreads();                                     // the reads of the block's previous query are over
        // 64 positions x 16 entries: zeros behind the query's length, behind F and for a token outside the table (never looked up)
        for (int i = tid; i < SLNLP_EDIT_MAX_LEN * FIELD_MAX; i += 256) {
            const int j = i >> 4, f = i & (FIELD_MAX - 1);
            int v = 0;
            if (j < m && f < F) {
                const int64_t c = Xq[(long)q * ldq + j];
                if (c >= 0 && c < Vt) v = codes[c * F + f];
            }
            qcode[j][f] = v;
        }
        if (tid < SLNLP_EDIT_MAX_LEN) {
            const int64_t c = tid < m ? Xq[(long)q * ldq + tid] : 0;
            qtok[tid] = c;
            qout[tid] = (c >= 0 && c < Vt) ? 0 : 1;
        }
        __syncthreads();
        for (int j = (int)j_begin + tid; j < j_end; j += 256) {
            const int64_t lr = Lr[j];
            int d;
            if (lr < 0 || lr > max_r) {
                d = FIELD_NONE;
            } else {
                const int64_t* row = Xr + (long)j * ldr;
                const int n = (int)lr;
                field_column_begin(column, words, gap);
                for (int t = 0; t < n; ++t) {
                    const int64_t c = row[t];
                    const bool inside = c >= 0 && c < Vt;
                    int rc[4 * G];
#pragma unroll
                    for (int f = 0; f < 4 * G; ++f) rc[f] = (inside && f < F) ? codes[c * F + f] : 0;
                    field_column_step(column, words, t + 1, gap, [&](int p) {
                        return field_sub(qtok[p] == c, (qout[p] != 0) | !inside, cost.template differ<G>(qcode[p], rc), cost.outside());
                    });
                }
                d = field_column_score(column, m, n, gap);
            }
            out[j] = (unsigned short)d;
        }
    }
}
#define SLNLP_FIELD_DIST(G)                                                                                                                \
    __device__ __forceinline__ void field_dist_body_g##G(const int64_t* __restrict__ Xq, long ldq, const int64_t* __restrict__ Lq, int nq,  \
                                                         const int64_t* __restrict__ Xr, long ldr, const int64_t* __restrict__ Lr, int nr,  \
                                                         int max_q, int max_r, int tile, const int* __restrict__ codes, int F, int Vt,      \
                                                         int gap, unsigned short* __restrict__ dist) {                                      \
        field_dist_impl<G>(Xq, ldq, Lq, nq, Xr, ldr, Lr, nr, max_q, max_r, tile, codes, F, Vt, gap, dist, FieldUnitCost{F});                \
    }                                                                                                                                      \
    SLNLP_ZKERNEL(field_dist_kernel_g##G, 256, field_dist_body_g##G)                                                                       \
    __device__ __forceinline__ void field_dist_w_body_g##G(const int64_t* __restrict__ Xq, long ldq, const int64_t* __restrict__ Lq, int nq, \
                                                           const int64_t* __restrict__ Xr, long ldr, const int64_t* __restrict__ Lr, int nr, \
                                                           int max_q, int max_r, int tile, const int* __restrict__ codes, int F, int Vt,    \
                                                           int gap, unsigned short* __restrict__ dist, FieldWeights fw, int W) {            \
        field_dist_impl<G>(Xq, ldq, Lq, nq, Xr, ldr, Lr, nr, max_q, max_r, tile, codes, F, Vt, gap, dist, FieldWeightedCost{fw, W});        \
    }                                                                                                                                      \
    SLNLP_ZKERNEL(field_dist_w_kernel_g##G, 256, field_dist_w_body_g##G)
SLNLP_FIELD_DIST(1)
SLNLP_FIELD_DIST(2)
SLNLP_FIELD_DIST(3)
SLNLP_FIELD_DIST(4)
#undef SLNLP_FIELD_DIST

// ------------------------------------------------------------------------------------------------------- selection ----
__device__ __forceinline__ void field_select_body(const unsigned short* __restrict__ dist, const int64_t* __restrict__ Lq,
                                                  const int64_t* __restrict__ exclude, int nq, int nr, int max_q, int k, int radius, int bins,
                                                  int* __restrict__ rows, int* __restrict__ nbr) {
    edit_select_generic<unsigned short, FIELD_NONE, FIELD_BINS_CAP, false>(dist, Lq, exclude, nq, nr, max_q, k, radius, bins, rows, nbr);
}
SLNLP_ZKERNEL(field_select_kernel, 256, field_select_body)

// ------------------------------------------------------------------------------------------------------- host side ----
// what a field search checks behind its sides and then states: the table -- codes 4-byte aligned, F in 1..16, Vt in 1..INT32_MAX --
// and the metric's unit, which bounds the gap (1..unit) and the distances (0..64 unit).  Unweighted (fweights unused) the unit is F;
// weighted, fweights is a HOST array of F ints in 0..16 and the unit their sum W in 1..16.
struct FieldMetric {
    const int32_t* codes;
    int64_t Vt, F, gap;
    bool weighted;
    FieldWeights fw;
    int unit;
    char says[32];                                           // of the radius refusal: "64 F=384"
};
static int field_check_metric(const char* what, const int32_t* codes, int64_t Vt, int64_t F, const int32_t* fweights, bool weighted, int64_t gap,
                              FieldMetric* out, Span* table) {
    SLNLP_CHECK_ARG(codes, "%s: null pointer (codes)", what);
    if (weighted) SLNLP_CHECK_ARG(fweights, "%s: null pointer (fweights: a host array of F weights)", what);
    SLNLP_CHECK_ARG(F >= 1 && F <= SLNLP_FIELD_MAX_FIELDS, "%s: F=%ld outside 1..%d", what, (long)F, SLNLP_FIELD_MAX_FIELDS);
    SLNLP_CHECK_ARG(Vt >= 1 && Vt <= INT_MAX, "%s: Vt=%ld outside 1..%d", what, (long)Vt, INT_MAX);
    *out = FieldMetric{codes, Vt, F, gap, weighted, FieldWeights{}, (int)F, ""};
    if (weighted) {
        int W = 0;
        for (int f = 0; f < F; ++f) {
            SLNLP_CHECK_ARG(fweights[f] >= 0 && fweights[f] <= SLNLP_FIELD_MAX_WEIGHT, "%s: fweights[%d]=%d outside 0..%d", what, f, (int)fweights[f],
                            SLNLP_FIELD_MAX_WEIGHT);
            out->fw.w[f] = fweights[f];
            W += fweights[f];
        }
        SLNLP_CHECK_ARG(W >= 1 && W <= SLNLP_FIELD_MAX_WEIGHT, "%s: the weights sum to W=%d outside 1..%d", what, W, SLNLP_FIELD_MAX_WEIGHT);
        out->unit = W;
    }
    const char* unit_name = weighted ? "W" : "F";
    SLNLP_CHECK_ARG(gap >= 1 && gap <= out->unit, "%s: gap=%ld outside 1..%s=%d", what, (long)gap, unit_name, out->unit);
    SLNLP_CHECK_ARG(((uintptr_t)codes & 3) == 0, "%s: misaligned pointer (codes: 4 bytes)", what);
    snprintf(out->says, sizeof out->says, "64 %s=%d", unit_name, SLNLP_EDIT_MAX_LEN * out->unit);
    *table = Span{codes, (size_t)Vt * (size_t)F * 4, "codes"};
    return 0;
}
static int launch_field_dist(const char* what, const EditSide& Q, const EditSide& R, const FieldMetric& m, unsigned short* dist, hipStream_t st) {
    int tile;
    const dim3 grid = edit_dist_grid(Q.n, R.n, &tile);
    const int groups = (int)(m.F + 3) / 4;                   // 1..4: the kernel built for that many groups of four fields
    if (m.weighted) {                                        // the weighted sibling: the weights by value behind the same arguments
        auto kern = groups == 1 ? field_dist_w_kernel_g1 : groups == 2 ? field_dist_w_kernel_g2 : groups == 3 ? field_dist_w_kernel_g3 : field_dist_w_kernel_g4;
        return zlaunch(kern, grid, 256, 0, st, what, Q.X, (long)Q.ld, Q.L, (int)Q.n, R.X, (long)R.ld, R.L, (int)R.n, Q.max_len, R.max_len, tile,
                       (const int*)m.codes, (int)m.F, (int)m.Vt, (int)m.gap, dist, m.fw, m.unit);
    }
    auto kern = groups == 1 ? field_dist_kernel_g1 : groups == 2 ? field_dist_kernel_g2 : groups == 3 ? field_dist_kernel_g3 : field_dist_kernel_g4;
    return zlaunch(kern, grid, 256, 0, st, what, Q.X, (long)Q.ld, Q.L, (int)Q.n, R.X, (long)R.ld, R.L, (int)R.n, Q.max_len, R.max_len, tile,
                   (const int*)m.codes, (int)m.F, (int)m.Vt, (int)m.gap, dist);
}

// the two kinds of call under either metric; names: the entry point and its three launches (*_distances: the entry point alone)
struct FieldNames {
    const char *what, *dist, *select, *head;
};
static int field_distances_any(const FieldNames& nm, const int64_t* Xq, int64_t ldq, const int64_t* Lq, int64_t nq, const int64_t* Xr, int64_t ldr,
                               const int64_t* Lr, int64_t nr, const int32_t* codes, int64_t Vt, int64_t F, const int32_t* fweights, bool weighted,
                               int64_t gap, uint16_t* dist, hipStream_t st) {
    EditSide Q, R;
    FieldMetric m;
    Span table;
    SLNLP_TRY(edit_check_side(nm.what, "query", Xq, ldq, Lq, nq, SLNLP_EDIT_MAX_LEN, &Q));
    SLNLP_TRY(edit_check_side(nm.what, "reference", Xr, ldr, Lr, nr, SLNLP_EDIT_MAX_LEN, &R));
    SLNLP_TRY(field_check_metric(nm.what, codes, Vt, F, fweights, weighted, gap, &m, &table));
    const EditSearch s{nm.what, nm.dist, nm.select, nm.head, 2, SLNLP_EDIT_MAX_LEN * (int64_t)m.unit, m.says, table};
    return edit_search_distances(s, Q, R, dist, [&](const char* what, void* d) { return launch_field_dist(what, Q, R, m, (unsigned short*)d, st); });
}

static int field_knn_rows_any(const FieldNames& nm, const int64_t* Xq, int64_t ldq, const int64_t* Lq, int64_t nq, const int64_t* Xr, int64_t ldr,
                              const int64_t* Lr, int64_t nr, const int32_t* codes, int64_t Vt, int64_t F, const int32_t* fweights, bool weighted,
                              int64_t gap, const int64_t* exclude, int64_t k, int64_t radius, void* scratch, int64_t scratch_bytes, int64_t* head,
                              int32_t* rows, int32_t* nbr, hipStream_t st) {
    EditSide Q, R;
    FieldMetric m;
    Span table;
    SLNLP_TRY(edit_check_side(nm.what, "query", Xq, ldq, Lq, nq, SLNLP_EDIT_MAX_LEN, &Q));
    SLNLP_TRY(edit_check_side(nm.what, "reference", Xr, ldr, Lr, nr, SLNLP_EDIT_MAX_LEN, &R));
    SLNLP_TRY(field_check_metric(nm.what, codes, Vt, F, fweights, weighted, gap, &m, &table));
    const EditSearch s{nm.what, nm.dist, nm.select, nm.head, 2, SLNLP_EDIT_MAX_LEN * (int64_t)m.unit, m.says, table};
    return edit_search_rows(
        s, Q, R, exclude, k, radius, scratch, scratch_bytes, head, rows, nbr, st,
        [&](const char* what, void* d) { return launch_field_dist(what, Q, R, m, (unsigned short*)d, st); },
        [&](const char* what, void* d) {
            return zlaunch(field_select_kernel, dim3(wave_rows_grid(nq)), 256, 0, st, what, (const unsigned short*)d, Lq, exclude, (int)nq, (int)nr,
                           Q.max_len, (int)k, (int)radius, (int)s.bound + 1, (int*)rows, (int*)nbr);
        });
}


}  // namespace slnlp

extern "C" int slnlp_field_distances(const int64_t* Xq, int64_t ldq, const int64_t* Lq, int64_t nq, const int64_t* Xr, int64_t ldr, const int64_t* Lr,
                                     int64_t nr, const int32_t* codes, int64_t Vt, int64_t F, int64_t gap, uint16_t* dist, void* stream) {
    return slnlp::field_distances_any({"field_distances"}, Xq, ldq, Lq, nq, Xr, ldr, Lr, nr, codes, Vt, F, nullptr, false, gap, dist, (hipStream_t)stream);
}
extern "C" int slnlp_field_distances_w(const int64_t* Xq, int64_t ldq, const int64_t* Lq, int64_t nq, const int64_t* Xr, int64_t ldr, const int64_t* Lr,
                                       int64_t nr, const int32_t* codes, int64_t Vt, int64_t F, const int32_t* fweights, int64_t gap, uint16_t* dist,
                                       void* stream) {
    return slnlp::field_distances_any({"field_distances_w"}, Xq, ldq, Lq, nq, Xr, ldr, Lr, nr, codes, Vt, F, fweights, true, gap, dist, (hipStream_t)stream);
}
extern "C" int64_t slnlp_field_knn_scratch_bytes(int64_t nq, int64_t nr) { return slnlp::edit_scratch_bytes("field_knn_scratch_bytes", nq, nr, 2); }
extern "C" int slnlp_field_knn_rows(const int64_t* Xq, int64_t ldq, const int64_t* Lq, int64_t nq, const int64_t* Xr, int64_t ldr, const int64_t* Lr,
                                    int64_t nr, const int32_t* codes, int64_t Vt, int64_t F, int64_t gap, const int64_t* exclude, int64_t k,
                                    int64_t radius, void* scratch, int64_t scratch_bytes, int64_t* head, int32_t* rows, int32_t* nbr, void* stream) {
    return slnlp::field_knn_rows_any({"field_knn_rows", "field_knn_distances", "field_knn_select", "field_knn_head"}, Xq, ldq, Lq, nq, Xr, ldr, Lr, nr, codes,
                                     Vt, F, nullptr, false, gap, exclude, k, radius, scratch, scratch_bytes, head, rows, nbr, (hipStream_t)stream);
}
extern "C" int slnlp_field_knn_rows_w(const int64_t* Xq, int64_t ldq, const int64_t* Lq, int64_t nq, const int64_t* Xr, int64_t ldr, const int64_t* Lr,
                                      int64_t nr, const int32_t* codes, int64_t Vt, int64_t F, const int32_t* fweights, int64_t gap,
                                      const int64_t* exclude, int64_t k, int64_t radius, void* scratch, int64_t scratch_bytes, int64_t* head,
                                      int32_t* rows, int32_t* nbr, void* stream) {
    return slnlp::field_knn_rows_any({"field_knn_rows_w", "field_knn_distances_w", "field_knn_select_w", "field_knn_head_w"}, Xq, ldq, Lq, nq, Xr, ldr, Lr,
                                     nr, codes, Vt, F, fweights, true, gap, exclude, k, radius, scratch, scratch_bytes, head, rows, nbr,
                                     (hipStream_t)stream);
}
extern "C" int slnlp_field_knn_logp(const int32_t* nbr, const int32_t* rows, const int64_t* Lq, const int64_t* Lr, const int64_t* yr, int64_t nq, int64_t nr,
                                    int64_t k, int64_t V, int64_t F, int weights, double tau, int normalize, double lam, const double* prior, float* logp,
                                    int64_t ld, int64_t* head, void* stream) {
    const char* what = "field_knn_logp";
    SLNLP_CHECK_ARG(F >= 1 && F <= SLNLP_FIELD_MAX_FIELDS, "%s: F=%ld outside 1..%d", what, (long)F, SLNLP_FIELD_MAX_FIELDS);
    return slnlp::edit_launch_logp(what, "field_knn_logp_head", (int)(SLNLP_EDIT_MAX_LEN * F), (int)F, nbr, rows, Lq, Lr, yr, nq, nr, k, V, weights, tau,
                                   normalize, lam, prior, logp, ld, head, (hipStream_t)stream);
}
