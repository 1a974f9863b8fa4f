// edit_long.hip -- edit_knn.hip's search for rows of up to 512 frames (slnlp.EditKNN(max_len=...), slnlp.split_audit(max_len=...);
// DESIGN.md section 4): all-pairs unit-cost Levenshtein distances by Myers' bit-vector recurrence in its MULTI-WORD form
// (edit_myers_multi.hpp), the query in 1 .. 8 64-bit words.  include/slnlp.h states the definitions and the buffers;
// tests/edit_long_ref.py restates them in numpy.  This file owns the two instantiations that are the long search's alone (the
// distance and the selection kernel over uint16) and its entry points; the checks and the launch order are edit_shared.hpp's shell.
//
// Rows and buffers are those of edit_knn.hip, but a row is USABLE when its length lies in 0 .. min(max_len, its row stride), max_len
// (1 .. SLNLP_EDIT_LONG_MAX_LEN = 512) a launch argument: only the first L tokens of a usable row are read, nothing of an unusable one
// is -- a row longer than max_len is refused, never truncated -- and tokens are compared as full int64 values.  EVERYTHING IS INTEGER
// until the votes and there are no atomics on global memory: each result is a pure function of the arguments, whatever the grid, the
// stream or the kernels beside it.
//
//   edit_long_dist    edit_dist.hpp's body -- written once for this search and edit_knn.hip's -- for queries of up to 512 frames: 8
//                     mask words per position behind a 1024-slot open hash, 40960 bytes of LDS a block (four blocks share a CU's
//                     160 KiB), and per query one branch to the loop built for the smallest W >= ceil(m / 64) of 1, 2, 3, 4, 6, 8
//                     words (no scratch memory: profiles/edit_long_timing.json lists the register counts;
//                     -DSLNLP_EDIT_LONG_ONLY_W=W builds one loop alone).  uint16 [nq, nr]; 65535 where either row is unusable.
//   edit_long_select  edit_shared.hpp's selection body over the uint16 matrix with max_len + 1 <= 513 bins.
//   the head and the votes are edit_knn.hip's kernels with the bound max_len and the unit 1.
#include <limits.h>
#include <stdio.h>

#include "common.hpp"
#include "edit_dist.hpp"
#include "edit_shared.hpp"
#include "launch.hpp"
#include "spans.hpp"

namespace slnlp {

constexpr int LONG_NONE = 65535;                             // the matrix entry of a pair with an unusable row
constexpr int LONG_BINS_CAP = SLNLP_EDIT_LONG_MAX_LEN + 1;   // the distances 0 .. 512

// ------------------------------------------------------------------------------------------------------- distances ----
// the shared body (edit_dist.hpp) for queries of up to 512 frames over the uint16 matrix: 8 mask words, a 1024-slot hash, 40960 bytes of LDS
__device__ __forceinline__ void edit_long_dist_body(const int64_t* __restrict__ Xq, long ldq, const int64_t* __restrict__ Lq, int nq,
                                                    const int64_t* __restrict__ Xr, long ldr, const int64_t* __restrict__ Lr, int nr, int max_q,
                                                    int max_r, int tile, unsigned short* __restrict__ dist) {
    edit_dist_generic<SLNLP_EDIT_LONG_MAX_LEN, unsigned short, LONG_NONE>(Xq, ldq, Lq, nq, Xr, ldr, Lr, nr, max_q, max_r, tile, dist);
}
SLNLP_ZKERNEL(edit_long_dist_kernel, 256, edit_long_dist_body)

// ------------------------------------------------------------------------------------------------------- selection ----
__device__ __forceinline__ void edit_long_select_body(const unsigned short* __restrict__ dist, const int64_t* __restrict__ Lq,
                                                      const int64_t* __restrict__ exclude, int nq, int nr, int max_q, int k, int radius, int bins,
                                                      int* __restrict__ rows, int* __restrict__ nbr) {
    edit_select_generic<unsigned short, LONG_NONE, LONG_BINS_CAP, false>(dist, Lq, exclude, nq, nr, max_q, k, radius, bins, rows, nbr);
}
SLNLP_ZKERNEL(edit_long_select_kernel, 256, edit_long_select_body)

// ------------------------------------------------------------------------------------------------------- host side ----
static int edit_long_check_max_len(const char* what, int64_t max_len) {
    SLNLP_CHECK_ARG(max_len >= 1 && max_len <= SLNLP_EDIT_LONG_MAX_LEN, "%s: max_len=%ld outside 1..%d", what, (long)max_len, SLNLP_EDIT_LONG_MAX_LEN);
    return 0;
}
// what this search states: a uint16 matrix, the distances 0 .. max_len; says: room for "max_len=512"
static EditSearch edit_long_search(const char* what, int64_t max_len, char (&says)[32]) {
    snprintf(says, sizeof says, "max_len=%ld", (long)max_len);
    return EditSearch{what, "edit_long_knn_distances", "edit_long_knn_select", "edit_long_knn_head", 2, max_len, says, Span{}};
}

}  // namespace slnlp

extern "C" int slnlp_edit_long_distances(const int64_t* Xq, int64_t ldq, const int64_t* Lq, int64_t nq, const int64_t* Xr, int64_t ldr, const int64_t* Lr,
                                         int64_t nr, int64_t max_len, uint16_t* dist, void* stream) {
    using namespace slnlp;
    const hipStream_t st = (hipStream_t)stream;
    char says[32];
    const EditSearch s = edit_long_search("edit_long_distances", max_len, says);
    EditSide Q, R;
    SLNLP_TRY(edit_long_check_max_len(s.what, max_len));
    SLNLP_TRY(edit_check_side(s.what, "query", Xq, ldq, Lq, nq, max_len, &Q));
    SLNLP_TRY(edit_check_side(s.what, "reference", Xr, ldr, Lr, nr, max_len, &R));
    return edit_search_distances(s, Q, R, dist,
                                 [&](const char* what, void* d) { return edit_launch_dist(edit_long_dist_kernel, what, Q, R, (unsigned short*)d, st); });
}
extern "C" int64_t slnlp_edit_long_knn_scratch_bytes(int64_t nq, int64_t nr) {
    return slnlp::edit_scratch_bytes("edit_long_knn_scratch_bytes", nq, nr, 2);
}
extern "C" int slnlp_edit_long_knn_rows(const int64_t* Xq, int64_t ldq, const int64_t* Lq, int64_t nq, const int64_t* Xr, int64_t ldr, const int64_t* Lr,
                                        int64_t nr, int64_t max_len, const int64_t* exclude, int64_t k, int64_t radius, void* scratch,
                                        int64_t scratch_bytes, int64_t* head, int32_t* rows, int32_t* nbr, void* stream) {
    using namespace slnlp;
    const hipStream_t st = (hipStream_t)stream;
    char says[32];
    const EditSearch s = edit_long_search("edit_long_knn_rows", max_len, says);
    EditSide Q, R;
    SLNLP_TRY(edit_long_check_max_len(s.what, max_len));
    SLNLP_TRY(edit_check_side(s.what, "query", Xq, ldq, Lq, nq, max_len, &Q));
    SLNLP_TRY(edit_check_side(s.what, "reference", Xr, ldr, Lr, nr, max_len, &R));
    return edit_search_rows(
        s, Q, R, exclude, k, radius, scratch, scratch_bytes, head, rows, nbr, st,
        [&](const char* what, void* d) { return edit_launch_dist(edit_long_dist_kernel, what, Q, R, (unsigned short*)d, st); },
        [&](const char* what, void* d) {
            return zlaunch(edit_long_select_kernel, dim3(wave_rows_grid(nq)), 256, 0, st, what, (const unsigned short*)d, Lq, exclude, (int)nq,
                           (int)nr, Q.max_len, (int)k, (int)radius, (int)max_len + 1, (int*)rows, (int*)nbr);
        });
}
extern "C" int slnlp_edit_long_knn_logp(const int32_t* nbr, const int32_t* rows, const int64_t* Lq, const int64_t* Lr, const int64_t* yr, int64_t nq,
                                        int64_t nr, int64_t k, int64_t V, int64_t max_len, int weights, double tau, int normalize, double lam,
                                        const double* prior, float* logp, int64_t ld, int64_t* head, void* stream) {
    using namespace slnlp;
    const char* what = "edit_long_knn_logp";
    SLNLP_TRY(edit_long_check_max_len(what, max_len));
    return edit_launch_logp(what, "edit_long_knn_logp_head", (int)max_len, 1, nbr, rows, Lq, Lr, yr, nq, nr, k, V, weights, tau, normalize, lam, prior, logp,
                            ld, head, (hipStream_t)stream);
}
