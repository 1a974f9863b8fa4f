// label_audit.hip -- the confident-learning audit of a set of labelled log-probs on the device (Northcutt, Jiang and Chuang 2021):
// per class a threshold on the self-confidence, per row the class it is confidently predicted as, the confident joint of (given
// label, confident class) with its most frequent off-diagonal cells, and the counts a report needs (LogProbJudge.label_issues;
// DESIGN.md section 4).  include/slnlp.h states the definitions and the buffer layout; tests/label_audit_ref.py restates them in
// numpy, line by line.  Also here: slnlp_scatter_logp, which assembles out-of-fold log-probs (slnlp.OutOfFold).
//
// z float32 log-probs [N, ld] (V columns used), y int64 [N], beta = beta_dev ? beta_dev[0] : 1; everything but z is fp64.  A row is
// USABLE when logp_row_argmax(...).finite holds (no NaN, a finite maximum: looked at first, code -2 otherwise) and its label lies in
// [0, V) (code -1 otherwise).  The probability of column c of row i is audit_prob() (logp_prob.hpp) on the row head of logp_row.hpp:
// 1 / s0 for a column at the maximum, exp(beta z_ic - a) / s0 for another -- topk_rows' and reliability_rows' bits.
//
// slnlp_label_audit queues a FIXED sequence of eight launches and never waits for the host:
//   audit_rows       one wave per row, four rows per block, rows over a grid-stride loop (wave_rows, common.hpp): pred, the
//                    self-confidence s = p_{i, y_i}, `other` = the probability of the first column other than y_i in score_beats'
//                    order (0 for V = 1), the normalised margin m = s - other, p_pred = 1 / s0 and the code.
//   audit_classes    one block of 256 threads per class c (prior_classes' grid and order): thread t adds s_i over its usable rows
//                    labelled c among t, t + 256, ... ascending, then block_reduce.hpp's fixed tree -- an order that depends on N
//                    alone; n_c the count, t_c = sum / n_c (n_c = 0: NaN, which compares false: nobody is confidently c).  With
//                    n_c = 1 the sum is s_i + 0 + ... and the division by 1.0 is exact, so that row's p >= t holds with equality.
//   audit_confident  one wave per row again: k_i = the first column with p_ic >= t_c in score_beats' order on z_i (-1: none) and the
//                    flags, bit 0 "k_i >= 0 and k_i != y_i" (the label issue), bit 1 "pred_i != y_i".  p_ic comes from the SAME
//                    statements as pass 1's s_i (the head is recomputed, not stored: its bits are a function of the row), which
//                    the n_c = 1 case depends on.  An unusable row gets k = -1 and no flag.
//   the joint        confusion.hip's own zero / count launches on (k, y): C[y_i][k_i] += 1, every other row -- k = -1, a bad label
//                    -- in the overflow cell; integer atomics, exact.  Then confusion_pairs' two stages: the M largest
//                    off-diagonal cells, the likely label swaps.
//   audit_summary    one block: usable rows, bad labels, NaN rows, usable rows without a confident class, issues, arg-max
//                    disagreements -- integer sums over a fixed tree.
// No floating-point atomics, no LDS beyond the trees, nothing depends on the grid or on timing: the result is a pure function of
// the arguments.
#include <limits.h>
#include <math.h>

#include "block_reduce.hpp"
#include "common.hpp"
#include "launch.hpp"
#include "logp_prob.hpp"
#include "logp_row.hpp"
#include "scale_row.hpp"
#include "spans.hpp"

// (audit_prob, the probability of a column given the row head, comes from logp_prob.hpp, included IN FRONT of the pragma below on
// purpose: it is formed under the compiler's default contraction, as topk_rows forms it.  Passes 1 and 3 both call it.)
// this file's own arithmetic (s - other, sum / n) is rounded operation by operation, as the restatement's numpy expressions are
#pragma clang fp contract(off)

namespace slnlp {

enum { AUDIT_USABLE = 0, AUDIT_BAD = 1, AUDIT_NAN = 2, AUDIT_UNCONFIDENT = 3, AUDIT_ISSUES = 4, AUDIT_DISAGREE = 5, AUDIT_COUNTS = 6 };

// the pieces of the buffer in bytes from its start (include/slnlp.h documents them); every piece is 8-byte aligned
struct AuditLayout {
    size_t t, s, m, n, joint, pairs, k, code, flags, pred, other, p_pred, work, total;
};
static size_t audit_even(size_t ints) { return (ints + (ints & 1)) * 4; }
static AuditLayout audit_layout(int64_t N, int64_t V, int M, size_t work_bytes) {
    const size_t n = (size_t)N, v = (size_t)V;
    AuditLayout L;
    size_t at = SLNLP_AUDIT_HEAD_BYTES;
    L.t = at;      at += v * 8;
    L.s = at;      at += n * 8;
    L.m = at;      at += n * 8;
    L.n = at;      at += audit_even(v);
    L.joint = at;  at += audit_even(v * v + 1);
    L.pairs = at;  at += audit_even(3 * (size_t)M);
    L.k = at;      at += audit_even(n);
    L.code = at;   at += audit_even(n);
    L.flags = at;  at += audit_even(n);
    L.pred = at;   at += audit_even(n);
    L.other = at;  at += n * 8;
    L.p_pred = at; at += n * 8;
    L.work = at;   at += work_bytes;
    L.total = at;
    return L;
}

// ---------------------------------------------------------------------------------------------------------- pass 1 ----
__device__ __forceinline__ void audit_rows_body(const float* __restrict__ logp, long ld, const int64_t* __restrict__ y, int N, int V,
                                                const double* __restrict__ beta_dev, int* __restrict__ pred, int* __restrict__ code,
                                                double* __restrict__ s, double* __restrict__ other, double* __restrict__ m,
                                                double* __restrict__ p_pred) {
    const double beta = beta_dev ? beta_dev[0] : 1.0;
    const double qnan = __builtin_bit_cast(double, 0x7ff8000000000000ull);
    wave_rows(N, [&](long r, int lane) {
        const float* row = logp + r * ld;
        const int64_t label = y[r];
        const LogpRowMax top = logp_row_argmax(row, V, lane);
        if (!top.finite) {                               // wave-uniform: the row has no softmax (looked at before the label)
            if (lane == 0) {
                pred[r] = top.pred; code[r] = -2;
                s[r] = qnan; other[r] = qnan; m[r] = qnan; p_pred[r] = qnan;
            }
            return;
        }
        const float zmax = top.zmax;
        const LogpRowSums h = logp_row_sums(row, V, lane, beta, zmax);
        if (label < 0 || label >= V) {                   // never used as an index
            if (lane == 0) {
                pred[r] = top.pred; code[r] = -1;
                s[r] = qnan; other[r] = qnan; m[r] = qnan; p_pred[r] = 1.0 / h.s0;
            }
            return;
        }
        const int lab = (int)label;
        float bv = -INFINITY;                            // the first column other than the label (V = 1: none, INT_MAX stays)
        int bi = INT_MAX;
        for (int j = lane; j < V; j += 64) {
            if (j == lab) continue;
            const float x = row[j];
            if (score_beats(x, j, bv, bi)) { bv = x; bi = j; }
        }
        wave_best(bv, bi);
        if (lane == 0) {
            const double si = audit_prob(row[lab], zmax, beta, h.a, h.s0);
            const double oi = bi == INT_MAX ? 0.0 : audit_prob(bv, zmax, beta, h.a, h.s0);
            pred[r] = top.pred; code[r] = 0;
            s[r] = si; other[r] = oi; m[r] = si - oi; p_pred[r] = 1.0 / h.s0;
        }
    });
}
SLNLP_ZKERNEL(audit_rows_kernel, 256, audit_rows_body)

// ---------------------------------------------------------------------------------------------------------- pass 2 ----
// n_c and t_c = (sum of s_i over the usable rows labelled c) / n_c: block c
__device__ __forceinline__ void audit_classes_body(const int64_t* __restrict__ y, const int* __restrict__ code, const double* __restrict__ s,
                                                   int N, double* __restrict__ t, int* __restrict__ n) {
    __shared__ double red[256];
    __shared__ int cnt[256];
    const int tid = threadIdx.x;
    const int64_t c = blockIdx.x;
    double sum = 0.0;
    int count = 0;
    for (long r = tid; r < N; r += 256) {
        if (code[r] == 0 && y[r] == c) { sum += s[r]; ++count; }
    }
    red[tid] = sum;
    cnt[tid] = count;
    block_tree<1>(&red, tid, TreeSum{});
    block_tree<1>(&cnt, tid, TreeSum{});
    if (tid == 0) {
        const int nc = cnt[0];
        n[c] = nc;
        t[c] = nc > 0 ? red[0] / (double)nc : __builtin_bit_cast(double, 0x7ff8000000000000ull);
    }
}
SLNLP_ZKERNEL(audit_classes_kernel, 256, audit_classes_body)

// ---------------------------------------------------------------------------------------------------------- pass 3 ----
__device__ __forceinline__ void audit_confident_body(const float* __restrict__ logp, long ld, const int64_t* __restrict__ y, int N, int V,
                                                     const double* __restrict__ beta_dev, const int* __restrict__ code,
                                                     const double* __restrict__ t, int* __restrict__ k, int* __restrict__ flags) {
    const double beta = beta_dev ? beta_dev[0] : 1.0;
    // (wave_rows' loop, written out: through the helper this kernel's register counts change -- profiles/judging_shell_isa.txt)
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane((int)(blockIdx.x * 4 + (threadIdx.x >> 6)));
    const int nwaves = gridDim.x * 4;
    for (long r = wave; r < N; r += nwaves) {
        if (code[r] != 0) {                              // wave-uniform (one address for the wave): an unusable row
            if (lane == 0) { k[r] = -1; flags[r] = 0; }
            continue;
        }
        const float* row = logp + r * ld;
        const int lab = (int)y[r];                       // in [0, V): pass 1 said so
        const LogpRowMax top = logp_row_argmax(row, V, lane);
        const float zmax = top.zmax;
        const LogpRowSums h = logp_row_sums(row, V, lane, beta, zmax);
        float bv = -INFINITY;                            // the first member of K_i = { c : p_ic >= t_c } (none: INT_MAX stays)
        int bi = INT_MAX;
        for (int j = lane; j < V; j += 64) {
            const float x = row[j];
            if (audit_prob(x, zmax, beta, h.a, h.s0) >= t[j] && score_beats(x, j, bv, bi)) { bv = x; bi = j; }
        }
        wave_best(bv, bi);
        if (lane == 0) {
            const int kk = bi == INT_MAX ? -1 : bi;
            k[r] = kk;
            flags[r] = ((kk >= 0 && kk != lab) ? 1 : 0) | (top.pred != lab ? 2 : 0);
        }
    }
}
SLNLP_ZKERNEL(audit_confident_kernel, 256, audit_confident_body)

// --------------------------------------------------------------------------------------------------------- summary ----
__device__ __forceinline__ void audit_summary_body(const int* __restrict__ code, const int* __restrict__ k, const int* __restrict__ flags,
                                                   int N, int64_t* __restrict__ head) {
    __shared__ int part[AUDIT_COUNTS][256];
    const int tid = threadIdx.x;
    int c[AUDIT_COUNTS] = {0, 0, 0, 0, 0, 0};
    for (long r = tid; r < N; r += 256) {
        const int cd = code[r], f = flags[r];
        if (cd == 0) { ++c[AUDIT_USABLE]; c[AUDIT_UNCONFIDENT] += k[r] < 0 ? 1 : 0; }
        else if (cd == -1) ++c[AUDIT_BAD];
        else ++c[AUDIT_NAN];
        c[AUDIT_ISSUES] += f & 1;
        c[AUDIT_DISAGREE] += (f >> 1) & 1;
    }
#pragma unroll
    for (int q = 0; q < AUDIT_COUNTS; ++q) part[q][tid] = c[q];
    block_tree<AUDIT_COUNTS>(part, tid, TreeSum{});
    if (tid < 8) head[tid] = tid < AUDIT_COUNTS ? (int64_t)part[tid][0] : 0;
}
SLNLP_ZKERNEL(audit_summary_kernel, 256, audit_summary_body)

// --------------------------------------------------------------------------------------------------------- scatter ----
// out[rows[i], :] = row i of logp: scale_logp's row (scale_row.hpp) with a state, the float32 values themselves without
__device__ __forceinline__ void scatter_logp_body(const float* __restrict__ logp, long ld, int n, int V, const double* __restrict__ beta_dev,
                                                  const int64_t* __restrict__ rows, float* __restrict__ out, long ld_out, long N_out) {
    wave_rows(n, [&](long r, int lane) {
        const int64_t to = rows[r];
        if (to < 0 || to >= N_out) return;               // wave-uniform; never used as an address
        const float* row = logp + r * ld;
        float* dst = out + to * ld_out;
        if (beta_dev) {
            scale_logp_row(row, dst, V, lane, beta_dev[0]);
        } else {
            for (int j = lane; j < V; j += 64) dst[j] = row[j];
        }
    });
}
SLNLP_ZKERNEL(scatter_logp_kernel, 256, scatter_logp_body)

// ------------------------------------------------------------------------------------------------------- host side ----
int label_audit(const float* logp, int64_t ld, const int64_t* y, int64_t N, int64_t V, const double* beta_dev, int M, void* buf,
                int64_t buf_bytes, hipStream_t st) {
    SLNLP_CHECK_ARG(logp && y && buf, "label_audit: null pointer");
    Span z;
    SLNLP_TRY(check_logp_matrix("label_audit", logp, N, INT_MAX, V, SLNLP_CONFUSION_MAX_V, ld, &z));
    SLNLP_CHECK_ARG(M >= 1 && M <= SLNLP_PAIRS_MAX, "label_audit: M=%d outside 1..%d", M, SLNLP_PAIRS_MAX);
    const int64_t work_bytes = slnlp_confusion_pairs_workspace_bytes(V, M);
    SLNLP_CHECK_ARG(work_bytes >= 0, "label_audit: no pairs workspace for V=%ld and M=%d", (long)V, M);
    const AuditLayout L = audit_layout(N, V, M, (size_t)work_bytes);
    SLNLP_CHECK_ARG(buf_bytes >= 0 && (size_t)buf_bytes >= L.total, "label_audit: buf of %ld bytes is too small, %ld rows of %ld classes and %d pairs need %ld",
                    (long)buf_bytes, (long)N, (long)V, M, (long)L.total);
    SLNLP_CHECK_ARG(((uintptr_t)logp & 3) == 0 && (((uintptr_t)y | (uintptr_t)beta_dev | (uintptr_t)buf) & 7) == 0,
                    "label_audit: misaligned pointer (logp: 4 bytes; y, beta, buf: 8 bytes)");
    const Span in[3] = {z, {y, (size_t)N * 8, "y"}, {beta_dev, 8, "beta"}};
    const Span out[1] = {{buf, L.total, "buf"}};
    SLNLP_TRY(check_no_overlap("label_audit", out, in));
    char* b = (char*)buf;
    double* t = (double*)(b + L.t);
    double* s = (double*)(b + L.s);
    double* m = (double*)(b + L.m);
    int* n = (int*)(b + L.n);
    int* joint = (int*)(b + L.joint);
    int* pairs = (int*)(b + L.pairs);
    int* k = (int*)(b + L.k);
    int* code = (int*)(b + L.code);
    int* flags = (int*)(b + L.flags);
    int* pred = (int*)(b + L.pred);
    double* other = (double*)(b + L.other);
    double* p_pred = (double*)(b + L.p_pred);
    const int blocks = wave_rows_grid(N);
    SLNLP_TRY(zlaunch(audit_rows_kernel, dim3(blocks), 256, 0, st, "label_audit_rows", logp, (long)ld, y, (int)N, (int)V, beta_dev, pred, code, s,
                      other, m, p_pred));
    SLNLP_TRY(zlaunch(audit_classes_kernel, dim3((unsigned)V), 256, 0, st, "label_audit_classes", y, (const int*)code, (const double*)s, (int)N, t, n));
    SLNLP_TRY(zlaunch(audit_confident_kernel, dim3(blocks), 256, 0, st, "label_audit_confident", logp, (long)ld, y, (int)N, (int)V, beta_dev,
                      (const int*)code, (const double*)t, k, flags));
    SLNLP_TRY(slnlp_confusion_matrix(k, y, N, V, joint, st));                                     // confusion.hip's zero and count launches
    SLNLP_TRY(slnlp_confusion_pairs(joint, V, M, pairs, b + L.work, work_bytes, st));            // and its two pair stages
    return zlaunch(audit_summary_kernel, dim3(1), 256, 0, st, "label_audit_summary", (const int*)code, (const int*)k, (const int*)flags, (int)N,
                   (int64_t*)buf);
}

int scatter_logp(const float* logp, int64_t ld, int64_t n, int64_t V, const double* beta_dev, const int64_t* rows, float* out,
                 int64_t ld_out, int64_t N_out, hipStream_t st) {
    SLNLP_CHECK_ARG(logp && rows && out, "scatter_logp: null pointer");
    Span z, o[1];
    SLNLP_TRY(check_logp_matrix("scatter_logp", logp, n, INT_MAX, V, INT_MAX, ld, &z));
    SLNLP_CHECK_ARG(N_out >= 1 && N_out <= INT_MAX, "scatter_logp: N_out=%ld outside 1..%d", (long)N_out, INT_MAX);
    SLNLP_TRY(check_out_matrix("scatter_logp", out, N_out, "N_out", V, ld_out, &o[0]));
    SLNLP_CHECK_ARG((((uintptr_t)logp | (uintptr_t)out) & 3) == 0 && (((uintptr_t)beta_dev | (uintptr_t)rows) & 7) == 0,
                    "scatter_logp: misaligned pointer (logp, out: 4 bytes; beta, rows: 8 bytes)");
    const Span in[3] = {z, {beta_dev, 8, "beta"}, {rows, (size_t)n * 8, "rows"}};
    SLNLP_TRY(check_no_overlap("scatter_logp", o, in));
    return zlaunch(scatter_logp_kernel, dim3(wave_rows_grid(n)), 256, 0, st, "scatter_logp", logp, (long)ld, (int)n, (int)V, beta_dev, rows, out, (long)ld_out,
                   (long)N_out);
}

}  // namespace slnlp

extern "C" int slnlp_label_audit(const float* logp, int64_t ld, const int64_t* y, int64_t N, int64_t V, const double* beta_dev, int M,
                                 void* buf, int64_t buf_bytes, void* stream) {
    return slnlp::label_audit(logp, ld, y, N, V, beta_dev, M, buf, buf_bytes, (hipStream_t)stream);
}
extern "C" int slnlp_scatter_logp(const float* logp, int64_t ld, int64_t n, int64_t V, const double* beta_dev, const int64_t* rows,
                                  float* out, int64_t ld_out, int64_t N_out, void* stream) {
    return slnlp::scatter_logp(logp, ld, n, V, beta_dev, rows, out, ld_out, N_out, (hipStream_t)stream);
}
