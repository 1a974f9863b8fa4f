// attribution.hip -- occlusion attribution on the device (LogProbJudge.attribute): what in the input a
// prediction rests on.  A VARIANT of a row hides one unit of it -- a window of frames (masked by <unk>, or deleted) or one
// phonological field in every frame (substituted through a table) -- the forward passes run again on the variants, and the fall of
// the class's log-probability is the unit's attribution.  include/slnlp.h states the definitions and the buffers;
// tests/attribution_ref.py restates them in numpy, line by line.  Three entry points:
//
//   slnlp_occlude_rows        the variant builder, augment_rows' shape: ONE WAVE per variant (wave_rows, common.hpp), lanes stride the
//                             positions 64 at a time, DROP closes the row up with the keep ballot / lanes_below compaction.  Integer
//                             arithmetic only, no atomics, no LDS.  Positions >= len of the input are never read; an invalid variant
//                             reads nothing and writes an all-pad row of length 0.
//   slnlp_attribution_rows    one wave per variant: the variant's row of log-probs against its base row, both through the shared
//                             row head (logp_row.hpp) at the state's beta: drop, dp, kl, the variant's arg-max and a code.
//   slnlp_attribution_summary four queued launches, no host wait: a wave per row over the row's segment of the variant table; a thread
//                             per variant for its table cell; a block per (class, bin) cell, summed with block_sum_rows so that a
//                             cell's bits depend on M alone; one block for the head.  No floating-point atomics.
// The result of each is a pure function of its arguments: nothing depends on the grid or on timing.
#include <limits.h>
#include <math.h>

#include "block_reduce.hpp"
#include "common.hpp"
#include "launch.hpp"
#include "logp_row.hpp"
#include "spans.hpp"

namespace slnlp {

// The probability and the log-probability of a column with float32 log-prob zf, given the row head of logp_row.hpp: label_audit's
// audit_prob and reliability_rows' `beta z - a` minus log1p(rest), under the compiler's default contraction as they are there -- so
// these stand IN FRONT of the pragma below.
__device__ __forceinline__ double attr_prob(float zf, float zmax, double beta, double a, double s0) {
    return zf == zmax ? 1.0 / s0 : exp(beta * (double)zf - a) / s0;
}
__device__ __forceinline__ double attr_logp(float zf, double beta, double a, double l1p) { return (beta * (double)zf - a) - l1p; }

}  // namespace slnlp

// this file's own arithmetic (differences, products of the kl terms, sums) is rounded operation by operation, as the restatement's is
#pragma clang fp contract(off)

namespace slnlp {

enum { OCC_MASK = SLNLP_OCCLUDE_MASK, OCC_DROP = SLNLP_OCCLUDE_DROP, OCC_SUBSTITUTE = SLNLP_OCCLUDE_SUBSTITUTE };
enum { ATTR_USABLE = 0, ATTR_BAD = 1, ATTR_NAN = 2, ATTR_INVALID = 3, ATTR_FLIPS = 4, ATTR_COUNTS = 5 };

__device__ __forceinline__ bool attr_finite(double x) { return fabs(x) < (double)INFINITY; }          // false for a NaN

// over the whole wave (all 64 lanes active); every lane gets the result
__device__ __forceinline__ int wave_min_i(int v) {
    v = min(v, dpp_mov_i<DPP_XOR1>(v));
    v = min(v, dpp_mov_i<DPP_XOR2>(v));
    v = min(v, dpp_mov_i<DPP_HALF_MIRROR>(v));
    v = min(v, dpp_mov_i<DPP_MIRROR>(v));
    return min(min(__builtin_amdgcn_readlane(v, 0), __builtin_amdgcn_readlane(v, 16)),
               min(__builtin_amdgcn_readlane(v, 32), __builtin_amdgcn_readlane(v, 48)));
}

// ---------------------------------------------------------------------------------------------------- the builder ----
__device__ __forceinline__ void occlude_rows_body(const int64_t* __restrict__ X, const int64_t* __restrict__ L, const int64_t* __restrict__ y,
                                                  int n, int S, const int* __restrict__ variants, int M, int kind, int width, int stride,
                                                  int64_t pad, int64_t unk, const int64_t* __restrict__ sub, int64_t Vx, int F,
                                                  int64_t* __restrict__ X_out, int64_t* __restrict__ L_out, int64_t* __restrict__ y_out) {
    wave_rows<int>(M, [&](int j, int lane) {             // j, row, unit, len: the same in every lane, so is every branch below
        const int row = variants[3 * (long)j], unit = variants[3 * (long)j + 1];
        int64_t* dst = X_out + (long)j * S;
        const bool in_rows = row >= 0 && row < n;
        int len = 0;
        if (in_rows) {
            const int64_t l64 = L[row];
            len = l64 < 0 ? 0 : (l64 > S ? S : (int)l64);
        }
        long lo = 0, hi = 0;                             // the window [lo, hi) of MASK / DROP
        bool valid;
        if (kind == OCC_SUBSTITUTE) {
            valid = in_rows && unit >= 0 && unit < F && len >= 1;
        } else {
            lo = (long)unit * stride;
            valid = in_rows && unit >= 0 && lo < len;
            hi = lo + width < len ? lo + width : len;
        }
        if (!valid) {                                    // reads nothing more; never used as an address
            for (int c = lane; c < S; c += 64) dst[c] = pad;
            if (lane == 0) { L_out[j] = 0; y_out[j] = 0; }
            return;
        }
        const int64_t* src = X + (long)row * S;
        int base = len;                                  // the variant's length
        if (kind == OCC_SUBSTITUTE) {
            for (int t = lane; t < len; t += 64) {
                const int64_t v = src[t];
                dst[t] = (v >= 0 && v < Vx) ? sub[v * F + unit] : v;
            }
        } else if (kind == OCC_MASK || (lo == 0 && hi == len)) {     // a window over the whole row is masked: a row never loses all its frames
            for (int t = lane; t < len; t += 64) dst[t] = (t >= lo && t < hi) ? unk : src[t];
        } else {
            base = 0;
            for (int t0 = 0; t0 < len; t0 += 64) {
                const int t = t0 + lane;
                const bool keep = t < len && !(t >= lo && t < hi);
                const unsigned long long ballot = __ballot(keep);
                if (keep) dst[base + lanes_below(ballot)] = src[t];                                   // slot <= t < S
                base += __popcll(ballot);
            }
        }
        for (int c = base + lane; c < S; c += 64) dst[c] = pad;
        if (lane == 0) { L_out[j] = base; y_out[j] = y[row]; }
    });
}
SLNLP_ZKERNEL(occlude_rows_kernel, 256, occlude_rows_body)

// ------------------------------------------------------------------------------------------------ variant rows ----
__device__ __forceinline__ void attribution_rows_body(const float* __restrict__ base, long ld_b, const float* __restrict__ var, long ld_v,
                                                      const int64_t* __restrict__ y, const int* __restrict__ variants, int N, int M, int V,
                                                      int target, const double* __restrict__ beta_dev, long off, double* __restrict__ vals,
                                                      int* __restrict__ ints) {
    const double beta = beta_dev ? beta_dev[0] : 1.0;
    const double qnan = __builtin_bit_cast(double, 0x7ff8000000000000ull);
    wave_rows(M, [&](long j, int lane) {
        const long g = off + j;
        const int row = variants[3 * g];
        double* out = vals + 3 * g;
        int* io = ints + 2 * g;
        auto refuse = [&](int amax, int code) {
            if (lane == 0) { out[0] = qnan; out[1] = qnan; out[2] = qnan; io[0] = amax; io[1] = code; }
        };
        if (row < 0 || row >= N) return refuse(-1, -3);  // wave-uniform; never used as an index
        const float* rb = base + (long)row * ld_b;
        const float* rv = var + j * ld_v;
        const LogpRowMax tb = logp_row_argmax(rb, V, lane);
        const LogpRowMax tv = logp_row_argmax(rv, V, lane);
        if (!tb.finite || !tv.finite) return refuse(tv.pred, -2);
        int c = tb.pred;
        if (target == 0) {
            const int64_t label = y[row];
            if (label < 0 || label >= V) return refuse(tv.pred, -1);
            c = (int)label;
        }
        const LogpRowSums hb = logp_row_sums(rb, V, lane, beta, tb.zmax);
        const LogpRowSums hv = logp_row_sums(rv, V, lane, beta, tv.zmax);
        const double lb = log1p(hb.rest), lv = log1p(hv.rest);
        double kl = 0.0;
        for (int k = lane; k < V; k += 64) {
            const float zb = rb[k];
            const double pb = attr_prob(zb, tb.zmax, beta, hb.a, hb.s0);
            if (pb > 0.0) kl += pb * (attr_logp(zb, beta, hb.a, lb) - attr_logp(rv[k], beta, hv.a, lv));
        }
        kl = wave_sum_d(kl);
        if (lane == 0) {
            const float zb = rb[c], zv = rv[c];
            out[0] = attr_logp(zb, beta, hb.a, lb) - attr_logp(zv, beta, hv.a, lv);
            out[1] = attr_prob(zb, tb.zmax, beta, hb.a, hb.s0) - attr_prob(zv, tv.zmax, beta, hv.a, hv.s0);
            out[2] = kl;
            io[0] = tv.pred; io[1] = 0;
        }
    });
}
SLNLP_ZKERNEL(attribution_rows_kernel, 256, attribution_rows_body)

// ----------------------------------------------------------------------------------------------------- summary ----
// per row: rows_i [N, 6] = base arg-max, target, code of the base row, usable variants, flips, top_unit; rows_d [N, 4] = lp_b(c),
// top_drop, min_drop, sum_drop
__device__ __forceinline__ void attribution_row_body(const float* __restrict__ base, long ld_b, const int64_t* __restrict__ y,
                                                     const int* __restrict__ variants, const int* __restrict__ row_start, int N, int M, int V,
                                                     int target, const double* __restrict__ beta_dev, const double* __restrict__ vals,
                                                     const int* __restrict__ ints, int* __restrict__ rows_i, double* __restrict__ rows_d) {
    const double beta = beta_dev ? beta_dev[0] : 1.0;
    const double qnan = __builtin_bit_cast(double, 0x7ff8000000000000ull);
    wave_rows(N, [&](long r, int lane) {
        const float* rb = base + r * ld_b;
        const LogpRowMax tb = logp_row_argmax(rb, V, lane);
        int code = 0, c = -1;
        if (!tb.finite) {
            code = -2;
        } else if (target == 0) {
            const int64_t label = y[r];
            if (label < 0 || label >= V) code = -1;
            else c = (int)label;
        } else {
            c = tb.pred;
        }
        double lpb = qnan;
        if (code == 0) {                                 // wave-uniform
            const LogpRowSums hb = logp_row_sums(rb, V, lane, beta, tb.zmax);
            lpb = attr_logp(rb[c], beta, hb.a, log1p(hb.rest));
        }
        int s = row_start[r], e = row_start[r + 1];      // the row's segment, clamped into [0, M]: never trusted as an address
        s = s < 0 ? 0 : (s > M ? M : s);
        e = e < s ? s : (e > M ? M : e);
        int usable = 0, flips = 0, bu = INT_MAX;
        double best = -(double)INFINITY, least = (double)INFINITY, sum = 0.0;
        for (long q = s + lane; q < e; q += 64) {
            if (variants[3 * q] != (int)r || ints[2 * q + 1] != 0) continue;
            ++usable;
            flips += ints[2 * q] != tb.pred ? 1 : 0;
            const double d = vals[3 * q];
            if (!attr_finite(d)) continue;
            const int u = variants[3 * q + 1];
            sum += d;
            least = fmin(least, d);
            if (d > best || (d == best && u < bu)) { best = d; bu = u; }
        }
        usable = wave_sum_i(usable);
        flips = wave_sum_i(flips);
        sum = wave_sum_d(sum);
        const double top = wave_max_d(best);
        const double low = -wave_max_d(-least);
        const int unit = wave_min_i((bu != INT_MAX && best == top) ? bu : INT_MAX);
        if (lane == 0) {
            const bool any = unit != INT_MAX;
            int* ri = rows_i + 6 * r;
            double* rd = rows_d + 4 * r;
            ri[0] = tb.pred; ri[1] = c; ri[2] = code; ri[3] = usable; ri[4] = flips; ri[5] = any ? unit : -1;
            rd[0] = lpb; rd[1] = any ? top : qnan; rd[2] = any ? low : qnan; rd[3] = sum;
        }
    });
}
SLNLP_ZKERNEL(attribution_row_kernel, 256, attribution_row_body)

// per variant: cell[g] = ((target class * n_bins + bin) << 1) | flip for a usable variant with a bin in [0, n_bins), else -1
__device__ __forceinline__ void attribution_cells_body(const int* __restrict__ variants, const int* __restrict__ ints,
                                                       const int* __restrict__ rows_i, int N, int M, int V, int n_bins, int* __restrict__ cell) {
    for (long g = blockIdx.x * 256L + threadIdx.x; g < M; g += gridDim.x * 256L) {
        const int row = variants[3 * g], bin = variants[3 * g + 2];
        int out = -1;
        if (ints[2 * g + 1] == 0 && row >= 0 && row < N && bin >= 0 && bin < n_bins) {
            const int c = rows_i[6 * (long)row + 1];
            if (c >= 0 && c < V) out = ((c * n_bins + bin) << 1) | (ints[2 * g] != rows_i[6 * (long)row] ? 1 : 0);
        }
        cell[g] = out;
    }
}
SLNLP_ZKERNEL(attribution_cells_kernel, 256, attribution_cells_body)

// block (class c, bin b): thread t adds its variants t, t + 256, ... ascending, then the fixed tree -- an order that depends on M alone
__device__ __forceinline__ void attribution_table_body(const int* __restrict__ cell, const double* __restrict__ vals, int M,
                                                       int64_t* __restrict__ table_i, double* __restrict__ table_d) {
    __shared__ double red[2][256];
    __shared__ int cnt[3][256];
    const int tid = threadIdx.x;
    const int id = blockIdx.x;
    block_sum_rows<2>(red, tid, M, [&](long g, double* acc) {
        const int cg = cell[g];
        if (cg < 0 || (cg >> 1) != id) return;
        const double d = vals[3 * g], k = vals[3 * g + 2];
        if (attr_finite(d) && attr_finite(k)) { acc[0] += d; acc[1] += k; }
    });
    const double sum_drop = red[0][0], sum_kl = red[1][0];
    block_sum_rows<3>(cnt, tid, M, [&](long g, int* acc) {
        const int cg = cell[g];
        if (cg < 0 || (cg >> 1) != id) return;
        const bool fin = attr_finite(vals[3 * g]) && attr_finite(vals[3 * g + 2]);
        acc[0] += fin ? 1 : 0;
        acc[1] += cg & 1;
        acc[2] += fin ? 0 : 1;
    });
    if (tid == 0) {
        table_i[3 * (long)id] = cnt[0][0]; table_i[3 * (long)id + 1] = cnt[1][0]; table_i[3 * (long)id + 2] = cnt[2][0];
        table_d[2 * (long)id] = sum_drop; table_d[2 * (long)id + 1] = sum_kl;
    }
}
SLNLP_ZKERNEL(attribution_table_kernel, 256, attribution_table_body)

__device__ __forceinline__ void attribution_head_body(const int* __restrict__ variants, const int* __restrict__ ints,
                                                      const int* __restrict__ rows_i, int N, int M, int64_t* __restrict__ head) {
    __shared__ int part[ATTR_COUNTS][256];
    const int tid = threadIdx.x;
    int c[ATTR_COUNTS] = {0, 0, 0, 0, 0};
    for (long g = tid; g < M; g += 256) {
        const int cd = ints[2 * g + 1], row = variants[3 * g];
        if (cd == 0) {
            ++c[ATTR_USABLE];
            if (row >= 0 && row < N) c[ATTR_FLIPS] += ints[2 * g] != rows_i[6 * (long)row] ? 1 : 0;
        } else if (cd == -1) ++c[ATTR_BAD];
        else if (cd == -2) ++c[ATTR_NAN];
        else ++c[ATTR_INVALID];
    }
#pragma unroll
    for (int q = 0; q < ATTR_COUNTS; ++q) part[q][tid] = c[q];
    block_tree<ATTR_COUNTS>(part, tid, TreeSum{});
    if (tid < 8) head[tid] = tid < ATTR_COUNTS ? (int64_t)part[tid][0] : 0;
}
SLNLP_ZKERNEL(attribution_head_kernel, 256, attribution_head_body)

// ------------------------------------------------------------------------------------------------------- host side ----
int occlude_rows(const int64_t* X, const int64_t* L, const int64_t* y, int64_t n, int64_t S, const int32_t* variants, int64_t M, int kind,
                 int64_t width, int64_t stride, int64_t pad, int64_t unk, const int64_t* sub, int64_t Vx, int64_t F, int64_t* X_out,
                 int64_t* L_out, int64_t* y_out, hipStream_t st) {
    SLNLP_CHECK_ARG(X && L && y && variants && X_out && L_out && y_out, "occlude_rows: null pointer");
    SLNLP_CHECK_ARG(n >= 1 && n <= INT_MAX, "occlude_rows: n=%ld outside 1..%d", (long)n, INT_MAX);
    SLNLP_CHECK_ARG(S >= 1 && S <= INT_MAX, "occlude_rows: S=%ld outside 1..%d", (long)S, INT_MAX);
    SLNLP_CHECK_ARG(M >= 1 && M <= INT_MAX / 3, "occlude_rows: M=%ld outside 1..%d", (long)M, INT_MAX / 3);
    SLNLP_CHECK_ARG(S <= INT64_MAX / 8 / n, "occlude_rows: n=%ld times S=%ld is no addressable matrix", (long)n, (long)S);
    SLNLP_CHECK_ARG(S <= INT64_MAX / 8 / M, "occlude_rows: M=%ld times S=%ld is no addressable matrix", (long)M, (long)S);
    SLNLP_CHECK_ARG(kind == OCC_MASK || kind == OCC_DROP || kind == OCC_SUBSTITUTE, "occlude_rows: kind=%d, expected 0 (mask), 1 (drop) or 2 (substitute)", kind);
    size_t sub_bytes = 0;
    if (kind == OCC_SUBSTITUTE) {
        SLNLP_CHECK_ARG(sub, "occlude_rows: substitute needs the table sub");
        SLNLP_CHECK_ARG(F >= 1 && F <= SLNLP_ATTR_MAX_BINS, "occlude_rows: F=%ld outside 1..%d", (long)F, SLNLP_ATTR_MAX_BINS);
        SLNLP_CHECK_ARG(Vx >= 1 && Vx <= INT64_MAX / 8 / F, "occlude_rows: Vx=%ld times F=%ld is no addressable table", (long)Vx, (long)F);
        sub_bytes = (size_t)Vx * (size_t)F * 8;
    } else {
        SLNLP_CHECK_ARG(width >= 1 && width <= S, "occlude_rows: width=%ld outside 1..S=%ld", (long)width, (long)S);
        SLNLP_CHECK_ARG(stride >= 1 && stride <= S, "occlude_rows: stride=%ld outside 1..S=%ld", (long)stride, (long)S);
        sub = nullptr; Vx = 0; F = 0;
    }
    SLNLP_CHECK_ARG(((uintptr_t)variants & 3) == 0 &&
                    (((uintptr_t)X | (uintptr_t)L | (uintptr_t)y | (uintptr_t)sub | (uintptr_t)X_out | (uintptr_t)L_out | (uintptr_t)y_out) & 7) == 0,
                    "occlude_rows: misaligned pointer (variants: 4 bytes; the others: 8 bytes)");
    // not in-place: a variant's stores would run ahead of another variant's loads of the same row
    const Span in[5] = {{X, (size_t)n * (size_t)S * 8, "X"}, {L, (size_t)n * 8, "L"}, {y, (size_t)n * 8, "y"},
                        {variants, (size_t)M * 12, "variants"}, {sub, sub_bytes, "sub"}};
    const Span out[3] = {{X_out, (size_t)M * (size_t)S * 8, "X_out"}, {L_out, (size_t)M * 8, "L_out"}, {y_out, (size_t)M * 8, "y_out"}};
    SLNLP_TRY(check_no_overlap("occlude_rows", out, in));
    return zlaunch(occlude_rows_kernel, dim3(wave_rows_grid(M)), 256, 0, st, "occlude_rows", X, L, y, (int)n, (int)S, (const int*)variants, (int)M, kind,
                   (int)(kind == OCC_SUBSTITUTE ? 1 : width), (int)(kind == OCC_SUBSTITUTE ? 1 : stride), pad, unk, sub, Vx, (int)F, X_out, L_out, y_out);
}

// what attribution_rows and attribution_summary check alike
static int check_attribution(const char* what, const float* base, int64_t ld_b, const int64_t* y, const int32_t* variants, int64_t N, int64_t M_all,
                             int64_t V, int target, const double* beta_dev, const double* vals, const int32_t* ints, Span* b) {
    SLNLP_CHECK_ARG(base && variants && vals && ints, "%s: null pointer", what);
    SLNLP_TRY(check_logp_matrix(what, base, N, INT_MAX, V, SLNLP_CONFUSION_MAX_V, ld_b, b));
    b->name = "base";
    SLNLP_CHECK_ARG(M_all >= 1 && M_all <= INT_MAX / 3, "%s: %ld variants, outside 1..%d", what, (long)M_all, INT_MAX / 3);
    SLNLP_CHECK_ARG(target == 0 || target == 1, "%s: target=%d, expected 0 (the label) or 1 (the base row's arg-max)", what, target);
    SLNLP_CHECK_ARG(target == 1 || y, "%s: target 0 needs the labels y", what);
    SLNLP_CHECK_ARG((((uintptr_t)base | (uintptr_t)variants | (uintptr_t)ints) & 3) == 0 && (((uintptr_t)y | (uintptr_t)beta_dev | (uintptr_t)vals) & 7) == 0,
                    "%s: misaligned pointer (base, var, variants, ints: 4 bytes; y, beta, vals: 8 bytes)", what);
    return 0;
}

int attribution_rows(const float* base, int64_t ld_b, const float* var, int64_t ld_v, const int64_t* y, const int32_t* variants, int64_t N,
                     int64_t M, int64_t V, int target, const double* beta_dev, int64_t off, double* vals, int32_t* ints, hipStream_t st) {
    const char* what = "attribution_rows";
    SLNLP_CHECK_ARG(var, "%s: null pointer", what);
    SLNLP_CHECK_ARG(M >= 1 && M <= INT_MAX / 3 && off >= 0 && off <= INT_MAX / 3 - M, "%s: M=%ld at off=%ld outside the %d variants a table holds", what,
                    (long)M, (long)off, INT_MAX / 3);
    Span b, v;
    SLNLP_TRY(check_attribution(what, base, ld_b, y, variants, N, off + M, V, target, beta_dev, vals, ints, &b));
    SLNLP_TRY(check_logp_matrix(what, var, M, INT_MAX, V, SLNLP_CONFUSION_MAX_V, ld_v, &v));
    v.name = "var";
    SLNLP_CHECK_ARG(((uintptr_t)var & 3) == 0, "%s: misaligned pointer (base, var, variants, ints: 4 bytes; y, beta, vals: 8 bytes)", what);
    const size_t m_all = (size_t)(off + M);
    const Span in[5] = {b, v, {y, (size_t)N * 8, "y"}, {variants, m_all * 12, "variants"}, {beta_dev, 8, "beta"}};
    const Span out[2] = {{vals, m_all * 24, "vals"}, {ints, m_all * 8, "ints"}};
    SLNLP_TRY(check_no_overlap(what, out, in));
    return zlaunch(attribution_rows_kernel, dim3(wave_rows_grid(M)), 256, 0, st, what, base, (long)ld_b, var, (long)ld_v, y, (const int*)variants, (int)N,
                   (int)M, (int)V, target, beta_dev, (long)off, vals, (int*)ints);
}

int attribution_summary(const float* base, int64_t ld_b, const int64_t* y, const int32_t* variants, const int32_t* row_start, int64_t N, int64_t M,
                        int64_t V, int n_bins, int target, const double* beta_dev, const double* vals, const int32_t* ints, int32_t* cell,
                        int64_t* head, int64_t* table_i, double* table_d, int32_t* rows_i, double* rows_d, hipStream_t st) {
    const char* what = "attribution_summary";
    SLNLP_CHECK_ARG(row_start && cell && head && table_i && table_d && rows_i && rows_d, "%s: null pointer", what);
    Span b;
    SLNLP_TRY(check_attribution(what, base, ld_b, y, variants, N, M, V, target, beta_dev, vals, ints, &b));
    SLNLP_CHECK_ARG(n_bins >= 1 && n_bins <= SLNLP_ATTR_MAX_BINS, "%s: n_bins=%d outside 1..%d", what, n_bins, SLNLP_ATTR_MAX_BINS);
    SLNLP_CHECK_ARG((((uintptr_t)row_start | (uintptr_t)cell | (uintptr_t)rows_i) & 3) == 0 &&
                    (((uintptr_t)head | (uintptr_t)table_i | (uintptr_t)table_d | (uintptr_t)rows_d) & 7) == 0,
                    "%s: misaligned pointer (row_start, cell, rows_i: 4 bytes; head, table_i, table_d, rows_d: 8 bytes)", what);
    const size_t cells = (size_t)V * (size_t)n_bins, m = (size_t)M, n = (size_t)N;
    const Span in[7] = {b, {y, n * 8, "y"}, {variants, m * 12, "variants"}, {row_start, (n + 1) * 4, "row_start"}, {beta_dev, 8, "beta"},
                        {vals, m * 24, "vals"}, {ints, m * 8, "ints"}};
    const Span out[6] = {{cell, m * 4, "cell"}, {head, SLNLP_ATTR_HEAD_BYTES, "head"}, {table_i, cells * 24, "table_i"}, {table_d, cells * 16, "table_d"},
                         {rows_i, n * 24, "rows_i"}, {rows_d, n * 32, "rows_d"}};
    SLNLP_TRY(check_no_overlap(what, out, in));
    SLNLP_TRY(zlaunch(attribution_row_kernel, dim3(wave_rows_grid(N)), 256, 0, st, "attribution_summary_rows", base, (long)ld_b, y, (const int*)variants,
                      (const int*)row_start, (int)N, (int)M, (int)V, target, beta_dev, vals, (const int*)ints, (int*)rows_i, rows_d));
    const int vblocks = (int)((M + 255) / 256 < 1024 ? (M + 255) / 256 : 1024);
    SLNLP_TRY(zlaunch(attribution_cells_kernel, dim3(vblocks), 256, 0, st, "attribution_summary_cells", (const int*)variants, (const int*)ints,
                      (const int*)rows_i, (int)N, (int)M, (int)V, n_bins, (int*)cell));
    SLNLP_TRY(zlaunch(attribution_table_kernel, dim3((unsigned)cells), 256, 0, st, "attribution_summary_table", (const int*)cell, vals, (int)M, table_i,
                      table_d));
    return zlaunch(attribution_head_kernel, dim3(1), 256, 0, st, "attribution_summary_head", (const int*)variants, (const int*)ints, (const int*)rows_i,
                   (int)N, (int)M, head);
}

}  // namespace slnlp

extern "C" int slnlp_occlude_rows(const int64_t* X, const int64_t* L, const int64_t* y, int64_t n, int64_t S, const int32_t* variants, int64_t M,
                                  int kind, int64_t width, int64_t stride, int64_t pad, int64_t unk, const int64_t* sub, int64_t Vx, int64_t F,
                                  int64_t* X_out, int64_t* L_out, int64_t* y_out, void* stream) {
    return slnlp::occlude_rows(X, L, y, n, S, variants, M, kind, width, stride, pad, unk, sub, Vx, F, X_out, L_out, y_out, (hipStream_t)stream);
}
extern "C" int slnlp_attribution_rows(const float* base, int64_t ld_b, const float* var, int64_t ld_v, const int64_t* y, const int32_t* variants,
                                      int64_t N, int64_t M, int64_t V, int target, const double* beta_dev, int64_t off, double* vals, int32_t* ints,
                                      void* stream) {
    return slnlp::attribution_rows(base, ld_b, var, ld_v, y, variants, N, M, V, target, beta_dev, off, vals, ints, (hipStream_t)stream);
}
extern "C" int slnlp_attribution_summary(const float* base, int64_t ld_b, const int64_t* y, const int32_t* variants, const int32_t* row_start,
                                         int64_t N, int64_t M, int64_t V, int n_bins, int target, const double* beta_dev, const double* vals,
                                         const int32_t* ints, int32_t* cell, int64_t* head, int64_t* table_i, double* table_d, int32_t* rows_i,
                                         double* rows_d, void* stream) {
    return slnlp::attribution_summary(base, ld_b, y, variants, row_start, N, M, V, n_bins, target, beta_dev, vals, ints, cell, head, table_i, table_d,
                                      rows_i, rows_d, (hipStream_t)stream);
}
