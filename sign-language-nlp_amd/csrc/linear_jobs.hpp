// linear_jobs.hpp -- the one place that fills a slnlp_gemm_args for a Linear y = x W^T + b and for its two gradient products
// (include/slnlp.h: forward k-major x k-major, dgrad k-major x m-major, wgrad m-major x m-major).  Host only, no kernels: the
// plans (tf_plan.hpp, rnn_plan.hip) choose operand views and the kernel family; the builders fill exactly the fields of the views
// they are given -- everything else stays zero, which is how the kernels tell one family's job from another's.
#pragma once
#include "common.hpp"
#include "plan_core.hpp"

namespace slnlp {

// An operand as ONE family of kernels reads it.  An activation may exist both ways (f and p set): `kind` says which a job names.
struct Mat {
    enum Kind {
        F32,       // fp32 at f, row stride ld: the kernel splits it itself (gemm.hip; the weights of gemm_rows.hip)
        PLANES,    // pre-split bf16 hi / lo planes p, row stride ld (gemm_planes.hip)
        ROWS,      // the same planes of a B-row operand, which a plan may hand to the register-direct kernel (gemm_rows.hip)
        Q8         // the e4m3 byte plane p.q8 (fp8 forward products)
    };
    const float* f = nullptr;
    PP p;
    long ld = 0;
    Kind kind = F32;
};
static inline Mat f32(const float* f, long ld) { Mat m; m.f = f; m.ld = ld; return m; }
static inline Mat planes(const PP& p, long ld, Mat::Kind kind = Mat::PLANES, const float* f = nullptr) { Mat m; m.f = f; m.p = p; m.ld = ld; m.kind = kind; return m; }

// What follows the product.  Order in the kernels: +bias -> activation -> *gate -> dropout -> +resid; the result goes to C (fp32)
// and / or to planes.  gate, resid and C share one row stride: ld, or the job's N when ld is 0.
struct Epi {
    const float* bias = nullptr;
    int act = 0;                                  // 1 ReLU, 2 tanh
    float drop_p = 0.f;
    int drop_site = 0, drop_head_dim = 0;         // head_dim > 0: one draw per (row, head)
    const unsigned long long* rng = nullptr;
    const float* gate = nullptr;
    float gate_scale = 0.f;
    const float* resid = nullptr;
    const PP* out = nullptr;                      // also emit the result as planes (row stride N)
    const float* col_scale = nullptr;             // fp8: per-row scales of the quantised weights
    long ld = 0;
    Epi& biased(const float* b, int a = 0) { bias = b; act = a; return *this; }
    Epi& relu() { act = 1; return *this; }
    Epi& dropped(float p, int site, int head_dim = 0) { drop_p = p; drop_site = site; drop_head_dim = head_dim; return *this; }
    Epi& gated(const float* g, float scale) { gate = g; gate_scale = scale; return *this; }
    Epi& plus(const float* r) { resid = r; return *this; }
    Epi& also(const PP& planes) { out = &planes; return *this; }
    Epi& stride(long l) { ld = l; return *this; }
};

namespace detail {
static inline void operand(const Mat& m, const float*& f, int64_t& ld, const uint16_t*& hi, const uint16_t*& lo, int64_t& ld_p) {
    if (m.kind == Mat::F32) { f = m.f; ld = m.ld; return; }
    hi = m.kind == Mat::Q8 ? reinterpret_cast<const uint16_t*>(m.p.q8) : m.p.hi;
    if (m.kind != Mat::Q8) lo = m.p.lo;
    ld_p = m.ld;
}
// C[M, N] = A B with the epilogue `e`; a_kmajor / b_kmajor as in slnlp.h
static inline slnlp_gemm_args job(const Mat& A, int a_kmajor, const Mat& B, int b_kmajor, int M, int N, int K, float* C, const Epi& e, int precision) {
    slnlp_gemm_args a;
    memset(&a, 0, sizeof(a));
    operand(A, a.A, a.lda, a.A_hi, a.A_lo, a.lda_p);
    operand(B, a.B, a.ldb, a.B_hi, a.B_lo, a.ldb_p);
    a.a_kmajor = a_kmajor; a.b_kmajor = b_kmajor;
    a.C = C; a.ldc = e.ld ? e.ld : N; a.M = M; a.N = N; a.K = K;
    a.bias = e.bias; a.relu = e.act;
    a.drop_p = e.drop_p; a.drop_site = e.drop_site; a.rng = e.rng; a.drop_head_dim = e.drop_head_dim;
    a.resid = e.resid;
    if (e.out) { a.C_hi = e.out->hi; a.C_lo = e.out->lo; a.C_q8 = e.out->q8; a.ldc_p = N; }
    a.col_scale = e.col_scale;
    a.precision = precision;
    return a;
}
}  // namespace detail

// y[M, N] = x[M, K] W[N, K]^T + bias (act) (dropout) (+ resid)
static inline slnlp_gemm_args linear_job(const Mat& x, const Mat& W, int M, int N, int K, float* y, const Epi& e, int precision) {
    slnlp_gemm_args a = detail::job(x, 1, W, 1, M, N, K, y, e, precision);
    a.ldr = a.ldc;
    return a;
}
// dx[M, Kin] = dy[M, Nout] W[Nout, Kin] (* gate) (dropout) (+ resid)
static inline slnlp_gemm_args dgrad_job(const Mat& dy, const Mat& W, int M, int Nout, int Kin, float* dx, const Epi& e, int precision) {
    slnlp_gemm_args a = detail::job(dy, 1, W, 0, M, Kin, Nout, dx, e, precision);
    a.gate = e.gate; a.ldg = a.ldc; a.gate_scale = e.gate_scale;
    a.ldr = a.ldc;
    return a;
}
// dW[Nout, Kin] (row stride ldw, 0: Kin) = dy[T, Nout]^T x[T, Kin];  db[Nout] = colsum(dy)
static inline slnlp_gemm_args wgrad_job(const Mat& dy, const Mat& x, int T, int Nout, int Kin, float* dW, float* db, int precision, long ldw = 0) {
    slnlp_gemm_args a = detail::job(dy, 0, x, 0, Nout, Kin, T, dW, Epi().stride(ldw), precision);
    a.rowsum_a = db;
    return a;
}

// `H` GEMMs of one shape in one job (gemm.hip, batched jobs): GEMM h reads A + h*sa, B + h*sb and writes C + h*sc
static inline slnlp_gemm_args batched(slnlp_gemm_args a, int H, long sa, long sb, long sc) {
    a.batch = H; a.batch_stride_a = sa; a.batch_stride_b = sb; a.batch_stride_c = sc;
    return a;
}
// per-head products of the decoder's cross-attention (attention_mem.hip); W = rows h*dh.. of a [E, E] block of in_proj
// x[B, H*dh] (columns h*dh..) -> out[B, H, E]:  out_h = x_h W_h      (qk = Wk_h^T q_h;  d mbar = Wv_h^T d ctx_h)
static inline slnlp_gemm_args head_expand(const float* x, const float* W, float* out, int B, int H, int dh, int precision) {
    const int E = H * dh;
    slnlp_gemm_args a = dgrad_job(f32(x, E), f32(W, E), B, dh, E, out, Epi(), precision);
    a.ldc = (long)H * E;
    return batched(a, H, dh, (long)dh * E, E);
}
// x[B, H, E] -> out[B, H*dh] (columns h*dh..):  out_h = x_h W_h^T (+ resid in place), also as planes when `outp`      (ctx_h = Wv_h mbar;  d q_h = Wk_h d qk)
static inline slnlp_gemm_args head_reduce(const float* x, const float* W, float* out, const float* resid, const PP* outp, int B, int H, int dh, int precision) {
    const int E = H * dh;
    slnlp_gemm_args a = linear_job(f32(x, (long)H * E), f32(W, E), B, dh, E, out, Epi().plus(resid).stride(E), precision);
    if (outp) { a.C_hi = outp->hi; a.C_lo = outp->lo; a.ldc_p = E; }
    return batched(a, H, E, (long)dh * E, dh);
}
// dW_h[dh, E] = dy_h^T x_h:  dy[B, H*dh] (columns h*dh..), x[B, H, E], dW = rows h*dh.. of an [E, E] gradient block
static inline slnlp_gemm_args head_wgrad(const float* dy, const float* x, float* dW, int B, int H, int dh, int precision) {
    const int E = H * dh;
    return batched(wgrad_job(f32(dy, E), f32(x, (long)H * E), B, dh, E, dW, nullptr, precision), H, dh, E, (long)dh * E);
}

}  // namespace slnlp
