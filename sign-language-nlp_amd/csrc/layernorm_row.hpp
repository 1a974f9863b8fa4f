// layernorm_row.hpp -- the arithmetic of ONE LayerNorm row on ONE wave, shared by the stand-alone forward kernel (elementwise.hip:
// layernorm_fwd_kernel) and the B-row product that normalises its own operand (gemm_rows.hip: gemm_rows_ln_kernel).  Both hold
// the row the same way and reduce it the same way, so a row has the same bits whichever kernel normalised it.
#pragma once
#include "common.hpp"

namespace slnlp {

constexpr int LN_MAXU = 4;  // float4 per lane -> E <= 1024 (register-resident columns)

// The row in registers: slot u of lane l holds columns 4 l + 256 u .. + 3 (zeros where that is past E), gamma and beta likewise.
// Two-pass statistics (wave_sum of the sum, then of the squared deviations), then emit(u, c, o) for every slot u inside E: o = the
// four normalised values of its columns c .. c + 3.  All 64 lanes must be active.
template <class Emit>
__device__ __forceinline__ void layernorm_row(const float4 (&v)[LN_MAXU], const float4 (&g)[LN_MAXU], const float4 (&bt)[LN_MAXU], int E, float eps,
                                              int lane, float& mean_out, float& rstd_out, Emit&& emit) {
    float s = 0.f;
#pragma unroll
    for (int u = 0; u < LN_MAXU; ++u) s += v[u].x + v[u].y + v[u].z + v[u].w;      // out-of-range slots hold zeros
    const float mean = wave_sum(s) / (float)E;
    float q = 0.f;
#pragma unroll
    for (int u = 0; u < LN_MAXU; ++u) {
        if (lane * 4 + u * 256 < E) {
            const float a = v[u].x - mean, b = v[u].y - mean, cc = v[u].z - mean, d = v[u].w - mean;
            q += a * a + b * b + cc * cc + d * d;
        }
    }
    const float rstd = 1.f / sqrtf(wave_sum(q) / (float)E + eps);
#pragma unroll
    for (int u = 0; u < LN_MAXU; ++u) {
        const int c = lane * 4 + u * 256;
        if (c < E) {
            float4 o;
            o.x = (v[u].x - mean) * rstd * g[u].x + bt[u].x; o.y = (v[u].y - mean) * rstd * g[u].y + bt[u].y;
            o.z = (v[u].z - mean) * rstd * g[u].z + bt[u].z; o.w = (v[u].w - mean) * rstd * g[u].w + bt[u].w;
            emit(u, c, o);
        }
    }
    mean_out = mean;
    rstd_out = rstd;
}

}  // namespace slnlp
