// rnn_cell.hpp -- the LSTM / GRU cell arithmetic of ONE (row, hidden unit) element, forward and backward, written once.
// The stand-alone forward cell kernel (rnn.hip), the fused timestep on both tilings, the fused backward timestep and the
// persistent layer kernel (rnn_step.hip) all call these, so "same bits" between them holds by construction (rnn.hip's
// backward cell kernels keep the backward formulas in place, for their register allocation).  Gate order follows
// torch.nn.LSTM (i,f,g,o) / torch.nn.GRU (r,z,n).  The expressions keep their shape on purpose: hipcc contracts them to FMAs
// in the backend, and a reshaped expression is a different rounding.  The two sums of two products are the exception: there
// either product may legally become the FMA's, the backend's pick moved with the inlining context (the LSTM backward came
// out with the other one: different bits), so they are spelled as the fmaf every kernel has compiled to so far.
// Loads and stores stay with the callers.
#pragma once
#include "common.hpp"

namespace slnlp {

__device__ __forceinline__ float sigm(float x) { return 1.f / (1.f + expf(-x)); }
// the LSTM's new cell state gf * cprev + gi * gg (forward, and the backward's tanh argument: the same bits)
__device__ __forceinline__ float lstm_cnew(float gi, float gf, float gg, float cprev) { return fmaf(gf, cprev, gi * gg); }

template <bool LSTM>
struct RnnCellFwd {
    float act[LSTM ? 4 : 3];    // gate activations, as saved for the backward
    float hnew, cnew, hn;       // cnew: LSTM only; hn (the n gate's recurrent pre-activation): GRU only
};

// xp / hp: the input-side and recurrent-side pre-activations of the element's gates.  A fused kernel passes acc + b_hh as
// hp, i.e. xp + (acc + b_hh): what the GEMM's bias epilogue followed by the stand-alone cell computes.
template <bool LSTM>
__device__ __forceinline__ RnnCellFwd<LSTM> rnn_cell_fwd_elem(const float (&xp)[LSTM ? 4 : 3], const float (&hp)[LSTM ? 4 : 3],
                                                             float hprev, float cprev) {
    RnnCellFwd<LSTM> o;
    if constexpr (LSTM) {
        const float gi = sigm(xp[0] + hp[0]);
        const float gf = sigm(xp[1] + hp[1]);
        const float gg = tanhf(xp[2] + hp[2]);
        const float go = sigm(xp[3] + hp[3]);
        o.cnew = lstm_cnew(gi, gf, gg, cprev);
        o.hnew = go * tanhf(o.cnew);
        o.act[0] = gi; o.act[1] = gf; o.act[2] = gg; o.act[3] = go;
        o.hn = 0.f;
    } else {
        const float hn = hp[2];
        const float r = sigm(xp[0] + hp[0]);
        const float z = sigm(xp[1] + hp[1]);
        const float nn = tanhf(xp[2] + r * hn);
        o.hnew = fmaf(z, hprev, (1.f - z) * nn);    // (1.f - z) * nn + z * hprev
        o.act[0] = r; o.act[1] = z; o.act[2] = nn;
        o.hn = hn;
        o.cnew = 0.f;
    }
    return o;
}

// the layer-output value of the element: `fill` past the sequence's length (pad_packed_sequence), inverted dropout inside it
__device__ __forceinline__ float rnn_cell_out(bool valid, float hnew, float fill, float drop_p, unsigned drop_thr, int drop_site,
                                              const unsigned long long* __restrict__ rng, unsigned row, unsigned col) {
    float o = valid ? hnew : fill;
    if (drop_p > 0.f && valid) o = dropout_keep(rng, drop_site, row, col, drop_thr) ? o / (1.f - drop_p) : 0.f;
    return o;
}

template <bool LSTM>
struct RnnCellBwd {
    float dg[LSTM ? 4 : 3];     // gradients of the gate pre-activations (the GRU's input side)
    float dgh_n;                // GRU: the n gate's gradient on the recurrent side (its r and z gradients are dg[0], dg[1])
    float dc_state, carry;      // LSTM: the new running dc; the part of dh that bypasses the recurrent matmul
};

// dh: the finished gradient w.r.t. the element's output state; a0..a3: the saved gate activations; (s0, s1) = (cprev, dc_state)
// for the LSTM, (hprev, hn) for the GRU.  Valid timesteps only: the callers handle a masked one themselves.
template <bool LSTM>
__device__ __forceinline__ RnnCellBwd<LSTM> rnn_cell_bwd_elem(float dh, float a0, float a1, float a2, float a3, float s0, float s1) {
    RnnCellBwd<LSTM> o;
    if constexpr (LSTM) {
        const float gi = a0, gf = a1, gg = a2, go = a3;
        const float cprev = s0;
        const float tc = tanhf(lstm_cnew(gi, gf, gg, cprev));
        const float dc = s1 + dh * go * (1.f - tc * tc);
        o.dg[0] = dc * gg * gi * (1.f - gi);
        o.dg[1] = dc * cprev * gf * (1.f - gf);
        o.dg[2] = dc * gi * (1.f - gg * gg);
        o.dg[3] = dh * tc * go * (1.f - go);
        o.dgh_n = 0.f;
        o.dc_state = dc * gf;
        o.carry = 0.f;
    } else {
        const float r = a0, z = a1, nn = a2;
        const float hprev = s0, hn = s1;
        const float dn_pre = dh * (1.f - z) * (1.f - nn * nn);
        const float dr_pre = dn_pre * hn * r * (1.f - r);
        const float dz_pre = dh * (hprev - nn) * z * (1.f - z);
        o.dg[0] = dr_pre; o.dg[1] = dz_pre; o.dg[2] = dn_pre;
        o.dgh_n = dn_pre * r;
        o.dc_state = 0.f;
        o.carry = dh * z;
    }
    return o;
}

}  // namespace slnlp
