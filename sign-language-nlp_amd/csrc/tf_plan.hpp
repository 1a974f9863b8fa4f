// tf_plan.hpp -- the Transformer plan object: arena layout, workspace carving, and the two operations a layer is written in:
// linear() and linear_bwd(), which pick the kernel family (fp32-operand, plane, B-row, fp8) from the operand views of the plan's
// mode and take their jobs from linear_jobs.hpp.  Shared by tf_plan.hip (the single-fit entry points) and lockstep.hip (K plans
// advancing through one launch sequence).
#pragma once
#include <map>
#include <string>
#include <vector>

#include "common.hpp"
#include "gemm_jobs.hpp"
#include "launch.hpp"
#include "linear_jobs.hpp"
#include "plan_core.hpp"

namespace slnlp {

struct EncP { long in_w, in_b, out_w, out_b, l1_w, l1_b, l2_w, l2_b, n1_w, n1_b, n2_w, n2_b; };
struct DecP {
    long sin_w, sin_b, sout_w, sout_b, cin_w, cin_b, cout_w, cout_b, l1_w, l1_b, l2_w, l2_b;
    long n1_w, n1_b, n2_w, n2_b, n3_w, n3_b;
};
struct Layout {
    std::vector<ParamEnt> ents;
    long src_emb, tgt_emb, encn_w, encn_b, decn_w, decn_b, lin_w, lin_b, total;
    std::vector<EncP> enc;
    std::vector<DecP> dec;
};

// Reference state_dict order (transformer.py:32-47 construction order; the
// *_pos_encoding.pe buffers are not parameters and live outside the arena).
// Every tensor starts on a 16-byte boundary so float4 access is always legal.
static Layout build_layout(const slnlp_tf_config& c) {
    Layout L;
    long cur = 0;
    auto add = [&](const std::string& n, long d0, long d1) -> long {
        ParamEnt e;
        e.name = n;
        e.shape[0] = d0;
        e.shape[1] = d1;
        e.ndim = d1 > 0 ? 2 : 1;
        e.numel = d1 > 0 ? d0 * d1 : d0;
        e.off = cur;
        cur = align_up(cur + e.numel, 4);
        L.ents.push_back(e);
        return e.off;
    };
    const long E = c.E, F = c.F;
    L.src_emb = add("src_embedding.weight", c.Vs, E);
    L.tgt_emb = add("tgt_embedding.weight", c.Vt, E);
    for (int i = 0; i < c.N; ++i) {
        const std::string p = "transformer.encoder.layers." + std::to_string(i) + ".";
        EncP e;
        e.in_w = add(p + "self_attn.in_proj_weight", 3 * E, E);
        e.in_b = add(p + "self_attn.in_proj_bias", 3 * E, 0);
        e.out_w = add(p + "self_attn.out_proj.weight", E, E);
        e.out_b = add(p + "self_attn.out_proj.bias", E, 0);
        e.l1_w = add(p + "linear1.weight", F, E);
        e.l1_b = add(p + "linear1.bias", F, 0);
        e.l2_w = add(p + "linear2.weight", E, F);
        e.l2_b = add(p + "linear2.bias", E, 0);
        e.n1_w = add(p + "norm1.weight", E, 0);
        e.n1_b = add(p + "norm1.bias", E, 0);
        e.n2_w = add(p + "norm2.weight", E, 0);
        e.n2_b = add(p + "norm2.bias", E, 0);
        L.enc.push_back(e);
    }
    L.encn_w = add("transformer.encoder.norm.weight", E, 0);
    L.encn_b = add("transformer.encoder.norm.bias", E, 0);
    for (int i = 0; i < c.N; ++i) {
        const std::string p = "transformer.decoder.layers." + std::to_string(i) + ".";
        DecP d;
        d.sin_w = add(p + "self_attn.in_proj_weight", 3 * E, E);
        d.sin_b = add(p + "self_attn.in_proj_bias", 3 * E, 0);
        d.sout_w = add(p + "self_attn.out_proj.weight", E, E);
        d.sout_b = add(p + "self_attn.out_proj.bias", E, 0);
        d.cin_w = add(p + "multihead_attn.in_proj_weight", 3 * E, E);
        d.cin_b = add(p + "multihead_attn.in_proj_bias", 3 * E, 0);
        d.cout_w = add(p + "multihead_attn.out_proj.weight", E, E);
        d.cout_b = add(p + "multihead_attn.out_proj.bias", E, 0);
        d.l1_w = add(p + "linear1.weight", F, E);
        d.l1_b = add(p + "linear1.bias", F, 0);
        d.l2_w = add(p + "linear2.weight", E, F);
        d.l2_b = add(p + "linear2.bias", E, 0);
        d.n1_w = add(p + "norm1.weight", E, 0);
        d.n1_b = add(p + "norm1.bias", E, 0);
        d.n2_w = add(p + "norm2.weight", E, 0);
        d.n2_b = add(p + "norm2.bias", E, 0);
        d.n3_w = add(p + "norm3.weight", E, 0);
        d.n3_b = add(p + "norm3.bias", E, 0);
        L.dec.push_back(d);
    }
    L.decn_w = add("transformer.decoder.norm.weight", E, 0);
    L.decn_b = add("transformer.decoder.norm.bias", E, 0);
    L.lin_w = add("linear.weight", c.Vt, E);
    L.lin_b = add("linear.bias", c.Vt, 0);
    L.total = cur;
    return L;
}

static int check_cfg(const slnlp_tf_config* c) {
    SLNLP_CHECK_ARG(c, "tf: null config");
    SLNLP_CHECK_ARG(c->E > 0 && c->H > 0 && c->E % c->H == 0, "tf: E=%d not divisible by H=%d", c->E, c->H);
    const int dh = c->E / c->H;
    SLNLP_CHECK_ARG(c->E % 4 == 0 && c->E <= 1024, "tf: E=%d must be a multiple of 4 and <= 1024", c->E);
    SLNLP_CHECK_ARG(dh % 4 == 0 && dh <= 256 && (dh <= 64 || dh % 64 == 0), "tf: head_dim %d unsupported", dh);
    SLNLP_CHECK_ARG(c->H <= 64, "tf: num_heads %d > 64 (per-head LDS tables of the cross-attention backward)", c->H);
    SLNLP_CHECK_ARG(c->F > 0 && c->F % 4 == 0, "tf: hidden_size %d must be a multiple of 4", c->F);
    SLNLP_CHECK_ARG(c->N > 0 && c->Vs > 1 && c->Vt > 1, "tf: bad N/vocab");
    SLNLP_CHECK_ARG(c->B > 0 && c->B <= 1024, "tf: batch %d outside 1..1024", c->B);
    // S <= 64: one-tile MFMA attention; longer sequences take the wave-per-row kernels (attention_long.hip).  5000 = rows of
    // the reference's positional table (positional_encoding.py:23); B * S <= 65536: the embedding backward's chunk table
    SLNLP_CHECK_ARG(c->S > 0 && c->S <= 5000, "tf: seq_len %d outside 1..5000", c->S);
    SLNLP_CHECK_ARG((long)c->B * c->S <= 65536, "tf: batch %d x seq_len %d exceeds 65536 tokens per step", c->B, c->S);
    SLNLP_CHECK_ARG(c->dropout >= 0.f && c->dropout < 1.f, "tf: dropout %f", c->dropout);
    SLNLP_CHECK_ARG(c->precision == 1 || c->precision == 3 || c->precision == 8, "tf: precision %d (1, 3 or 8)", c->precision);
    SLNLP_CHECK_ARG(c->precision != 8 || (c->E % 128 == 0 && c->F % 128 == 0),
                    "tf: precision 8 (fp8 forward products) needs embedding_size and hidden_size to be multiples of 128");
    return 0;
}

// ------------------------------------------------------------- workspace ----
// forward activations kept for backward + this layer's gradient buffers.  Every gradient buffer is
// written exactly once per step: there is nothing to overwrite until the next step.
struct EncA {
    float *qkv, *probs, *ctx, *y1, *st1, *x1, *h, *y2, *st2, *x2, *lnp1, *lnp2;
    float *gA2, *gB2, *gh, *gx1, *gA1, *gB1, *gctx, *gqkv, *gx0;
    PP ctxp, x1p, hp, x2p, d2p, ghp, d1p, gqkvp;
};
struct DecA {
    float *v, *y1, *st1, *t1, *q, *xprobs, *xctx, *y2, *st2, *t2, *h, *y3, *st3, *t3, *lnp1, *lnp2, *lnp3;
    float *qk, *mbar, *psum;                 // cross-attention without K / V projections (attention_mem.hip): kept for the backward
    float *gA3, *gB3, *gh, *gt2, *gA2, *gB2, *gxctx, *gq, *gt1, *gA1, *gB1, *gv, *gt0;
    float *dmbar, *dsc, *dqk, *dcp;          // its gradients: d mbar, d scores, d qk [B*H, .], d ctx * sum_s p_s [B, E]
    PP vp, t1p, xctxp, t2p, hp, t3p;         // operands of the layer's B-row products as planes (gemm_rows.hip); rows padded to 64
    PP d3p, ghp, d2p, gqp, d1p, gvp;         // ... and the gradients its backward pairs contract (dY of linear2, linear1, cross out / q, self out / v)
};
struct Ws {
    float *x0, *t0, *mem, *st_mem, *lnp_mem, *tfin, *st_fin, *lnp_fin, *logits, *dlogits, *logp, *row_nll;
    std::vector<EncA> enc;
    std::vector<DecA> dec;
    float *gfin, *gtl, *gmem, *gxl;     // d tfin, d t_last, d memory, d x_last
    void *emb_scratch_src, *emb_scratch_tgt;
    unsigned char* emb_keep;   // 4 keep bits per float4 of the source embedding's dropout (read by its backward)
    PP x0p, memp, wp;                   // wp: planes of the whole parameter arena (same offsets)
    PP t0p, tfinp;                      // target embedding / final decoder LayerNorm as planes (operands of B-row products)
    unsigned char* wq;                  // precision 8: e4m3 plane of the arena (same offsets; only the GEMM weight rows are filled)
    float* wscale;                      // [qrows] per-row scales
    QuantRow* qrow_table;               // [qrows] device table for the quantiser
    long n_qrows;
    char *planes_begin, *planes_end;    // activation planes region (re-zeroed when the batch size changes)
    float* opt_partials;
    float* attn_scratch;    // S > 64: dS of one self-attention backward ([B,H,S,S], shared by all layers)
    char* gscr[1];          // split-K scratch of the grouped GEMM launches (one stream: one scratch)
    size_t gscr_bytes;
    // the encoder's deferred weight gradients (one batched launch per backward, slnlp_tf_plan::wbatch): device job table and block
    // map, and the batch's own split-K scratch (a region per job: all of them are in flight at once)
    PlaneJob* wb_tab;
    int* wb_map;
    size_t wb_map_cap;
    char* wb_scr;
    size_t wb_scr_bytes;
    slnlp_ln_reduce_entry* ln_table;
    LnPartialEntry* ln_ptable;   // the same LayerNorms' (dy, x, stats, partial) for the one ln_param_partial launch of a backward
    XmemDmemLayer* dmem_tab;     // [N] the decoder layers' cross-attention gradient buffers for the one xmem_dmem_all launch of a backward
    size_t bytes;
};

constexpr int MAX_SPLITK = WD_MAX_SPLITK;
// weight-gradient GEMMs contract over the T tokens: aim at ~10 K-tiles (of 64) per workgroup
static int splitk_for(int T) {
    const int n = ((T + 63) / 64 + 5) / 10;
    return n < 1 ? 1 : n > MAX_SPLITK ? MAX_SPLITK : n;
}

// The four Linear layers of an encoder layer in the order backward meets them (linear2, linear1, out_proj, in_proj): the shapes of
// the gradient pair of dY [tokens, nout] against x [tokens, kin] -- all the deferral rule (gemm_planes_wd_defer) looks at
static void enc_pair_shapes(const slnlp_tf_config& c, int k, int tokens, slnlp_gemm_args* wg, slnlp_gemm_args* dg) {
    const int nout = k == 1 ? c.F : k == 3 ? 3 * c.E : c.E, kin = k == 0 ? c.F : c.E;
    memset(wg, 0, sizeof(*wg));
    memset(dg, 0, sizeof(*dg));
    wg->M = nout; wg->N = kin; wg->K = tokens; wg->precision = 3;
    dg->M = tokens; dg->N = kin; dg->K = nout; dg->precision = 3;
}

static Ws carve(const slnlp_tf_config& c, void* base) {
    Ws w;
    Bump b(base);
    const size_t B = c.B, S = c.S, E = c.E, F = c.F, H = c.H, M = B * S, Vp = align_up(c.Vt, 4);
    // (dgamma, dbeta) chunk sums per LayerNorm: [chunks of the full batch][2][E] (encoder: S B rows, decoder: B rows)
    const size_t lnpE = (size_t)ln_bwd_blocks((int)(B * S)) * 2 * E, lnpD = (size_t)ln_bwd_blocks((int)B) * 2 * E;
    // plane path with single-tile attention (E, F multiples of 64, S <= 64): the attention context, d qkv, the gated FFN gradient and the
    // dropout-masked LayerNorm gradients exist as bf16 planes only -- their fp32 twins have no writer and no reader and are not carved
    // (34 MB per layer at cfg2; the debug layout omits them)
    const bool lean = (E % 64 == 0) && (F % 64 == 0) && S <= 64;
    auto opt = [&](size_t n) -> float* { return lean ? nullptr : b.take<float>(n); };
    w.x0 = b.take<float>(M * E);
    w.t0 = b.take<float>(B * E);
    for (int i = 0; i < c.N; ++i) {
        EncA a;
        a.qkv = b.take<float>(M * 3 * E);
        a.probs = b.take<float>(B * H * S * S);
        a.ctx = opt(M * E);
        a.y1 = b.take<float>(M * E);
        a.st1 = b.take<float>(M * 2);
        a.x1 = b.take<float>(M * E);
        a.h = b.take<float>(M * F);
        a.y2 = b.take<float>(M * E);
        a.st2 = b.take<float>(M * 2);
        a.x2 = b.take<float>(M * E);
        a.lnp1 = b.take<float>(lnpE);
        a.lnp2 = b.take<float>(lnpE);
        a.gA2 = b.take<float>(M * E);
        a.gB2 = opt(M * E);
        a.gh = opt(M * F);
        a.gx1 = b.take<float>(M * E);
        a.gA1 = b.take<float>(M * E);
        a.gB1 = opt(M * E);
        a.gctx = b.take<float>(M * E);
        a.gqkv = opt(M * 3 * E);
        a.gx0 = b.take<float>(M * E);
        w.enc.push_back(a);
    }
    w.mem = b.take<float>(M * E);
    w.st_mem = b.take<float>(M * 2);
    w.lnp_mem = b.take<float>(lnpE);
    for (int i = 0; i < c.N; ++i) {
        DecA a;
        a.v = b.take<float>(B * E);
        a.y1 = b.take<float>(B * E);
        a.st1 = b.take<float>(B * 2);
        a.t1 = b.take<float>(B * E);
        a.q = b.take<float>(B * E);
        a.qk = b.take<float>(B * H * E);
        a.mbar = b.take<float>(B * H * E);
        a.psum = b.take<float>(B * H);
        a.xprobs = b.take<float>(B * H * S);
        a.xctx = b.take<float>(B * E);
        a.y2 = b.take<float>(B * E);
        a.st2 = b.take<float>(B * 2);
        a.t2 = b.take<float>(B * E);
        a.h = b.take<float>(B * F);
        a.y3 = b.take<float>(B * E);
        a.st3 = b.take<float>(B * 2);
        a.t3 = b.take<float>(B * E);
        a.lnp1 = b.take<float>(lnpD);
        a.lnp2 = b.take<float>(lnpD);
        a.lnp3 = b.take<float>(lnpD);
        a.gA3 = b.take<float>(B * E);
        a.gB3 = b.take<float>(B * E);
        a.gh = b.take<float>(B * F);
        a.gt2 = b.take<float>(B * E);
        a.gA2 = b.take<float>(B * E);
        a.gB2 = b.take<float>(B * E);
        a.gxctx = b.take<float>(B * E);
        a.gq = b.take<float>(B * E);
        a.dmbar = b.take<float>(B * H * E);
        a.dsc = b.take<float>(B * H * S);
        a.dqk = b.take<float>(B * H * E);
        a.dcp = b.take<float>(B * E);
        a.gt1 = b.take<float>(B * E);
        a.gA1 = b.take<float>(B * E);
        a.gB1 = b.take<float>(B * E);
        a.gv = b.take<float>(B * E);
        a.gt0 = b.take<float>(B * E);
        w.dec.push_back(a);
    }
    w.tfin = b.take<float>(B * E);
    w.st_fin = b.take<float>(B * 2);
    w.lnp_fin = b.take<float>(lnpD);
    w.logits = b.take<float>(B * Vp);
    w.dlogits = b.take<float>(B * Vp);
    w.logp = b.take<float>(B * c.Vt);
    w.row_nll = b.take<float>(B);
    w.gfin = b.take<float>(B * E);
    w.gtl = b.take<float>(B * E);
    w.gmem = b.take<float>(M * E);
    w.gxl = b.take<float>(M * E);
    w.emb_scratch_src = b.take<char>(embed_bwd_scratch_bytes(c.B, c.S, c.E));
    w.emb_scratch_tgt = b.take<char>(embed_bwd_scratch_bytes(c.B, 1, c.E));
    w.emb_keep = b.take<unsigned char>(M * E / 4);
    w.opt_partials = b.take<float>(1024);
    w.attn_scratch = c.S > 64 ? (float*)b.take<char>(attn_long_scratch_bytes(c.B, c.S, c.H)) : nullptr;
    w.ln_table = b.take<slnlp_ln_reduce_entry>(5 * c.N + 2);
    w.ln_ptable = b.take<LnPartialEntry>(5 * c.N + 2);
    w.dmem_tab = b.take<XmemDmemLayer>(c.N);
    // the batched weight-gradient launch: every (layer, Linear) whose pair defers its weight gradient at SOME batch size 1..B, with
    // the largest split factor it takes there -- room for the tables and the scratch of whichever batch size comes
    std::vector<slnlp_gemm_args> wb_jobs;
    std::vector<int> wb_split;
    for (int k = 0; k < 4 && (E % 64 == 0) && (F % 64 == 0); ++k) {
        slnlp_gemm_args wg, dg;
        int split = 0;
        for (size_t bb = 1; bb <= B; ++bb) {
            enc_pair_shapes(c, k, (int)(bb * S), &wg, &dg);
            split = std::max(split, gemm_planes_wd_defer(wg, dg));
        }
        for (int i = 0; i < c.N && split > 0; ++i) { wb_jobs.push_back(wg); wb_split.push_back(split); }
    }
    w.wb_map_cap = wb_jobs.empty() ? 0 : plane_batch_map_capacity(wb_jobs.data(), wb_split.data(), (int)wb_jobs.size());
    w.wb_tab = b.take<PlaneJob>(wb_jobs.size());
    w.wb_map = b.take<int>(w.wb_map_cap);
    // ---- bf16 operand planes (only used when E and F are multiples of 64)
    const size_t Mp = (M + 63) / 64 * 64;
    const bool q8 = c.precision == 8;
    auto pp = [&](size_t cols, bool fwd_operand = false) {
        PP q;
        q.hi = b.take<unsigned short>(Mp * cols);
        q.lo = b.take<unsigned short>(Mp * cols);
        if (q8 && fwd_operand) q.q8 = b.take<unsigned char>(Mp * cols);
        return q;
    };
    const size_t wtot = (size_t)build_layout(c).total + 64 * 3 * (E > F ? E : F);   // tail pad: tiles may over-read rows
    w.wp.hi = b.take<unsigned short>(wtot);
    w.wp.lo = b.take<unsigned short>(wtot);
    w.n_qrows = (long)c.N * (3 * E + E + F + E);                          // encoder in_proj, out_proj, linear1, linear2
    w.wq = q8 ? b.take<unsigned char>(wtot) : nullptr;
    w.wscale = q8 ? b.take<float>(w.n_qrows) : nullptr;
    w.qrow_table = q8 ? b.take<QuantRow>(w.n_qrows) : nullptr;
    b.cur = (b.cur + 255) & ~(size_t)255;
    w.planes_begin = b.base + b.cur;
    w.x0p = pp(E, true);
    w.memp = pp(E, true);
    for (int i = 0; i < c.N; ++i) {
        EncA& a = w.enc[i];
        a.ctxp = pp(E, true); a.x1p = pp(E, true); a.hp = pp(F, true); a.x2p = pp(E, true);
        a.d2p = pp(E); a.ghp = pp(F); a.d1p = pp(E); a.gqkvp = pp(3 * E);
    }
    {   // the decoder's B-row operands (rows padded to 64: the padding stays zero from the region's memset)
        const size_t Bp = (B + 63) / 64 * 64;
        auto ppd = [&](size_t cols) {
            PP q;
            q.hi = b.take<unsigned short>(Bp * cols);
            q.lo = b.take<unsigned short>(Bp * cols);
            return q;
        };
        w.t0p = ppd(E);
        w.tfinp = ppd(E);
        for (int i = 0; i < c.N; ++i) {
            DecA& a = w.dec[i];
            a.vp = ppd(E); a.t1p = ppd(E); a.xctxp = ppd(E); a.t2p = ppd(E); a.hp = ppd(F); a.t3p = ppd(E);
            a.d3p = ppd(E); a.ghp = ppd(F); a.d2p = ppd(E); a.gqp = ppd(E); a.d1p = ppd(E); a.gvp = ppd(E);
        }
    }
    {   // grouped-launch scratch lives in the zero-on-demand region: its arrival counters must start at zero
        // (the weight gradients' partial tiles: [3E or F] x [E or F] outputs rounded up to the widest (256 x 256) tile, x MAX_SPLITK)
        const size_t nx = ((E > F ? E : F) + 255) / 256 * 256, ny = ((3 * E > F ? 3 * E : F) + 255) / 256 * 256;
        w.gscr_bytes = 16384 + nx * ny * MAX_SPLITK * sizeof(float) + ny * MAX_SPLITK * sizeof(float);
        w.gscr_bytes = (w.gscr_bytes + 255) & ~(size_t)255;
        w.gscr[0] = b.take<char>(w.gscr_bytes);
        w.wb_scr_bytes = wb_jobs.empty() ? 0 : (plane_batch_scratch_bytes(wb_jobs.data(), wb_split.data(), (int)wb_jobs.size()) + 255) & ~(size_t)255;
        w.wb_scr = b.take<char>(w.wb_scr_bytes);
    }
    b.cur = (b.cur + 255) & ~(size_t)255;
    w.planes_end = b.base + b.cur;
    w.bytes = (b.cur + 255) & ~(size_t)255;
    return w;
}

}  // namespace slnlp

using namespace slnlp;   // internal header, included only by the plan translation units

// dropout site ids
enum { SITE_SRC_EMB = 1, SITE_TGT_EMB = 2, SITE_LAYER0 = 16, SITE_PER_LAYER = 8 };

// What is not the model -- buffers, settings, captured graphs, the update call, the lockstep outputs -- is PlanCore's
struct slnlp_tf_plan : PlanCore {
    slnlp_tf_config cfg;
    Layout L;
    Ws w;
    const int64_t* last_X = nullptr;
    const int64_t* last_y = nullptr;
    int nbE = 0, nbD = 0;  // (dgamma, dbeta) chunk counts of the FULL batch (fixed: the reduce table is static)
    // slnlp_tf_set_dmem_batched: d memory of all decoder layers (and their d bv) in ONE launch behind the decoder's layer loop
    // (attention_mem.hip: xmem_dmem_all) instead of a launch per layer inside it -- nothing on the decoder's chain reads d memory
    bool dmem_batched = true;
    // slnlp_tf_set_dec_ln_fused (initial value: SLNLP_DEC_LN_FUSED=0|1, default 1): a decoder LayerNorm that feeds exactly one B-row
    // product on the chain (norm1 -> the cross-attention query projection, norm2 -> linear1, norm3 -> the next layer's V projection,
    // the final norm -> the generator) runs as that product's prologue instead of a launch of its own (ln_linear)
    bool dec_ln_fused = true;
    // precision 8: the forward products run on the fp8 MFMA (e4m3 activations, scale 1; e4m3 weights with one scale per
    // output row, re-quantised from the fp32 master weights whenever the arena has moved); the backward stays split-bf16
    int prec3() const { return cfg.precision == 8 ? 3 : cfg.precision; }
    unsigned long long wq_gen = 0;
    std::map<long, long> qrow0;          // arena offset of a quantised weight block -> its first row in wscale
    int ensure_wq(hipStream_t st) {
        if (cfg.precision != 8) return 0;
        unsigned long long g = params_generation(buf.params);
        if (g != 0 && g == wq_gen) return 0;
        SLNLP_TRY(quant_rows_fp8(buf.params, 0, (int)w.n_qrows, 0, w.wq, 0, w.wscale, w.qrow_table, st));
        if (g == 0) g = bump_params_generation(buf.params);
        wq_gen = g;
        return 0;
    }
    unsigned long long wplanes_gen = 0;   // generation of the parameter arena the weight planes were made from (0: never)
    // weights as bf16 planes: made by the optimizer kernel of the previous step, or here when the arena has changed since
    int ensure_wplanes(hipStream_t st) {
        if (!use_planes) return 0;
        unsigned long long g = params_generation(buf.params);
        if (g != 0 && g == wplanes_gen) return 0;
        SLNLP_TRY(split_planes(buf.params, L.total, 1, (int)L.total, w.wp.hi, w.wp.lo, L.total, st));
        if (g == 0) g = bump_params_generation(buf.params);
        wplanes_gen = g;
        return 0;
    }
    // the arena range whose planes have readers: the encoder layers' weights (plane GEMMs) and, for plans whose batches are too tall
    // for the B-row kernel (rows_for), the decoder's and the generator's.  Everything else -- the embedding tables, the decoder's weights
    // in a plan of B-row products (gemm_rows.hip splits them in registers) -- is read as fp32.  The optimizer kernels write planes for
    // this range only
    long wplane_begin() const { return L.enc.empty() ? 0 : L.enc[0].in_w; }
    long wplane_end() const { return L.enc.empty() ? 0 : (use_rows && cfg.B <= ROWS_MAX_B ? L.encn_w : L.total); }
    // The decoder's products of B rows: the B-row kernel up to one block of 64 rows (a launch lasts as long as one workgroup loads; 16 x 16
    // tiles), the plane GEMM above (configs[4], B = 256, E = 1024: 15 us per gradient pair against 22 -- 47 before the bias gradient
    // became an MFMA product -- and 11 against 13 forward; tools/bench_rows_shapes.py)
    static constexpr int ROWS_MAX_B = 64;
    bool rows_for(int B, int drop_head_dim) const { return B <= ROWS_MAX_B || drop_head_dim != 0; }   // (per-head dropout is not built into the plane GEMM)
    // the optimizer just rewrote the arena (and, with planes, the planes with it)
    void params_stepped() override {
        const unsigned long long g = bump_params_generation(buf.params);
        if (use_planes) wplanes_gen = g;
    }
    // the captured step always re-splits the weights: a replay cannot check the arena's generation
    void before_capture() override { wplanes_gen = 0; }
    UpdateRanges update_ranges() const override {
        UpdateRanges r;
        if (use_planes) r.wp = w.wp.out();
        r.wp_begin = wplane_begin();
        r.wp_end = wplane_end();
        return r;
    }
    // outside a recorded lockstep program: re-zeroed plane padding when B changes; the weight planes (the update kernel keeps
    // them current) and, precision 8, the re-quantised weights
    int prepare(int B, hipStream_t st) override {
        SLNLP_TRY(prepare_planes(B, st));
        SLNLP_TRY(ensure_wplanes(st));
        return ensure_wq(st);
    }
    bool same_shape(const PlanCore& other) const override {
        const slnlp_tf_config &c = cfg, &c0 = static_cast<const slnlp_tf_plan&>(other).cfg;
        return c.E == c0.E && c.H == c0.H && c.N == c0.N && c.F == c0.F && c.Vs == c0.Vs && c.Vt == c0.Vt && c.B == c0.B && c.S == c0.S &&
               c.precision == c0.precision && (c.dropout > 0.f) == (c0.dropout > 0.f);
    }
    int forward(const int64_t* X, const int64_t* y, const int64_t*, int B, int train, float* logp, hipStream_t st) override {
        return slnlp_tf_forward(this, X, y, B, train, logp, st);
    }
    int backward(hipStream_t st) override { return slnlp_tf_backward(this, st); }
    bool use_planes = false;   // E, F multiples of 64: M = S*B GEMMs run on pre-split bf16 planes (gemm_planes.hip)
    bool use_rows = false;     // ... and the decoder's B-row products on planes, register-direct (gemm_rows.hip; K <= 1024)
    float* P(long off) const { return buf.params + off; }
    float* G(long off) const { return buf.grads + off; }
    int enc_site(int l, int k) const { return SITE_LAYER0 + l * SITE_PER_LAYER + k; }
    int dec_site(int l, int k) const { return SITE_LAYER0 + (cfg.N + l) * SITE_PER_LAYER + k; }

    int dec_self_block(int l, int B, float p, hipStream_t st) const;

    // ---- an activation as the operand of the plan's mode: the encoder's S*B-row products read planes when use_planes, the decoder's
    // B-row products when use_rows; else both read fp32.  (The fp32 pointer travels along: residuals and LayerNorms read it.)
    Mat view(const float* f, const PP& p, long ld) const { return use_planes ? planes(p, ld, Mat::PLANES, f) : f32(f, ld); }
    Mat rview(const float* f, const PP& p, long ld) const { return use_rows ? planes(p, ld, Mat::ROWS, f) : f32(f, ld); }
    PlaneOut pout(const PP& p) const { return use_planes ? p.out() : PlaneOut{}; }     // ... and what their producers emit beside fp32
    PlaneOut rout(const PP& p) const { return use_rows ? p.out() : PlaneOut{}; }

    // y[M, N] = x[M, K] W^T + b with the epilogue `e`; W, b at arena offsets woff, boff.  The family follows x's view: fp32 operands
    // (gemm.hip); B-row planes against fp32 weights, register-direct (gemm_rows.hip) where rows_for says so; else the plane GEMM --
    // for the encoder at precision 8 on e4m3 planes with per-row weight scales.  Only a product of planes also emits planes.
    int linear(const Mat& x, long woff, long boff, int M, int N, int K, float* y, Epi e, hipStream_t st) const {
        e.bias = P(boff);
        e.rng = buf.rng;
        if (x.kind == Mat::F32) {
            e.out = nullptr;
            return gemm(linear_job(x, f32(P(woff), K), M, N, K, y, e, prec3()), st);
        }
        if (x.kind == Mat::ROWS) {
            const bool rows = rows_for(M, e.drop_head_dim);
            const slnlp_gemm_args a = linear_job(x, rows ? f32(P(woff), K) : planes(w.wp.at(woff), K), M, N, K, y, e, prec3());
            return rows ? gemm_rows(a, st) : gemm(a, st);
        }
        if (cfg.precision != 8) return gemm(linear_job(x, planes(w.wp.at(woff), K), M, N, K, y, e, prec3()), st);
        PP wq;
        wq.q8 = w.wq + woff;
        e.col_scale = w.wscale + qrow0.at(woff);
        return gemm(linear_job(planes(x.p, K, Mat::Q8), planes(wq, K, Mat::Q8), M, N, K, y, e, 8), st);
    }
    // t = LayerNorm(xin) (gamma, beta at arena offsets gw, gb; fp32, planes tp and stats out) followed by the Linear y[M, N] = t W^T + b
    // that alone reads t on the chain.  One launch (gemm_rows.hip: the LayerNorm is the product's prologue, same bits) where the
    // product is a solo fit's 16 x 16-tile B-row launch; otherwise the two launches.  A recorder always sees the two: lockstep
    // programs keep their length, and their merged launches never take the prologue's kernel.
    int ln_linear(const float* xin, long gw, long gb, float* t, float* stats, const PP& tp, long woff, long boff, int M, int N, float* y, Epi e,
                  hipStream_t st) const {
        const int E = cfg.E;
        if (dec_ln_fused && use_rows && rows_for(M, e.drop_head_dim) && gemm_rows_ln_covers(M, N, E) && !recording()) {
            e.bias = P(boff);
            e.rng = buf.rng;
            RowsLn ln;
            ln.x = xin; ln.ldx = E; ln.gamma = P(gw); ln.beta = P(gb); ln.eps = 1e-5f; ln.y = t; ln.stats = stats; ln.y_hi = tp.hi; ln.y_lo = tp.lo; ln.ldp = E;
            return gemm_rows_ln(linear_job(rview(t, tp, E), f32(P(woff), E), M, N, E, y, e, prec3()), ln, st);
        }
        SLNLP_TRY(layernorm_fwd(xin, P(gw), P(gb), M, E, 1e-5f, t, stats, st, rout(tp)));
        return linear(rview(t, tp, E), woff, boff, M, N, E, y, e, st);
    }
    // The gradient pair of that Linear: wg: dW = dY^T x, db = colsum(dY) into the gradient arena at woff, boff; dg: dX = dY W with the
    // epilogue `e` (gate, per-head dropout, residual; fp32 and / or planes out).  Same family rule, from dY's view.  A data gradient
    // without a mask carries no dropout fields; the B-row kernel's always names the rng.
    void linear_bwd_jobs(const Mat& dy, long woff, long boff, const Mat& x, int T, int Nout, int Kin, float* dx, Epi e,
                         slnlp_gemm_args* wg, slnlp_gemm_args* dg) const {
        const bool f = dy.kind == Mat::F32, rows = dy.kind == Mat::ROWS && rows_for(T, e.drop_head_dim), pg = !f && !rows;
        if (f) e.out = nullptr;
        if (!rows && e.drop_p == 0.f) e.drop_site = e.drop_head_dim = 0;
        if (rows || e.drop_p > 0.f) e.rng = buf.rng;
        *wg = wgrad_job(dy, x, T, Nout, Kin, G(woff), G(boff), pg ? wgrad_prec(prec3()) : prec3());
        *dg = dgrad_job(dy, pg ? planes(w.wp.at(woff), Kin) : f32(P(woff), Kin), T, Nout, Kin, dx, e, pg ? dgrad_prec(prec3()) : prec3());
    }
    // ... in ONE launch: the grouped fp32-operand kernel; gemm_rows_bwd; or the plane GEMM's pair, whose weight gradient (split-K over
    // the tokens) fills the CUs the data gradient leaves idle -- no cross-queue edge to pay for (measured 4-10 us each; split factor,
    // one launch or two: gemm_planes.hip).  dgrad_alone: the weight gradient runs elsewhere (wb_defers)
    int launch_pair(const slnlp_gemm_args& wg, const slnlp_gemm_args& dg, bool dgrad_alone, hipStream_t st) const {
        if (dgrad_alone) return gemm(dg, st);
        if (dg.A_hi && dg.B_hi) return gemm_planes_wd(wg, dg, w.gscr[0], w.gscr_bytes, st);
        if (dg.A_hi) return gemm_rows_bwd(dg, wg, st);
        const slnlp_gemm_args jobs[2] = {wg, dg};
        return gemm_group(jobs, 2, st);
    }
    int linear_bwd(const Mat& dy, long woff, long boff, const Mat& x, int T, int Nout, int Kin, float* dx, const Epi& e, hipStream_t st) const {
        slnlp_gemm_args wg, dg;
        linear_bwd_jobs(dy, woff, boff, x, T, Nout, Kin, dx, e, &wg, &dg);
        return launch_pair(wg, dg, false, st);
    }
    // LayerNorm backward in front of a sub-layer's gradient pair: dx -> gA, and the pair's dY -- dx, dropout-masked when p > 0 -- as
    // what the pair reads: planes dyp (`as_planes`), or fp32 (gA itself at p = 0, else the masked copy gB)
    int ln_bwd_dy(bool as_planes, const float* dy, const float* y, long gamma, const float* stats, int rows, float* gA, float* gB, const PP& dyp,
                  float p, int site, float* partial, int full_rows, hipStream_t st) const {
        const PlaneOut none{}, out = as_planes ? dyp.out() : none;
        return layernorm_bwd(dy, y, P(gamma), stats, rows, cfg.E, nullptr, gA, (p > 0.f && !as_planes) ? gB : nullptr, p, site, buf.rng,
                             partial, nullptr, full_rows, st, p == 0.f ? out : none, p > 0.f ? out : none);
    }
    // ---- the encoder's weight gradients off the chain.  Backward is one dependent chain of launches, and a pair's launch ends with
    // its longest workgroup: at these shapes a weight-gradient slice, whose result nothing reads before the optimizer.  Where the
    // shapes say so (gemm_planes_wd_defer) the chain carries the data gradient alone and the layer loop is followed by ONE launch
    // of all deferred weight gradients (plane_batch_*): throughput-sized tiles, a job's panels in one XCD's L2, the split factor --
    // hence every sum -- of the pair's launch.  Every operand is still intact then (each gradient buffer is written once per
    // step).  Under a lockstep recorder the pairs stay together: merged launches are throughput-sized already.
    // Pair k (linear2, linear1, out_proj, in_proj: the order backward meets them) of encoder layer l at batch size B, after a forward
    // with dropout last_p.  (Plane path: the sub-layer's GEMMs read planes only -- d h has no fp32 copy.)
    void enc_pair(int l, int k, int B, slnlp_gemm_args* wg, slnlp_gemm_args* dg) const {
        const int E = cfg.E, F = cfg.F, M = cfg.S * B;
        const float p = last_p;
        const EncP& q = L.enc[l];
        const EncA& a = w.enc[l];
        if (k == 0)
            linear_bwd_jobs(view(p > 0.f ? a.gB2 : a.gA2, a.d2p, E), q.l2_w, q.l2_b, view(a.h, a.hp, F), M, E, F, use_planes ? nullptr : a.gh,
                            Epi().gated(a.h, 1.f / (1.f - p)).also(a.ghp), wg, dg);
        else if (k == 1)
            linear_bwd_jobs(view(a.gh, a.ghp, F), q.l1_w, q.l1_b, view(a.x1, a.x1p, E), M, F, E, a.gx1, Epi().plus(a.gA2), wg, dg);
        else if (k == 2)
            linear_bwd_jobs(view(p > 0.f ? a.gB1 : a.gA1, a.d1p, E), q.out_w, q.out_b, view(a.ctx, a.ctxp, E), M, E, E, a.gctx, Epi(), wg, dg);
        else
            linear_bwd_jobs(view(a.gqkv, a.gqkvp, 3 * E), q.in_w, q.in_b, l > 0 ? view(w.enc[l - 1].x2, w.enc[l - 1].x2p, E) : view(w.x0, w.x0p, E),
                            M, 3 * E, E, a.gx0, Epi().plus(a.gA1), wg, dg);
    }
    PlaneBatch wbatch;                  // the deferred jobs of a backward at batch size wbatch_B (device copies: w.wb_tab, w.wb_map)
    std::vector<char> wb_deferred;      // [4 l + k]: the pair's weight gradient is a job of the batch
    std::vector<int> wb_map_host;       // the block map as uploaded (padded to the device map's size)
    int wbatch_B = -1, wbatch_geo = -2; // batch size / forced tile geometry (plane_geo_forced) the tables were built for
    // every pointer in the tables is the plan's own: they change with the batch size alone (K = tokens, hence split factors and
    // scratch regions) -- rebuilt where the planes' padding is re-zeroed, outside any capture
    int build_wbatch(int B, hipStream_t st) {
        std::vector<slnlp_gemm_args> jobs;
        std::vector<int> split;
        wb_deferred.assign(4 * (size_t)cfg.N, 0);
        for (int l = cfg.N - 1; l >= 0; --l)
            for (int k = 0; k < 4; ++k) {
                slnlp_gemm_args wg, dg;
                enc_pair(l, k, B, &wg, &dg);
                const int n = gemm_planes_wd_defer(wg, dg);
                if (n == 0) continue;
                wb_deferred[4 * l + k] = 1;
                jobs.push_back(wg);
                split.push_back(n);
            }
        SLNLP_TRY(plane_batch_build(jobs.data(), split.data(), (int)jobs.size(), w.wb_scr, w.wb_scr_bytes, w.wb_map_cap, wbatch));
        wbatch_B = B;
        wbatch_geo = plane_geo_forced();
        if (wbatch.jobs.empty()) return 0;
        // the whole map travels, padding (-1: no work) to its end: a launch sized for another geometry's map stays inside it
        wb_map_host = wbatch.map;
        wb_map_host.resize(w.wb_map_cap, -1);
        if (hipMemcpyAsync(w.wb_tab, wbatch.jobs.data(), wbatch.jobs.size() * sizeof(PlaneJob), hipMemcpyHostToDevice, st) != hipSuccess ||
            hipMemcpyAsync(w.wb_map, wb_map_host.data(), wb_map_host.size() * sizeof(int), hipMemcpyHostToDevice, st) != hipSuccess) {
            set_error("tf: uploading the weight-gradient batch tables failed: %s", hipGetErrorString(hipGetLastError()));
            return SLNLP_ERR_LAUNCH;
        }
        return 0;
    }
    bool wb_defers(int l, int k) const { return !recording() && !wb_deferred.empty() && wb_deferred[4 * l + k]; }
    // pair k of encoder layer l on the chain: the data gradient alone where the weight gradient is a job of the batch
    int enc_pair_launch(int l, int k, int B, hipStream_t st) const {
        slnlp_gemm_args wg, dg;
        enc_pair(l, k, B, &wg, &dg);
        return launch_pair(wg, dg, wb_defers(l, k), st);
    }
    // zero padding of the activation planes is per batch size: re-zero when it changes (outside any capture)
    int prepare_planes(int B, hipStream_t st) override {
        if (!use_planes) return 0;
        if (B != planes_B) {
            if (hipMemsetAsync(w.planes_begin, 0, (size_t)(w.planes_end - w.planes_begin), st) != hipSuccess) {
                set_error("tf: zeroing operand planes failed");
                return SLNLP_ERR_LAUNCH;
            }
            planes_B = B;
        }
        if (B != wbatch_B || plane_geo_forced() != wbatch_geo) SLNLP_TRY(build_wbatch(B, st));
        return 0;
    }
    int forward_impl(const int64_t* X, const int64_t* y, int B, int train, float* logp_out, hipStream_t st);
};

