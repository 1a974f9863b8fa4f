// tf_plan.hip -- host-side plan for the whole model.Transformer step.
//
// Drop-in target: /root/reference/model/transformer.py:10-109 (constructor
// defines the parameter set, forward :60-90 defines the arithmetic) driven by
// the skorch step zero_grad -> forward -> CrossEntropyLoss(ignore_index) ->
// backward -> clip_grad_norm_ -> SGD.
//
// The plan owns (a) the layout of the flat fp32 parameter arena (names/shapes =
// reference state_dict), (b) the layout of the activation workspace and (c) the
// launch sequence.  Nothing here allocates device memory: the caller hands in
// arena / workspace pointers.  Every launch goes to the caller's stream, so the
// whole step can be captured into one hipGraph (slnlp_tf_graph_*).
#include <map>
#include <string>
#include <vector>

#include "common.hpp"
#include "launch.hpp"
#include "tf_plan.hpp"

using namespace slnlp;

extern "C" {

int slnlp_tf_num_params(const slnlp_tf_config* cfg) {
    if (check_cfg(cfg)) return -1;
    return (int)build_layout(*cfg).ents.size();
}

int slnlp_tf_param_info(const slnlp_tf_config* cfg, int i, char* name, int64_t shape[2], int* ndim, int64_t* offset) {
    SLNLP_TRY(check_cfg(cfg));
    return param_info(build_layout(*cfg).ents, i, "tf_param_info", name, shape, ndim, offset);
}

int64_t slnlp_tf_arena_floats(const slnlp_tf_config* cfg) {
    if (check_cfg(cfg)) return -1;
    return build_layout(*cfg).total;
}

int64_t slnlp_tf_workspace_bytes(const slnlp_tf_config* cfg) {
    if (check_cfg(cfg)) return -1;
    return (int64_t)carve(*cfg, nullptr).bytes;
}

void slnlp_tf_destroy(slnlp_tf_plan* plan) {
    if (plan) plan->destroy();
}

int slnlp_tf_create(const slnlp_tf_config* cfg, const slnlp_tf_buffers* buf, slnlp_tf_plan** out) {
    SLNLP_TRY(check_cfg(cfg));
    SLNLP_CHECK_ARG(buf && out, "tf_create: null argument");
    SLNLP_CHECK_ARG(buf->params && buf->grads && buf->momentum && buf->pe && buf->workspace && buf->rng && buf->lr &&
                        buf->scalars,
                    "tf_create: every buffer pointer is required");
    SLNLP_CHECK_ARG((((uintptr_t)buf->params | (uintptr_t)buf->grads | (uintptr_t)buf->momentum |
                      (uintptr_t)buf->workspace | (uintptr_t)buf->pe) & 255) == 0,
                    "tf_create: arenas / workspace / pe must be 256-byte aligned");
    slnlp_tf_plan* p = new slnlp_tf_plan();
    p->cfg = *cfg;
    p->buf = *buf;
    p->L = build_layout(*cfg);
    p->w = carve(*cfg, buf->workspace);
    p->arena = p->L.total; p->opt_partials = p->w.opt_partials;
    p->max_B = cfg->B; p->S = cfg->S; p->Vt = cfg->Vt; p->dropout = cfg->dropout;
    bool ok = attn_init() == 0 && gemm_planes_init() == 0;
    p->use_planes = (cfg->E % 64 == 0) && (cfg->F % 64 == 0);
    {   // SLNLP_DEC_ROWS=0: the decoder's products on gemm.hip's fp32-operand kernel again (A / B measurements; another arithmetic:
        // that kernel splits its operands itself, with a truncated head)
        const char* e = getenv("SLNLP_DEC_ROWS");
        p->use_rows = p->use_planes && cfg->E <= 1024 && cfg->F <= 1024 && !(e && atoi(e) == 0);
    }
    {   // SLNLP_DEC_LN_FUSED=0: a new plan starts with the decoder's LayerNorms as launches of their own (A / B of one build)
        const char* e = getenv("SLNLP_DEC_LN_FUSED");
        p->dec_ln_fused = !(e && atoi(e) == 0);
    }
    if (ok && cfg->precision == 8) {     // rows the fp8 forward products read: one {offset, K} entry each, uploaded once
        std::vector<QuantRow> rows;
        auto block = [&](long off, int nrows, int K) {
            p->qrow0[off] = (long)rows.size();
            for (int r = 0; r < nrows; ++r) rows.push_back(QuantRow{off + (long)r * K, K, 0});
        };
        const int E = cfg->E, F = cfg->F;
        for (int i = 0; i < cfg->N; ++i) {
            const EncP& q = p->L.enc[i];
            block(q.in_w, 3 * E, E); block(q.out_w, E, E); block(q.l1_w, F, E); block(q.l2_w, E, F);
        }
        ok = (long)rows.size() == p->w.n_qrows &&
             hipMemcpy(p->w.qrow_table, rows.data(), rows.size() * sizeof(QuantRow), hipMemcpyHostToDevice) == hipSuccess;
    }
    // LN (dgamma, dbeta) tables, one entry per LayerNorm, uploaded once: what ln_param_partial reads (the dy / x / stats of the
    // LayerNorm's backward, all still intact at the end of backward: every gradient buffer is written once per step) and what
    // ln_param_reduce adds.  nblk is the FULL batch's chunk count; a smaller batch's trailing chunks are written as zeros.
    std::vector<slnlp_ln_reduce_entry> tab;
    std::vector<LnPartialEntry> ptab;
    const int nbE = p->nbE = ln_bwd_blocks(cfg->B * cfg->S), nbD = p->nbD = ln_bwd_blocks(cfg->B);
    auto ent = [&](float* part, long gw, long gb, int dec, const float* dy, const float* x, const float* stats) {
        slnlp_ln_reduce_entry e;
        e.partial = part; e.dgamma = p->G(gw); e.dbeta = p->G(gb); e.nblk = dec ? nbD : nbE; e.E = cfg->E;
        tab.push_back(e);
        LnPartialEntry q;
        q.dy = dy; q.x = x; q.stats = stats; q.partial = part; q.dec = dec; q.pad = 0;
        ptab.push_back(q);
    };
    {
        const Ws& w = p->w;
        const int N = cfg->N;
        for (int i = 0; i < N; ++i) {
            const EncA& a = w.enc[i];
            ent(a.lnp1, p->L.enc[i].n1_w, p->L.enc[i].n1_b, 0, a.gx1, a.y1, a.st1);
            ent(a.lnp2, p->L.enc[i].n2_w, p->L.enc[i].n2_b, 0, i + 1 < N ? w.enc[i + 1].gx0 : w.gxl, a.y2, a.st2);
        }
        ent(w.lnp_mem, p->L.encn_w, p->L.encn_b, 0, w.gmem, w.enc[N - 1].x2, w.st_mem);
        for (int i = 0; i < N; ++i) {
            const DecA& a = w.dec[i];
            ent(a.lnp1, p->L.dec[i].n1_w, p->L.dec[i].n1_b, 1, a.gt1, a.y1, a.st1);
            ent(a.lnp2, p->L.dec[i].n2_w, p->L.dec[i].n2_b, 1, a.gt2, a.y2, a.st2);
            ent(a.lnp3, p->L.dec[i].n3_w, p->L.dec[i].n3_b, 1, i + 1 < N ? w.dec[i + 1].gt0 : w.gtl, a.y3, a.st3);
        }
        ent(w.lnp_fin, p->L.decn_w, p->L.decn_b, 1, w.gfin, w.dec[N - 1].t3, w.st_fin);
    }
    // the decoder layers' cross-attention gradient buffers (xmem_dmem_all): pointers of the plan's own, uploaded once
    std::vector<XmemDmemLayer> dtab;
    for (int i = 0; i < cfg->N; ++i) {
        const DecA& a = p->w.dec[i];
        XmemDmemLayer e;
        e.probs = a.xprobs; e.dsc = a.dsc; e.dmbar = a.dmbar; e.qk = a.qk; e.dcp = a.dcp;
        e.dbv = p->G(p->L.dec[i].cin_b) + 2 * cfg->E; e.drop_site = p->dec_site(i, 2); e.pad = 0;
        dtab.push_back(e);
    }
    ok = ok && hipMemcpy(p->w.dmem_tab, dtab.data(), dtab.size() * sizeof(dtab[0]), hipMemcpyHostToDevice) == hipSuccess;
    ok = ok && hipMemcpy(p->w.ln_table, tab.data(), tab.size() * sizeof(tab[0]), hipMemcpyHostToDevice) == hipSuccess &&
         hipMemcpy(p->w.ln_ptable, ptab.data(), ptab.size() * sizeof(ptab[0]), hipMemcpyHostToDevice) == hipSuccess &&
         hipMemset(buf->grads, 0, p->L.total * sizeof(float)) == hipSuccess &&
         // the memset runs on the null stream, which does NOT order itself against the caller's non-blocking stream: without
         // this wait it can land after the first backward has written gradients (seen with several host threads, whose
         // initialisation kernels queue up on the null stream: grid scores differed from run to run)
         hipStreamSynchronize(nullptr) == hipSuccess;
    if (!ok) {
        set_error("tf_create: device initialisation failed: %s", hipGetErrorString(hipGetLastError()));
        slnlp_tf_destroy(p);
        return SLNLP_ERR_LAUNCH;
    }
    *out = p;
    return 0;
}

}  // extern "C"

// Decoder layer l up to its cross-attention query: self-attention over ONE key (softmax == 1 -> out_proj(v_proj(t));
// the q/k rows of in_proj are dead; in train mode the weight-1 "attention" is still dropped per (row, head) -- fused into
// the V projection), residual + norm1, then q = in_proj_q(t1) (transformer.py:82-87).  The layer's input t is the target
// embedding or the layer below's norm3 output -- that LayerNorm runs here, with the V projection that alone reads it on the chain.
int slnlp_tf_plan::dec_self_block(int l, int B, float p, hipStream_t st) const {
    const int E = cfg.E, dh = E / cfg.H;
    const DecP& q = L.dec[l];
    const DecA& a = w.dec[l];
    // (B-row products on planes, gemm_rows.hip: every producer also emits its output as the next product's operand)
    const Epi ev = Epi().dropped(p, dec_site(l, 0), dh).also(a.vp);
    const float* t = l == 0 ? w.t0 : w.dec[l - 1].t3;
    if (l == 0) {
        SLNLP_TRY(linear(rview(w.t0, w.t0p, E), q.sin_w + 2L * E * E, q.sin_b + 2 * E, B, E, E, a.v, ev, st));
    } else {
        const DecP& qb = L.dec[l - 1];
        const DecA& b = w.dec[l - 1];
        SLNLP_TRY(ln_linear(b.y3, qb.n3_w, qb.n3_b, b.t3, b.st3, b.t3p, q.sin_w + 2L * E * E, q.sin_b + 2 * E, B, E, a.v, ev, st));
    }
    SLNLP_TRY(linear(rview(a.v, a.vp, E), q.sout_w, q.sout_b, B, E, E, a.y1, Epi().dropped(p, dec_site(l, 1)).plus(t), st));
    return ln_linear(a.y1, q.n1_w, q.n1_b, a.t1, a.st1, a.t1p, q.cin_w, q.cin_b, B, E, a.q, Epi(), st);
}

int slnlp_tf_plan::forward_impl(const int64_t* X, const int64_t* y, int B, int train, float* logp_out, hipStream_t st) {
    const slnlp_tf_config& c = cfg;
    const int E = c.E, F = c.F, H = c.H, S = c.S, dh = E / H, M = S * B, Vp = (int)align_up(c.Vt, 4);
    const float p = train ? c.dropout : 0.f;
    const unsigned long long* rng = buf.rng;
    last_B = B; last_p = p; last_X = X; last_y = y;

    // The target side up to the first cross-attention (embedding, layer 0's single-key self-attention block and its
    // query projection: five B-row launches) depends on nothing the encoder computes; everything runs on the caller's
    // ONE stream in program order (round 1 forked it to a side stream: -3 % and a data race).
    const bool up = use_planes;
    if (up) {   // weights as bf16 planes: current unless the arena changed outside the fused optimizer step
        SLNLP_TRY(prepare_planes(B, st));
        SLNLP_TRY(ensure_wplanes(st));
        SLNLP_TRY(ensure_wq(st));
    }
    SLNLP_TRY(embed_fwd(y, 1, B, 1, E, c.Vt, P(L.tgt_emb), buf.pe, w.t0, sqrtf((float)E), p, SITE_TGT_EMB, rng, c.pad_tgt, st, rout(w.t0p)));
    SLNLP_TRY(dec_self_block(0, B, p, st));
    SLNLP_TRY(embed_fwd(X, S, B, S, E, c.Vs, P(L.src_emb), buf.pe, w.x0, sqrtf((float)E), p, SITE_SRC_EMB, rng, -1, st, pout(w.x0p), w.emb_keep));

    Mat x = view(w.x0, w.x0p, E);
    for (int l = 0; l < c.N; ++l) {
        const EncP& q = L.enc[l];
        const EncA& a = w.enc[l];
        SLNLP_TRY(linear(x, q.in_w, q.in_b, M, 3 * E, E, a.qkv, Epi(), st));
        // (ctx and, in backward, d qkv leave the attention kernels as planes only when the sequence fits the single-tile kernels:
        //  their fp32 copies have no reader in the plane path)
        SLNLP_TRY(attn_self_fwd(a.qkv, X, S, c.pad_src, 1, B, S, H, dh, (up && S <= 64) ? nullptr : a.ctx, a.probs, p, enc_site(l, 0), rng, st, pout(a.ctxp)));
        SLNLP_TRY(linear(view(a.ctx, a.ctxp, E), q.out_w, q.out_b, M, E, E, a.y1, Epi().dropped(p, enc_site(l, 1)).plus(x.f), st));
        SLNLP_TRY(layernorm_fwd(a.y1, P(q.n1_w), P(q.n1_b), M, E, 1e-5f, a.x1, a.st1, st, pout(a.x1p)));
        SLNLP_TRY(linear(view(a.x1, a.x1p, E), q.l1_w, q.l1_b, M, F, E, a.h, Epi().relu().dropped(p, enc_site(l, 2)).also(a.hp), st));
        SLNLP_TRY(linear(view(a.h, a.hp, F), q.l2_w, q.l2_b, M, E, F, a.y2, Epi().dropped(p, enc_site(l, 3)).plus(a.x1), st));
        SLNLP_TRY(layernorm_fwd(a.y2, P(q.n2_w), P(q.n2_b), M, E, 1e-5f, a.x2, a.st2, st, pout(a.x2p)));
        x = view(a.x2, a.x2p, E);
    }
    SLNLP_TRY(layernorm_fwd(x.f, P(L.encn_w), P(L.encn_b), M, E, 1e-5f, w.mem, w.st_mem, st, pout(w.memp)));

    // The decoder's LayerNorms go through ln_linear with the one product that reads them on the chain (one launch for both where
    // gemm_rows.hip's prologue kernel covers it): norm1 + the query projection and, for l > 0, the layer below's norm3 + the V
    // projection in dec_self_block; norm2 + linear1 here; the final norm + the generator behind the loop.  Only the last layer's
    // norm3 feeds a LayerNorm, not a product, and keeps its launch.
    for (int l = 0; l < c.N; ++l) {
        const DecP& q = L.dec[l];
        const DecA& a = w.dec[l];
        if (l > 0) SLNLP_TRY(dec_self_block(l, B, p, st));   // (layer 0's block ran ahead of the encoder, above)
        // cross-attention over the memory itself: with ONE query per sequence the K / V projections of the S memory rows
        // re-associate into B-row products (attention_mem.hip) -- no [S*B, 2E] projection, no K|V gradient GEMMs:
        // qk = Wk_h^T q_h (batched GEMM) -> scores / softmax / dropout / mbar (+ ctx0 = bv sum_s p_s) -> ctx = Wv_h mbar + ctx0
        // (... and as planes, for the out projection)
        const float *Wk = P(q.cin_w) + (long)E * E, *Wv = P(q.cin_w) + 2L * E * E;
        const slnlp_gemm_args j1 = head_expand(a.q, Wk, a.qk, B, H, dh, prec3());
        SLNLP_TRY(gemm_group(&j1, 1, st));
        SLNLP_TRY(xmem_fwd(a.qk, w.mem, P(q.cin_b) + 2 * E, B, S, H, dh, a.mbar, a.psum, a.xprobs, a.xctx, p, dec_site(l, 2), rng, st));
        const slnlp_gemm_args j2 = head_reduce(a.mbar, Wv, a.xctx, a.xctx, use_rows ? &a.xctxp : nullptr, B, H, dh, prec3());
        SLNLP_TRY(gemm_group(&j2, 1, st));
        SLNLP_TRY(linear(rview(a.xctx, a.xctxp, E), q.cout_w, q.cout_b, B, E, E, a.y2, Epi().dropped(p, dec_site(l, 3)).plus(a.t1), st));
        SLNLP_TRY(ln_linear(a.y2, q.n2_w, q.n2_b, a.t2, a.st2, a.t2p, q.l1_w, q.l1_b, B, F, a.h, Epi().relu().dropped(p, dec_site(l, 4)).also(a.hp), st));
        SLNLP_TRY(linear(rview(a.h, a.hp, F), q.l2_w, q.l2_b, B, E, F, a.y3, Epi().dropped(p, dec_site(l, 5)).plus(a.t2), st));
        if (l == c.N - 1) SLNLP_TRY(layernorm_fwd(a.y3, P(q.n3_w), P(q.n3_b), B, E, 1e-5f, a.t3, a.st3, st, rout(a.t3p)));
    }
    SLNLP_TRY(ln_linear(w.dec[c.N - 1].t3, L.decn_w, L.decn_b, w.tfin, w.st_fin, w.tfinp, L.lin_w, L.lin_b, B, c.Vt, w.logits, Epi().stride(Vp), st));
    // log_softmax (transformer.py:88-89) + the criterion skorch applies to it (helper.py:61-70)
    // the caller's copy of the log-probs is written by the same kernel (no device-to-device copy); in lockstep it lands
    // in the epoch buffer at the batch's row offset and the loss in the epoch's loss history
    SLNLP_TRY(lsm_nll(w.logits, Vp, y, B, c.Vt, c.pad_tgt, w.logp, buf.scalars, train ? w.dlogits : nullptr, Vp,
                      w.row_nll, st, nullptr, logp_out ? logp_out : ls_logp, logp_out ? nullptr : ls_dyn,
                      logp_out ? nullptr : ls_loss, (!logp_out && ls_dyn) ? ls_dyn + 1 : nullptr, opts.loss()));
    return 0;
}

extern "C" {

int slnlp_tf_forward(slnlp_tf_plan* pl, const int64_t* X, const int64_t* y, int B, int train, float* logp_out,
                     void* stream) {
    SLNLP_CHECK_ARG(pl && X && y, "tf_forward: `X` and `y` are required parameters");  // transformer.py:61-62
    SLNLP_CHECK_ARG(B > 0 && B <= pl->cfg.B, "tf_forward: batch %d outside 1..%d", B, pl->cfg.B);
    StepScope scope((hipStream_t)stream);
    SLNLP_TRY(scope.rc);
    return pl->forward_impl(X, y, B, train, logp_out, (hipStream_t)stream);
}

int slnlp_tf_seed_dlogp(slnlp_tf_plan* pl, const float* dlogp, void* stream) {
    SLNLP_CHECK_ARG(pl && dlogp && pl->last_B > 0, "tf_seed_dlogp: needs a prior forward");
    return lsm_bwd(pl->w.logp, dlogp, pl->last_B, pl->cfg.Vt, pl->w.dlogits, align_up(pl->cfg.Vt, 4), (hipStream_t)stream);
}

int slnlp_tf_backward(slnlp_tf_plan* pl, void* stream) {
    SLNLP_CHECK_ARG(pl && pl->last_B > 0, "tf_backward: needs a prior forward(train)");
    hipStream_t st = (hipStream_t)stream;
    StepScope scope(st);
    SLNLP_TRY(scope.rc);
    const slnlp_tf_config& c = pl->cfg;
    const Ws& w = pl->w;
    const Layout& L = pl->L;
    const int B = pl->last_B, E = c.E, F = c.F, H = c.H, S = c.S, dh = E / H, M = S * B, Vp = (int)align_up(c.Vt, 4);
    const float p = pl->last_p, ik = 1.f / (1.f - p);
    const unsigned long long* rng = pl->buf.rng;
    const int64_t *X = pl->last_X, *y = pl->last_y;
    const bool up = pl->use_planes;
    // Everything runs on the caller's stream; the weight gradient of each dY shares a launch with its data gradient -- but the
    // encoder's where the pair's launch would wait for it: those run in one batched launch behind the layer loop (tf_plan.hpp).

    // generator: logits = tfin lin_w^T + lin_b (fp32 operands in every mode)
    SLNLP_TRY(pl->linear_bwd(f32(w.dlogits, Vp), L.lin_w, L.lin_b, f32(w.tfin, E), B, c.Vt, E, w.gfin, Epi(), st));
    SLNLP_TRY(layernorm_bwd(w.gfin, w.dec[c.N - 1].t3, pl->P(L.decn_w), w.st_fin, B, E, nullptr, w.gtl, nullptr, 0.f, 0,
                            rng, nullptr, nullptr, 0, st));
    const float* dt = w.gtl;  // gradient w.r.t. the current decoder layer's output
    // d memory has no reader before the encoder's final LayerNorm: the layers leave it (and d bv) to one launch behind the loop
    float* const gmem_l = pl->dmem_batched ? nullptr : w.gmem;
    const bool ur = pl->use_rows;
    for (int l = c.N - 1; l >= 0; --l) {
        const DecP& q = L.dec[l];
        const DecA& a = w.dec[l];
        const Mat t_in = l > 0 ? pl->rview(w.dec[l - 1].t3, w.dec[l - 1].t3p, E) : pl->rview(w.t0, w.t0p, E);
        // Each LayerNorm backward emits the sub-layer's dY the way the pair reads it; every Linear's backward pair is ONE launch, whose
        // data gradient emits the next dY (B-row products: as planes; d h and d v then have no fp32 copy)
        // norm3 / FFN
        SLNLP_TRY(pl->ln_bwd_dy(ur, dt, a.y3, q.n3_w, a.st3, B, a.gA3, a.gB3, a.d3p, p, pl->dec_site(l, 5), nullptr, 0, st));
        SLNLP_TRY(pl->linear_bwd(pl->rview(p > 0.f ? a.gB3 : a.gA3, a.d3p, E), q.l2_w, q.l2_b, pl->rview(a.h, a.hp, F), B, E, F, ur ? nullptr : a.gh,
                                 Epi().gated(a.h, ik).also(a.ghp), st));
        SLNLP_TRY(pl->linear_bwd(pl->rview(a.gh, a.ghp, F), q.l1_w, q.l1_b, pl->rview(a.t2, a.t2p, E), B, F, E, a.gt2, Epi().plus(a.gA3), st));
        // norm2 / cross-attention
        SLNLP_TRY(pl->ln_bwd_dy(ur, a.gt2, a.y2, q.n2_w, a.st2, B, a.gA2, a.gB2, a.d2p, p, pl->dec_site(l, 3), nullptr, 0, st));
        SLNLP_TRY(pl->linear_bwd(pl->rview(p > 0.f ? a.gB2 : a.gA2, a.d2p, E), q.cout_w, q.cout_b, pl->rview(a.xctx, a.xctxp, E), B, E, E, a.gxctx, Epi(), st));
        // d ctx -> d mbar = Wv_h^T d ctx_h (batched GEMM) -> d scores, d qk (d memory, accumulated over the decoder layers in
        // layer order, and d bv: here per layer, or for all layers behind the loop -- dmem_batched) -> ONE launch of three batched jobs: d q_h = Wk_h d qk, d Wk_h = q_h^T (x) d qk, d Wv_h = d ctx_h^T (x) mbar.
        // d bk is exactly zero (a shift of all scores): nothing writes it, the gradient arena was zeroed at plan creation.
        {
            const float *Wk = pl->P(q.cin_w) + (long)E * E, *Wv = pl->P(q.cin_w) + 2L * E * E;
            const int pr = pl->prec3();
            const slnlp_gemm_args j1 = head_expand(a.gxctx, Wv, a.dmbar, B, H, dh, pr);
            SLNLP_TRY(gemm_group(&j1, 1, st));
            SLNLP_TRY(xmem_bwd(w.mem, pl->P(q.cin_b) + 2 * E, a.xprobs, a.psum, a.qk, a.dmbar, a.gxctx, B, S, H, dh, a.dsc, a.dqk, a.dcp,
                               pl->G(q.cin_b) + 2 * E, gmem_l, l == c.N - 1 ? 0 : 1, p, pl->dec_site(l, 2), rng, st));
            const slnlp_gemm_args jobs[3] = {head_reduce(a.dqk, Wk, a.gq, nullptr, ur ? &a.gqp : nullptr, B, H, dh, pr),
                                             head_wgrad(a.q, a.dqk, pl->G(q.cin_w) + (long)E * E, B, H, dh, pr),
                                             head_wgrad(a.gxctx, a.mbar, pl->G(q.cin_w) + 2L * E * E, B, H, dh, pr)};
            SLNLP_TRY(gemm_group(jobs, 3, st));
        }
        SLNLP_TRY(pl->linear_bwd(pl->rview(a.gq, a.gqp, E), q.cin_w, q.cin_b, pl->rview(a.t1, a.t1p, E), B, E, E, a.gt1, Epi().plus(a.gA2), st));
        // norm1 / self-attention (single key; its per-(row, head) dropout: the same mask as the forward V projection)
        SLNLP_TRY(pl->ln_bwd_dy(ur, a.gt1, a.y1, q.n1_w, a.st1, B, a.gA1, a.gB1, a.d1p, p, pl->dec_site(l, 1), nullptr, 0, st));
        SLNLP_TRY(pl->linear_bwd(pl->rview(p > 0.f ? a.gB1 : a.gA1, a.d1p, E), q.sout_w, q.sout_b, pl->rview(a.v, a.vp, E), B, E, E, ur ? nullptr : a.gv,
                                 Epi().dropped(p, pl->dec_site(l, 0), p > 0.f ? dh : 0).also(a.gvp), st));
        // softmax over one element has zero gradient: the q/k rows of in_proj (weight and bias) get exactly 0.
        // Nothing ever writes them, and the gradient arena is zeroed at plan creation, so they stay zero.
        SLNLP_TRY(pl->linear_bwd(pl->rview(a.gv, a.gvp, E), q.sin_w + 2L * E * E, q.sin_b + 2 * E, t_in, B, E, E, a.gt0, Epi().plus(a.gA1), st));
        dt = a.gt0;
    }
    if (pl->dmem_batched) SLNLP_TRY(xmem_dmem_all(w.dmem_tab, c.N, B, S, H, dh, w.gmem, p, rng, st));
    SLNLP_TRY(embed_bwd(y, 1, B, 1, E, c.Vt, dt, pl->G(L.tgt_emb), sqrtf((float)E), -1, p, SITE_TGT_EMB, rng, w.emb_scratch_tgt, st));

    // encoder: needs the complete d memory
    // (a tall batch: the encoder's LayerNorm backward kernels also write their (dgamma, dbeta) chunk sums, elementwise.hip)
    const int Mfull = c.B * c.S;
    const bool lnf = ln_bwd_fused(Mfull);
    SLNLP_TRY(layernorm_bwd(w.gmem, w.enc[c.N - 1].x2, pl->P(L.encn_w), w.st_mem, M, E, nullptr, w.gxl, nullptr, 0.f, 0,
                            rng, lnf ? w.lnp_mem : nullptr, nullptr, Mfull, st));
    const float* dx = w.gxl;
    for (int l = c.N - 1; l >= 0; --l) {
        const EncP& q = L.enc[l];
        const EncA& a = w.enc[l];
        // LayerNorm backward also emits the bf16 planes of the gradient that feeds the sub-layer's GEMMs
        // (the dropout-masked copy when dropout is on, else dx itself)
        // (plane path: the sub-layer's GEMMs read the planes only, so neither the masked fp32 copy nor the fp32 ReLU-gated
        //  gradient of the FFN hidden layer is stored)
        SLNLP_TRY(pl->ln_bwd_dy(up, dx, a.y2, q.n2_w, a.st2, M, a.gA2, a.gB2, a.d2p, p, pl->enc_site(l, 3), lnf ? a.lnp2 : nullptr, Mfull, st));
        SLNLP_TRY(pl->enc_pair_launch(l, 0, B, st));     // linear2: d h (ReLU-gated)
        SLNLP_TRY(pl->enc_pair_launch(l, 1, B, st));     // linear1: d x1 (+ the residual branch)
        SLNLP_TRY(pl->ln_bwd_dy(up, a.gx1, a.y1, q.n1_w, a.st1, M, a.gA1, a.gB1, a.d1p, p, pl->enc_site(l, 1), lnf ? a.lnp1 : nullptr, Mfull, st));
        SLNLP_TRY(pl->enc_pair_launch(l, 2, B, st));     // out_proj: d ctx
        SLNLP_TRY(attn_self_bwd(a.qkv, a.probs, a.gctx, B, S, H, dh, (up && S <= 64) ? nullptr : a.gqkv, p, pl->enc_site(l, 0), rng, st, pl->pout(a.gqkvp), w.attn_scratch));
        SLNLP_TRY(pl->enc_pair_launch(l, 3, B, st));     // in_proj: d x0 (+ the residual branch)
        dx = a.gx0;
    }
    // the weight gradients the loop left behind (tf_plan.hpp: enc_pair_launch), all in one launch; nothing below reads a dW
    if (up && !recording()) SLNLP_TRY(plane_batch_launch(pl->wbatch, w.wb_tab, w.wb_map, st));
    SLNLP_TRY(embed_bwd(X, S, B, S, E, c.Vs, dx, pl->G(L.src_emb), sqrtf((float)E), -1, p, SITE_SRC_EMB, rng, w.emb_scratch_src, st, w.emb_keep));
    // every LayerNorm's (dgamma, dbeta): chunk sums in one launch, then the chunks added in order
    SLNLP_TRY(ln_param_partial(w.ln_ptable, nullptr, 5 * c.N + 2, E, M, B, c.B * c.S, c.B, st));
    SLNLP_TRY(ln_param_reduce(w.ln_table, 5 * c.N + 2, E, st));
    return 0;
}

int slnlp_tf_optim(slnlp_tf_plan* pl, float momentum, float max_norm, void* stream) {
    SLNLP_CHECK_ARG(pl, "tf_optim: null plan");
    return pl->update_sgd(momentum, max_norm, (hipStream_t)stream);
}

int slnlp_tf_optim_adam(slnlp_tf_plan* pl, float* exp_avg_sq, float beta1, float beta2, float eps, float weight_decay,
                        float max_norm, void* stream) {
    SLNLP_CHECK_ARG(pl && exp_avg_sq, "tf_optim_adam: null argument");
    return pl->update_adam(exp_avg_sq, beta1, beta2, eps, weight_decay, max_norm, (hipStream_t)stream);
}

int slnlp_tf_set_destroy_sync(slnlp_tf_plan* pl, int on) {
    SLNLP_CHECK_ARG(pl, "tf_set_destroy_sync: null plan");
    pl->destroy_sync = on ? 1 : 0;
    return 0;
}

int slnlp_tf_set_dmem_batched(slnlp_tf_plan* pl, int on) {
    SLNLP_CHECK_ARG(pl, "tf_set_dmem_batched: null plan");
    if (pl->dmem_batched == (on != 0)) return 0;
    pl->dmem_batched = on != 0;
    ++pl->opts.gen;            // a lockstep group re-records its programs: the launch sequence changed
    pl->drop_graphs();
    return 0;
}

int slnlp_tf_set_dec_ln_fused(slnlp_tf_plan* pl, int on) {
    SLNLP_CHECK_ARG(pl, "tf_set_dec_ln_fused: null plan");
    if (pl->dec_ln_fused == (on != 0)) return 0;
    pl->dec_ln_fused = on != 0;
    ++pl->opts.gen;            // (as every switch of the launch sequence; a recorded program itself never holds the fused launch)
    pl->drop_graphs();
    return 0;
}

int slnlp_tf_set_criterion(slnlp_tf_plan* pl, const float* class_weight, float label_smoothing, int reduction, void* stream) {
    SLNLP_CHECK_ARG(pl, "tf_set_criterion: null plan");
    return pl->set_criterion(class_weight, label_smoothing, reduction, (hipStream_t)stream);
}

int slnlp_tf_set_update(slnlp_tf_plan* pl, int kind, float dampening, float weight_decay, int nesterov) {
    SLNLP_CHECK_ARG(pl, "tf_set_update: null plan");
    return pl->set_update(kind, dampening, weight_decay, nesterov);
}

int slnlp_tf_set_param_groups(slnlp_tf_plan* pl, int n_segments, const int64_t* seg_begin, const int32_t* seg_group, int n_groups,
                              const float* weight_decay, const float* lr_dev, void* stream) {
    SLNLP_CHECK_ARG(pl, "tf_set_param_groups: null plan");
    return pl->set_param_groups("tf_set_param_groups", n_segments, seg_begin, seg_group, n_groups, weight_decay, lr_dev, (hipStream_t)stream);
}

int slnlp_tf_set_averaging(slnlp_tf_plan* pl, float* avg, float* count, int kind, float decay) {
    SLNLP_CHECK_ARG(pl, "tf_set_averaging: null plan");
    return pl->set_averaging("tf_set_averaging", avg, count, kind, decay);
}

// The parameter arena was written from outside the library (load_state_dict, a torch optimizer, an in-place edit):
// derived data is stale.  The Python engines call this when the arena tensor's version counter has moved.
int slnlp_tf_params_changed(slnlp_tf_plan* pl) {
    SLNLP_CHECK_ARG(pl, "tf_params_changed: null plan");
    bump_params_generation(pl->buf.params);
    return 0;
}

int slnlp_tf_train_step(slnlp_tf_plan* pl, const int64_t* X, const int64_t* y, int B, float momentum, float max_norm,
                        float* logp, void* stream) {
    SLNLP_CHECK_ARG(pl, "tf_forward: `X` and `y` are required parameters");      // (what the step's forward says about a null plan)
    return pl->train_step(X, y, nullptr, B, momentum, max_norm, logp, (hipStream_t)stream);
}

int slnlp_tf_graph_capture_train(slnlp_tf_plan* pl, const int64_t* X, const int64_t* y, int B, float momentum,
                                 float max_norm, float* logp, void* stream) {
    SLNLP_CHECK_ARG(pl, "tf_graph_capture_train: needs a plan and a non-default stream");
    return pl->graph_capture_train("tf_graph_capture_train", X, y, nullptr, B, momentum, max_norm, logp, (hipStream_t)stream);
}

int slnlp_tf_graph_launch(slnlp_tf_plan* pl, int B, void* stream) {
    SLNLP_CHECK_ARG(pl, "tf_graph_launch: null plan");
    return pl->graph_launch("tf_graph_launch", B, (hipStream_t)stream);
}

// Debug helper: "name offset" lines (byte offsets into the workspace, in carve order) of every fp32 activation /
// gradient buffer -- lets a test locate a difference between two plans' workspaces.
int slnlp_tf_debug_layout(const slnlp_tf_config* cfg, char* out, int64_t out_bytes) {
    SLNLP_TRY(check_cfg(cfg));
    SLNLP_CHECK_ARG(out && out_bytes > 0, "tf_debug_layout: no output buffer");
    const Ws w = carve(*cfg, nullptr);
    std::string s;
    bool first = true;          // (only the very first buffer may sit at offset 0: any other null pointer is a buffer this configuration does not carve)
    auto add = [&](const std::string& n, const void* p) {
        if (p == nullptr && !first) return;
        first = false;
        s += n + " " + std::to_string((size_t)(const char*)p) + "\n";
    };
#define F(pre, st, f) add(pre + std::string(#f), st.f)
    add("x0", w.x0); add("t0", w.t0);
    for (int i = 0; i < cfg->N; ++i) {
        const EncA& a = w.enc[i];
        const std::string pre = "enc" + std::to_string(i) + ".";
        F(pre, a, qkv); F(pre, a, probs); F(pre, a, ctx); F(pre, a, y1); F(pre, a, st1); F(pre, a, x1); F(pre, a, h); F(pre, a, y2); F(pre, a, st2);
        F(pre, a, x2); F(pre, a, lnp1); F(pre, a, lnp2); F(pre, a, gA2); F(pre, a, gB2); F(pre, a, gh); F(pre, a, gx1); F(pre, a, gA1); F(pre, a, gB1);
        F(pre, a, gctx); F(pre, a, gqkv); F(pre, a, gx0);
    }
    add("mem", w.mem); add("st_mem", w.st_mem); add("lnp_mem", w.lnp_mem);
    for (int i = 0; i < cfg->N; ++i) {
        const DecA& a = w.dec[i];
        const std::string pre = "dec" + std::to_string(i) + ".";
        F(pre, a, v); F(pre, a, y1); F(pre, a, st1); F(pre, a, t1); F(pre, a, q); F(pre, a, qk); F(pre, a, mbar); F(pre, a, psum); F(pre, a, xprobs); F(pre, a, xctx); F(pre, a, y2);
        F(pre, a, st2); F(pre, a, t2); F(pre, a, h); F(pre, a, y3); F(pre, a, st3); F(pre, a, t3); F(pre, a, lnp1); F(pre, a, lnp2); F(pre, a, lnp3);
        F(pre, a, gA3); F(pre, a, gB3); F(pre, a, gh); F(pre, a, gt2); F(pre, a, gA2); F(pre, a, gB2); F(pre, a, gxctx); F(pre, a, gq); F(pre, a, dmbar); F(pre, a, dsc); F(pre, a, dqk); F(pre, a, dcp);
        F(pre, a, gt1); F(pre, a, gA1); F(pre, a, gB1); F(pre, a, gv); F(pre, a, gt0);
    }
#undef F
    add("tfin", w.tfin); add("st_fin", w.st_fin); add("lnp_fin", w.lnp_fin); add("logits", w.logits); add("dlogits", w.dlogits);
    add("logp", w.logp); add("row_nll", w.row_nll); add("gfin", w.gfin); add("gtl", w.gtl); add("gmem", w.gmem); add("gxl", w.gxl);
    add("emb_scratch_src", w.emb_scratch_src); add("emb_scratch_tgt", w.emb_scratch_tgt); add("emb_keep", w.emb_keep);
    add("opt_partials", w.opt_partials); add("ln_table", w.ln_table); add("wp.hi", w.wp.hi); add("wp.lo", w.wp.lo);
    add("planes_begin", w.planes_begin); add("gscr0", w.gscr[0]); add("planes_end", w.planes_end);
    add("end", (const char*)nullptr + w.bytes);
    SLNLP_CHECK_ARG((int64_t)s.size() + 1 <= out_bytes, "tf_debug_layout: needs %zu bytes", s.size() + 1);
    memcpy(out, s.c_str(), s.size() + 1);
    return 0;
}

int slnlp_tf_tap(slnlp_tf_plan* pl, const char* name, float* out, int64_t max_floats, int64_t* n_out, void* stream) {
    SLNLP_CHECK_ARG(pl && name && out && pl->last_B > 0, "tf_tap: bad args / no forward yet");
    const slnlp_tf_config& c = pl->cfg;
    const int B = pl->last_B, M = B * c.S, E = c.E, Vp = (int)align_up(c.Vt, 4);
    const std::string n(name);
    const float* src = nullptr;
    int64_t rows = 0, cols = E, ld = E;
    if (n == "src_embed") { src = pl->w.x0; rows = M; }
    else if (n == "tgt_embed") { src = pl->w.t0; rows = B; }
    else if (n == "memory") { src = pl->w.mem; rows = M; }
    else if (n == "dmemory") { src = pl->w.gmem; rows = M; }
    else if (n == "logits") { src = pl->w.logits; rows = B; cols = c.Vt; ld = Vp; }
    else if (n == "dlogits") { src = pl->w.dlogits; rows = B; cols = c.Vt; ld = Vp; }
    else if (n.rfind("enc", 0) == 0 && n.find('.') != std::string::npos) {
        // "enc<l>.<planes>": an operand of the layer's gradient GEMMs as the bf16 planes the kernels read -- the hi plane's [rows, cols]
        // 16-bit words, then the lo plane's, packed into rows * cols floats
        const int l = atoi(name + 3);
        SLNLP_CHECK_ARG(l >= 0 && l < c.N && pl->use_planes, "tf_tap: %s", name);
        const EncA& a = pl->w.enc[l];
        const std::string f = n.substr(n.find('.') + 1);
        const PP* q = f == "d2p" ? &a.d2p : f == "hp" ? &a.hp : f == "ghp" ? &a.ghp : f == "x1p" ? &a.x1p : f == "d1p" ? &a.d1p : f == "ctxp" ? &a.ctxp :
                      f == "gqkvp" ? &a.gqkvp : f == "x2p" ? &a.x2p : f == "xinp" ? (l > 0 ? &pl->w.enc[l - 1].x2p : &pl->w.x0p) : nullptr;
        SLNLP_CHECK_ARG(q, "tf_tap: unknown tap '%s'", name);
        cols = (f == "hp" || f == "ghp") ? c.F : f == "gqkvp" ? 3 * E : E;
        const int64_t words = (int64_t)M * cols;
        SLNLP_CHECK_ARG(words <= max_floats, "tf_tap: buffer too small (%ld needed)", (long)words);
        if (hipMemcpyAsync(out, q->hi, words * 2, hipMemcpyDeviceToDevice, (hipStream_t)stream) != hipSuccess ||
            hipMemcpyAsync(reinterpret_cast<char*>(out) + words * 2, q->lo, words * 2, hipMemcpyDeviceToDevice, (hipStream_t)stream) != hipSuccess) {
            set_error("tf_tap: copy failed");
            return SLNLP_ERR_LAUNCH;
        }
        if (n_out) *n_out = words;
        return 0;
    }
    else if (n.rfind("enc", 0) == 0) { int l = atoi(name + 3); SLNLP_CHECK_ARG(l >= 0 && l < c.N, "tf_tap: %s", name); src = pl->w.enc[l].x2; rows = M; }
    else if (n.rfind("dec", 0) == 0) { int l = atoi(name + 3); SLNLP_CHECK_ARG(l >= 0 && l < c.N, "tf_tap: %s", name); src = pl->w.dec[l].t3; rows = B; }
    SLNLP_CHECK_ARG(src, "tf_tap: unknown tap '%s'", name);
    SLNLP_CHECK_ARG(rows * cols <= max_floats, "tf_tap: buffer too small (%ld needed)", (long)(rows * cols));
    if (hipMemcpy2DAsync(out, cols * sizeof(float), src, ld * sizeof(float), cols * sizeof(float), rows,
                         hipMemcpyDeviceToDevice, (hipStream_t)stream) != hipSuccess) {
        set_error("tf_tap: copy failed");
        return SLNLP_ERR_LAUNCH;
    }
    if (n_out) *n_out = rows * cols;
    return 0;
}

}  // extern "C"
