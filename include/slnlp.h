/* slnlp.h -- C ABI of libslnlp.so, the MI355X (gfx950) hot path for
 * amorim-cleison/sign-language-nlp.
 *
 * The reference has no native code and no FFI: its hot path is the Python
 * call `module(**{"X","lengths","y"})` + criterion + backward + clip + SGD that
 * skorch issues per batch.  The entry points below are
 * what a binding for that path attaches to; each cites the reference interface
 * it replaces as /root/reference/<file>:<line>.
 *
 * Conventions
 *  - plain pointers + sizes, no torch types; every pointer is a DEVICE pointer
 *    into memory the caller owns (the library never allocates or frees
 *    persistent memory); `stream` is a hipStream_t passed as void*;
 *  - all floating-point tensors are fp32 row-major; token ids / labels /
 *    lengths are int64 exactly as `collate_data` builds them (helper.py:293-304);
 *  - activations are sequence-first like the reference: token row m = s*B + b;
 *  - return 0 on success, an SLNLP_ERR_* code otherwise (never aborts);
 *    `slnlp_last_error()` returns a thread-local message;
 *  - every launch is asynchronous on `stream` and hipGraph-capturable (no
 *    allocation, no synchronisation inside).
 */
#ifndef SLNLP_H
#define SLNLP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SLNLP_OK 0
#define SLNLP_ERR_INVALID_ARG 1
#define SLNLP_ERR_LAUNCH 2
#define SLNLP_ERR_UNSUPPORTED 3

#define SLNLP_ABI_VERSION 1

const char* slnlp_last_error(void);
int slnlp_abi_version(void);

/* ------------------------------------------------------------------ GEMM --
 * C[M,N] = epilogue( sum_k A(m,k) * B(n,k) ) on bf16 MFMA with fp32
 * accumulate.  Replaces every torch.nn.Linear / in_proj / out_proj matmul the
 * reference reaches through nn.Transformer (model/transformer.py:40-48,82-88)
 * and nn.LSTM/GRU/Linear (model/base/encoder_decoder_attn_bkp.py:95-100,
 * 186-200,297-299), and their autograd backward (dgrad / wgrad).
 *
 * Operand (i,k) lives at ptr + i*ld + k when *_kmajor, else at ptr + k*ld + i.
 *   forward   y = x W^T      : A=x   kmajor, B=W  kmajor
 *   dgrad     dx = dy W      : A=dy  kmajor, B=W  NOT kmajor (k = W row)
 *   wgrad     dW = dy^T x    : A=dy  NOT kmajor, B=x NOT kmajor (k = token)
 * precision: 1 = single bf16 pass (~5e-3 rel); 3 = split-bf16 hi/lo, three MFMA
 * passes (~2e-5 rel, the parity-grade default).
 * Epilogue order: +bias[n] -> activation (relu: 1 = ReLU, 2 = tanh) -> *gate -> dropout -> +resid.
 * gate_mode 0: C *= (gate > 0 ? gate_scale : 0)   (ReLU + inverted-dropout backward, gate = saved output)
 * gate_mode 1: C *= (1 - gate^2)                   (tanh backward, gate = saved tanh output)
 */
typedef struct slnlp_gemm_args {
    const float* A; int64_t lda; int32_t a_kmajor;
    const float* B; int64_t ldb; int32_t b_kmajor;
    float* C; int64_t ldc;
    int32_t M, N, K;
    const float* bias;            /* [N] or NULL */
    int32_t relu;                 /* max(x,0) after bias */
    const float* gate; int64_t ldg; float gate_scale; /* C *= gate>0 ? gate_scale : 0 (ReLU+dropout backward) */
    float drop_p; int32_t drop_site; const unsigned long long* rng; /* inverted dropout, mask regenerated from rng */
    const float* resid; int64_t ldr; /* added last; may alias C */
    float* rowsum_a;              /* [M] or NULL: sum_k A(m,k) (bias grad fused into wgrad) */
    int32_t precision;            /* 1 or 3 */
    int32_t gate_mode;            /* see above */
    /* Optional PRE-SPLIT operands (bf16 hi / lo planes, row-major, rows and columns zero-padded to
     * multiples of 64, row stride ld*_p elements).  When A_hi and B_hi are set the GEMM stages them by
     * LDS-DMA and does no conversion (A, B, lda, ldb are then ignored; *_lo required for precision 3).
     * C_hi / C_lo (optional): also emit the result as planes for the next GEMM. C may then be NULL.
     * Every GEMM (slnlp_gemm, slnlp_gemm_group, slnlp_gemm_rows, slnlp_gemm_rows_bwd) stores plane words (m < M, n < N) only:
     * the words past (M, N) -- inside the 64-aligned box and beyond -- are left as they are, never zeroed.  The zero padding the
     * next GEMM reads therefore comes from the planes' allocation, and survives every producer. */
    const uint16_t* A_hi; const uint16_t* A_lo; int64_t lda_p;
    const uint16_t* B_hi; const uint16_t* B_lo; int64_t ldb_p;
    uint16_t* C_hi; uint16_t* C_lo; int64_t ldc_p;
    /* > 0: the dropout of this GEMM is per (row, head) instead of per element -- element (m, n) keeps or drops
     * with site element (m * (N / drop_head_dim) + n / drop_head_dim, 0).  That is nn.MultiheadAttention's
     * attention-weight dropout when there is a single key (decoder self-attention, tgt length 1): the softmax
     * weight is the scalar 1 per (row, head).  fp32-operand GEMMs only. */
    int32_t drop_head_dim;
    /* precision 8 -- "fp8 MFMA weights" (BASELINE.json configs[4]), forward products only, both operands k-major:
     * A_hi / B_hi are then OCP e4m3 BYTE planes (row strides lda_p / ldb_p in bytes; rows zero-padded to multiples of 64, K
     * to multiples of 128), contracted on the fp8 MFMA; col_scale[n] (optional) multiplies column n of the product -- the
     * per-row scale of a quantised weight matrix.  C_q8 (optional): also emit the result as an e4m3 plane, row stride ldc_p. */
    const float* col_scale;
    uint8_t* C_q8;
    /* batch > 1 (fp32-operand jobs of slnlp_gemm_group only): the job is `batch` GEMMs of this shape; GEMM z reads
     * A + z * batch_stride_a, B + z * batch_stride_b and writes C + z * batch_stride_c (resid, when set, moves with C) --
     * e.g. the per-head products of the decoder's cross-attention (attention_mem.hip).  0 or 1: a single GEMM. */
    int32_t batch;
    int64_t batch_stride_a, batch_stride_b, batch_stride_c;
} slnlp_gemm_args;

int slnlp_gemm(const slnlp_gemm_args* args, void* stream);
/* Grouped launch: up to 4 independent GEMMs (all with pre-split plane operands, or all with fp32 operands -- then
 * split_k / scratch are ignored) in ONE kernel launch -- e.g. the data gradient
 * and the weight gradient of one dY, which replace autograd's separate mm calls for nn.Linear
 * (transformer.py:40-48 -> torch).  split_k[i] > 1 (or NULL = all 1) divides job i's K loop over that many
 * workgroups per output tile; the partial tiles meet in `scratch` and are added in split order by the last
 * workgroup to arrive, so the result is deterministic (no float atomics).  scratch: at least
 * slnlp_gemm_group_scratch_bytes(...) bytes, 16-byte aligned, its first 16 KiB zero before the first use (the
 * library leaves them zero); one scratch buffer must not serve two launches that may run concurrently. */
int64_t slnlp_gemm_group_scratch_bytes(const slnlp_gemm_args* jobs, const int32_t* split_k, int njobs);
/* Output tile of the plane-GEMM launches: 0 = automatic (128 x 128 once a launch holds >= 200 of them -- merged lockstep
 * launches, the configs[4] shapes, cfg2's in_proj gradients -- 256 x 256 for forward launches with K >= 1024 that fill the
 * chip's rounds; 96 x 64 for a launch of ONE job with k-major A and no split-K that is more than one workgroup per CU at
 * 64 x 64 and at most one at 96 x 64 -- cfg2's 2400-row products with N = 512; else 64 x 64); forced: 64, 128 (128 x 128,
 * 64-k stages), 12832 (128 x 128, 32-k stages), 256 (256 x 256, 32-k stages), 96 (96 x 64 wherever it can run -- one job,
 * k-major A, no split-K -- and 64 x 64 for every other launch).  A tuning / test knob: results do not depend on it (the K
 * partition, hence every element's accumulation order, is the same for every geometry). */
int slnlp_set_plane_tile(int tile);
/* The geometry a launch of these plane jobs takes (slnlp_gemm / slnlp_gemm_group; split_k may be NULL): index into
 * {64 x 64, 128 x 128 64-k, 128 x 128 32-k, 256 x 256 32-k, 96 x 64}.  Reads shapes, layouts and the knob above only: no device. */
int slnlp_plane_geo(const slnlp_gemm_args* jobs, const int32_t* split_k, int njobs);
/* Thread groups per workgroup of the fp32-operand GEMM launches (slnlp_gemm, fp32 jobs of slnlp_gemm_group, the plans' 50-row
 * products): 0 = automatic (two -- each walks one half of the K tiles -- for launches of <= 128 workgroups with at least four K
 * tiles; one for everything larger, merged lockstep launches included), 1 or 2 forced.  A tuning / test knob: the K sum is
 * defined as (first half of the tiles) + (second half) whichever way it is scheduled, so results do not depend on it. */
int slnlp_set_gemm_ks(int ks);
/* Tile of the fused recurrent forward timestep (slnlp_rnn_step_fwd) when ONE fit launches it: 1 (default) = 16 batch rows x 16
 * hidden units x all gates per workgroup -- 256 workgroups at B = 50, Hd = 512, two directions, 160 KB of operands each -- 0 = the
 * 64-row tile (64 workgroups of 256 KB) that merged lockstep launches keep.  A tuning / test knob: same K order, same cell
 * arithmetic per element, same bits.  Env: SLNLP_RNN_STEP_RT. */
int slnlp_set_rnn_step_tile(int rows16);
/* the same knob for precision-8 launches: 0 = automatic (128 x 128 once the launch holds >= 512 of them), 64 or 128 */
int slnlp_set_fp8_tile(int tile);
int slnlp_gemm_group(const slnlp_gemm_args* jobs, const int32_t* split_k, int njobs, void* scratch,
                     int64_t scratch_bytes, void* stream);
/* The gradient pair of one dY over plane operands -- wgrad: dW = dY^T x (A, B not k-major, rowsum_a = db), dgrad: dX = dY W (A k-major,
 * B not) -- launched the way the training plans launch it: the library picks the weight gradient's K-split and whether the two
 * share ONE grouped launch (the weight gradient's workgroups fill the CUs the data gradient leaves idle) or, when both are large,
 * take a launch each with the tile that suits each.  scratch as for slnlp_gemm_group with split factors up to 8.
 * slnlp_gemm_wd_plan reports the choice (geometry codes: 0 = 64 x 64, 1 = 128 x 128 / 64-k, 2 = 128 x 128 / 32-k, 3 = 256 x 256). */
int slnlp_gemm_wd(const slnlp_gemm_args* wgrad, const slnlp_gemm_args* dgrad, void* scratch, int64_t scratch_bytes, void* stream);
int slnlp_gemm_wd_plan(const slnlp_gemm_args* wgrad, const slnlp_gemm_args* dgrad, int32_t* split, int32_t* separate, int32_t* geo_wgrad,
                       int32_t* geo_dgrad);
/* The decoder's products: the reference decodes ONE target position (transformer.py:82-87), so every nn.Linear of its
 * decoder (and the generator, transformer.py:46-48,88) is y[B rows, N] = x[B rows, K] W[N, K]^T on a dependent chain.
 * x as k-major bf16 hi / lo planes (A_hi / A_lo / lda_p; rows zero-padded to multiples of 64, stride a multiple of 64 covering
 * K), the weight W as fp32 (B / ldb, k-major, K a multiple of 64): the kernel splits it in registers -- hi = bf16(w), lo =
 * bf16(w - hi), the bits a plane of W would hold -- so nobody maintains planes of these weights.  Each wave loads its MFMA
 * fragments straight from memory: no LDS staging, no barrier in the K loop.  Same epilogue fields as slnlp_gemm (bias, relu,
 * gate, dropout incl. drop_head_dim, resid, C and / or C_hi / C_lo); the K sum is per 64-k tile: partial products from zero, added
 * in tile order.  Meant for up to 64 rows (one block of rows; more work, the plans use the plane GEMM there). */
int slnlp_gemm_rows(const slnlp_gemm_args* args, void* stream);
/* slnlp_layernorm_fwd followed by slnlp_gemm_rows on its output, in ONE launch and with their bits: x [M, K] (row stride ldx) is
 * the LayerNorm's INPUT; every 16 x 16-tile workgroup normalises its 16 rows itself (the stand-alone kernel's row arithmetic),
 * splits them and contracts them with W as slnlp_gemm_rows does.  args as for slnlp_gemm_rows, A_hi / A_lo / lda_p not read.
 * The first column tile's workgroups also store what the LayerNorm launch stores, for rows < M: y [M, K] (row stride K), (mean,
 * rstd) to stats [M, 2] (or NULL) and y as planes y_hi / y_lo (row stride ldp; both or neither) -- rows >= M of the planes stay
 * as they are.  K a multiple of 64, at most 1024; the launch must be one that takes the 16 x 16 tile (slnlp_set_rows_tile -1 or
 * 0); x and y (and resid / gate and y) must not overlap -- other workgroups still read while the first column tile's write. */
int slnlp_gemm_rows_ln(const slnlp_gemm_args* args, const float* x, int64_t ldx, const float* gamma, const float* beta, float eps,
                       float* y, float* stats, uint16_t* y_hi, uint16_t* y_lo, int64_t ldp, void* stream);
/* The backward pair of such a product in ONE launch (autograd's two mm calls for nn.Linear at batch rows):
 *   dgrad: dX[B rows, Kin] = dY[B rows, Nout] W[Nout, Kin] (+ the slnlp_gemm epilogue: gate, dropout, residual, planes out) --
 *          A = dY planes k-major, B = W as fp32 (B / ldb), NOT k-major (m-major: k = W's row; Nout a multiple of 64, Kin of 4);
 *   wgrad: dW[Nout, Kin] = dY^T x, rowsum_a = db[Nout] = column sums of dY (optional; computed as dY^T 1 on the MFMA) -- A = the same
 *          dY planes, B = x planes, both NOT k-major, K = the batch rows (plane rows beyond them must be zero), C = dW fp32, no epilogue.
 * Same precision for both; K sums per 64-k tile in tile order, as slnlp_gemm_rows. */
int slnlp_gemm_rows_bwd(const slnlp_gemm_args* dgrad, const slnlp_gemm_args* wgrad, void* stream);
/* Output tile of slnlp_gemm_rows launches: -1 = automatic (16 x 16 for one fit's launch -- it is bound by what ONE compute unit can
 * load, so the panels are spread over as many as possible -- 64 x 16 or 64 x 32 for the merged launches of fits in lockstep, which
 * pay for total bytes instead); 0 / 1 / 2 force 16 x 16, 64 x 16, 64 x 32.  A tuning / test knob: the K sum is defined per 64-k
 * tile (partial products added in tile order), so results do not depend on it. */
int slnlp_set_rows_tile(int tile);
/* fp32 [R,K] rows (row stride ld) -> OCP e4m3 rows with one fp32 scale per row: scale[r] = max|x[r,:]| / 448 (1 for an
 * all-zero row), q[r,k] = e4m3(x[r,k] / scale[r]); row stride of q = ldq bytes.  The weight operand of precision 8. */
int slnlp_quant_rows_fp8(const float* x, int64_t ld, int R, int K, uint8_t* q, int64_t ldq, float* scale, void* stream);
/* fp32 [R,C] (row stride ld) -> bf16 hi/lo planes with row stride ldp (lo may be NULL); writes the valid
 * region only -- the planes' zero padding comes from their allocation. */
int slnlp_split_planes(const float* x, int64_t ld, int R, int C, uint16_t* hi, uint16_t* lo, int64_t ldp, void* stream);

/* ------------------------------------------------------------- embedding --
 * x[s*B+b, :] = table[ids[b,s], :] * sqrt(E) + pe[s, :], then dropout.
 * model/transformer.py:106-109 forward_embedding; positional_encoding.py:48-49.
 * ids is batch-first int64 [B,S] with row stride ld_ids (for y: S=1). */
int slnlp_embed_fwd(const int64_t* ids, int64_t ld_ids, int B, int S, int E, int V,
                    const float* table, const float* pe /* NULL: no positional term */, float* out,
                    float scale /* sqrt(E) for the Transformer, 1 for the RNN models (bkp.py:49) */,
                    float drop_p, int drop_site, const unsigned long long* rng,
                    int64_t nan_idx /* id whose rows become NaN (decoder <pad> target), or -1: none (an id of -1 is a zero row like any id outside [0, V)) */, void* stream);
/* dtable[v,:] = sqrt(E) * sum_{tokens with id v} dropout_bwd(dx[token,:]);
 * rows with no token are zeroed.  Deterministic (fixed summation tree, no
 * float atomics).  scratch: slnlp_embed_bwd_scratch_bytes(B,S,E) bytes. */
int64_t slnlp_embed_bwd_scratch_bytes(int B, int S, int E);
int slnlp_embed_bwd(const int64_t* ids, int64_t ld_ids, int B, int S, int E, int V,
                    const float* dx, float* dtable, float scale,
                    int64_t zero_row /* nn.Embedding(padding_idx): this row gets no gradient; -1 = none */,
                    float drop_p, int drop_site, const unsigned long long* rng,
                    void* scratch, void* stream);

/* -------------------------------------------------------- self attention --
 * Encoder self-attention core for one layer, all (b,h) pairs: scores =
 * q k^T / sqrt(dh), blocked where key j > query i (causal, transformer.py:68 /
 * util.py:11-42) or ids[b,j] == pad (util.py:45-61), softmax, dropout, @ v.
 * qkv [S*B, 3E] is the in_proj output (q | k | v); ctx [S*B, E]; probs
 * [B,H,S,S] keeps the pre-dropout softmax for backward.  Requires S <= 64. */
int slnlp_attn_self_fwd(const float* qkv, const int64_t* ids, int64_t ld_ids, int64_t pad_idx,
                        int causal, int B, int S, int H, int dh,
                        float* ctx, float* probs,
                        float drop_p, int drop_site, const unsigned long long* rng, void* stream);
int slnlp_attn_self_bwd(const float* qkv, const float* probs, const float* dctx,
                        int B, int S, int H, int dh, float* dqkv,
                        float drop_p, int drop_site, const unsigned long long* rng, void* stream);

/* Decoder cross-attention with ONE query per sequence (tgt length 1) over S
 * memory positions, no masks (transformer.py:82-87 passes neither memory_mask
 * nor memory_key_padding_mask).  q [B,E]; kv rows m = s*B+b with row stride
 * ld_kv, k at column 0 and v at column E; probs [B,H,S]. */
/* Sequences longer than 64 (any S up to the reference's 5000-row positional table) take wave-per-row kernels instead of
 * the one-tile MFMA kernels -- same arguments and semantics; only the self-attention backward needs more: a scratch buffer
 * of slnlp_attn_long_scratch_bytes(B, S, H) bytes (the dS tensor between its row pass and its column pass). */
int64_t slnlp_attn_long_scratch_bytes(int B, int S, int H);
int slnlp_attn_self_bwd_long(const float* qkv, const float* probs, const float* dctx, int B, int S, int H, int dh,
                             float* dqkv, float* scratch, float drop_p, int drop_site, const unsigned long long* rng,
                             void* stream);
int slnlp_attn_cross_fwd(const float* q, const float* kv, int64_t ld_kv, int B, int S, int H, int dh,
                         float* ctx, float* probs,
                         float drop_p, int drop_site, const unsigned long long* rng, void* stream);
int slnlp_attn_cross_bwd(const float* q, const float* kv, int64_t ld_kv, const float* probs,
                         const float* dctx, int B, int S, int H, int dh,
                         float* dq, float* dkv, int64_t ld_dkv,
                         float drop_p, int drop_site, const unsigned long long* rng, void* stream);
/* The three launchers above with the arguments the plans pass: the output also (or only) as bf16 hi / lo planes, uint16 bit
 * patterns with the row stride of the fp32 tensor (E for ctx, 3E for dqkv, ld_dkv for dkv), hi = bf16(x) rounded to nearest,
 * lo = bf16(x - hi); q8 adds ctx as OCP e4m3 bytes (saturating at +-448).  hi and lo go together, q8 needs them.  ctx / dqkv
 * may be NULL with both planes and S <= 64: then only the planes are written (16-byte row pieces when dh % 8 == 0, the planes
 * are 16-byte aligned and there is no q8; element stores otherwise -- the same bits).  long_scratch: as for
 * slnlp_attn_self_bwd_long, required for S > 64.  SLNLP_ERR_INVALID_ARG with a message before any launch otherwise. */
int slnlp_attn_self_fwd_ex(const float* qkv, const int64_t* ids, int64_t ld_ids, int64_t pad_idx, int causal, int B, int S, int H,
                           int dh, float* ctx /* or NULL */, float* probs, float drop_p, int drop_site,
                           const unsigned long long* rng, uint16_t* hi, uint16_t* lo, uint8_t* q8, void* stream);
int slnlp_attn_self_bwd_ex(const float* qkv, const float* probs, const float* dctx, int B, int S, int H, int dh,
                           float* dqkv /* or NULL */, float drop_p, int drop_site, const unsigned long long* rng,
                           float* long_scratch, uint16_t* hi, uint16_t* lo, void* stream);
int slnlp_attn_cross_bwd_ex(const float* q, const float* kv, int64_t ld_kv, const float* probs, const float* dctx, int B, int S,
                            int H, int dh, float* dq, float* dkv, int64_t ld_dkv, float drop_p, int drop_site,
                            const unsigned long long* rng, uint16_t* hi, uint16_t* lo, void* stream);

/* The same attention WITHOUT projecting the memory (csrc/attention_mem.hip; what the Transformer plan's decoder runs): with one
 * query per sequence, k_s = Wk mem_s + bk and v_s = Wv mem_s + bv re-associate into per-head B-row products around kernels that
 * read the memory rows themselves.  mem [S*B, E], rows m = s*B + b; per (sequence, head) row bh = b*H + h:
 *   forward   qk [B*H, E] = Wk_h^T q_h (the caller's product)  ->  probs [B*H, S] = softmax_s(qk . mem_s / sqrt(dh)) (before
 *             dropout), pd = dropout(probs) at site element (bh, s), psum [B*H] = sum_s pd, mbar [B*H, E] = sum_s pd mem_s,
 *             ctx0 [B, E] = bv_h psum (the caller's product Wv_h mbar adds onto it: that is ctx)
 *   backward  dmbar [B*H, E] = Wv_h^T d ctx_h (the caller's product), dctx [B, E]  ->  dsc [B*H, S] = d score_s =
 *             probs (t - sum_s probs t) / sqrt(dh) with t = dropout(dmbar . mem_s + dctx_h . bv_h), dqk [B*H, E] = sum_s dsc
 *             mem_s, dcp [B, E] = dctx_h psum; then, unless dmem is NULL, dmem [S*B, E] (= or, accumulate != 0, +=) sum_h (pd
 *             dmbar + dsc qk) and dbv [E] = the column sums of dcp.  d bk is exactly zero and is not written.
 * slnlp_attn_mem_dmem_all: dmem and every layer's dbv of N layers in ONE launch, from a DEVICE table of their buffers (all
 * written by slnlp_attn_mem_bwd calls with dmem NULL): dmem = the bits of N accumulating calls for layers N-1 ... 0.
 * H <= 64, dh a multiple of 4 and <= 256, H * dh <= 1024, S <= 5000. */
int slnlp_attn_mem_fwd(const float* qk, const float* mem, const float* bv, int B, int S, int H, int dh, float* mbar, float* psum,
                       float* probs, float* ctx0, float drop_p, int drop_site, const unsigned long long* rng, void* stream);
int slnlp_attn_mem_bwd(const float* mem, const float* bv, const float* probs, const float* psum, const float* qk,
                       const float* dmbar, const float* dctx, int B, int S, int H, int dh, float* dsc, float* dqk, float* dcp,
                       float* dbv, float* dmem /* or NULL */, int accumulate, float drop_p, int drop_site,
                       const unsigned long long* rng, void* stream);
typedef struct slnlp_xmem_dmem_layer {
    const float *probs, *dsc, *dmbar, *qk, *dcp;
    float* dbv;
    int32_t drop_site;
    int32_t pad;
} slnlp_xmem_dmem_layer;
int slnlp_attn_mem_dmem_all(const slnlp_xmem_dmem_layer* table_dev, int N, int B, int S, int H, int dh, float* dmem, float drop_p,
                            const unsigned long long* rng, void* stream);
/* Heads of one sequence that a workgroup of the two kernels above serves from one pass over the memory rows: 0 = automatic
 * (two, or what the environment variable SLNLP_XMEM_HEADS names), 1 / 2 / 4 forced; a value that does not divide H or whose
 * LDS does not fit falls back to the next smaller one.  A tuning / test knob: per output element the arithmetic and its
 * order are the same, so results do not depend on it. */
int slnlp_set_xmem_heads(int hp);

/* -------------------------------------------------------------- layernorm --
 * y = (x - mean) * rstd * gamma + beta, eps added to the biased variance
 * (torch.nn.LayerNorm as used by nn.Transformer, eps 1e-5).  stats [rows,2] =
 * (mean, rstd) kept for backward.  The residual add is fused into the GEMM
 * that produced x. */
int slnlp_layernorm_fwd(const float* x, const float* gamma, const float* beta, int rows, int E,
                        float eps, float* y, float* stats, void* stream);
/* dx (+ optional add_to_dx [rows,E]) ; dx_drop (optional) = dropout_bwd(dx) at
 * drop_site for the sub-layer branch; partial [nblk,2,E] per-block partial
 * (dgamma, dbeta) sums, reduced later by slnlp_ln_param_reduce. nblk is
 * returned through *nblk_out (<= SLNLP_LN_MAX_PARTIALS).  Blocks are 16 rows; for rows >= 1024 the row kernel
 * sums them itself (one pass over dy and x), below a separate column-sum launch does. */
#define SLNLP_LN_MAX_PARTIALS 1024
int slnlp_layernorm_bwd(const float* dy, const float* x, const float* gamma, const float* stats,
                        int rows, int E, const float* add_to_dx, float* dx, float* dx_drop,
                        float drop_p, int drop_site, const unsigned long long* rng,
                        float* partial, int* nblk_out, void* stream);
/* table: n entries of {partial ptr, nblk, dgamma ptr, dbeta ptr} in DEVICE memory */
typedef struct slnlp_ln_reduce_entry {
    const float* partial; float* dgamma; float* dbeta; int32_t nblk; int32_t E;
} slnlp_ln_reduce_entry;
int slnlp_ln_param_reduce(const slnlp_ln_reduce_entry* table_dev, int n, int max_E, void* stream);

/* The embedding and LayerNorm launchers with the arguments the plans pass (host code around the same kernels; what
 * tests/test_elementwise_edges_gpu.py calls).  Every one returns SLNLP_ERR_INVALID_ARG with a message before anything is launched
 * for a null required pointer, a bad shape (E % 4 != 0; E > 1024 for LayerNorm; more than 65536 tokens for the embedding
 * backward), dropout without its rng, or one plane of a pair without the other.
 *   hi / lo (optional, both or neither): the fp32 output also as bf16 planes of the same shape -- hi = bf16(v) rounded to
 *     nearest, lo = bf16(v - hi).
 *   keep_mask (optional, [B*S*E/4] bytes): under dropout slnlp_embed_fwd_ex records the keep bits of each float4 (bit e = column
 *     c + e kept), and slnlp_embed_bwd_ex reads them instead of drawing the lots again.  A keep_mask also sends a batch of at most
 *     64 tokens through the chunk + combine launches instead of the single launch: same bits.
 *   full_rows (0: rows): the rows of the caller's FULL batch.  The chunks of the (dgamma, dbeta) partial sums follow it, so a
 *     shorter last batch writes the same nblk = ceil(full_rows / chunk) chunks, the trailing ones zero.  partial (with
 *     nblk_out) and dx_drop may be NULL: no column sums / no fp32 dropout copy (drop_hi / drop_lo alone still get it).
 *   slnlp_ln_param_partial: the (dgamma, dbeta) chunk sums of n LayerNorms in one launch from a DEVICE table; entry.dec picks the
 *     row class (rows_dec / full_rows_dec or rows_enc / full_rows_enc).  Chunks are 16 rows (more past 16384 full rows); an entry
 *     writes partial[chunk][2][E] for every chunk of its class's FULL batch, zeros past its last row.  Encoder entries are
 *     skipped when full_rows_enc >= 1024: slnlp_layernorm_bwd(_ex) summed those chunks itself. */
int slnlp_embed_fwd_ex(const int64_t* ids, int64_t ld_ids, int B, int S, int E, int V, const float* table, const float* pe,
                       float* out, float scale, float drop_p, int drop_site, const unsigned long long* rng, int64_t nan_idx,
                       uint16_t* hi, uint16_t* lo, unsigned char* keep_mask, void* stream);
int slnlp_embed_bwd_ex(const int64_t* ids, int64_t ld_ids, int B, int S, int E, int V, const float* dx, float* dtable, float scale,
                       int64_t zero_row, float drop_p, int drop_site, const unsigned long long* rng, void* scratch,
                       const unsigned char* keep_mask, void* stream);
int slnlp_layernorm_fwd_ex(const float* x, const float* gamma, const float* beta, int rows, int E, float eps, float* y,
                           float* stats, uint16_t* hi, uint16_t* lo, void* stream);
int slnlp_layernorm_bwd_ex(const float* dy, const float* x, const float* gamma, const float* stats, int rows, int E,
                           const float* add_to_dx, float* dx, float* dx_drop, float drop_p, int drop_site,
                           const unsigned long long* rng, float* partial, int* nblk_out, int full_rows, uint16_t* dx_hi,
                           uint16_t* dx_lo, uint16_t* drop_hi, uint16_t* drop_lo, void* stream);
typedef struct slnlp_ln_partial_entry {
    const float* dy; const float* x; const float* stats; float* partial;
    int32_t dec;   /* 1: a decoder LayerNorm (rows_dec), 0: an encoder one (rows_enc) */
    int32_t pad;
} slnlp_ln_partial_entry;
int slnlp_ln_param_partial(const slnlp_ln_partial_entry* table_dev, int n, int E, int rows_enc, int rows_dec, int full_rows_enc,
                           int full_rows_dec, void* stream);

/* ------------------------------------------------------------------ loss --
 * logp = log_softmax(logits) (transformer.py:88-89 / bkp.py:75-76) and
 * CrossEntropyLoss(ignore_index) ON THE LOG-PROBS as skorch applies it
 * (helper.py:61-70): loss = -mean_{y!=ignore} log_softmax(logp)[y].
 * Writes logp [B,V] (ld = V), loss[0], and (if dlogits) d loss / d logits. */
int slnlp_lsm_nll(const float* logits, int64_t ld_logits, const int64_t* y, int B, int V,
                  int64_t ignore_index, float* logp, float* loss, float* dlogits, int64_t ld_dlogits,
                  float* row_scratch /* [B] */, void* stream);
/* slnlp_lsm_nll with the rest of CrossEntropyLoss (torch's composition, on the log-probs):
 * class_weight [V] (device, or NULL: all ones), label_smoothing in [0, 1], reduction 0 = "mean" (divided by the
 * summed class weight of the kept rows; NaN when no row is kept) or 1 = "sum".  At (NULL, 0, 0) the result is
 * bit-identical to slnlp_lsm_nll. */
int slnlp_lsm_nll_ex(const float* logits, int64_t ld_logits, const int64_t* y, int B, int V, int64_t ignore_index,
                     const float* class_weight, float label_smoothing, int reduction, float* logp, float* loss,
                     float* dlogits, int64_t ld_dlogits, float* row_scratch /* [B] */, void* stream);
/* backward of log_softmax alone, for callers that own the criterion (torch
 * autograd): dlogits = dlogp - exp(logp) * rowsum(dlogp). */
int slnlp_lsm_bwd(const float* logp, const float* dlogp, int B, int V, float* dlogits,
                  int64_t ld_dlogits, void* stream);

/* -------------------------------------------------------------- optimizer --
 * clip_grad_norm_(max_norm, 2) + SGD(momentum, dampening 0, nesterov False,
 * no weight decay) over ONE flat parameter arena (helper.py:227-229,
 * config-transformer.yaml:19-20,40-43).  lr is read from device memory so a
 * captured graph follows ReduceLROnPlateau.  norm_out[0] receives the pre-clip
 * total norm; rng[1] (the dropout step counter) is incremented if rng != NULL. */
int slnlp_clip_sgd_step(float* params, const float* grads, float* momentum_buf, int64_t n,
                        const float* lr_dev, float momentum, float max_norm,
                        float* partials /* [1024] scratch */, float* norm_out,
                        unsigned long long* rng, void* stream);

/* slnlp_clip_sgd_step with the rest of torch.optim.SGD (torch/optim/sgd.py _single_tensor_sgd): d = g' + weight_decay p;
 * buf = d on the first step, m buf + (1 - dampening) d after; d = d + m buf (nesterov) or buf; p -= lr d.
 * step_count[0] (float, device) counts the steps taken (0 before the first) and is advanced by one; required unless the
 * settings are plain SGD-momentum.  Floats [skip_begin, skip_end) (multiples of 4; empty when skip_end <= skip_begin) are a
 * parameter torch never steps and stay untouched.  nesterov needs momentum > 0 and dampening 0, as in torch. */
int slnlp_clip_sgd_step_ex(float* params, const float* grads, float* momentum_buf, int64_t n, const float* lr_dev,
                           float momentum, float dampening, float weight_decay, int nesterov, float max_norm,
                           float* partials /* [1024] scratch */, float* norm_out, float* step_count, int64_t skip_begin,
                           int64_t skip_end, void* stream);
/* clip_grad_norm_ + torch.optim.AdamW: p *= 1 - lr weight_decay, then the Adam update without an L2 term; the skip range
 * as in slnlp_clip_sgd_step_ex; step_count as in slnlp_clip_adam_step. */
int slnlp_clip_adamw_step(float* params, const float* grads, float* exp_avg, float* exp_avg_sq, int64_t n,
                          const float* lr_dev, float beta1, float beta2, float eps, float weight_decay, float max_norm,
                          float* partials /* [1024] scratch */, float* norm_out, float* step_count, int64_t skip_begin,
                          int64_t skip_end, void* stream);

/* clip_grad_norm_ + torch.optim.Adam (amsgrad False; torch/optim/adam.py _single_tensor_adam) over one flat arena:
 * step_count[0] (float, device) holds the number of steps taken so far and is advanced by one. */
int slnlp_clip_adam_step(float* params, const float* grads, float* exp_avg, float* exp_avg_sq, int64_t n,
                         const float* lr_dev, float beta1, float beta2, float eps, float weight_decay, float max_norm,
                         float* partials /* [1024] scratch */, float* norm_out, float* step_count, void* stream);

/* Per-parameter-group learning rate and weight decay (torch's optimizer param_groups) for the two updates above.  The
 * arena of n floats is cut into n_segments segments: segment s covers floats [seg_begin[s], seg_begin[s + 1]) -- the last
 * one runs to n -- and belongs to group seg_group[s] in [0, n_groups).  seg_begin[0] is 0, the entries are multiples of 4
 * and strictly increasing; at most 1024 segments (SLNLP_ERR_INVALID_ARG above that).  seg_begin, seg_group and
 * weight_decay [n_groups] are HOST arrays, copied into device memory the handle owns (the upload is ordered on stream).
 * The groups' learning rates are not part of the table: every step reads them from lr_dev [n_groups] in device memory. */
typedef struct slnlp_param_groups slnlp_param_groups;
int slnlp_param_groups_create(int64_t n, int n_segments, const int64_t* seg_begin, const int32_t* seg_group, int n_groups,
                              const float* weight_decay, void* stream, slnlp_param_groups** out);
void slnlp_param_groups_destroy(slnlp_param_groups* groups);
/* slnlp_clip_sgd_step_ex / slnlp_clip_adam_step / slnlp_clip_adamw_step (decoupled != 0) with lr and weight decay taken per
 * element from its group: same two launches, same norm, same clip, same counters.  One segment that covers the arena gives
 * the bits of the one-group entry points. */
int slnlp_clip_sgd_step_groups(float* params, const float* grads, float* momentum_buf, int64_t n,
                               const slnlp_param_groups* groups, const float* lr_dev /* [n_groups] */, float momentum,
                               float dampening, int nesterov, float max_norm, float* partials /* [1024] scratch */,
                               float* norm_out, float* step_count, int64_t skip_begin, int64_t skip_end, void* stream);
int slnlp_clip_adam_step_groups(float* params, const float* grads, float* exp_avg, float* exp_avg_sq, int64_t n,
                                const slnlp_param_groups* groups, const float* lr_dev /* [n_groups] */, float beta1,
                                float beta2, float eps, int decoupled, float max_norm, float* partials /* [1024] scratch */,
                                float* norm_out, float* step_count, int64_t skip_begin, int64_t skip_end, void* stream);

/* ---------------------------------------------------------- weight averaging --
 * A running average of a parameter arena, kept on the device: torch.optim.swa_utils.AveragedModel without the host.
 * slnlp_average_step feeds `params` (n floats, a multiple of 4; 16-byte aligned, like avg) into `avg`.  count[0] is a device
 * float, the number of models averaged so far; with c its value BEFORE the call:
 *   c == 0            avg = params, bit for bit
 *   SLNLP_AVG_SWA     avg += (params - avg) / (c + 1)          AveragedModel's default avg_fn
 *   SLNLP_AVG_EMA     avg += (params - avg) * (1 - decay)      get_ema_multi_avg_fn(decay), 0 < decay < 1
 * and count[0] = c + 1 afterwards (its own one-thread launch behind the update, so every block read the same c).  Floats
 * [skip_begin, skip_end) (multiples of 4; empty: none) are copied, never averaged: a parameter torch never steps stays equal to
 * the model's.  Two launches, no host wait; capturable.
 * slnlp_swap_arenas exchanges two arenas of n floats in place, in one launch; two swaps restore every bit.  After a swap into
 * a plan's parameter arena tell the plan (slnlp_tf_params_changed). */
#define SLNLP_AVG_SWA 0
#define SLNLP_AVG_EMA 1
int slnlp_average_step(float* avg, const float* params, int64_t n, float* count, int kind, float decay, int64_t skip_begin,
                       int64_t skip_end, void* stream);
int slnlp_swap_arenas(float* a, float* b, int64_t n, void* stream);

/* ------------------------------------------------------------ epoch scoring --
 * An epoch's log-probs reduced to what the scoring metrics are functions of (slnlp/metrics.py forms the scores on the host).
 * logp float32 [N, ld], V <= ld columns used; y int64 [N].  Per row i, with v = logp[i, y[i]]:
 *   pred[i]    index of the first maximum (np.argmax: a NaN is larger than everything, the first NaN wins)
 *   picked[i]  v, bit for bit
 *   rank[i]    #{j : logp[i, j] > v} + #{j > y[i] : logp[i, j] == v}: where sklearn's top_k_accuracy_score finds the true class
 *              (0 = first); V, never a hit, when the row holds a NaN
 *   counts     int32 [3 V + 1]: true_sum [V], pred_sum [V], tp_sum [V] (rows with y = c, with pred = c, with both), then n_bad
 * A label outside [0, V) is not used as an index: picked[i] = NaN, rank[i] = V, n_bad += 1, and the row enters pred_sum only.
 * counts is zeroed by the call, on the stream; the sums are integer atomics, so the result does not depend on scheduling.
 * Two launches, no host wait.  Invalid arguments -- a null pointer, N < 1, V < 1, ld < V, N above INT32_MAX or 3 V + 1 above it,
 * an output overlapping an input or another output -- return SLNLP_ERR_INVALID_ARG before anything is launched. */
int slnlp_score_rows(const float* logp, int64_t ld, const int64_t* y, int64_t N, int V, int32_t* pred, float* picked,
                     int32_t* rank, int32_t* counts, void* stream);

/* ------------------------------------------------------ temperature calibration --
 * One scalar T fitted on held-out log-probs and applied as softmax(z / T): the arg-max never moves, the log-loss does.
 * logp float32 [N, ld], V <= ld columns used; y int64 [N]; beta = 1 / T.  Rows whose label lies outside [0, V) are counted
 * and excluded (never used as an index); M rows remain.  Per row i, p = softmax(beta z_i):
 *   f_i = logsumexp_c(beta z_ic) - beta z_iy       g_i = sum_c p_c z_ic - z_iy       h_i = sum_c p_c z_ic^2 - (sum_c p_c z_ic)^2
 *   s_i = |sum_c p_c z_ic| + |z_iy|                f, g, h, s: their means over the M rows (g = df/dbeta, h = d2f/dbeta2 >= 0)
 * slnlp_fit_temperature minimises f over beta in [2^-6, 2^6], in fp64 throughout (z itself is float32):
 *   1. at beta = 2^-6: |g| <= 2^-44 s there AND at beta = 1 -> beta = 1, SLNLP_CAL_FLAT; else g >= 0 -> beta = 2^-6, SLNLP_CAL_BOUND
 *   2. at beta = 2^6:  g <= 0 -> beta = 2^6, SLNLP_CAL_BOUND
 *   3. lo = 2^-6, hi = 2^6, beta = 1; at most 32 times: evaluate at beta; |g| <= 2^-44 s -> SLNLP_CAL_GRADIENT (result beta);
 *      g < 0 ? lo = beta : hi = beta; beta' = beta exp(-g / (g + beta h)) (the Newton step in ln beta) when g + beta h > 0
 *      and lo < beta' < hi, else sqrt(lo hi); |ln(beta' / beta)| <= 2^-40 -> SLNLP_CAL_STEP (result beta'); after the 32nd
 *      evaluation -> SLNLP_CAL_CAP (result beta'); else beta = beta'.
 * M == 0 gives beta = 1, SLNLP_CAL_FLAT, both f = 0.
 * state: SLNLP_CAL_STATE_BYTES of device memory, 8-byte aligned, written by the call (no need to clear it):
 *   double [0] beta   [1] T = 1 / beta   [2] f at beta = 1   [3] f at the result   [4..7] the iteration's own
 *   int64  [8] reason (SLNLP_CAL_*)   [9] iterations (evaluations of step 3; 0 for FLAT / BOUND)   [10] M   [11] labels out
 *          of range   [12..15] the iteration's own
 * scratch: slnlp_fit_temperature_scratch_bytes(N) bytes (-1 and a message for N outside 1..INT32_MAX), 32-byte aligned: the
 * per-row terms of one evaluation.  The call queues a fixed sequence of 72 launches on stream (36 evaluations of two launches:
 * beta = 1, the two bounds, 32 iterations, the result; once the reason is set the iteration launches return at once) and
 * never waits for the host.  The result is a function of the arguments alone: the row terms are summed by one block in an
 * order that depends on N only.  Errors (SLNLP_ERR_INVALID_ARG with a message, before anything is launched): a null pointer,
 * N or V outside 1..INT32_MAX, ld < V, scratch too small or misaligned, state or scratch overlapping an input or each other.
 *
 * slnlp_scale_logp: out[i, c] = beta z_ic - logsumexp_c'(beta z_ic'), the calibrated log-probs; beta = beta_dev[0] is read
 * from device memory (a state's first double), so the call never waits for the host.  Per row in fp64 with the maximum
 * subtracted, rounded once to float32.  out may be logp itself with ld_out == ld (in place: every column is re-read by the
 * lane that stores it, after the row's logsumexp is complete); any other overlap is SLNLP_ERR_INVALID_ARG.  One launch. */
#define SLNLP_CAL_STATE_BYTES 128
#define SLNLP_CAL_FLAT 1
#define SLNLP_CAL_BOUND 2
#define SLNLP_CAL_GRADIENT 3
#define SLNLP_CAL_STEP 4
#define SLNLP_CAL_CAP 5
int64_t slnlp_fit_temperature_scratch_bytes(int64_t N);
int slnlp_fit_temperature(const float* logp, int64_t ld, const int64_t* y, int64_t N, int64_t V, void* state, void* scratch,
                          int64_t scratch_bytes, void* stream);
int slnlp_scale_logp(const float* logp, int64_t ld, int64_t N, int64_t V, const double* beta_dev, float* out, int64_t ld_out,
                     void* stream);

/* ------------------------------------------- bias-corrected temperature calibration --
 * A temperature AND a per-class bias fitted on held-out log-probs, applied as softmax(beta z + b) (Alexandari, Kundaje and
 * Shrikumar 2020: BCTS) -- slnlp_shift_logp with log_w = b and a state's beta.  Unlike a temperature, the bias can move the
 * arg-max: it removes a per-class offset such as ln(pi_valid / pi_train) of a fit trained under other class priors.
 * logp, y, the excluded rows and M as for slnlp_fit_temperature; 1 <= V <= SLNLP_BIAS_CAL_MAX_V.  theta = (beta, b_0 .. b_{V-1});
 * p_i = softmax(beta z_i + b), m_i = sum_c p_ic z_ic, n_c = the share of the M rows labelled c; in fp64 throughout (z is float32):
 *   F(theta) = mean_i [ logsumexp_c(beta z_ic + b_c) - beta z_iy - b_y ] + (lambda / 2) sum_c b_c^2,  lambda = 1 / (bias_sd^2 M)
 *   g_beta = mean_i (m_i - z_iy)                        g_b = mean_i p_i - n + lambda b
 *   H_beta,beta = mean_i (sum_c p_ic z_ic^2 - m_i^2)    H_beta,b = mean_i p_i (z_i - m_i)    H_bb = diag(mean_i p_i + lambda) - P^T P / M
 * -- the MAP estimate under a N(0, bias_sd^2) prior on every bias (bias_sd finite and > 0), jointly convex in (beta, b).
 * slnlp_fit_bias_temperature minimises F over beta in [2^-6, 2^6] by a damped Newton iteration:
 *   1. theta = (1, 0); evaluate F, g there (evaluation 1).  M == 0 or V == 1 -> theta = (1, 0), SLNLP_CAL_FLAT, 0 evaluations.
 *   2. max |g| <= tol -> SLNLP_CAL_GRADIENT (result theta); 48 evaluations made -> SLNLP_CAL_CAP (result theta).
 *   3. H = L L^T by Cholesky; a pivot <= 0 (or NaN) -> SLNLP_CAL_PIVOT (result theta: it cannot happen in exact arithmetic, so
 *      it is reported, not patched).  d = -H^-1 g, t = 1.
 *   4. halve t while the beta of theta + t d lies outside [2^-6, 2^6] (no evaluation); evaluate F', g' at theta + t d;
 *      F' <= F + 1e-4 t g^T d -> theta = theta + t d, F = F', g = g', go to 2; else 48 evaluations made -> SLNLP_CAL_CAP (result
 *      theta); else t = t / 2 and 4 again.  A rejected candidate counts as an evaluation.
 * state: as slnlp_fit_temperature's -- double [0] beta  [1] T = 1 / beta  [2] the mean log-loss at (1, 0)  [3] the mean log-loss at
 * the result (both WITHOUT the penalty)  [4..7] the iteration's own; int64 [8] reason  [9] evaluations  [10] M  [11] labels out of
 * range  [12..15] the iteration's own (13: halvings, 14: Newton directions) -- so slnlp_scale_logp, slnlp_shift_logp and every
 * beta_dev argument read it unchanged.  bias: double [V] device memory, b at the result (what slnlp_shift_logp takes as log_w).
 * tol: finite and >= 0, an ABSOLUTE bound on max |g|.  scratch: slnlp_fit_bias_temperature_scratch_bytes(N, V) bytes (-1 and a
 * message for N outside 1..INT32_MAX or V outside 1..SLNLP_BIAS_CAL_MAX_V), 32-byte aligned: p_i as fp64 [N, V rounded up to 16],
 * the row terms, the column sums, theta, the candidate, g, d and the (V + 1)^2 system.
 * The call queues a fixed sequence of 48 x 5 - 2 + 3 = 241 launches on stream and never waits for the host: per evaluation the
 * rows (a wave per row), the column sums (a block per class: thread t adds rows t, t + 256, ... in increasing order, then a
 * fixed binary tree), ONE block that forms F and g and takes the accept / halve / stop decision, P^T P over the lower
 * triangle's 16 x 16 tiles (v_mfma_f64_16x16x4_f64, the rows in increasing order; nothing after a rejected candidate), and ONE
 * block for the factorisation, the solves and the next candidate; then the evaluation at the result.  Once the reason is set
 * the launches read it and return at once.  No atomics: the result is a function of the arguments alone.
 * Errors (SLNLP_ERR_INVALID_ARG with a message, before anything is launched): a null pointer, N outside 1..INT32_MAX, V outside
 * 1..SLNLP_BIAS_CAL_MAX_V, ld < V, bias_sd or tol out of range, scratch too small or misaligned, a misaligned pointer, state,
 * bias or scratch overlapping an input or each other. */
#define SLNLP_BIAS_CAL_MAX_V 512
#define SLNLP_CAL_PIVOT 6
int64_t slnlp_fit_bias_temperature_scratch_bytes(int64_t N, int64_t V);
int slnlp_fit_bias_temperature(const float* logp, int64_t ld, const int64_t* y, int64_t N, int64_t V, double bias_sd, double tol,
                               void* state, double* bias, void* scratch, int64_t scratch_bytes, void* stream);

/* -------------------------------------------------------- label-shift adaptation --
 * A classifier trained under the class priors pi_s and used under pi_t is corrected exactly by p_t(c | x) ~ p_s(c | x)
 * pi_t(c) / pi_s(c).  slnlp_fit_priors estimates pi_t from UNLABELLED rows by the EM of Saerens, Latinne and Decaestecker (2002),
 * slnlp_shift_logp applies a log-ratio to log-probs (slnlp.PriorShift).  logp float32 [N, ld], V <= ld columns used; beta =
 * beta_dev ? beta_dev[0] : 1 exactly, device memory as for slnlp_reliability_rows; log_source double [V] in device memory,
 * the FINITE values ln pi_s(c); everything but z itself is fp64.
 *
 * slnlp_fit_priors: a row that holds a NaN or whose maximum is not finite (slnlp_reliability_rows' code -2 rows) is excluded
 * and counted; M rows remain.  With lw^0 = 0 and pi^0_c = exp(log_source_c), for t = 0, 1, ...:
 *   a_ic = beta z_ic + lw^t_c (the product rounded, then the sum)      lse_i = max_c a_ic + log sum_c exp(a_ic - max_c a_ic)
 *   S_c = sum_i exp(a_ic - lse_i) over the M rows                      pi^{t+1}_c = S_c / M
 *   d^t = max_c |pi^{t+1}_c - pi^t_c|;   d^t <= tol -> SLNLP_PRIOR_TOL;   else t == max_iter -> SLNLP_PRIOR_CAP;
 *   else lw^{t+1}_c = ln max(pi^{t+1}_c, 2^-1022) - log_source_c
 * (a row's responsibilities sum to 1, so pi needs no normalisation across classes).  The result is pi = pi^{t+1}, log_w_c =
 * ln max(pi_c, 2^-1022) - log_source_c, iterations = t + 1; one more evaluation at log_w gives gain = (1 / M) sum_i (lse_i(log_w)
 * - lse_i(0)), the log-likelihood per row that the rows gain from the new priors (>= 0 up to rounding; EM never lowers it).
 * max_iter in 0..SLNLP_PRIOR_MAX_ITER (0: one evaluation, pi = the mean prediction), tol finite and >= 0.
 * M == 0 gives table rows 0 and 1 = pi^0, log_w = 0, gain = 0, d = 0, iterations = 0 and SLNLP_PRIOR_EMPTY.
 *   table double [3, V]: row 0 = pi^1, the mean of softmax(beta z_i) over the M rows (the model's own mean prediction);
 *                        row 1 = pi; row 2 = log_w
 *   state: SLNLP_PRIOR_STATE_BYTES of device memory, 8-byte aligned, written by the call (no need to clear it):
 *     double [0] gain   [1] the last d   [2..7] zero
 *     int64  [8] reason (SLNLP_PRIOR_*)   [9] iterations   [10] M   [11] excluded rows   [12..15] zero
 *   scratch: slnlp_fit_priors_scratch_bytes(N, V) bytes (-1 and a message for N or V outside 1..INT32_MAX), 8-byte aligned.
 * The call queues a fixed sequence of 3 (max_iter + 1) + 2 launches on stream -- per iteration the rows' lse_i (a wave per row),
 * S_c (a block per class: thread t adds rows t, t + 256, ... in increasing order, then a fixed binary tree over the 256 partial
 * sums) and one block that forms pi, log_w, d and takes the stop decision; then the evaluation at the result and the gain --
 * and never waits for the host: once the reason is set, the iteration launches read it and return at once.  No atomics: the
 * result is a function of the arguments alone.
 *
 * slnlp_shift_logp: out[i, c] = (beta z_ic + log_w_c) - logsumexp_c'(beta z_ic' + log_w_c'), log_w double [V] in device memory
 * (table row 2), per row in fp64 with the maximum subtracted, rounded once to float32.  log_w_c = -inf is legal and gives -inf in
 * that column; a row that holds a NaN, whose maximum is not finite, or whose largest beta z_ic + log_w_c is not finite gets NaN
 * in every column.  out may be logp itself with ld_out == ld (slnlp_scale_logp's rule); any other overlap is an error.  One
 * launch.
 *
 * Errors of both (SLNLP_ERR_INVALID_ARG with a message, before anything is launched): a null pointer (beta_dev may be null), N
 * or V outside 1..INT32_MAX, ld or ld_out < V, max_iter or tol out of range, scratch too small, a misaligned pointer (logp and
 * out 4 bytes, the others 8), an output overlapping an input or another output. */
#define SLNLP_PRIOR_MAX_ITER 1024
#define SLNLP_PRIOR_STATE_BYTES 128
#define SLNLP_PRIOR_TOL 1
#define SLNLP_PRIOR_CAP 2
#define SLNLP_PRIOR_EMPTY 3
int64_t slnlp_fit_priors_scratch_bytes(int64_t N, int64_t V);
int slnlp_fit_priors(const float* logp, int64_t ld, int64_t N, int64_t V, const double* beta_dev, const double* log_source,
                     int max_iter, double tol, double* table, void* state, void* scratch, int64_t scratch_bytes, void* stream);
int slnlp_shift_logp(const float* logp, int64_t ld, int64_t N, int64_t V, const double* beta_dev, const double* log_w, float* out,
                     int64_t ld_out, void* stream);

/* ------------------------------------------------------ reliability diagnostics --
 * What expected / maximum calibration error (ECE, MCE), the multiclass Brier score and the log-loss of a set of log-probs are
 * functions of (slnlp/ops.py forms the scores on the host).  logp float32 [N, ld], V <= ld columns used; y int64 [N]; bins = B
 * in 1..SLNLP_REL_MAX_BINS; beta = beta_dev ? beta_dev[0] : 1 exactly -- beta_dev is device memory (a calibration state's
 * first double), so the call never waits for the host; p = softmax(beta z_i) is never materialised.  Per row i, in fp64
 * throughout (z itself is float32), with zmax the float32 row maximum, a = beta zmax, e_c = exp(beta z_c - a), k the number
 * of columns at the maximum (e = 1 exactly: counted, not summed), rest = sum_{c not at max} e_c + (k - 1), s0 = 1 + rest:
 *   pred    index of the first maximum (slnlp_score_rows' order)          correct = (pred == y_i)
 *   conf    1 / s0, the probability of the arg-max class
 *   brier   sum_c (p_c - 1[c = y_i])^2 = (k + sum_{c not at max} e_c^2) / s0^2 - 2 exp(beta z_y - a) / s0 + 1
 *   nll     log1p(rest) - (beta z_y - a)                                   (slnlp_fit_temperature's f_i)
 *   bin     clamp(ceil(conf B) - 1, 0, B - 1), from the conf that is stored: equal-width bins (b / B, (b + 1) / B], closed on
 *           the right (Guo et al. 2017), so conf = 1 and conf one ulp below 1 both land in bin B - 1
 * rows  double [N, 4]:     (conf, brier, nll, code); code = 2 bin + correct for a scored row; code = -1 and three zeros for a
 *                          label outside [0, V) (looked at first, never used as an index); code = -2 and three NaN for a row
 *                          that holds a NaN or whose maximum is not finite
 * table double [B + 1, 4]: row b < B = (count, sum conf, sum correct, 0) over the scored rows of bin b; row B = (sum brier,
 *                          sum nll, n_bad_label, n_nan), the two sums over the scored rows only
 * Two launches: the rows (a wave per row, no LDS), then B + 1 blocks of 256 threads, block b summing bin b (block B the totals):
 * thread t adds rows t, t + 256, ... in increasing order, then a fixed binary tree over the 256 partial sums.  No atomics: the
 * result is a function of the arguments alone.  rows and table are 32-byte aligned.  Errors (SLNLP_ERR_INVALID_ARG with a
 * message, before anything is launched): a null pointer (beta_dev may be null), N or V outside 1..INT32_MAX, bins outside
 * 1..SLNLP_REL_MAX_BINS, ld < V, a misaligned pointer, an output overlapping an input or the other output. */
#define SLNLP_REL_MAX_BINS 64
int slnlp_reliability_rows(const float* logp, int64_t ld, const int64_t* y, int64_t N, int64_t V, int bins, const double* beta_dev,
                           double* rows, double* table, void* stream);

/* ----------------------------------------------------------------- error analysis --
 * Which classes are wrong and what they were mistaken for: the top-k classes of every row, the confusion matrix and its
 * most-confused pairs (slnlp/ops.py and slnlp/metrics.py form the report on the host; NeuralNetClassifier.error_analysis).
 *
 * slnlp_topk_rows: logp float32 [N, ld], V <= ld columns used; k in 1..min(V, SLNLP_TOPK_MAX); beta as for
 * slnlp_reliability_rows (beta_dev may be null: beta = 1).  idx int32 [N, k]: per row the first k columns in the total order of
 * slnlp_score_rows' arg-max on the float32 values -- a NaN comes before everything (several NaNs by ascending index), then
 * larger values first, equal values by ascending index; -inf is an ordinary value.  Column 0 is therefore slnlp_score_rows'
 * pred and np.argmax.  NOT sklearn's top-k tie order (top_k_accuracy_score puts the HIGHER index first among equal scores;
 * rank[] of slnlp_score_rows follows sklearn, this list follows the arg-max).  prob float64 [N, k]: prob[i, j] =
 * exp(beta z_c - a) / s0 for c = idx[i, j], with slnlp_reliability_rows' fp64 decomposition (zmax the float32 row maximum,
 * a = beta zmax, columns at the maximum counted and not exponentiated, s0 = 1 + rest): prob[i, 0] is that call's conf bit for
 * bit.  A row that holds a NaN or whose maximum is not finite gets NaN probabilities; its indices still follow the order.
 * One launch (a wave per row, k - 1 selection rounds over the row, no LDS, no atomics); the result is a function of the
 * arguments alone.  Errors: a null pointer (but beta_dev), N or V outside 1..INT32_MAX, k out of range, ld < V, a misaligned
 * pointer (idx 4, prob and beta_dev 8 bytes), an output overlapping an input or the other output.
 *
 * slnlp_confusion_matrix: pred int32 [N] (what slnlp_score_rows wrote), y int64 [N], V in 1..SLNLP_CONFUSION_MAX_V; counts
 * int32 [V V + 1] is zeroed by the call, on the stream, then counts[y_i V + pred_i] += 1 for every row whose label and
 * prediction both lie in [0, V) -- rows true, columns predicted -- and counts[V V] += 1 for every other row (a value outside
 * [0, V) is never used as an index).  Integer atomics: the result does not depend on scheduling.  Two launches.
 *
 * slnlp_confusion_pairs: counts int32 [V V] as above (the tail entry is not read); pairs int32 [M, 3], M in
 * 1..SLNLP_PAIRS_MAX: the M largest off-diagonal cells with a count above 0, ordered by count descending, then true class
 * ascending, then predicted class ascending (the last two: the flat index ascending); row m = (true, predicted, count), unused
 * rows = (-1, -1, 0).  work: slnlp_confusion_pairs_workspace_bytes(V, M) bytes of device memory (-1 and a message for V or M out
 * of range), 8-byte aligned, written by the call (no need to clear it; more than needed changes nothing).  Two launches: blocks
 * select the first M cells of a contiguous slice each, one block merges their lists; the order is total, so the result is the
 * same however the cells are sliced.
 *
 * All three return SLNLP_ERR_INVALID_ARG with a message before anything is launched. */
#define SLNLP_TOPK_MAX 64
#define SLNLP_CONFUSION_MAX_V 4096
#define SLNLP_PAIRS_MAX 64
int slnlp_topk_rows(const float* logp, int64_t ld, int64_t N, int64_t V, int k, const double* beta_dev, int32_t* idx, double* prob,
                    void* stream);
int slnlp_confusion_matrix(const int32_t* pred, const int64_t* y, int64_t N, int64_t V, int32_t* counts, void* stream);
int64_t slnlp_confusion_pairs_workspace_bytes(int64_t V, int M);
int slnlp_confusion_pairs(const int32_t* counts, int64_t V, int M, int32_t* pairs, void* work, int64_t work_bytes, void* stream);

/* ------------------------------------------------------ bootstrap of the scores --
 * B bootstrap replicates of the scoring metrics of one set of predictions: every replicate draws N rows with replacement
 * from the per-row results that are already on the device and reduces them to the metrics (slnlp/metrics.py summarises the
 * replicates on the host: bootstrap_intervals, bootstrap_difference; NeuralNetClassifier.score_interval / compare).
 * y int64 [N], pred int32 [N] and rank int32 [N] as slnlp_score_rows takes / leaves them (rank may be null iff top_k == 0);
 * values double [N, ldv], Q <= ldv columns used (null iff Q == 0) -- slnlp_reliability_rows' rows directly with ldv = 4,
 * Q = 3: conf, brier, nll.  V in 1..SLNLP_CONFUSION_MAX_V; top_k = 0 or in [1, V); B in 1..SLNLP_BOOT_MAX_REPLICATES.
 *
 * The draw.  Random words: Threefry-4x32, the dropout masks' 12 rounds, key (seed low word, seed high word, 0, 0).  Draw j in
 * [0, N) of replicate b: q = j >> 2, w = j & 3, X0..X3 the output words at counter (q, b, SLNLP_BOOT_STAGE, 0); the row is
 * (X_w * N) >> 32.  All four words of a call are used (the last call of a replicate may use fewer).  The draw is a function of
 * (seed, b, j, N) alone, not of the predictions: two calls with one seed on two fits' outputs see the same resamples (a paired
 * bootstrap), and replicate b does not depend on B.
 *
 * Per replicate, over its N drawn rows r (a value outside [0, V) is never used as an index -- slnlp_score_rows' rule):
 *   true_sum[y_r] += 1 when the label is in range, else n_bad += 1;  pred_sum[pred_r] += 1 when the prediction is in range;
 *   tp_sum[y_r] += 1 when both are in range and equal;  hits += 1 when the label is in range and rank_r < top_k;
 *   for each value column its fp64 sum (a NaN propagates).
 * stats double [B, SLNLP_BOOT_FIXED + Q], row b, with the definitions of slnlp/metrics.py (sklearn's, zero_division = 0):
 *   [0] accuracy = sum tp_sum / N         [1..3] precision, recall, f1 macro        [4..6] precision, recall, f1 weighted
 *   [7] balanced_accuracy                 [8] top_k_accuracy = hits / N (NaN when top_k == 0)       [9..] the Q column means
 * Per class precision = tp / pred_sum, recall = tp / true_sum, f1 = 2 tp / (true_sum + pred_sum), 0 where the denominator is 0.
 * The macro scores are their means and the weighted scores their true_sum-weighted means (0 when no label is in range) over
 * the classes PRESENT IN THE REPLICATE (true_sum + pred_sum > 0); balanced_accuracy is the mean recall over the classes with
 * true_sum > 0 (NaN when there is none): a replicate that loses a rare class changes the denominators.
 * One difference from metrics._scores, for callers that pass values outside the classes (slnlp_score_rows' pred never is one):
 * accuracy is sum tp_sum / N, so a row counts as correct only when its label is a class -- a label and a prediction that are the
 * SAME value outside [0, V) are not a correct row here, while mean(y == pred) would count them.
 * counts int32 [B, 3 V + 1] or null: row b = true_sum | pred_sum | tp_sum | n_bad, slnlp_score_rows' layout.
 *
 * One launch: a block of 256 threads per replicate, the class counts in LDS (integer atomics: sums of integers do not depend
 * on the order of arrival).  Every fp64 sum is formed in a fixed order -- thread t adds draws (classes) t, t + 256, ... in
 * increasing order, then a fixed binary tree over the 256 partial sums -- so the result is a function of the arguments alone.
 * No global atomics.  Errors (SLNLP_ERR_INVALID_ARG with a message, before anything is launched): a null pointer other than
 * the nullable ones, N outside 1..INT32_MAX, V outside 1..SLNLP_CONFUSION_MAX_V, B outside 1..SLNLP_BOOT_MAX_REPLICATES, Q
 * outside 0..SLNLP_BOOT_MAX_VALUES, ldv < Q, top_k < 0 or >= V when nonzero, a misaligned pointer (y, values, stats 8 bytes;
 * pred, rank, counts 4), an output overlapping an input or the other output. */
#define SLNLP_BOOT_MAX_REPLICATES 65536
#define SLNLP_BOOT_MAX_VALUES 8
#define SLNLP_BOOT_FIXED 9              /* the count-derived columns of stats */
#define SLNLP_BOOT_STAGE 0x626f6f74u    /* the draw's counter word 2; slnlp_balanced_order uses 0, 1, 2 */
int slnlp_bootstrap_scores(const int64_t* y, const int32_t* pred, const int32_t* rank, const double* values, int64_t ldv, int Q,
                           int64_t N, int V, int top_k, int B, uint64_t seed, double* stats, int32_t* counts, void* stream);

/* ------------------------------------------------------ ensembles of log-probs --
 * K fits' log-probs combined into one set of log-probs in the layout every row entry point above reads, and in the same pass
 * the per-row uncertainty decomposition (slnlp/ops.py's ensemble_rows; slnlp/ensemble.py's VotingEnsemble).
 * logp: a HOST array of K device pointers, K in 1..SLNLP_ENSEMBLE_MAX_MEMBERS; member k is float32 [N, ld[k]], V <= ld[k]
 * columns used; ld: a host array.  beta_dev: a host array of K device pointers, or null; an entry may be null.  A null entry (or
 * a null array) means beta_k = 1 exactly, otherwise beta_k = beta_dev[k][0] is read on the device (a calibration state's first
 * double, as slnlp_reliability_rows takes it), so the call never waits for the host.  weights: a host array of K finite doubles
 * > 0, or null; the call normalises them in fp64, w_k = weights[k] / (their sum in increasing k); null: w_k = 1 / K.  The
 * members travel to the kernel by value in its argument struct: no device table is uploaded, and the host arrays may be freed
 * as soon as the call returns.  out float32 [N, ld_out]; rows double [N, 4] or null (then no diagnostics are formed).
 *
 * Per row i, in fp64 throughout (z itself is float32):
 *   member term   slnlp_scale_logp's expression before its rounding: zmax_k the float32 row maximum, a_k = beta_k zmax_k, the
 *                 columns at the maximum counted and not exponentiated:
 *                 l_kc = (beta_k z_kc - a_k) - log1p(rest_k + (n_at_max_k - 1)),  p_kc = exp(l_kc); a -inf column is an ordinary
 *                 value with p = 0
 *   mixture       (every mode) m_c = max_k l_kc, mix_c = m_c + log(sum_k w_k exp(l_kc - m_c)) with k increasing, -inf when m_c is
 *   SLNLP_VOTE_SOFT   out_c = (float) mix_c: the arithmetic mean of the members' probabilities
 *   SLNLP_VOTE_LOG    u_c = sum_k w_k l_kc with k increasing, out_c = (float)((u_c - umax) - log(sum_c exp(u_c - umax))): the
 *                 weighted geometric mean, renormalised (a product of experts)
 *   rows[i]       with pbar_c = exp(mix_c) whatever the mode:
 *     [0] H_total = -sum_c pbar_c mix_c                              the entropy of the mixture
 *     [1] H_mean  = sum_k w_k (-sum_c p_kc l_kc)                     the expected entropy of a member
 *     [2] MI      = sum_k w_k sum_c p_kc (l_kc - mix_c)              their difference, the mutual information -- summed directly
 *                   and not formed as [0] - [1], so nothing cancels: MI >= 0 up to rounding, MI <= -sum_k w_k log w_k
 *     [3] n_disagree: the members whose own arg-max -- the first maximum of their float32 row, slnlp_score_rows' order, which
 *                   beta > 0 does not move -- is not the first maximum of the float32 out row as stored
 *     terms with a zero probability are 0.
 * A row in which a member holds a NaN or has a row maximum that is not finite, or (SLNLP_VOTE_LOG) whose every u_c is -inf, gets
 * NaN in every out column and rows = (NaN, NaN, NaN, -2): slnlp_reliability_rows' NaN-row convention.
 *
 * One launch: 256 threads, a wave per row, lanes stride the columns; no LDS, no atomics.  Every sum is formed in a fixed order
 * (a lane's columns ascending, the members ascending within a column, then the wave butterfly), so the result is a function of
 * the arguments alone.  The second pass re-reads the K rows, every column by the lane that uses it: out may alias NO input.
 * Errors (SLNLP_ERR_INVALID_ARG with a message, before anything is launched): a null logp, ld or out, or a null member pointer;
 * K outside 1..SLNLP_ENSEMBLE_MAX_MEMBERS; N or V outside 1..INT32_MAX; an unknown mode; ld[k] < V or ld_out < V; a weight that
 * is not finite or not > 0; a misaligned pointer (members and out 4 bytes, betas 8, rows 32); out or rows overlapping a
 * member, a beta or each other. */
#define SLNLP_ENSEMBLE_MAX_MEMBERS 32
#define SLNLP_VOTE_SOFT 0     /* arithmetic mean of the members' probabilities */
#define SLNLP_VOTE_LOG  1     /* weighted geometric mean, renormalised (product of experts) */
int slnlp_ensemble_rows(const float* const* logp, const int64_t* ld, const double* const* beta_dev, const double* weights,
                        int K, int64_t N, int64_t V, int mode, float* out, int64_t ld_out, double* rows, void* stream);

/* ------------------------------------------------------------ ranking metrics --
 * What the one-vs-rest ROC AUC and the average precision of every class are functions of (slnlp/metrics.py forms the scores on
 * the host: auc_macro, auc_weighted, ap_macro, ap_weighted; NeuralNetClassifier.ranking).  logp float32 [N, ld], V <= ld columns
 * used; y int64 [N].  For class c the rows with y = c are its positives (P_c), every other row with a label in [0, V) is a
 * negative (Q_c); the score of row j for class c is z[j, c], the float32 log-prob as stored: ties are ties of the float32 values
 * (slnlp_score_rows' rank convention), -0.0 equals +0.0, -inf is an ordinary value.  Per row i, with c = y_i and x = z[i, c]:
 *   gt_neg = #{negatives j: z[j, c] > x}   eq_neg = #{negatives j: z[j, c] == x}   ge_pos = #{positives j: z[j, c] >= x} (i itself counts)
 * rows  int32 [N, 4] or null: (gt_neg, eq_neg, ge_pos, code).  code 0: counted; -1: a label outside [0, V) (looked at first, never
 *       used as an index; neither a positive nor a negative of any class; the counts are 0); -2: column c holds a NaN in some row
 *       with a valid label, which leaves class c undefined (the counts are 0).
 * table double [V + 1, 4]: row c < V = (P_c, the NaN entries of column c over the rows with a valid label,
 *       sum_{i in c} (2 (Q_c - gt_neg) - eq_neg), sum_{i in c} ge_pos / (ge_pos + gt_neg + eq_neg)); the two sums are 0 for a class
 *       with a NaN; row V = (rows with a valid label, rows with a bad label, 0, 0).  The third column is an exact integer
 *       (N <= SLNLP_RANK_MAX_ROWS keeps 2 N^2 below 2^53).  AUC_c = table[c][2] / (2 P_c Q_c): Mann-Whitney with half credit for
 *       ties, sklearn's trapezoid.  AP_c = table[c][3] / P_c: sklearn's step-wise average_precision_score (tied positives share a
 *       threshold and contribute the same term).  Both are undefined for P_c = 0, Q_c = 0 or a NaN in the column.
 * One launch, one block of 256 threads per class: the class's positives are compacted into LDS in ascending row order (ballots,
 * no cursor), sorted there, and the column is streamed against them with two binary searches per row and integer LDS atomics on
 * three histograms; suffix sums give the counts.  More than SLNLP_RANK_CHUNK positives: the same per chunk.  The sums are formed
 * in a fixed order (sorted position, fixed tree, chunks ascending) and no global atomics are used: the result is a function of
 * the arguments alone.  Errors (SLNLP_ERR_INVALID_ARG with a message, before anything is launched): a null logp, y or table; N
 * outside 1..SLNLP_RANK_MAX_ROWS; V outside 1..INT32_MAX - 1; ld < V; a misaligned pointer (logp 4 bytes, y 8, rows 16, table
 * 32); an output overlapping an input or the other output. */
#define SLNLP_RANK_CHUNK 2048
#define SLNLP_RANK_MAX_ROWS 67108863    /* 2^26 - 1 */
int slnlp_ranking_rows(const float* logp, int64_t ld, const int64_t* y, int64_t N, int64_t V, int32_t* rows, double* table, void* stream);

/* -------------------------------------------------- conformal prediction sets --
 * Split conformal prediction on a set of log-probs (NeuralNetClassifier.conformalize / predict_set / coverage; slnlp/metrics.py's
 * conformal_report): per sample the set of classes that holds the true one with probability 1 - alpha, given a threshold that
 * is an order statistic of the scores of held-out rows.  tests/conformal_ref.py restates everything below in numpy.
 *
 * Probabilities.  logp float32 [N, ld], V <= ld columns used; beta = beta_dev ? beta_dev[0] : 1.  p_c = exp(beta z_c - a) / s0
 * with slnlp_topk_rows' / slnlp_reliability_rows' fp64 decomposition (zmax the float32 row maximum, a = beta zmax, the columns
 * at the maximum counted, the others summed, s0 = 1 + rest): p of the arg-max is slnlp_reliability_rows' conf bit for bit.
 * Order.  Within a row the classes stand in the arg-max's total order: larger value first, equal values by ascending column;
 * -0.0 equals +0.0; -inf is an ordinary value with p = 0.  rank(c) is 1-based in that order; before(c) is the sum of p over the
 * classes in front of c, added in ascending rank order in fp64 (a lane adds its contiguous run of ranks, the 64 lane totals are
 * added from lane 0 upwards): a fixed order that depends on neither grid nor timing.
 * Score of class c.  method SLNLP_CONFORMAL_LAC: s(c) = 1 - p_c.  method SLNLP_CONFORMAL_APS: s(c) = before(c) + u p_c +
 * lam max(0, rank(c) - k_reg); lam = 0 is APS (Romano, Sesia, Candes 2020), lam > 0 RAPS (Angelopoulos et al. 2021).
 * u = 1 unless `randomized`; then ONE u per row, shared by its classes: u = (w + 0.5) 2^-32 with w word 0 of the Threefry
 * call at counter (row, draw, SLNLP_CONFORMAL_STAGE, 0) under key (seed low word, seed high word, 0, 0), the 12 rounds of the
 * dropout masks -- a counter no other draw of the library uses with that key (slnlp_balanced_order: stages 0, 1, 2; the
 * augmentation: the timestep; the bootstrap: SLNLP_BOOT_STAGE).  `draw` tells calibration draws from prediction draws.
 * Codes.  0 an ordinary row.  -2 a row that holds a NaN or whose maximum is not finite (looked at first): no sort, size 0,
 * every set word 0, rank 0, score NaN.  -1: y given and the label outside [0, V) (never used as an index): the set and its
 * size are formed, rank and covered are 0, the score is NaN.
 *
 * slnlp_conformal_rows.  y int64 [N] or null.  qhat_dev: null, or a device double read on the device (state[0] of
 * slnlp_conformal_quantile: no host round trip between calibrating and predicting); the set of a row is {c : s(c) <= qhat}
 * and may be empty (LAC, or deterministic APS when the top probability exceeds qhat): reported, not patched.
 *   score double [N] or null (needs y): s(y_i), NaN for a code other than 0
 *   rows  int32 [N, 4] or null: (set size, rank(y_i) or 0 without y, covered 0 / 1, code); size and covered 0 without qhat_dev
 *   sets  uint32 [N, W] or null (needs qhat_dev), W = ceil(V / 32): bit c & 31 of word c >> 5 is set iff c is in the set; the
 *         padding bits of the last word are 0
 * One launch, one wave per row: the row is sorted in LDS as 64-bit keys (~order key of the value << 32 | column, ascending)
 * by one bitonic network over the next power of two >= max(V, 64); every lane then owns a contiguous run of ranks, decodes
 * the values, forms p, before and the scores and sets its bits in an LDS mask with integer ORs; the words leave in whole
 * stores.  No global atomics: the result is a function of the arguments alone.
 *
 * slnlp_conformal_quantile.  Over the n rows with code 0 (rows[i][3]): k = ceil((double)(n + 1) * (1.0 - alpha)) in fp64 and
 * qhat the k-th smallest score, +inf when k > n (n = 0 included).  state double [4] = (qhat, n, k, rows with a code other than
 * 0).  One block: an exact radix select over order-preserving uint64 keys of the scores, 8 passes over 256-bin integer
 * histograms in LDS (correct, not fast, for large N).
 *
 * slnlp_conformal_summary.  table int64 [V + 1, 4], zeroed by the call on the stream; over the rows with code 0 whose label
 * lies in [0, V): row c < V, columns 0..2 = (rows of class c, covered rows, sum of their set sizes); column 3 of row s = the
 * rows whose set has size s, s = 0..V; table[V][0] = every other row.  Integer atomics.  Two launches.
 *
 * Errors (SLNLP_ERR_INVALID_ARG with a message, before anything is launched): a null logp / score and rows of the quantile /
 * rows, y and table of the summary / state; V outside 1..SLNLP_CONFORMAL_MAX_V; ld < V; N outside 1..INT32_MAX; alpha outside
 * (0, 1); lam negative or not finite; k_reg < 0; an unknown method; score without y; sets without qhat_dev; a misaligned
 * pointer (logp, sets 4 bytes; y, beta_dev, qhat_dev, score 8; rows 16; state, table 32); an output overlapping an input or
 * another output. */
#define SLNLP_CONFORMAL_MAX_V 1024
#define SLNLP_CONFORMAL_LAC 0
#define SLNLP_CONFORMAL_APS 1
#define SLNLP_CONFORMAL_STAGE 0x636f6e66u   /* the draw's counter word 2 ("conf") */
#define SLNLP_CONFORMAL_STATE_BYTES 32      /* double[4] */
int slnlp_conformal_rows(const float* logp, int64_t ld, const int64_t* y, int64_t N, int64_t V, const double* beta_dev, int method,
                         double lam, int k_reg, int randomized, uint64_t seed, uint32_t draw, const double* qhat_dev, double* score,
                         int32_t* rows, uint32_t* sets, void* stream);
int slnlp_conformal_quantile(const double* score, const int32_t* rows, int64_t N, double alpha, double* state, void* stream);
int slnlp_conformal_summary(const int32_t* rows, const int64_t* y, int64_t N, int64_t V, int64_t* table, void* stream);

/* ------------------------------------------------------- selective prediction --
 * Whether the confidence of a set of log-probs ranks its own errors, and where to cut when the model may decline to answer
 * (NeuralNetClassifier.risk_coverage / fit_rejection / predict_selective; slnlp/metrics.py's selective_report): the risk-coverage
 * curve, its area (AURC, Geifman & El-Yaniv) and the reject option.  tests/selective_ref.py restates everything below in numpy.
 *
 * Per row.  logp float32 [N, ld], V <= ld columns used; y int64 [N] or null; beta = beta_dev ? beta_dev[0] : 1.  zmax, a = beta zmax,
 * n_max, rest and s0 = 1 + rest are slnlp_topk_rows' / slnlp_reliability_rows' fp64 decomposition (e_c = exp(beta z_c - a) over the
 * columns NOT at the maximum, those at the maximum counted).
 *   pred   the arg-max in slnlp_score_rows' order (a NaN first, larger values first, equal values by ascending column)
 *   code   -2: the row holds a NaN or its maximum is not finite (looked at first); -1: y given and the label outside [0, V) (never
 *          used as an index); else 0.  Rows with another code than 0 are EXCLUDED: they take part in no count below.
 *   wrong  1 iff y is given, the code is 0 and pred != y_i
 *   kappa  the confidence, fp64; the order of kappa is the order of acceptance.  NaN for code -2; formed for code -1.
 *          SLNLP_SEL_MAX_PROB     1 / s0: slnlp_topk_rows' prob[i][0] and slnlp_reliability_rows' conf bit for bit
 *          SLNLP_SEL_MARGIN       p(1) - p(2): 0 when n_max >= 2, else (1 - e2) / s0 with e2 the largest e_c (V = 1: e2 = 0, kappa 1)
 *          SLNLP_SEL_NEG_ENTROPY  sum_c p_c ln p_c = (sum_c e_c t_c) / s0 - log1p(rest), t_c = beta z_c - a; a term with e_c == 0
 *                                 counts as 0; each lane adds its columns in ascending order, the lanes meet in a fixed tree
 *   accepted  kappa >= tau with tau = tau_dev[0] (a device double[4] whose first entry is the threshold, like the conformal state:
 *          no host round trip between choosing and applying it); 0 without tau_dev and for code -2
 * slnlp_selective_rows writes kappa double [N] and rows int32 [N, 4] = (pred, wrong, accepted, code).  One launch, one wave per row.
 *
 * Per included row.  slnlp_selective_counts takes kappa and rows as above (or as a caller made them); a row is included when its
 * code is 0 and its kappa is no NaN (a code-0 row with a NaN kappa is counted with the -2 rows).  With n the included rows:
 *   ge_i = #{included j: kappa_j >= kappa_i}        ge_wrong_i = #{included j with wrong_j != 0: kappa_j >= kappa_i}
 * exact integers; ties are ties of the fp64 values and -0.0 equals +0.0.  The threshold tau = kappa_i accepts ge_i rows at
 * selective risk ge_wrong_i / ge_i and coverage ge_i / n.  counts int32 [N, 2] = (ge, ge_wrong); (0, 0) for an excluded row.
 * table double [SLNLP_SEL_TABLE_HEAD + ceil(N / SLNLP_SEL_CHUNK)]:
 *   [0..7]   n, E = the included wrong rows, rows with code -1, every other excluded row, S = sum_i ge_wrong_i / ge_i, AURC = S / n
 *            (NaN for n = 0), 0, 0.  AURC is the mean of the prefix risks when no two rows tie and, unlike it, a function of the
 *            multiset of rows.
 *   [8 + 2 l], [9 + 2 l], l < 8    coverage at risk: (ge, ge_wrong) of the largest ge_i with (double)ge_wrong_i <= risks[l] * (double)ge_i,
 *            (0, 0) when there is none and for l >= nr
 *   [24 + 2 l], [25 + 2 l], l < 8  risk at coverage: (ge, ge_wrong) of the smallest ge_i >= ceil(coverages[l] * (double)n), (0, 0)
 *            for n = 0 and for l >= nc
 *   [40 + b]  the sum of ge_wrong_i / ge_i over chunk b of included rows (0 for a chunk that holds none): S adds them ascending
 * risks / coverages are HOST arrays of nr / nc <= SLNLP_SEL_MAX_LEVELS numbers in [0, 1], copied by the call.
 * Three launches on the stream, no host wait: the level cells take their neutral elements; one block of 256 threads per chunk of
 * SLNLP_SEL_CHUNK included rows (chunked by included ordinal in ascending row order: ballots, no cursor) sorts its chunk's
 * order-preserving 64-bit keys in LDS, streams all N rows against them with a binary search and integer LDS atomics on two
 * histograms, takes suffix sums, adds its terms in a fixed order and reduces the levels with 64-bit integer atomic max / min on
 * (ge << 32 | ge_wrong), which commute; one block adds the chunk sums in ascending order and writes the table.  No float atomics:
 * the result is a function of the arguments alone.  Every chunk's block reads all N rows, so the work is O(N^2 / SLNLP_SEL_CHUNK x
 * log SLNLP_SEL_CHUNK); SLNLP_SEL_MAX_ROWS bounds that work (and keeps the counts in int32): it is NOT a measured limit.
 *
 * Errors (SLNLP_ERR_INVALID_ARG with a message, before anything is launched): a null logp, kappa, rows, counts or table, null
 * risks / coverages with a count above 0; N outside 1..SLNLP_SEL_MAX_ROWS; V outside 1..INT32_MAX - 1; ld < V; an unknown score;
 * nr or nc outside 0..SLNLP_SEL_MAX_LEVELS; a level outside [0, 1] (a NaN included); a misaligned pointer (logp 4 bytes; y,
 * beta_dev, tau_dev, kappa, counts 8; rows 16; table 32); an output overlapping an input or the other output. */
#define SLNLP_SEL_MAX_PROB 0
#define SLNLP_SEL_MARGIN 1
#define SLNLP_SEL_NEG_ENTROPY 2
#define SLNLP_SEL_CHUNK 2048
#define SLNLP_SEL_MAX_LEVELS 8
#define SLNLP_SEL_TABLE_HEAD 40
#define SLNLP_SEL_MAX_ROWS 1048576      /* 2^20: 512 chunks; bounds the quadratic work, not a measured limit */
#define SLNLP_SEL_STATE_BYTES 32        /* double[4]: tau first */
int slnlp_selective_rows(const float* logp, int64_t ld, const int64_t* y, int64_t N, int64_t V, int score, const double* beta_dev,
                         const double* tau_dev, double* kappa, int32_t* rows, void* stream);
int slnlp_selective_counts(const double* kappa, const int32_t* rows, int64_t N, const double* risks, int nr, const double* coverages,
                           int nc, int32_t* counts, double* table, void* stream);

/* --------------------------------------------------------------- label audit --
 * Confident learning (Northcutt, Jiang and Chuang 2021) on a set of labelled log-probs (LogProbJudge.label_issues; slnlp/metrics.py's
 * label_audit_report): which rows' labels are probably wrong, what they should probably be, and how noisy the labels are.  It is
 * meaningful on log-probs of rows the model has NOT been fitted on (slnlp.OutOfFold).  tests/label_audit_ref.py restates everything
 * below in numpy.
 *
 * logp float32 [N, ld], V <= ld columns used (padding is never read); y int64 [N]; beta = beta_dev ? beta_dev[0] : 1.  Everything
 * but logp is fp64.  zmax, a = beta zmax and s0 are slnlp_topk_rows' / slnlp_reliability_rows' fp64 decomposition, and THE
 * PROBABILITY of column c of row i is
 *   p_ic = 1 / s0 for a column at the maximum, exp(beta z_ic - a) / s0 for any other
 * -- slnlp_topk_rows' prob bit for bit -- wherever it is formed below: the same (row, column) gives the same bits in every pass.
 *   code   -2: the row holds a NaN or its maximum is not finite (looked at first); -1: the label lies outside [0, V) (never used as
 *          an index); else 0.  Only rows with code 0 are USABLE: the others enter no sum and no count but nan_rows / bad_labels.
 *   pred   the arg-max in slnlp_score_rows' order (a NaN first, larger values first, equal values by ascending column)
 *   s      p_{i, y_i}, the self-confidence             other  p of the first column other than y_i in that order; 0 for V = 1
 *   m      s - other, the normalised margin            p_pred 1 / s0 (formed for code -1 too)
 *          s, other and m are NaN for an unusable row, p_pred for code -2
 *   n_c    the usable rows labelled c                  t_c    (sum of their s) / n_c; NaN for n_c = 0.  Thread t of a block of 256
 *          adds its rows t, t + 256, ... ascending, a fixed binary tree adds the threads: the order depends on N alone.  With
 *          n_c = 1 the division by 1.0 is exact and t_c is that row's s, so its own p >= t_c holds with equality
 *   k      the first column c with p_ic >= t_c in the arg-max's order on z_i (a NaN t_c compares false); -1: none, or not usable
 *   flags  bit 0: k >= 0 and k != y_i, the label issue; bit 1: pred != y_i; 0 for an unusable row
 *   joint  int32 [V V + 1]: cell y_i V + k_i counts the usable rows with k_i >= 0, the last entry every other row
 *          (slnlp_confusion_matrix on (k, y)); pairs int32 [M, 3] = (given, confident, count): slnlp_confusion_pairs of the joint
 *
 * buf, in bytes from its start, with e(x) = x rounded up to an even number (every piece is 8-byte aligned):
 *   head    int64 [8]: usable rows, bad_labels, nan_rows, usable rows with k = -1, issues (bit 0), arg-max disagreements (bit 1), 0, 0
 *   t       double [V]          s      double [N]           m      double [N]
 *   n       int32 [e(V)]        joint  int32 [e(V V + 1)]   pairs  int32 [e(3 M)]
 *   k       int32 [e(N)]        code   int32 [e(N)]         flags  int32 [e(N)]
 *   pred    int32 [e(N)]        other  double [N]           p_pred double [N]
 *   work    slnlp_confusion_pairs_workspace_bytes(V, M) bytes
 * in this order, SLNLP_AUDIT_HEAD_BYTES first; buf_bytes must cover all of it.  What a report needs ends with flags.
 *
 * Eight launches on the stream, no host wait: the rows (a wave per row), the classes (a block per class), the confident classes
 * (a wave per row), slnlp_confusion_matrix's two, slnlp_confusion_pairs' two, one block for the head.  No floating-point atomics:
 * the result is a function of the arguments alone.
 *
 * slnlp_scatter_logp: out[rows[i], c] for i < n, c < V is row i of logp -- with beta_dev, slnlp_scale_logp's value for that row
 * bit for bit (one row body serves both); with null, the float32 value itself.  rows int64 [n]; an index outside [0, N_out) is
 * skipped and never used as an address; rows of out that no index names are left alone.  The indices must be distinct (the
 * caller checks: two equal ones race).  out float32 [N_out, ld_out] must not overlap any input.  One launch, a wave per row.
 *
 * Errors (SLNLP_ERR_INVALID_ARG with a message, before anything is launched): a null logp, y, buf, rows or out; N, n or N_out
 * outside 1..INT32_MAX; V outside 1..SLNLP_CONFUSION_MAX_V (label_audit: the joint is V x V) or 1..INT32_MAX (scatter_logp); ld or
 * ld_out < V; M outside 1..SLNLP_PAIRS_MAX; buf_bytes too small; a misaligned pointer (logp, out 4 bytes; y, beta_dev, buf, rows 8);
 * an output overlapping an input. */
#define SLNLP_AUDIT_HEAD_BYTES 64
int slnlp_label_audit(const float* logp, int64_t ld, const int64_t* y, int64_t N, int64_t V, const double* beta_dev, int M, void* buf,
                      int64_t buf_bytes, void* stream);
int slnlp_scatter_logp(const float* logp, int64_t ld, int64_t n, int64_t V, const double* beta_dev, const int64_t* rows, float* out,
                       int64_t ld_out, int64_t N_out, void* stream);

/* ---------------------------------------------------------- training dynamics --
 * What happened to every train row DURING a fit, kept on the device epoch by epoch (NeuralNetClassifier(train_dynamics=True);
 * slnlp/metrics.py's train_dynamics_report): dataset cartography (Swayamdipta et al. 2020: confidence, variability, correctness),
 * forgetting events (Toneva et al. 2019) and the area under the margin, AUM (Pleiss et al. 2020).  The statistics describe the
 * memorisation itself, so -- unlike the label audit -- they are meant for a fit's own train rows.  tests/train_dynamics_ref.py
 * restates everything below in numpy.
 *
 * One call takes ONE epoch's train log-probs: logp float32 [n_visit, ld], V <= ld columns used (padding is never read), in VISIT
 * order; y int64 [n_visit] the labels in visit order; order int64 [n_visit] the dataset row r of visit i (NULL: r = i); N the rows
 * of the dataset; epoch >= 1 its number.  ALL PER-ROW STATE IS INTEGER, so the result is a pure function of the arguments: it
 * depends neither on the order of the visits within the epoch nor on the order in which atomics land, and no floating-point atomic
 * is involved (under a balanced resample a row is visited several times per epoch: visits to one row do collide).  Per visit i:
 *   code     -3: r lies outside [0, N) (never used as an address); -2: the row holds a NaN or its maximum is not finite (looked at
 *            before the label, as in slnlp_label_audit); -1: the label lies outside [0, V) (never used as an index); else 0.  Only a
 *            visit with code 0 is USABLE: the others enter no sum and no count but the head's three skipped counts.
 *   pred     the arg-max in slnlp_score_rows' order (a NaN first, larger values first, equal values by ascending column); written
 *            for every code.  correct = (pred == y_i), 0 for an unusable visit
 *   q        uint64 rint(min(p, 1) 2^20) with p = p_{i, y_i}, slnlp_label_audit's self-confidence at beta = 1 bit for bit
 *            (1 / s0 for a label at the maximum, exp(z_iy - a) / s0 otherwise, on slnlp_topk_rows' fp64 row head); 0 if unusable
 *   mq       int64 rint(clamp((double)z_iy - (double)z_i,other, -1024, 1024) 2^20), `other` the first column other than y_i in
 *            the arg-max's order; 0 for V = 1 and for an unusable visit.  Both operands are float32, so the difference is exact
 *            in fp64 and mq restatable bit for bit; a label at -inf gives -1024 2^20, a label that is the only finite column
 *            +1024 2^20.  No exp is involved
 * and a usable visit adds into row r with integer atomics: v_e += 1, c_e += correct (the epoch's scratch), sum_q += q,
 * sum_q2 += q q, sum_mq += mq (two's complement).  Then THE FOLD, per dataset row with v_e > 0:
 *   a = (c_e == v_e), the row was right at EVERY visit of the epoch;
 *   visits += v_e; correct_visits += c_e; epochs_seen += 1; epochs_correct += a; forgetting += (last == 1 && !a);
 *   first_learned = epoch if it is still -1 and a holds; last = a (-1: never seen); v_e = c_e = 0.
 * With one visit per epoch that is Toneva's forgetting event at epoch granularity.  A row whose visits reach 2^23
 * (SLNLP_DYN_VISIT_BITS) sets the head's overflow flag: q q <= 2^40, so sum_q2 < 2^63 up to 2^23 visits; |mq| <= 2^30, so
 * |sum_mq| < 2^53.  Beyond it the sums wrap.
 *
 * state, in bytes from its start, with e(x) = x rounded up to an even number (every piece is 8-byte aligned):
 *   head     int64 [8]: epochs folded, usable visits, bad labels (code -1), NaN rows (-2), bad row indices (-3), rows seen so far,
 *            overflow (0 / 1), 0 -- all cumulative over the calls since the reset
 *   sum_q    uint64 [N]         sum_q2         uint64 [N]        sum_mq         int64 [N]
 *   visits   uint32 [e(N)]      correct_visits uint32 [e(N)]     epochs_seen    int32 [e(N)]
 *   epochs_correct int32 [e(N)] forgetting     int32 [e(N)]      first_learned  int32 [e(N)]      last  int32 [e(N)]
 *   v_e      uint32 [e(N)]      c_e            uint32 [e(N)]
 * in this order, SLNLP_DYN_HEAD_BYTES first: slnlp_train_dynamics_state_bytes(N) in all (-1 and a message for N outside
 * 1..INT32_MAX).  What a report needs ends with last.  visits, the per-visit scratch of ONE call (overwritten by the next):
 *   q uint64 [n]    mq int64 [n]    code int32 [e(n)]    correct int32 [e(n)]    pred int32 [e(n)]      with n = n_visit:
 * 16 n + 12 e(n) bytes, which visits_bytes must cover.
 *
 * slnlp_train_dynamics_reset: one launch of the library's own that zeroes the state and sets first_learned and last to -1.
 * slnlp_train_dynamics_epoch: a fixed sequence of two launches on the stream, no host wait: the visits (a wave per visit
 * position), the fold (a thread per dataset row and per visit position; the head's counts are integer sums over a fixed tree per
 * block and one integer atomic per block and count).
 *
 * Errors (SLNLP_ERR_INVALID_ARG with a message, before anything is launched): a null logp, y, state or visits; N, n_visit or epoch
 * outside 1..INT32_MAX; V outside 1..INT32_MAX; ld < V; state_bytes or visits_bytes too small; a misaligned pointer (logp 4 bytes;
 * y, order, state, visits 8); state or visits overlapping an input or each other. */
#define SLNLP_DYN_HEAD_BYTES 64
#define SLNLP_DYN_FRAC_BITS 20          /* q and mq are fixed point with this many fraction bits */
#define SLNLP_DYN_VISIT_BITS 23         /* a row at 2^23 visits sets the overflow flag */
int64_t slnlp_train_dynamics_state_bytes(int64_t N);
int slnlp_train_dynamics_reset(void* state, int64_t state_bytes, int64_t N, void* stream);
int slnlp_train_dynamics_epoch(const float* logp, int64_t ld, const int64_t* y, const int64_t* order, int64_t n_visit, int64_t V,
                               int64_t N, int64_t epoch, void* state, int64_t state_bytes, void* visits, int64_t visits_bytes,
                               void* stream);

/* -------------------------------------------------------------- batch gather --
 * One train batch in visit order (a shuffled epoch, iterator_train__shuffle): row i of the outputs is row
 * order[row0 + i] of the dataset X int64 [rows, S] / lengths int64 [rows] / y int64 [rows]; order == NULL: row row0 + i.
 * lengths and len_out are both NULL or both given.  B x S ids to X_out, B entries to len_out / y_out.  One launch: a wave
 * moves a row, so loads and stores are whole lines.  The indices (and row0 + B against the order's length) are the
 * caller's contract, like every pointer here.  Everything a fit stages that is not a lockstep group goes through this:
 * the eager step, the staging buffers of a captured graph, the torch-stepped loop. */
int slnlp_gather_batch(const int64_t* X, const int64_t* lengths, const int64_t* y, const int64_t* order, int64_t row0,
                       int B, int S, int64_t* X_out, int64_t* len_out, int64_t* y_out, void* stream);

/* ------------------------------------------------------ class-balanced epochs --
 * The visit order of a class-balanced train epoch (iterator_train__balance), drawn on the device straight into an order
 * table (slnlp_gather_batch, slnlp_*_lockstep_set_order).  Labels y [n] in [0, n_classes); a class that is present, with n_c
 * rows, keeps u_c of them and is visited t_c times: the reference's smoothed targets around the mean size u of the present
 * classes, smooth(v) = round-half-even(u + ln v), u_c = min(n_c, smooth(n_c)), t_c = max(u_c, smooth(u_c)).  An epoch
 * visits n_bal = sum t_c rows, the same number every epoch.
 * Random words: Threefry-4x32, the dropout masks' 12 rounds, key (seed low word, seed high word, 0, 0), counter
 * (index, epoch, stage, 0).  Of the output words X0..X3 a 64-bit key is X1 << 32 | X0, the over-sampling word is X0.
 *   stage 0, index = row i: the rows of a class are ranked by (key, i) ascending; the u_c lowest ranks are kept,
 *            kept_c[r] = the row of rank r;
 *   stage 1, index = base_c + j: extra j in [0, t_c - u_c) of class c (base_c: the class's first slot) takes
 *            kept_c[(X0 * u_c) >> 32];
 *   stage 2, index = slot: the slots -- class after class in ascending id, each class's kept rows then its extras -- are
 *            ranked by (key, slot) ascending; order_out[rank] = the slot's row.
 * The result is a function of (y, seed, epoch) alone: no atomics, nothing depends on the grid or on timing.
 * slnlp_balance_plan_create reads the labels from HOST memory and keeps the per-class tables (and the scratch of a draw) in
 * device memory it owns; the upload is ordered on stream.  Errors (SLNLP_ERR_INVALID_ARG, with a message): null pointers,
 * n < 1, a label outside [0, n_classes), n or n_bal above SLNLP_BALANCE_MAX_ROWS (the ranks are counted, which is quadratic).
 * slnlp_balanced_order: two launches on stream, no host synchronisation, no allocation.  y_dev: the same labels on the
 * device, read only for y_out [n_bal] = the labels in visit order (both may be NULL); epoch in [0, 2^32).  A plan serves one
 * draw at a time (its scratch links the two launches): draws of one plan on several streams need an order between them. */
#define SLNLP_BALANCE_MAX_ROWS 65536
typedef struct slnlp_balance_plan slnlp_balance_plan;
int slnlp_balance_plan_create(const int64_t* y_host, int64_t n, int n_classes, void* stream, slnlp_balance_plan** out);
int64_t slnlp_balance_plan_rows(const slnlp_balance_plan* plan);          /* n_bal */
void slnlp_balance_plan_destroy(slnlp_balance_plan* plan);
int slnlp_balanced_order(const slnlp_balance_plan* plan, const int64_t* y_dev, uint64_t seed, int64_t epoch,
                         int64_t* order_out /* [n_bal] */, int64_t* y_out /* [n_bal] or NULL: labels in visit order */,
                         void* stream);

/* ------------------------------------------------- train-time input augmentation --
 * One epoch's augmented copy of a train split (iterator_train__augment): frame dropping deletes random timesteps, token
 * masking replaces random tokens by unk.  X int64 [n, S], L int64 [n]; row i has len = clamp(L[i], 0, S).  Every position
 * t < len makes one Threefry-4x32 call, the dropout masks' 12 rounds, key (seed low word, seed high word, 0, 0), counter
 * (i, epoch, t, 0); of the output words only X0 is used:
 *   the position draws drop iff (X0 & 0xFFFF) < thr16(p_drop), and mask iff (X0 >> 16) < thr16(p_mask),
 *   thr16(p) = min(floor(p * 65536 + 0.5), 65535), the dropout masks' threshold rule.
 * When every position t < len of a row drew drop, none is dropped: a row never loses all of its frames.  The kept positions,
 * in ascending t, are written compacted to X_out[i, 0 .. len'): unk where the position drew mask, X[i, t] otherwise;
 * X_out[i, len' .. S) = pad; L_out[i] = len'.  Positions >= len of X are never read.  The result is a function of the
 * arguments alone: no atomics, nothing depends on the grid or on timing.  One launch on stream, no host synchronisation, no
 * allocation.  Errors (SLNLP_ERR_INVALID_ARG with a message, before anything is launched): a null pointer, n < 1, S < 1,
 * epoch outside [0, 2^32), a probability outside [0, 1), an output buffer overlapping an input (the kernel is not in-place)
 * or the other output. */
int slnlp_augment_rows(const int64_t* X, const int64_t* L, int64_t n, int64_t S, int64_t pad, int64_t unk, float p_drop,
                       float p_mask, uint64_t seed, int64_t epoch, int64_t* X_out /* [n, S] */, int64_t* L_out /* [n] */,
                       void* stream);

/* --------------------------------------------------------- occlusion attribution --
 * What in the input a prediction rests on (LogProbJudge.attribute; slnlp/metrics.py's attribution_report): hide one UNIT of a row
 * -- a window of frames, or one phonological field in every frame -- run the forward passes again and measure how far the
 * log-probability of the class falls.  tests/attribution_ref.py restates everything below in numpy.
 *
 * THE VARIANT TABLE (slnlp.ops.occlusion_variants builds it on the host): variants int32 [M, 3] = (row, unit, bin), sorted by
 * (row, unit); row_start int32 [N + 1], the offset of each row's first variant.  bin in [0, n_bins) keys the summary's table.
 *
 * slnlp_occlude_rows builds the variants' inputs.  X int64 [n, S], L int64 [n], y int64 [n]; row i has len = clamp(L[i], 0, S).
 * Variant j = (row, unit, .) writes X_out[j, :], L_out[j], y_out[j] = y[row] (the Transformer's decoder consumes it):
 *   SLNLP_OCCLUDE_MASK        the window [lo, hi) = [unit stride, min(unit stride + width, len)) becomes unk; positions below len
 *                             outside it are copied, X_out[j, len .. S) = pad, L_out[j] = len
 *   SLNLP_OCCLUDE_DROP        the window's positions are deleted and the rest closes up in ascending order; the tail is pad,
 *                             L_out[j] = len - (hi - lo).  A window that covers the whole row (lo = 0, hi = len) is MASKED
 *                             instead: a row never loses all of its frames
 *   SLNLP_OCCLUDE_SUBSTITUTE  every position t < len takes sub[X[row, t] F + unit] when 0 <= X[row, t] < Vx, else X[row, t] itself;
 *                             the tail is pad, L_out[j] = len.  sub int64 [Vx, F] (slnlp.ingest.field_substitutions); width and
 *                             stride are not read
 * Positions >= len of X are never read.  A variant is INVALID when its row lies outside [0, n), or its unit is invalid for that
 * row -- unit < 0; a window starting at or behind len (so every unit of a row of length 0); a field outside [0, F) or a row of
 * length 0 under SUBSTITUTE: it reads nothing and writes an all-pad row with L_out = 0 and y_out = 0.  One wave per variant,
 * integers only, no LDS, no atomics: a function of the arguments alone.  One launch on stream, no host wait.
 *
 * slnlp_attribution_rows judges M variant rows var float32 [M, ld_v] against their base rows base float32 [N, ld_b] (V columns
 * used of each, padding never read).  variants, vals and ints are the WHOLE table's arrays: row j of var is variant off + j, and
 * entries off .. off + M - 1 are read and written (the caller has room for off + M).  beta = state ? state[0] : 1.  Both rows go
 * through slnlp_topk_rows' / slnlp_reliability_rows' fp64 row head: zmax, a = beta zmax, rest = sum e - 1, s0 = 1 + rest, and
 *   p(k) = 1 / s0 at the maximum, exp(beta z_k - a) / s0 elsewhere;    lp(k) = (beta z_k - a) - log1p(rest)
 * The target c is y[row] (target 0; y may be null with target 1) or the base row's arg-max (target 1).  At variant off + j:
 *   vals double [., 3]   drop = lp_b(c) - lp_v(c);  dp = p_b(c) - p_v(c);  kl = sum_k p_b(k) (lp_b(k) - lp_v(k)), terms with
 *                        p_b(k) == 0 count as 0; lane l adds its columns l, l + 64, ... ascending, then the wave's fixed order
 *   ints int32 [., 2]    the variant row's arg-max (slnlp_score_rows' order), and a code: 0 usable; -3 the variant's row lies
 *                        outside [0, N) (looked at first; arg-max -1, nothing else is read); -2 the base or the variant row holds
 *                        a NaN or has no finite maximum; -1 the label lies outside [0, V) (never used as an index)
 * A row with a non-zero code stores NaN in all three values.  A usable variant may still have a drop of +-inf or NaN (-inf at the
 * target in one or both rows) and a kl of +inf: IEEE arithmetic on the definitions above.  One launch, a wave per variant.
 *
 * slnlp_attribution_summary reduces a finished table; four launches, no host wait, no floating-point atomics.
 *   rows_i int32 [N, 6]   per row: the base arg-max, the target c (-1 when there is none), the base row's code (0, -1, -2 as
 *                         above), the number of usable variants, the number of flips (usable variants whose arg-max is not the
 *                         base's), top_unit (-1 for none)
 *   rows_d double [N, 4]  lp_b(c) (NaN without a target); top_drop, the largest finite drop of the row's usable variants -- ties to the
 *                         smaller unit -- and min_drop, the least (NaN for none); sum_drop over the finite drops (lane l of the
 *                         row's wave adds entries l, l + 64, ... of the row's segment, then the wave's fixed order)
 *                         A row's segment is row_start[r] .. row_start[r + 1] clamped into [0, M]; entries of another row are skipped.
 *   cell int32 [M]        scratch: ((c n_bins + bin) << 1) | flip of a usable variant whose bin lies in [0, n_bins), else -1
 *   table_i int64 [V, n_bins, 3], table_d double [V, n_bins, 2], keyed by (target class, bin): count -- the usable variants whose
 *                         drop and kl are both finite, the ones in the sums --, flips over all usable variants of the cell,
 *                         nonfinite -- the usable variants with a drop or kl that is not finite, counted here and kept out of the
 *                         sums --; the sums of drop and of kl.  One block per cell: thread t adds variants t, t + 256, ...
 *                         ascending, a fixed binary tree adds the 256 threads, so a cell's bits depend on M alone.
 *   head int64 [8]        usable, bad-label (-1), non-finite (-2) and invalid (-3) variants, total flips, 0, 0, 0
 *
 * Errors (SLNLP_ERR_INVALID_ARG with a message, before anything is launched): a null pointer (sub only under SUBSTITUTE, y only
 * with target 0, state never); n, N, S or M outside 1..INT32_MAX (M, off + M: INT32_MAX / 3); a kind or target that is none of the
 * above; width or stride outside 1..S; F or n_bins outside 1..SLNLP_ATTR_MAX_BINS; V outside 1..SLNLP_CONFUSION_MAX_V; ld < V; a
 * misaligned pointer; an output overlapping an input or another output. */
#define SLNLP_OCCLUDE_MASK 0
#define SLNLP_OCCLUDE_DROP 1
#define SLNLP_OCCLUDE_SUBSTITUTE 2
#define SLNLP_ATTR_MAX_BINS 64
#define SLNLP_ATTR_HEAD_BYTES 64
int slnlp_occlude_rows(const int64_t* X, const int64_t* L, const int64_t* y, int64_t n, int64_t S, const int32_t* variants, int64_t M,
                       int kind, int64_t width, int64_t stride, int64_t pad, int64_t unk, const int64_t* sub, int64_t Vx, int64_t F,
                       int64_t* X_out /* [M, S] */, int64_t* L_out /* [M] */, int64_t* y_out /* [M] */, void* stream);
int slnlp_attribution_rows(const float* base, int64_t ld_b, const float* var, int64_t ld_v, const int64_t* y, const int32_t* variants,
                           int64_t N, int64_t M, int64_t V, int target, const double* state, int64_t off, double* vals, int32_t* ints,
                           void* stream);
int slnlp_attribution_summary(const float* base, int64_t ld_b, const int64_t* y, const int32_t* variants, const int32_t* row_start,
                              int64_t N, int64_t M, int64_t V, int n_bins, int target, const double* state, const double* vals,
                              const int32_t* ints, int32_t* cell, int64_t* head, int64_t* table_i, double* table_d, int32_t* rows_i,
                              double* rows_d, void* stream);

/* ------------------------------------------- edit-distance nearest neighbours (csrc/edit_knn.hip) --
 * All-pairs unit-cost Levenshtein distances between two sets of token rows and the k nearest references of every query: the
 * non-neural baseline (slnlp.EditKNN) and the audit of a split (slnlp.split_audit).  Everything is integer until the votes, there
 * are no floating-point atomics, and every result is a pure function of the arguments: the same bytes on every run, on any stream,
 * beside other kernels.
 *
 * Xq int64 [nq, .] with row stride ldq (in tokens, >= 1), Lq int64 [nq]; Xr / ldr / Lr [nr] the references.  A row is USABLE when
 * its length L lies in 0..min(SLNLP_EDIT_MAX_LEN, its row stride); only the first L tokens of a usable row are read, tokens are
 * compared as full int64 values, and nothing past L -- and nothing of an unusable row -- influences anything.  Rows longer than 64
 * tokens are REFUSED (flagged and counted), never truncated: the kernel is Myers' bit-vector recurrence with the query in one
 * 64-bit word.  The slnlp_edit_long_* entry points below run the multi-word recurrence and take rows of up to 512 tokens.
 *
 * slnlp_edit_distances: dist uint8 [nq, nr], the distance of every (query, reference) pair (at most 64), 255 where either row is
 * unusable.  One launch.
 *
 * slnlp_edit_knn_rows: distances into scratch (slnlp_edit_knn_scratch_bytes: one byte per pair; nq nr <= SLNLP_EDIT_MAX_PAIRS,
 * -1 with a message otherwise), then the selection and the head: three queued launches, no host wait.  Per query the k
 * (1..SLNLP_EDIT_MAX_K) usable references of smallest distance, ordered by (distance, reference index) ascending -- ties at the k-th
 * distance go to the lower index.  exclude int64 [nq] or null: the one reference index query i skips (leave-one-out), -1 none; any
 * other value outside 0..nr-1 skips nothing and sets SLNLP_EDIT_CODE_EXCLUDE.  An unusable reference is never a neighbour; an
 * unusable query gets none and SLNLP_EDIT_CODE_QUERY.
 *   nbr  int32 [nq, k, 2]   (distance, reference index), (-1, -1) past found
 *   rows int32 [nq, 4]      found, the usable references (but the excluded one) with distance <= radius (0..64), the nearest
 *                           distance or -1, the code bits
 *   head int64 [8]          unusable queries, unusable references, then 0 (the third is written by the votes)
 *
 * slnlp_edit_knn_logp: neighbours to float32 log-probs [nq, V] with row stride ld, one wave per query in fp64, neighbours in list
 * order: w_j = 1 (SLNLP_EDIT_UNIFORM) or exp(-d_j / (tau n_j)) (SLNLP_EDIT_DISTANCE), n_j = max(Lq, Lr_j, 1) when normalize, else 1;
 * s_c = the sum of w_j over the neighbours with label yr[index_j] = c, W the sum of all w_j; p_c = (s_c + lam prior_c) / (W + lam)
 * with prior float64 [V]; logp_c = (float) log(p_c).  A neighbour whose label lies outside 0..V-1 is skipped, out of W as well, and
 * counted in head[2].  found = 0: the log of the prior.  A query with SLNLP_EDIT_CODE_QUERY: a row of NaN -- reported, not patched.
 * Two queued launches.
 *
 * Errors (SLNLP_ERR_INVALID_ARG with a message, before anything is launched): a null pointer (exclude may be null); nq or nr
 * outside 1..SLNLP_EDIT_MAX_ROWS (2^30: the kernels' 32-bit row loops step past the end by less than a block), V outside 1..INT32_MAX; more than SLNLP_EDIT_MAX_PAIRS pairs; a row stride < 1; k outside 1..SLNLP_EDIT_MAX_K; radius outside
 * 0..64; weights or normalize that is none of the above; tau or lam not finite and > 0; ld < V; a scratch that is too small; a
 * misaligned pointer; an output overlapping an input or another output. */
#define SLNLP_EDIT_MAX_LEN 64
#define SLNLP_EDIT_MAX_K 64
#define SLNLP_EDIT_MAX_ROWS 1073741824
#define SLNLP_EDIT_MAX_PAIRS 2147483648LL
#define SLNLP_EDIT_HEAD_BYTES 64
#define SLNLP_EDIT_CODE_QUERY 1
#define SLNLP_EDIT_CODE_EXCLUDE 2
#define SLNLP_EDIT_UNIFORM 0
#define SLNLP_EDIT_DISTANCE 1
int slnlp_edit_distances(const int64_t* Xq, int64_t ldq, const int64_t* Lq, int64_t nq, const int64_t* Xr, int64_t ldr, const int64_t* Lr,
                         int64_t nr, uint8_t* dist /* [nq, nr] */, void* stream);
int64_t slnlp_edit_knn_scratch_bytes(int64_t nq, int64_t nr);
int slnlp_edit_knn_rows(const int64_t* Xq, int64_t ldq, const int64_t* Lq, int64_t nq, const int64_t* Xr, int64_t ldr, const int64_t* Lr,
                        int64_t nr, const int64_t* exclude, int64_t k, int64_t radius, void* scratch, int64_t scratch_bytes,
                        int64_t* head /* [8] */, int32_t* rows /* [nq, 4] */, int32_t* nbr /* [nq, k, 2] */, void* stream);
int slnlp_edit_knn_logp(const int32_t* nbr, const int32_t* rows, const int64_t* Lq, const int64_t* Lr, const int64_t* yr, int64_t nq,
                        int64_t nr, int64_t k, int64_t V, int weights, double tau, int normalize, double lam, const double* prior,
                        float* logp, int64_t ld, int64_t* head, void* stream);

/* ------------------------------------------- edit-distance neighbours of long rows (csrc/edit_long.hip) --
 * The same search for rows of up to SLNLP_EDIT_LONG_MAX_LEN = 512 tokens (slnlp.EditKNN(max_len=...), slnlp.split_audit(max_len=...)):
 * the unit-cost Levenshtein distance by Myers' recurrence in its MULTI-WORD form, the query in ceil(L / 64) = 1..8 64-bit words
 * (csrc/edit_myers_multi.hpp).  Everything is an integer until the votes; every result is a pure function of the arguments, as
 * above.  The slnlp_edit_* entry points above are untouched by it: their limit, bytes and messages are what they were.
 *
 * max_len in 1..SLNLP_EDIT_LONG_MAX_LEN is an argument of every entry point.  A row is USABLE when its length L lies in
 * 0..min(max_len, its row stride); only the first L tokens of a usable row are read, tokens are compared as full int64 values, and
 * nothing past L -- and nothing of an unusable row -- influences anything.  A row longer than max_len is REFUSED (flagged and
 * counted) although it may fit its row stride, never truncated.  d(q, r) <= max(len q, len r) <= max_len.  Where every row has at most
 * 64 tokens the distances are those of slnlp_edit_distances, value for value.
 *
 * slnlp_edit_long_distances: dist uint16 [nq, nr], 65535 where either row is unusable.  One launch.
 *
 * slnlp_edit_long_knn_rows: distances into scratch (slnlp_edit_long_knn_scratch_bytes: TWO bytes per pair, 2-byte aligned; nq nr <=
 * SLNLP_EDIT_MAX_PAIRS, -1 with a message otherwise), then the selection and the head as slnlp_edit_knn_rows: the k
 * (1..SLNLP_EDIT_MAX_K) usable references of smallest distance ordered by (distance, index), ties at the k-th distance to the lower
 * index, exclude as above, radius in 0..max_len.  It writes the same head / rows / nbr buffers; the code bit SLNLP_EDIT_CODE_QUERY
 * says that the query's length lies outside 0..min(max_len, ldq).  Three queued launches, no host wait.
 *
 * slnlp_edit_long_knn_logp: the vote of slnlp_edit_knn_logp, operation for operation, but a neighbour is listed when 0 <= d <=
 * max_len (slnlp_edit_knn_logp lists none beyond 64).  Two queued launches.
 *
 * Errors (SLNLP_ERR_INVALID_ARG with a message that names the entry point, before anything is launched): those of the
 * slnlp_edit_* entry points, and: max_len outside 1..SLNLP_EDIT_LONG_MAX_LEN, radius outside 0..max_len, a null or misaligned dist
 * (2 bytes), a scratch that is too small or not 2-byte aligned.
 *
 * The phonology-weighted search below has no long form: its rows stay at SLNLP_EDIT_MAX_LEN = 64 tokens. */
#define SLNLP_EDIT_LONG_MAX_LEN 512
int slnlp_edit_long_distances(const int64_t* Xq, int64_t ldq, const int64_t* Lq, int64_t nq, const int64_t* Xr, int64_t ldr, const int64_t* Lr,
                              int64_t nr, int64_t max_len, uint16_t* dist /* [nq, nr] */, void* stream);
int64_t slnlp_edit_long_knn_scratch_bytes(int64_t nq, int64_t nr);
int slnlp_edit_long_knn_rows(const int64_t* Xq, int64_t ldq, const int64_t* Lq, int64_t nq, const int64_t* Xr, int64_t ldr, const int64_t* Lr,
                             int64_t nr, int64_t max_len, const int64_t* exclude, int64_t k, int64_t radius, void* scratch,
                             int64_t scratch_bytes, int64_t* head /* [8] */, int32_t* rows /* [nq, 4] */, int32_t* nbr /* [nq, k, 2] */,
                             void* stream);
int slnlp_edit_long_knn_logp(const int32_t* nbr, const int32_t* rows, const int64_t* Lq, const int64_t* Lr, const int64_t* yr, int64_t nq,
                             int64_t nr, int64_t k, int64_t V, int64_t max_len, int weights, double tau, int normalize, double lam,
                             const double* prior, float* logp, int64_t ld, int64_t* head, void* stream);

/* ------------------------------------------- near-duplicate groups of one data set (csrc/dup_groups.hip) --
 * The connected components of "rows within radius edits of each other" (slnlp.duplicate_groups): the undirected graph over the N
 * rows of ONE data set whose edges are the pairs {i, j}, i != j, with d(i, j) <= radius; every row is labelled with the LOWEST row
 * index of its component.  That labelling is unique, so the result is a pure function of the arguments: the same bytes on every
 * run, on any stream, beside other kernels.  Integers only, integer atomics only.
 *
 * The distances are what slnlp_edit_distances (width 1: uint8, 255 for a pair with an unusable row), slnlp_edit_long_distances and
 * slnlp_field_distances[_w] (width 2: uint16, 65535) write, with the data set on both sides.  The N x N matrix need not be
 * resident: the caller forms the rows q0 .. q0 + nq - 1 against all N rows, links them, and reuses the memory for the next chunk.
 * Every row is linked exactly once; the chunks may come in any order.  Three entry points, all queued, no host wait:
 *
 * slnlp_dup_groups_begin: parent[i] = i, degree[i] = 0, head zeroed.  One launch.
 *
 * slnlp_dup_groups_link: dist [nq, N] of `width` bytes an element, row qi the distances of row i = q0 + qi.  A wave per row:
 * degree[i] = #{j != i : dist[qi, j] <= radius}, and for every such j < i the trees of i and j are joined by hooking the LARGER
 * root under the SMALLER (a 32-bit compare-and-swap on parent) -- the distance is symmetric, so j < i sees every edge once.  A row
 * whose own entry dist[qi, q0 + qi] is the sentinel is UNUSABLE: it links to nothing, keeps degree 0 and is counted in head[2].
 * One launch.
 *
 * slnlp_dup_groups_finish: group[i] = the root of i = the lowest row index of its component; head[0] = the groups (rows with
 * group[i] == i), head[1] = the edges = the degree sum halved.  Two launches.  It may be called again after further links.
 *
 *   head int64 [8]    groups | edges within the radius | unusable rows | code | the degree sum | 0 0 0
 *
 * code is 0.  Every loop of these kernels counts its rounds to N + 1 although none can need them (a walk to the root descends
 * strictly; a failed compare-and-swap means another hook completed, and at most N - 1 exist); a thread that ran out sets code to 1
 * and leaves, and the result is then not to be used.
 *
 * Errors (SLNLP_ERR_INVALID_ARG with a message that names the entry point, before anything is launched): a null pointer; N or nq
 * outside 1..SLNLP_EDIT_MAX_ROWS; q0 < 0 or q0 + nq > N; more than SLNLP_EDIT_MAX_PAIRS pairs; width not 1 or 2; radius outside
 * 0..254 (width 1) or 0..65534 (width 2); a misaligned pointer (dist: width bytes; parent, degree, group: 4; head: 8); an output
 * overlapping an input or another output. */
#define SLNLP_DUP_HEAD_BYTES 64
int slnlp_dup_groups_begin(int32_t* parent /* [N] */, int32_t* degree /* [N] */, int64_t N, int64_t* head /* [8] */, void* stream);
int slnlp_dup_groups_link(const void* dist /* [nq, N] */, int width, int64_t nq, int64_t N, int64_t q0, int64_t radius,
                          int32_t* parent /* [N] */, int32_t* degree /* [N] */, int64_t* head /* [8] */, void* stream);
int slnlp_dup_groups_finish(const int32_t* parent /* [N] */, int64_t N, int32_t* group /* [N] */, int64_t* head /* [8] */, void* stream);

/* ------------------------------------------- gloss structure of one data set (csrc/gloss_structure.hip) --
 * What the LABELS of a data set look like under one of the edit distances above (slnlp.gloss_structure): a silhouette per row, a
 * medoid per class, and the class-to-class distance table.  The device forms the integers; the host divides.  Integers only,
 * integer atomics only: the result is a pure function of the arguments -- the same bytes on every run, on any stream, and for any
 * chunking of the rows.
 *
 * The data set has N rows; label[i] is in 0..C-1, or -1 for a row LEFT OUT (the host gives -1 to the rows the metric refuses).  d is
 * the N x N matrix slnlp_edit_distances (width 1: uint8, sentinel 255), slnlp_edit_long_distances or slnlp_field_distances[_w]
 * (width 2: uint16, sentinel 65535) writes with the data set on both sides; d <= max_distance.
 *
 *   n_c               #{j : label[j] = c}
 *   T[i, c]           for a labelled row i: the sum of d(i, j) over j != i with label[j] = c.  Exact; below 2^32, since begin refuses
 *                     max_distance N >= 2^32.
 *   own[i]            T[i, label[i]]
 *   other_class[i]    among the classes c != label[i] with n_c > 0 the one that minimises T[i, c] / n_c.  The comparison is exact:
 *                     T[i, a] n_b < T[i, b] n_a in 64-bit integers; ties go to the LOWER class.  -1 if there is no such class.
 *   other[i]          T[i, other_class[i]], 0 where other_class is -1.
 *   class_sum[a, b]   the sum over the rows i of class a of T[i, b]: int64, symmetric; the diagonal counts every within-class pair
 *                     twice.
 *   medoid[c]         the row of class c with the smallest own[i], ties to the LOWEST row; -1 for an empty class.
 *   A row left out writes own = other = 0 and other_class = -1, and is no column of anybody's sum.
 *
 * The host's values, in fp64 from those integers (sklearn's silhouette_samples conventions): a = own / (n - 1), b = other / n_other,
 * s = (b - a) / max(a, b), and s = 0 where the row's class has one member, where there is no other class, or where max(a, b) = 0;
 * the mean distance of classes a != b is class_sum[a, b] / (n_a n_b), of a class to itself class_sum[a, a] / (n_a (n_a - 1)).
 *
 * The N x N matrix need not be resident: the caller forms the rows q0 .. q0 + nq - 1 against all N rows, hands them to
 * slnlp_gloss_structure_rows and reuses the memory for the next chunk.  Every row arrives exactly once; the chunks may come in any
 * order.  Three entry points, all queued, no host wait:
 *
 * slnlp_gloss_structure_begin: count = the n_c (integer atomics), class_sum = 0, med_sum = UINT64_MAX, medoid = "none", head zeroed
 * but for the labelled rows and the rows left out.  Two launches.
 *
 * slnlp_gloss_structure_rows: dist [nq, N] of `width` bytes an element, row qi the distances of row i = q0 + qi.  A wave per row
 * adds every element into a table of C uint32 sums in LDS (LDS integer adds; four waves a block: 16 C bytes), then takes own,
 * other and other_class from the table, adds T[i, c] to class_sum[label[i], c] (64-bit atomic adds) and takes a 64-bit atomic
 * minimum of own[i] into med_sum[label[i]].  The sentinel at a pair of two labelled rows is a breach of the contract, not data:
 * it sets code bit 0 and adds nothing.  One launch.
 *
 * slnlp_gloss_structure_finish: every row with own[i] == med_sum[label[i]] takes a 32-bit atomic minimum of i into
 * medoid[label[i]]; then "none" becomes -1 and head[1] = the classes that have a medoid.  Two launches.
 *
 *   head int64 [8]    labelled rows | non-empty classes | rows left out | code | the sum of own | 0 0 0
 *
 * code is 0, or: bit 0 (1) the sentinel met at a labelled pair; bit 1 (2) a label outside -1..C-1 (such a row is treated as left
 * out by every kernel: no index is formed from its label).  With a code the result is not to be used.
 *
 * Errors (SLNLP_ERR_INVALID_ARG with a message that names the entry point, before anything is launched): a null pointer; N or nq
 * outside 1..SLNLP_EDIT_MAX_ROWS; C outside 1..SLNLP_GLOSS_MAX_CLASSES; max_distance outside 1..65534 or max_distance N >= 2^32;
 * q0 < 0 or q0 + nq > N; more than SLNLP_EDIT_MAX_PAIRS pairs; width not 1 or 2; a misaligned pointer (dist: width bytes; label,
 * count, own, other, other_class, medoid: 4; class_sum, med_sum, head: 8); an output overlapping an input or another output. */
#define SLNLP_GLOSS_HEAD_BYTES 64
#define SLNLP_GLOSS_MAX_CLASSES 1024
int slnlp_gloss_structure_begin(const int32_t* label /* [N] */, int64_t N, int64_t C, int64_t max_distance, int32_t* count /* [C] */,
                                int64_t* class_sum /* [C, C] */, int64_t* med_sum /* [C] */, int32_t* medoid /* [C] */, int64_t* head /* [8] */,
                                void* stream);
int slnlp_gloss_structure_rows(const void* dist /* [nq, N] */, int width, int64_t nq, int64_t N, int64_t q0, const int32_t* label /* [N] */,
                               int64_t C, const int32_t* count /* [C] */, uint32_t* own /* [N] */, uint32_t* other /* [N] */,
                               int32_t* other_class /* [N] */, int64_t* class_sum /* [C, C] */, int64_t* med_sum /* [C] */,
                               int64_t* head /* [8] */, void* stream);
int slnlp_gloss_structure_finish(const int32_t* label /* [N] */, const uint32_t* own /* [N] */, const int64_t* med_sum /* [C] */, int64_t N,
                                 int64_t C, int32_t* medoid /* [C] */, int64_t* head /* [8] */, void* stream);

/* ------------------------------------- phonology-weighted edit-distance neighbours (csrc/field_knn.hip) --
 * The same search under a WEIGHTED edit distance (slnlp.PhonoKNN, slnlp.split_audit(field_codes=...)): a token of this data is a
 * composition of F phonological fields, and substituting one frame for another costs the number of fields in which they differ.
 * Everything is an integer until the votes; every result is a pure function of the arguments, as above.
 *
 * codes   int32 [Vt, F] on the device, 1 <= F <= SLNLP_FIELD_MAX_FIELDS, 1 <= Vt <= INT32_MAX: row v holds the per-field value
 *         ids of token id v.
 * sub(a, b) for int64 tokens a, b: 0 if a == b (compared as whole int64 values); otherwise F if either token lies outside
 *         0..Vt-1 (the table is never read for such a token); otherwise #{f : codes[a, f] != codes[b, f]} -- which may be 0:
 *         the table defines which tokens are equivalent.
 * gap     in 1..F: the cost of inserting or deleting one frame.
 * d(q, r) the minimum total cost of substitutions, insertions and deletions that turn q into r;
 *         d <= F max(len q, len r) <= 64 F <= 1024.  With F = 1, codes[v, 0] = v and gap = 1 it is the unit Levenshtein distance.
 * Rows are USABLE exactly as above: a length in 0..min(SLNLP_EDIT_MAX_LEN, row stride); only the first L tokens of a usable row are
 * read, nothing of an unusable one is.
 *
 * slnlp_field_distances: dist uint16 [nq, nr], 65535 where either row is unusable.  One launch.
 *
 * slnlp_field_knn_rows: distances into scratch (slnlp_field_knn_scratch_bytes: TWO bytes per pair, 2-byte aligned), then the
 * selection and the head as slnlp_edit_knn_rows: the k (1..SLNLP_EDIT_MAX_K) usable references of smallest distance ordered by
 * (distance, index), ties at the k-th distance to the lower index, exclude as above, radius in 0..64 F.  It writes the same head /
 * rows / nbr buffers (nbr distances are int32).  Three queued launches, no host wait.
 *
 * slnlp_field_knn_logp: the vote of slnlp_edit_knn_logp with w_j = exp(-d_j / (tau n_j)), n_j = F (normalize ? max(Lq, Lr_j, 1) :
 * 1) -- tau is in frames in both metrics, and at F = 1 the vote is the unit-cost one operation for operation.  A neighbour is
 * listed when 0 <= d <= 64 F.  Two queued launches.
 *
 * Errors (SLNLP_ERR_INVALID_ARG with a message that names the entry point, before anything is launched): those of the
 * slnlp_edit_* entry points, and: F outside 1..SLNLP_FIELD_MAX_FIELDS, Vt outside 1..INT32_MAX, gap outside 1..F, radius outside
 * 0..64 F, a null or misaligned codes (4 bytes) or dist (2 bytes), codes overlapping any output. */
#define SLNLP_FIELD_MAX_FIELDS 16
int slnlp_field_distances(const int64_t* Xq, int64_t ldq, const int64_t* Lq, int64_t nq, const int64_t* Xr, int64_t ldr, const int64_t* Lr,
                          int64_t nr, const int32_t* codes /* [Vt, F] */, int64_t Vt, int64_t F, int64_t gap, uint16_t* dist /* [nq, nr] */,
                          void* stream);
int64_t slnlp_field_knn_scratch_bytes(int64_t nq, int64_t nr);
int slnlp_field_knn_rows(const int64_t* Xq, int64_t ldq, const int64_t* Lq, int64_t nq, const int64_t* Xr, int64_t ldr, const int64_t* Lr,
                         int64_t nr, const int32_t* codes, int64_t Vt, int64_t F, int64_t gap, const int64_t* exclude, int64_t k,
                         int64_t radius, void* scratch, int64_t scratch_bytes, int64_t* head /* [8] */, int32_t* rows /* [nq, 4] */,
                         int32_t* nbr /* [nq, k, 2] */, void* stream);
int slnlp_field_knn_logp(const int32_t* nbr, const int32_t* rows, const int64_t* Lq, const int64_t* Lr, const int64_t* yr, int64_t nq,
                         int64_t nr, int64_t k, int64_t V, int64_t F, int weights, double tau, int normalize, double lam,
                         const double* prior, float* logp, int64_t ld, int64_t* head, void* stream);

/* ------------------------------------------- per-field integer weights (csrc/field_knn.hip, csrc/score.hip) --
 * The same metric with a WEIGHT per field (slnlp.PhonoKNN(field_weights=...), slnlp.fit_field_weights).  All integers.
 *
 * fweights int32 [F] ON THE HOST (the weights reach the kernel by value, among its arguments), each in 0..SLNLP_FIELD_MAX_WEIGHT;
 *         their sum W lies in 1..SLNLP_FIELD_MAX_WEIGHT.  A field of weight 0 is ignored.
 * sub(a, b) 0 if a == b as int64 values; otherwise W (not F) if either token lies outside 0..Vt-1; otherwise the sum of
 *         fweights[f] over the fields with codes[a, f] != codes[b, f] -- which may be 0 for distinct tokens.
 * gap     in 1..W.
 * d(q, r) as above, at most 64 W <= 1024: the uint16 matrix, its 65535, the bins and the selection are those of the unweighted
 *         search with the bound 64 W.  With every weight 1 it IS the unweighted metric (W = F), value for value.
 * The vote is slnlp_field_knn_logp called with W where it takes F: its unit becomes W, so tau stays in frames.
 *
 * slnlp_field_distances_w / slnlp_field_knn_rows_w: slnlp_field_distances / slnlp_field_knn_rows under this metric; radius in
 * 0..64 W; the same scratch, head, rows and nbr.  Errors (SLNLP_ERR_INVALID_ARG, before anything is launched): those of the
 * unweighted entries, and a null fweights, a weight outside 0..16, W outside 1..16, gap outside 1..W, radius outside 0..64 W.
 *
 * slnlp_loo_objective: what a search over candidate weights ranks by.  logp float32 [N, ld] (V columns), y int64 [N]; slot
 * `slot` of the device table of C slots of SLNLP_LOO_SLOT_BYTES bytes gets
 *     int64 rows whose arg-max (the lowest index on a tie) is the label | fp64 sum of -logp[i, y_i] | int64 rows that hold a NaN
 *     | int64 rows whose label lies outside 0..V-1
 * A NaN row and a row with such a label count as wrong and add nothing to the sum.  The sum is taken in a fixed order that
 * depends on N alone: cell t of 256 adds the rows t, t + 256, ... in increasing order, then a binary tree (cells t and t + w for
 * w = 128, 64, .. 1) adds the cells.  One launch of one block, no atomics.  Errors: a null or misaligned pointer, N or V outside
 * 1..INT32_MAX, ld < V, C outside 1..SLNLP_LOO_MAX_SLOTS, slot outside 0..C-1, the table overlapping an input. */
#define SLNLP_FIELD_MAX_WEIGHT 16
#define SLNLP_LOO_SLOT_BYTES 32
#define SLNLP_LOO_MAX_SLOTS 65536
int slnlp_field_distances_w(const int64_t* Xq, int64_t ldq, const int64_t* Lq, int64_t nq, const int64_t* Xr, int64_t ldr, const int64_t* Lr,
                            int64_t nr, const int32_t* codes /* [Vt, F] */, int64_t Vt, int64_t F, const int32_t* fweights /* host [F] */,
                            int64_t gap, uint16_t* dist /* [nq, nr] */, void* stream);
int slnlp_field_knn_rows_w(const int64_t* Xq, int64_t ldq, const int64_t* Lq, int64_t nq, const int64_t* Xr, int64_t ldr, const int64_t* Lr,
                           int64_t nr, const int32_t* codes, int64_t Vt, int64_t F, const int32_t* fweights /* host [F] */, int64_t gap,
                           const int64_t* exclude, int64_t k, int64_t radius, void* scratch, int64_t scratch_bytes, int64_t* head /* [8] */,
                           int32_t* rows /* [nq, 4] */, int32_t* nbr /* [nq, k, 2] */, void* stream);
int slnlp_loo_objective(const float* logp, int64_t ld, const int64_t* y, int64_t N, int64_t V, void* table /* [C] slots */, int64_t C,
                        int64_t slot, void* stream);

/* debug / test helper: materialise the keep mask (1.0 / 0.0) of a dropout site */
int slnlp_dropout_mask(float* out, int R, int C, float p, int site,
                       const unsigned long long* rng, void* stream);

/* ---------------------------------------------------------- LSTM / GRU cell --
 * Point-wise cell of torch.nn.LSTM (gates i,f,g,o) / torch.nn.GRU (r,z,n) as the
 * reference instantiates them (bkp.py:95-100,186-190), one timestep of up to two
 * directions per launch.  xproj = x W_ih^T + b_ih and hproj = h_{t-1} W_hh^T + b_hh
 * come from slnlp_gemm.  Sequence b advances only while t < lengths[b]
 * (pack_padded_sequence, bkp.py:110-114); otherwise the state is carried and the
 * layer output is `fill` (pad_packed_sequence(padding_value=pad_idx), :120-123).
 * lengths == NULL: every row is valid (decoder step). */
typedef struct slnlp_rnn_cell_dir {
    const float* xproj;      /* [B, G*Hd] of this timestep */
    const float* hproj;      /* [B, G*Hd] */
    float* h;                /* [B, Hd] running state, updated in place */
    float* c;                /* LSTM: [B, Hd] running cell state */
    float* hprev_save;       /* [B, Hd] h before the update (kept for backward) */
    float* cprev_save;       /* LSTM */
    float* acts;             /* [B, G*Hd] gate activations (kept for backward) */
    float* hn_save;          /* GRU: [B, Hd] hidden part of the n gate */
    float* out;              /* layer output rows of this timestep (row stride ld_out), or NULL */
    int32_t t, out_row0, out_col0; /* timestep; (row, col) origin of `out` inside its dropout site */
} slnlp_rnn_cell_dir;
int slnlp_rnn_cell_fwd(int lstm, const slnlp_rnn_cell_dir* dirs, int ndir, int B, int Hd,
                       const int64_t* lengths, float fill, int64_t ld_out,
                       float drop_p, int drop_site, const unsigned long long* rng, void* stream);
/* Fused forward timestep: the recurrent GEMM h_{t-1} W_hh^T (+ b_hh) and the cell above in ONE launch (results are
 * bit-identical to slnlp_gemm + slnlp_rnn_cell_fwd).  The new state is written to h_out, which must not alias h_in
 * (workgroups of the same launch still read h_{t-1}): callers chain the per-timestep `hprev` slots, so h_in doubles as
 * the saved h_{t-1} of this step. */
typedef struct slnlp_rnn_step_dir {
    const float* h_in;       /* [B, Hd] state before the step (= what backward needs as h_{t-1}) */
    float* h_out;            /* [B, Hd] state after the step */
    const float* w_hh;       /* [G*Hd, Hd] */
    const float* b_hh;       /* [G*Hd] or NULL */
    const float* xproj;      /* [B, G*Hd] of this timestep (x W_ih^T + b_ih) */
    float* c;                /* LSTM: [B, Hd] running cell state, updated in place */
    float* cprev_save;       /* LSTM */
    float* acts;             /* [B, G*Hd] */
    float* hn_save;          /* GRU */
    float* out;              /* layer output rows of this timestep (row stride ld_out), or NULL */
    int32_t t, out_row0, out_col0;
} slnlp_rnn_step_dir;
int slnlp_rnn_step_fwd(int lstm, const slnlp_rnn_step_dir* dirs, int ndir, int B, int Hd,
                       const int64_t* lengths, float fill, int64_t ld_out,
                       float drop_p, int drop_site, const unsigned long long* rng, int precision, void* stream);
/* Persistent forward of ALL S timesteps of one (bi)directional layer in ONE launch: each workgroup keeps its slice
 * of W_hh in LDS for the whole sequence and the Hd/16 x ndir co-resident workgroups meet at a device-wide barrier
 * between timesteps (results bit-identical to S calls of slnlp_rnn_step_fwd).  Covered shapes: B <= 64,
 * Hd % 64 == 0, G * Hd * 64 bytes + 16 KiB of LDS <= 156 KiB (LSTM: Hd <= 512); otherwise *launched = 0 and nothing
 * was done -- use the per-timestep entry point.  The per-timestep arrays are indexed by time t; `hprev` is the state
 * chain: slot t holds the state BEFORE time t is processed (slot of the first processed timestep: zeros, set by the
 * caller), the last state goes to h_final.  sync: 3 device words {barrier count, barrier generation, error flag},
 * zero before the first use; a non-zero error flag afterwards means a workgroup gave up waiting (bounded spin) and
 * the results are invalid.  Do not run more such launches concurrently than fit the GPU (one workgroup per CU). */
typedef struct slnlp_rnn_layer_dir {
    float* hprev;            /* [S][B, Hd] state chain (input slot zeroed by the caller; the rest is written) */
    float* h_final;          /* [B, Hd] */
    const float* w_hh;       /* [G*Hd, Hd] */
    const float* b_hh;       /* [G*Hd] or NULL */
    const float* xproj;      /* [S][B, G*Hd] */
    float* c;                /* LSTM: [B, Hd] running cell state (zeroed by the caller), updated in place */
    float* cprev;            /* LSTM: [S][B, Hd] */
    float* acts;             /* [S][B, G*Hd] */
    float* hn;               /* GRU: [S][B, Hd] */
    float* out;              /* layer output [S*B, ld_out] at column out_col0, or NULL */
    int32_t out_col0;
    int32_t reverse;         /* 0: t = 0..S-1, 1: t = S-1..0 */
} slnlp_rnn_layer_dir;
int slnlp_rnn_layer_fwd(int lstm, const slnlp_rnn_layer_dir* dirs, int ndir, int B, int Hd, int S,
                        const int64_t* lengths, float fill, int64_t ld_out,
                        float drop_p, int drop_site, const unsigned long long* rng, int precision,
                        uint32_t* sync, int* launched, void* stream);
/* Backward of one timestep: consumes the running d(state) and d(out), emits the gate
 * gradients dgx (w.r.t. xproj) / dgh (w.r.t. hproj; LSTM: same buffer as dgx) and
 * `carry`, the part of dh that bypasses the recurrent matmul; the caller forms
 * dh_state(t-1) = dgh W_hh + carry with slnlp_gemm. */
typedef struct slnlp_rnn_cell_bwd_dir {
    float* dh_state; float* dc_state;
    const float* dout;       /* d(layer output) rows of this timestep (row stride ld_dout), or NULL */
    const float* acts; const float* cprev_save; const float* hprev_save; const float* hn_save;
    float* dgx; float* dgh; float* carry;
    int32_t t, out_row0, out_col0;
    /* optional: dh_state arrives as a sum of partial products (the caller split the K loop of dgh W_hh over
     * several GEMM jobs of one launch): dh = dh_state + sum_{e < n_extra} dh_extra[e * extra_stride + i] */
    const float* dh_extra; int64_t extra_stride; int32_t n_extra;
} slnlp_rnn_cell_bwd_dir;
int slnlp_rnn_cell_bwd(int lstm, const slnlp_rnn_cell_bwd_dir* dirs, int ndir, int B, int Hd,
                       const int64_t* lengths, int64_t ld_dout,
                       float drop_p, int drop_site, const unsigned long long* rng, void* stream);

/* One backward timestep in ONE launch: the recurrent data gradient of the step processed just before and this step's cell
 * backward (what autograd does for nn.LSTM / nn.GRU behind /root/reference/model/base/encoder_decoder_attn_bkp.py:95-132):
 *   dh = dgh_next W_hh + carry (+ dout)  ->  slnlp_rnn_cell_bwd's arithmetic  ->  dgx, dgh, dc_state, carry of this step.
 * dgh_next == NULL (both directions): the first step of a layer, dh = cell.dh_state.  cell.dh_extra / n_extra are ignored; the
 * product's partial sums are added in gate order, exactly as the K-sliced slnlp_gemm_group + slnlp_rnn_cell_bwd pair does.
 * Covered: Hd % 64 == 0 (any B); dgh_next / w_hh 16-byte aligned. */
typedef struct slnlp_rnn_step_bwd_dir {
    slnlp_rnn_cell_bwd_dir cell;
    const float* dgh_next;   /* [B, G*Hd] dgh written by the previous launch of this chain, or NULL */
    const float* w_hh;       /* [G*Hd, Hd] */
} slnlp_rnn_step_bwd_dir;
int slnlp_rnn_step_bwd(int lstm, const slnlp_rnn_step_bwd_dir* dirs, int ndir, int B, int Hd,
                       const int64_t* lengths, int64_t ld_dout,
                       float drop_p, int drop_site, const unsigned long long* rng, int precision, void* stream);

/* Bahdanau (MLP) attention, one query per sequence (bkp.py:304-327 with max_len 1):
 * scores[s] = w_e . tanh(q[b] + proj_key[s,b]); masked where ids[b,s] == pad; softmax;
 * ctx = alphas . value.  proj_key [S*B,Hd] / value [S*B,2Hd] rows are time-major. */
int slnlp_bahdanau_fwd(const float* q, const float* proj_key, const float* value, const float* w_energy,
                       const int64_t* ids, int64_t ld_ids, int64_t pad_idx, int B, int S, int Hd,
                       float* alphas, float* ctx, void* stream);
int slnlp_bahdanau_bwd(const float* q, const float* proj_key, const float* value, const float* w_energy,
                       const float* alphas, const float* dctx, int B, int S, int Hd,
                       float* dq, float* dproj_key, float* dvalue, float* dwe_partial /* [B,Hd] scratch */,
                       float* dw_energy, void* stream);

/* ------------------------------------------------------ Transformer plan --
 * Whole-model drop-in for model.Transformer (model/transformer.py:10-109):
 * the library owns the parameter-arena LAYOUT (names follow the reference
 * state_dict), the activation workspace layout and the launch sequence. */
typedef struct slnlp_tf_config {
    int32_t E, H, N, F;          /* embedding_size, num_heads, num_layers, hidden_size */
    int32_t Vs, Vt;              /* len(src_vocab), len(tgt_vocab) */
    int32_t B, S;                /* max batch, sequence length (S <= 64) */
    int32_t pad_src, pad_tgt;    /* vocab.stoi['<pad>'] (util.py:5-6) */
    float dropout;
    int32_t precision;           /* 1 | 3 */
} slnlp_tf_config;

int slnlp_tf_num_params(const slnlp_tf_config* cfg);
/* i-th parameter in reference state_dict order: name (<=127 chars), shape, offset (floats) */
int slnlp_tf_param_info(const slnlp_tf_config* cfg, int i, char* name, int64_t shape[2], int* ndim,
                        int64_t* offset);
int64_t slnlp_tf_arena_floats(const slnlp_tf_config* cfg);
int64_t slnlp_tf_workspace_bytes(const slnlp_tf_config* cfg);

typedef struct slnlp_tf_buffers {
    float* params;               /* arena, slnlp_tf_arena_floats */
    float* grads;                /* arena-shaped */
    float* momentum;             /* arena-shaped */
    const float* pe;             /* [>=S, E] positional table (positional_encoding.py:27-35) */
    void* workspace;             /* slnlp_tf_workspace_bytes */
    unsigned long long* rng;     /* [2] = {seed, step} */
    float* lr;                   /* [1] */
    float* scalars;              /* [4] = {loss, grad_norm, Adam step count, SGD step count} */
} slnlp_tf_buffers;

typedef struct slnlp_tf_plan slnlp_tf_plan;
int slnlp_tf_create(const slnlp_tf_config* cfg, const slnlp_tf_buffers* buf, slnlp_tf_plan** out);
void slnlp_tf_destroy(slnlp_tf_plan* plan);
/* forward: X int64 [B,S] (row stride S), y int64 [B] -> logp [B,Vt] (may be
 * NULL).  Always evaluates the criterion too (scalars[0] = loss); train != 0
 * applies dropout, keeps activations and seeds backward with d loss/d logits. */
int slnlp_tf_forward(slnlp_tf_plan* plan, const int64_t* X, const int64_t* y, int B, int train,
                     float* logp, void* stream);
/* re-seed backward from an external d loss / d logp (torch autograd owns the criterion) */
int slnlp_tf_seed_dlogp(slnlp_tf_plan* plan, const float* dlogp, void* stream);
/* backward through the whole model into buf.grads (every element written) */
int slnlp_tf_backward(slnlp_tf_plan* plan, void* stream);
/* clip + SGD-momentum on the arena; scalars[1] = pre-clip grad norm */
int slnlp_tf_optim(slnlp_tf_plan* plan, float momentum, float max_norm, void* stream);
/* clip + torch.optim.Adam (amsgrad False) on the arena -- north_star's "fused SGD-momentum/Adam update"; the reference
 * reaches any torch.optim class through pydoc.locate (helper.py:91-104).  exp_avg = buf.momentum, exp_avg_sq = an
 * arena-shaped buffer of the caller's (zero before the first step), step count = scalars[2] (device-side). */
int slnlp_tf_optim_adam(slnlp_tf_plan* plan, float* exp_avg_sq, float beta1, float beta2, float eps, float weight_decay,
                        float max_norm, void* stream);
/* forward(train) + loss + backward + optim in one call */
int slnlp_tf_train_step(slnlp_tf_plan* plan, const int64_t* X, const int64_t* y, int B,
                        float momentum, float max_norm, float* logp, void* stream);
/* Capture one train step over FIXED device buffers (X, y, logp) for batch size
 * B into a hipGraph kept inside the plan (one per distinct B);
 * slnlp_tf_graph_launch(B) replays it.  lr, the dropout step counter and the
 * data are read from device memory, so one captured graph serves every step
 * of a fit.  `stream` must not be the null stream. */
int slnlp_tf_graph_capture_train(slnlp_tf_plan* plan, const int64_t* X, const int64_t* y, int B,
                                 float momentum, float max_norm, float* logp, void* stream);
int slnlp_tf_graph_launch(slnlp_tf_plan* plan, int B, void* stream);
/* test helper: copy a named activation tap ("enc0", "memory", "dec1", "logits", ...; "dmemory": the gradient with respect to
 * the encoder memory, [S*B, E], after a backward); "enc<l>.<planes>" (d2p, hp, ghp, x1p, d1p,
 * ctxp, gqkvp, x2p, xinp): an operand of the layer's gradient GEMMs as its bf16 planes -- the hi plane's [rows, cols] 16-bit words,
 * then the lo plane's, in rows * cols floats */
int slnlp_tf_tap(slnlp_tf_plan* plan, const char* name, float* out, int64_t max_floats,
                 int64_t* n_out, void* stream);
/* The parameter arena was written from outside the library (load_state_dict, a torch optimizer, an in-place edit):
 * data derived from it (the bf16 weight planes the fused update keeps current) is rebuilt by the next forward. */
int slnlp_tf_params_changed(slnlp_tf_plan* plan);
/* test / debug helper: "name byte_offset" lines of the workspace's activation and gradient buffers, in layout order */
int slnlp_tf_debug_layout(const slnlp_tf_config* cfg, char* out, int64_t out_bytes);

/* slnlp_*_destroy wait for the device (hipDeviceSynchronize) before they return: the plan's buffers are the caller's and
 * may be freed next.  on = 0 drops that wait FOR THIS PLAN (never process-wide) -- only for a caller whose buffers come from
 * a stream-ordered allocator on the stream the plan ran on (torch's caching allocator), where the device-wide wait stalls
 * every other host thread's queued work each time a fit ends. */
int slnlp_tf_set_destroy_sync(slnlp_tf_plan* plan, int on);

/* Criterion and update settings of a plan (default: CrossEntropyLoss(ignore_index=pad) and plain SGD-momentum).
 * set_criterion: class_weight [Vt] in HOST memory (copied into device memory the plan owns, on `stream`; NULL: none),
 * label_smoothing in [0, 1], reduction 0 = "mean" / 1 = "sum"; used by every forward (train and eval).
 * set_update: kind SLNLP_UPDATE_SGD -- slnlp_tf_optim runs torch.optim.SGD with dampening / weight_decay / nesterov (the step
 * count lives in scalars[3]); SLNLP_UPDATE_ADAM / _ADAMW -- slnlp_tf_optim_adam runs Adam / AdamW (AdamW: decoupled decay)
 * with the weight_decay of that call, and a lockstep group's Adam update uses THIS weight_decay for the plan instead of the
 * group's (slnlp_tf_lockstep_set_adam), so fits that differ in it step in one group; dampening and nesterov must be 0.
 * A call that changes a setting drops the plan's captured graphs (re-capture with slnlp_tf_graph_capture_train), and a
 * lockstep group drops its programs, hands their table space back and re-records before its next step; a call that changes
 * nothing drops nothing. */
#define SLNLP_UPDATE_SGD 0
#define SLNLP_UPDATE_ADAM 1
#define SLNLP_UPDATE_ADAMW 2
int slnlp_tf_set_criterion(slnlp_tf_plan* plan, const float* class_weight, float label_smoothing, int reduction, void* stream);
int slnlp_tf_set_update(slnlp_tf_plan* plan, int kind, float dampening, float weight_decay, int nesterov);
/* Per-group lr / weight decay of the plan's update (arguments as slnlp_param_groups_create, over the plan's arena):
 * slnlp_tf_optim / slnlp_tf_optim_adam then step group g with lr_dev[g] (device memory, [n_groups], the caller's, read
 * every step) and weight_decay[g] instead of the plan's one lr and the one weight decay.  n_segments == 0 clears the table:
 * the one-group update again.  Drops the captured graphs and makes a lockstep group re-record, as slnlp_tf_set_update. */
int slnlp_tf_set_param_groups(slnlp_tf_plan* plan, int n_segments, const int64_t* seg_begin, const int32_t* seg_group,
                              int n_groups, const float* weight_decay, const float* lr_dev, void* stream);
/* Weight averaging riding the train step: with a non-NULL avg (arena-shaped, the caller's) every update of the plan -- slnlp_tf_optim,
 * slnlp_tf_optim_adam, slnlp_tf_train_step, a captured graph, a recorded lockstep program -- is followed by slnlp_average_step's
 * two launches on (avg, the plan's arena, count, kind, decay); the update kernels themselves are untouched.  NULL removes them.
 * A call that changes the setting drops the captured graphs and makes a lockstep group re-record, as slnlp_tf_set_update. */
int slnlp_tf_set_averaging(slnlp_tf_plan* plan, float* avg, float* count, int kind, float decay);
/* Where backward forms the gradient with respect to the encoder memory (and the cross-attention value biases' gradients).
 * on (default): one launch for all decoder layers behind the decoder's layer loop -- nothing on that chain reads the sum;
 * off: a launch per layer inside the loop, each adding onto the sum.  Same bits either way (the same fp32 operations in the
 * same order); the switch exists for A / B measurements and tests.  A change drops the plan's captured graphs and makes a
 * lockstep group re-record, as slnlp_tf_set_update does. */
int slnlp_tf_set_dmem_batched(slnlp_tf_plan* plan, int on);
/* The decoder's LayerNorms that feed exactly one B-row product on the chain (norm1 -> the cross-attention query projection,
 * norm2 -> linear1, norm3 -> the next layer's V projection, the final norm -> the generator).  on (default; a new plan starts
 * from the environment knob SLNLP_DEC_LN_FUSED=0|1): the LayerNorm is that product's prologue (slnlp_gemm_rows_ln), one launch
 * instead of two, wherever the product is a solo fit's 16 x 16-tile B-row launch; off: a launch each.  Same bits either way.
 * Recorded lockstep programs always hold the two launches.  A change drops the plan's captured graphs, as slnlp_tf_set_update. */
int slnlp_tf_set_dec_ln_fused(slnlp_tf_plan* plan, int on);

/* One kernel sequence per device (default).  The step entry points (slnlp_{tf,rnn}_{forward,backward,optim*,train_step,
 * graph_launch}, slnlp_*_lockstep_{step,epoch}) serialise per device: host threads enqueue whole steps in turn, and a step issued
 * on another stream than the device's previous step waits (event) for that stream's tail, so the library's kernels never overlap
 * across streams inside one process.  Why: MI355X / ROCm 7.2 compute packed fp32 VALU instructions (v_pk_{add,mul,fma}_f32 with
 * op_sel) wrongly in lanes 48-63 while another kernel's waves run MFMA on the same CU (reproducer
 * tools/probes/packed_fp32_repro.hip).  The shipped library is built WITHOUT those instructions (and tests/ disassemble it), so
 * its kernels are bit-stable on overlapping queues; the ordering is kept as the default because it costs nothing with one
 * stream and protects a caller of a library rebuilt with other flags.
 *   slnlp_set_thread_stream_policy(0): the CALLING host thread's steps skip the ordering (1: take part; -1: follow the
 *     process-wide policy again).  For a thread that owns a stream and wants its steps to overlap other threads' -- the grid
 *     search's worker threads (slnlp/net.py) -- never process-wide.
 *   slnlp_set_stream_policy(0): the process-wide switch (probes). */
int slnlp_set_thread_stream_policy(int serialise);
int slnlp_set_stream_policy(int serialise);

/* Split-bf16 passes of the gradient products that run on the plane GEMM (the [S*B]-row dgrad / wgrad of every encoder-side
 * Linear; what autograd computes for nn.Linear behind /root/reference/model/transformer.py:40-45,82-87): the DEFAULT FOR PLANS
 * CREATED AFTERWARDS -- a plan copies both counts at creation and keeps them for its life, so its eager steps, its captured
 * graph, its lockstep program and every host thread that steps it issue the same products; other plans are not touched.  3: the full split, A_lo B_hi + A_hi B_lo + A_hi B_hi (fp32-grade
 * products).  2: dY enters with its bf16 head only (rounded to nearest: unbiased), A_hi (B_hi + B_lo) -- a third less MFMA work,
 * a quarter less operand staging, a three-stage ring in the same LDS.  Default since round 4: wgrad 2, dgrad 2.  Measured against
 * the reference's golden training trajectories (tools/backward_pass_errors.py, profiles/r04_backward_pass_errors.jsonl; cfg2, five
 * steps): worst per-tensor gradient-norm error 2.3e-3 at (2, 2) against 2.6e-3 at (3, 3), loss 6e-5 against 3e-5 (bar 1e-3),
 * pre-clip gradient norm 4.3e-3 against 4.2e-3 (bar 5e-3), weights after five steps 2e-7 either way -- the gradient's distance to
 * the fp32 reference is set by ReLU gates that sit within rounding of zero, not by the 2^-9 rounding of dY.  The forward products
 * (logits, loss: the 1e-3 / bit-exact-argmax bar) always take 3 passes at precision 3.  Env: SLNLP_WGRAD_PASSES / SLNLP_DGRAD_PASSES. */
int slnlp_set_backward_passes(int wgrad, int dgrad);
int slnlp_get_backward_passes(int* wgrad, int* dgrad);

/* Measurement hook (bench.py's roofline): between _start and _stop every plane-GEMM group launch that goes out as a plain launch
 * (not under graph capture) is bracketed by two HIP events on ITS stream; _stop waits for them and returns up to max_out records --
 * the launch's workgroup count, job count, tile geometry (0: 64 x 64, 1: 128 x 128 / 64-k, 2: 128 x 128 / 32-k) and the time
 * between the events in microseconds: the dominant kernel timed inside the train step it belongs to.  Process-wide; not for
 * production steps (two event records per launch). */
typedef struct slnlp_timed_launch { int32_t blocks, njobs, geometry; float us; } slnlp_timed_launch;
int slnlp_launch_timer_start(int max_records);
int slnlp_launch_timer_stop(slnlp_timed_launch* out, int max_out);

/* ---------------------------------------------------------------- lockstep --
 * K Transformer fits of ONE shape (own weights, lr, dropout rate, seed and data) advancing through one launch
 * sequence: every call site of the step is launched once for all K fits, so a 50-row decoder stage becomes a
 * K x 50-row stage at the same latency.  Replaces the reference's one-fit-at-a-time dask tasks
 * (/root/reference/main.py:70-78, helper.py:490-526) for the fits of a work unit; each fit's results are
 * bit-identical to running it alone through slnlp_tf_train_step / slnlp_tf_forward.
 * The plans must outlive the group and must not be stepped on their own while it exists.
 * workspace: slnlp_tf_lockstep_workspace_bytes(cfg, K) bytes, 256-byte aligned, caller-owned (staging + tables). */
typedef struct slnlp_tf_lockstep slnlp_tf_lockstep;
int64_t slnlp_tf_lockstep_workspace_bytes(const slnlp_tf_config* cfg, int K);
int slnlp_tf_lockstep_create(slnlp_tf_plan** plans, int K, void* workspace, int64_t workspace_bytes, void* stream,
                             slnlp_tf_lockstep** out);
void slnlp_tf_lockstep_destroy(slnlp_tf_lockstep* group);
/* data slot (0..3, e.g. train / valid / test) of every fit: X[f] int64 [rows, S], y[f] int64 [rows] on the device,
 * and where a pass over it leaves its results: logp[f] float [rows, Vt], loss[f] float [ceil(rows / batch)] */
int slnlp_tf_lockstep_set_data(slnlp_tf_lockstep* group, int slot, const int64_t* const* X, const int64_t* const* y,
                               int64_t rows, float* const* logp, float* const* loss, void* stream);
/* rows [row0, row0 + B) of the slot, every fit: train != 0 -> forward + criterion + backward + clip + SGD-momentum,
 * else eval-mode forward + criterion.  Log-probs go to logp[f][row0 ..], the batch loss to loss[f][step_index]. */
int slnlp_tf_lockstep_step(slnlp_tf_lockstep* group, int slot, int64_t row0, int B, int step_index, int train,
                           float momentum, float max_norm, void* stream);
/* one pass over the slot in dataset order, batches of `batch` rows (the last may be shorter): no host sync inside */
int slnlp_tf_lockstep_epoch(slnlp_tf_lockstep* group, int slot, int batch, int train, float momentum, float max_norm,
                            void* stream);
/* kernel launches per step of the cached program for (slot, B, train), or -1 if none has been recorded yet */
int slnlp_tf_lockstep_num_launches(slnlp_tf_lockstep* group, int slot, int B, int train);
/* train with clip_grad_norm_ + Adam instead of SGD-momentum from now on (what slnlp_tf_optim_adam does for one fit):
 * exp_avg = each plan's momentum arena, exp_avg_sq[f] = an arena-shaped buffer of the caller's per fit (zero before the first
 * step), step count = each plan's scalars[2]; `momentum` of the step calls is then ignored.  Drops recorded train programs. */
int slnlp_tf_lockstep_set_adam(slnlp_tf_lockstep* group, float* const* exp_avg_sq, float beta1, float beta2, float eps,
                               float weight_decay);
/* per-fit learning-rate tables for per-batch schedules: table[f] = n_steps floats in device memory of the caller (kept alive
 * while set), the rate of fit f by batch index; a NULL entry leaves that fit's rate alone, a NULL `table` clears the setting.
 * From then on a TRAIN step with batch index step_index first stores table[f][step_index] into plan f's buf.lr -- inside the
 * gather launch every step already issues, so num_launches does not change -- and then runs the recorded program;
 * step_index >= n_steps is an argument error (nothing is launched).  Eval steps never touch buf.lr.  Drops no recorded program.
 * A plan with param groups (slnlp_tf_set_param_groups, G groups) has G rates per step: its table is n_steps x G floats, row
 * step_index goes to its lr_dev[0..G).  Fits with different groups, or with none, share a group: as soon as one fit has
 * groups every fit's update is recorded through the grouped kernel -- one launch per call site -- the fits without groups
 * with a one-segment table over their arena (their own buf.lr and weight decay: the one-group kernel's bits).
 * The pointer table's upload is ordered on `stream`, as set_data's. */
int slnlp_tf_lockstep_set_lr_table(slnlp_tf_lockstep* group, const float* const* table, int n_steps, void* stream);
/* per-fit visit order of one data slot (a shuffled epoch): order[f] = n_visit int64 row indices into fit f's dataset of that
 * slot, in device memory of the caller (kept alive while set); a NULL entry leaves that fit in dataset order, a NULL `order`
 * clears the setting for the slot.  n_visit is one number for the group: 1 .. rows, or -- when EVERY fit has a table (a
 * class-balanced epoch visits rows more than once) -- any length up to 2^31 - 1, and the slot's logp[f] / loss[f] buffers then
 * hold n_visit rows / ceil(n_visit / batch) losses (the caller's contract, like every pointer here).  From then on a step of that slot stages
 * row order[f][row0 + i] instead of row row0 + i -- ids, label and, for RNN fits, length -- with row0 + B <= n_visit, and
 * slnlp_tf_lockstep_epoch walks [0, n_visit).  Log-probs and batch losses keep landing at VISIT position (logp[f][row0 ..],
 * loss[f][step_index]).  Only the gather launch reads the table: no recorded program is dropped or re-recorded and
 * num_launches does not change.  The indices are the caller's contract.  set_data on the slot clears its order.  The pointer
 * table's upload is ordered on `stream`, as set_lr_table's. */
int slnlp_tf_lockstep_set_order(slnlp_tf_lockstep* group, int slot, const int64_t* const* order, int64_t n_visit, void* stream);
/* weight averaging for the group's train steps (slnlp_tf_set_averaging for K fits): avg[f] / count[f] per fit, one (kind, decay)
 * for the group.  The two launches run once per step over the K arenas; a fit whose avg[f] is NULL is not averaging yet and its
 * part of the launch does nothing.  While set, the group's setting stands in for the plans' own.  avg == NULL: off.  A call that
 * changes something drops the recorded programs (re-recorded by the next step); num_launches of a train step grows by 2. */
int slnlp_tf_lockstep_set_averaging(slnlp_tf_lockstep* group, float* const* avg, float* const* count, int kind, float decay);
int slnlp_tf_lockstep_set_destroy_sync(slnlp_tf_lockstep* group, int on);   /* as slnlp_tf_set_destroy_sync, for the group's tables */


/* ------------------------------------------------- enc-dec RNN (+attn) plan --
 * Whole-model drop-in for model.EncoderDecoder{LSTM,GRU}Attn
 * (model/base/encoder_decoder_attn_bkp.py:330-413): packed bidirectional encoder
 * (:102-132), bridge (:268-280), ONE Bahdanau-attention decoder step fed <bos>
 * (:202-266 with MAX_OUTPUT_LEN = 1, :332), generator on the decoder state (:40-46,69-76).
 * Same conventions as the Transformer plan; buffers are a slnlp_tf_buffers (pe unused). */
typedef struct slnlp_rnn_config {
    int32_t lstm;                /* 1 = LSTM, 0 = GRU */
    int32_t E, Hd, N;            /* embedding_size, hidden_size, num_layers */
    int32_t Vs, Vt, B, S;
    int32_t pad_src, pad_tgt, bos_idx;   /* bos_idx = tgt_vocab.stoi['<bos>'] (0 on a torchtext-0.6 vocab) */
    float dropout;
    int32_t precision;
} slnlp_rnn_config;
int slnlp_rnn_num_params(const slnlp_rnn_config* cfg);
int slnlp_rnn_param_info(const slnlp_rnn_config* cfg, int i, char* name, int64_t shape[2], int* ndim, int64_t* offset);
int64_t slnlp_rnn_arena_floats(const slnlp_rnn_config* cfg);
int64_t slnlp_rnn_workspace_bytes(const slnlp_rnn_config* cfg);
typedef struct slnlp_rnn_plan slnlp_rnn_plan;
int slnlp_rnn_create(const slnlp_rnn_config* cfg, const slnlp_tf_buffers* buf, slnlp_rnn_plan** out);
void slnlp_rnn_destroy(slnlp_rnn_plan* plan);
/* X int64 [B,S], y int64 [B] (only the criterion reads it: the decoder consumes <bos>), lengths int64 [B] */
int slnlp_rnn_forward(slnlp_rnn_plan* plan, const int64_t* X, const int64_t* y, const int64_t* lengths, int B,
                      int train, float* logp, void* stream);
/* on = 1: run each encoder layer's S timesteps as ONE persistent launch (slnlp_rnn_layer_fwd) instead of one launch
 * per timestep.  Default 0: measured no faster in round 1, and its Hd/16 x 2 workgroups must all be resident at
 * once, so never enable it when several fits share the GPU. */
int slnlp_rnn_set_persistent(slnlp_rnn_plan* plan, int on);
/* on = 1: the encoder's backward through time issues ONE launch per timestep (slnlp_rnn_step_bwd: recurrent data gradient +
 * cell backward; Hd % 64 == 0); on = 0 (default): the cell kernel + K-sliced grouped GEMM pair.  The fused launch halves the
 * launches of a backward pass but measured slower for one fit (cfg3 LSTM 9.11 vs 8.09 ms) and faster only
 * for many GRU fits in lockstep, so it is opt-in (env SLNLP_RNN_FUSED_BWD=1 sets it for new plans).  Same results to fp32
 * rounding.  Takes effect for launches issued (or recorded by a lockstep group) after the call. */
int slnlp_rnn_set_fused_backward(slnlp_rnn_plan* plan, int on);
/* *status = 0 when every device-wide barrier of the plan's persistent kernels completed, 1 if a workgroup timed out
 * (bounded spin; that step's results are invalid).  Synchronises the device. */
int slnlp_rnn_health(slnlp_rnn_plan* plan, int* status);
int slnlp_rnn_seed_dlogp(slnlp_rnn_plan* plan, const float* dlogp, void* stream);
int slnlp_rnn_backward(slnlp_rnn_plan* plan, void* stream);
int slnlp_rnn_optim(slnlp_rnn_plan* plan, float momentum, float max_norm, void* stream);
/* clip + torch.optim.Adam on the arena, as slnlp_tf_optim_adam (exp_avg = buf.momentum, step count = scalars[2]) */
int slnlp_rnn_optim_adam(slnlp_rnn_plan* plan, float* exp_avg_sq, float beta1, float beta2, float eps, float weight_decay,
                         float max_norm, void* stream);
int slnlp_rnn_set_destroy_sync(slnlp_rnn_plan* plan, int on);   /* as slnlp_tf_set_destroy_sync */
/* as slnlp_tf_set_criterion / slnlp_tf_set_update; the decoder's pre_output_layer (never given a gradient) is exempt from
 * weight decay, as torch skips a parameter whose grad is None */
int slnlp_rnn_set_criterion(slnlp_rnn_plan* plan, const float* class_weight, float label_smoothing, int reduction, void* stream);
int slnlp_rnn_set_update(slnlp_rnn_plan* plan, int kind, float dampening, float weight_decay, int nesterov);
/* as slnlp_tf_set_param_groups */
int slnlp_rnn_set_param_groups(slnlp_rnn_plan* plan, int n_segments, const int64_t* seg_begin, const int32_t* seg_group,
                               int n_groups, const float* weight_decay, const float* lr_dev, void* stream);
/* as slnlp_tf_set_averaging; the pre_output_layer (never stepped) is copied into the average, not averaged */
int slnlp_rnn_set_averaging(slnlp_rnn_plan* plan, float* avg, float* count, int kind, float decay);
int slnlp_rnn_train_step(slnlp_rnn_plan* plan, const int64_t* X, const int64_t* y, const int64_t* lengths, int B,
                         float momentum, float max_norm, float* logp, void* stream);
int slnlp_rnn_graph_capture_train(slnlp_rnn_plan* plan, const int64_t* X, const int64_t* y, const int64_t* lengths,
                                  int B, float momentum, float max_norm, float* logp, void* stream);
int slnlp_rnn_graph_launch(slnlp_rnn_plan* plan, int B, void* stream);
/* taps: "enc_out" [S*B,2Hd] (time-major), "enc_final" [N*B,2Hd], "alphas" [B,S], "context" [B,2Hd], "dec_out" [B,Hd], "logits" */
int slnlp_rnn_tap(slnlp_rnn_plan* plan, const char* name, float* out, int64_t max_floats, int64_t* n_out, void* stream);

/* Lockstep for K EncoderDecoder{LSTM,GRU}Attn fits of one shape -- the same contract as slnlp_tf_lockstep_* above
 * (one launch per call site for all K fits, each fit bit-identical to its solo run; replaces the one-fit-at-a-time
 * tasks of /root/reference/main.py:70-78).  The recurrence makes an RNN fit a chain of ~600 dependent small launches
 * per step, so K fits cost little more than one.  A data slot also carries lengths[f] int64 [rows]
 * (pack_padded_sequence semantics, bkp.py:110-114).  The persistent layer kernel must be off (it is by default). */
typedef struct slnlp_rnn_lockstep slnlp_rnn_lockstep;
int64_t slnlp_rnn_lockstep_workspace_bytes(const slnlp_rnn_config* cfg, int K);
int slnlp_rnn_lockstep_create(slnlp_rnn_plan** plans, int K, void* workspace, int64_t workspace_bytes, void* stream,
                              slnlp_rnn_lockstep** out);
void slnlp_rnn_lockstep_destroy(slnlp_rnn_lockstep* group);
int slnlp_rnn_lockstep_set_data(slnlp_rnn_lockstep* group, int slot, const int64_t* const* X, const int64_t* const* y,
                                const int64_t* const* lengths, int64_t rows, float* const* logp, float* const* loss,
                                void* stream);
int slnlp_rnn_lockstep_step(slnlp_rnn_lockstep* group, int slot, int64_t row0, int B, int step_index, int train,
                            float momentum, float max_norm, void* stream);
int slnlp_rnn_lockstep_epoch(slnlp_rnn_lockstep* group, int slot, int batch, int train, float momentum, float max_norm,
                             void* stream);
int slnlp_rnn_lockstep_num_launches(slnlp_rnn_lockstep* group, int slot, int B, int train);
int slnlp_rnn_lockstep_set_adam(slnlp_rnn_lockstep* group, float* const* exp_avg_sq, float beta1, float beta2, float eps,
                                float weight_decay);
int slnlp_rnn_lockstep_set_lr_table(slnlp_rnn_lockstep* group, const float* const* table, int n_steps, void* stream);
int slnlp_rnn_lockstep_set_order(slnlp_rnn_lockstep* group, int slot, const int64_t* const* order, int64_t n_visit, void* stream);
int slnlp_rnn_lockstep_set_averaging(slnlp_rnn_lockstep* group, float* const* avg, float* const* count, int kind, float decay);
int slnlp_rnn_lockstep_set_destroy_sync(slnlp_rnn_lockstep* group, int on);

#ifdef __cplusplus
}
#endif
#endif /* SLNLP_H */
