// gemm_rows.hip -- the decoder's B-row products on PRE-SPLIT operands, register-direct.
//
//   C[M,N] = epilogue( sum_k A(m,k) * B(n,k) ),  A = Ahi + Alo, B = Bhi + Blo  (bf16 planes, both k-major)
//
// The reference decodes ONE target position (transformer.py:82-87: tgt of length 1), so every Linear of its decoder is a
// [batch rows x E] x [E x E]^T product -- 50 rows at the headline config -- on a dependent chain of ~150 launches per step:
// 2 % of the step's FLOPs, 29 % of its time (r04).  Such a launch lasts as long as ONE workgroup does, and gemm.hip's workgroup
// spends its 5.8 us converting fp32 tiles to bf16 hi / lo on their way into LDS: two barriers and a convert / ds_write pass per
// 64-k step, four steps deep even with the K sum on two thread groups (profiles/r04_gemm_timeline.txt).  Here nothing is
// converted and nothing is staged:
//  * operands arrive as bf16 hi / lo planes written by their producers (the optimizer kernels for the weights; LayerNorm, the
//    embedding and this kernel's own epilogue for the activations), zero-padded to 64 rows / 64 k;
//  * a k-major plane row IS the MFMA fragment layout (lane (row l & 15, k-octet l >> 4) reads 16 contiguous bytes), so every
//    wave loads its own fragments straight into registers and issues its MFMAs as they land: no LDS staging, no barrier, no
//    VALU in the K loop; one memory round trip per launch;
//  * ONE MFMA tile (16 rows x 16 columns) per workgroup, 512 threads = 8 waves, wave w = the 64-k tiles w, w + 8, ...: every
//    byte of the workgroup's panels is loaded by one wave, each tile's partial product is computed from zero, and the partials
//    are added in tile order through LDS -- C = ((P_0 + P_1) + P_2) + ... -- this kernel's definition of the K sum
//    (gemm_rows_body: why the tile is this small);
//  * the epilogue (bias -> activation -> gate -> dropout -> residual; fp32 and / or planes out) runs in the accumulator layout;
//    its bias / gate / residual values and the dropout key are requested behind the operand loads, before the first MFMA.
// A SLNLP_ZKERNEL: K fits in lockstep share one launch through grid.z (launch.hpp).
#include <algorithm>
#include <atomic>

#include "common.hpp"
#include "gemm_jobs.hpp"
#include "launch.hpp"
#include "layernorm_row.hpp"
#include "spans.hpp"

namespace slnlp {

typedef __attribute__((ext_vector_type(8))) __bf16 bf16x8;
typedef __attribute__((ext_vector_type(4))) float f32x4;

struct RowsParams {
    slnlp_gemm_args a;
    unsigned drop_thr;
    float drop_scale;
};
__device__ __forceinline__ RowsParams as_global(RowsParams p) {
    launder(p.a);
    return p;
}

#if SLNLP_PROBE_FENCES == 256
// timeline probe build (tools/probes/probe_gemm_timeline.py): wave 0 of every workgroup records 100 MHz timestamps of its phases
constexpr int RTS_MAX = 1 << 14, RTS_W = 6;   // words: entry, first tile's operands landed, partials stored, K sum done, end, {grid, block}
__device__ unsigned long long g_rts[RTS_MAX][RTS_W];
__device__ unsigned g_rts_n;
#define RTS_MARK(slot) do { if (threadIdx.x == 0) rts[slot] = __builtin_amdgcn_s_memrealtime(); } while (0)
#else
#define RTS_MARK(slot) do { } while (0)
#endif

constexpr int RT_THREADS = 512, RT_WAVES = 8;
constexpr int RT_MAX_KTILES = 16;             // K <= 1024

// Work split.  Such a launch is bound by what ONE compute unit can load (about 33 GB/s of 16-byte fragment loads): a workgroup
// of a 64 x 16 tiling pulls the whole activation panel plus its weight columns -- 160 KB at K = 512, in 4.8 us whatever the kernel
// does with them (the fp32-operand kernel and a register-direct plane kernel with that tiling both measured 5.8 us per workgroup:
// profiles/r05_gemm_timeline.txt).  So the tile of a solo fit's launch is ONE MFMA tile, 16 rows x 16 columns, on 4 x N / 16
// workgroups (128 for a [50 x 512] product instead of 32): 64 KB and 3.1 us per workgroup.  K fits in lockstep fill the chip anyway
// and pay for bytes instead: their merged launch takes 64 x 16 or 64 x 32 tiles (5 / 3 MB of panel reads per product instead of 8).
// Geometry (MT x NT MFMA tiles per workgroup) is picked per launch (rows_geo) and NEVER changes a result:
// WAVE w takes the 64-k tiles w, w + 8, ... and computes each tile's partial product P_t from zero -- per 32-k step MT A and NT B
// fragments, hi and lo, every byte of the workgroup's panels loaded by exactly one wave.  The partials meet in LDS and are added
// in TILE ORDER -- C = ((P_0 + P_1) + P_2) + ... -- which is the DEFINITION of this kernel's K sum: one value per product however
// many waves, workgroups or fits share the launch, whatever the tile.
typedef __attribute__((ext_vector_type(4))) short s16x4;
typedef __attribute__((ext_vector_type(8))) short s16x8;
typedef __attribute__((address_space(3))) void* lds_vp;
typedef __attribute__((address_space(1))) const void* glb_vp;

// ---- m-major operands (the data gradient's W [k][n], both operands of a weight gradient): a wave stages ITS 64-k x 16-row
// image [64 k][16 rows] of a plane (2 KiB, 32-byte rows) by LDS-DMA and reads MFMA fragments with the transposing LDS read.  The
// image is private to the wave, so the only ordering needed is the wave's own s_waitcnt vmcnt (no barrier).
constexpr int RT_IMG = 64 * 16;               // elements of one image
__device__ __forceinline__ void rows_dma_image(const unsigned short* __restrict__ plane, long ld, int k0, int r0, unsigned short* img, int lane) {
    // two instructions of 64 lanes x 16 B: lane -> k-row 32 q + lane / 2, half lane % 2; the destination is wave-uniform base + lane x 16
#pragma unroll
    for (int q = 0; q < 2; ++q) {
        const unsigned short* src = plane + (long)(k0 + 32 * q + (lane >> 1)) * ld + r0 + 8 * (lane & 1);
        __builtin_amdgcn_global_load_lds((glb_vp)src, (lds_vp)(img + q * 512), 16, 0, 0);
    }
}
// fragment of rows 0 .. 15 of the image, k in [32 kk, 32 kk + 32): lane (i = l & 15) addresses k-row kb + i / 4, rows 4 (i % 4) .. + 3
// of a 4 (k) x 16 (row) block and receives the 4 k-values of row i (ds_read_b64_tr_b16)
__device__ __forceinline__ bf16x8 rows_tr_frag(const unsigned short* img, int kk, int lane) {
    const int i = lane & 15, kb = kk * 32 + ((lane >> 4) << 3) + (i >> 2);
    const unsigned short* p0 = img + kb * 16 + ((i & 3) << 2);
    typedef __attribute__((address_space(3))) s16x4* lds_p;
    const s16x4 v0 = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_p)(p0));
    const s16x4 v1 = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_p)(p0 + 4 * 16));
    const s16x8 v = {v0[0], v0[1], v0[2], v0[3], v1[0], v1[1], v1[2], v1[3]};
    return __builtin_bit_cast(bf16x8, v);
}

// ---- the WEIGHT operand of a product arrives as fp32 (row stride ldb) and is split in registers: hi = bf16(x) rounded to nearest,
// lo = bf16(x - hi) -- exactly split_bf16, i.e. the bits a plane of the weight would hold -- so the optimizer kernels need not keep
// bf16 planes of the decoder's weights (20 instead of 24 B per parameter and step for 58 % of the cfg2 parameters: a 15-fit lockstep
// step's sgd_kernel 1.87 -> 1.57 ms).  Same bytes per fragment as hi + lo planes (8 x 4 B).
template <int NSPLIT>
__device__ __forceinline__ void rows_split8(const float (&x)[8], bf16x8& hi, bf16x8& lo) {
#pragma unroll
    for (int e = 0; e < 8; ++e) {
        const __bf16 h = (__bf16)x[e];
        hi[e] = h;
        if (NSPLIT == 3) lo[e] = (__bf16)(x[e] - (float)h);
    }
}
// k-major weight rows ([n][k], the forward products): the lane's 8 consecutive k of its row, two 16-byte loads
__device__ __forceinline__ void rows_load8(const float* __restrict__ p, float (&x)[8]) {
    const float4 a = *reinterpret_cast<const float4*>(p), b = *reinterpret_cast<const float4*>(p + 4);
    x[0] = a.x; x[1] = a.y; x[2] = a.z; x[3] = a.w; x[4] = b.x; x[5] = b.y; x[6] = b.z; x[7] = b.w;
}
// m-major weight ([k][n], the data gradients): a wave-private fp32 image [64 k][16 n] (4 KiB) filled by four LDS-DMA instructions
// (lane -> k-row 16 q + lane / 4, 16-byte piece lane % 4; a piece never starts past column N - 4) ...
constexpr int RT_FIMG = 64 * 16;              // floats of one fp32 image
__device__ __forceinline__ void rows_dma_image_f32(const float* __restrict__ W, long ld, int k0, int c0, int N, float* img, int lane) {
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const int c = min(c0 + 4 * (lane & 3), N - 4);
        const float* src = W + (long)(k0 + 16 * q + (lane >> 2)) * ld + c;
        __builtin_amdgcn_global_load_lds((glb_vp)src, (lds_vp)(img + q * 256), 16, 0, 0);
    }
}
// ... and read back transposed: lane (column l & 15, k-octet l >> 4) takes its 8 k-values with 8 ds_read_b32
__device__ __forceinline__ void rows_img_col8(const float* img, int kk, int lane, float (&x)[8]) {
    const float* p = img + (kk * 32 + ((lane >> 4) << 3)) * 16 + (lane & 15);
#pragma unroll
    for (int e = 0; e < 8; ++e) x[e] = p[e * 16];
}

// rows_tile's epilogue of one MFMA tile (accumulator layout: the lane holds rows gm0 .. gm0 + 3 of column gn) as two functions, for
// gemm_rows_ln_body: what it reads is requested early (rows_epilogue_loads, by the lanes whose rows and column exist) and used
// behind the K sum (rows_epilogue).  rows_tile keeps its own text of the same statements: called from there, these functions
// move the instruction streams of every kernel above, which are held fixed (tools/diff_kernel_isa.py).
struct RowsEpi {
    float bias = 0.f, gt[4] = {0.f, 0.f, 0.f, 0.f}, rs[4] = {0.f, 0.f, 0.f, 0.f};
    DropKey dkey = {};
};
__device__ __forceinline__ void rows_epilogue_loads(const slnlp_gemm_args& g, int gm0, int gn, RowsEpi& e) {
    if (g.bias) e.bias = g.bias[gn];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int gm = gm0 + r < g.M ? gm0 + r : gm0;
        if (g.gate) e.gt[r] = g.gate[(long)gm * g.ldg + gn];
        if (g.resid) e.rs[r] = g.resid[(long)gm * g.ldr + gn];
    }
    if (g.drop_p > 0.f) e.dkey = dropout_key(g.rng, g.drop_site);
}
__device__ __forceinline__ void rows_epilogue(const RowsParams& p, const f32x4& acc, int gm0, int gn, const RowsEpi& e) {
    const slnlp_gemm_args& g = p.a;
    const int M = g.M, N = g.N;
    unsigned lot[4] = {0u, 0u, 0u, 0u};
    if (g.drop_p > 0.f) {
        if (g.drop_head_dim == 0) {
            const uint4 bits = dropout_bits8(e.dkey, (unsigned)gm0 >> 2, drop_cc((unsigned)gn));
            const int h = drop_half((unsigned)gn);
#pragma unroll
            for (int r = 0; r < 4; ++r) lot[r] = pick_lot(bits, h, r);
        } else {                                  // one keep / drop decision per (row, head), see slnlp.h
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const unsigned rh = (unsigned)(gm0 + r) * (unsigned)(N / g.drop_head_dim) + (unsigned)(gn / g.drop_head_dim);
                lot[r] = pick_lot(dropout_bits8(e.dkey, rh >> 2, 0u), 0, (int)(rh & 3u));
            }
        }
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int gm = gm0 + r;
        if (gm >= M) break;
        float v = acc[r] + e.bias;
        if (g.relu == 1) v = fmaxf(v, 0.f);
        else if (g.relu == 2) v = tanhf(v);
        if (g.gate) v = g.gate_mode == 1 ? v * (1.f - e.gt[r] * e.gt[r]) : (e.gt[r] > 0.f ? v * g.gate_scale : 0.f);
        if (g.drop_p > 0.f) v = (lot[r] >= p.drop_thr) ? v * p.drop_scale : 0.f;
        if (g.resid) v += e.rs[r];
        if (g.C) g.C[(long)gm * g.ldc + gn] = v;
        if (g.C_hi) {
            unsigned short h, l;
            split_bf16(v, h, l);
            g.C_hi[(long)gm * g.ldc_p + gn] = h;
            if (g.C_lo) g.C_lo[(long)gm * g.ldc_p + gn] = l;
        }
    }
}

// One product unit: output tile (bx, by) of 16 MT rows x 16 NT columns.  BK: the B operand is k-major (forward products: fragments
// straight from the plane) or m-major (data gradients: the wave's image through LDS, above).  smem: [partials][wave images].
template <int NSPLIT, int MT, int NT, bool BK>
__device__ __forceinline__ void rows_tile(const RowsParams& p, int bx, int by, float* part) {
    static_assert(MT * NT <= RT_WAVES, "one epilogue tile per wave");
    const slnlp_gemm_args& g = p.a;
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
#if SLNLP_PROBE_FENCES == 256
    unsigned long long rts[RTS_W] = {0, 0, 0, 0, 0, 0};
    struct RtsFlush {
        unsigned long long* t;
        __device__ ~RtsFlush() {
            if (threadIdx.x == 0) {
                t[4] = __builtin_amdgcn_s_memrealtime();
                t[5] = ((unsigned long long)(gridDim.x * gridDim.y) << 32) | (unsigned)(blockIdx.y * gridDim.x + blockIdx.x);
                const unsigned i = atomicAdd(&g_rts_n, 1u) & (unsigned)(RTS_MAX - 1);
                for (int k = 0; k < RTS_W; ++k) g_rts[i][k] = t[k];
            }
        }
    } rts_flush{rts};
    RTS_MARK(0);
#endif
    const int bn0 = bx * 16 * NT, bm0 = by * 16 * MT;
    const int M = g.M, N = g.N;
    const int ktiles = (g.K + 63) >> 6;
    // this lane's fragment rows and its k-octet inside a 32-k step.  The planes are zero-padded to multiples of 64 rows and weight
    // planes are followed by more of the arena; a tile that starts past the last row block re-reads the last valid tile instead
    // (its products belong to rows >= M / columns >= N, which nothing stores)
    const int am_last = ((M + 15) / 16 - 1) * 16, bn_last = ((N + 15) / 16 - 1) * 16;
    const long koct = 8 * (lane >> 4);
    const unsigned short *ah[MT], *al[MT];
    const float* bw[NT];                                   // k-major weight: this lane's row of column tile j, at its k-octet
    int bcol[NT];
#pragma unroll
    for (int i = 0; i < MT; ++i) {
        const long off = (long)(min(bm0 + 16 * i, am_last) + (lane & 15)) * g.lda_p + koct;
        ah[i] = g.A_hi + off; al[i] = g.A_lo + off;
    }
#pragma unroll
    for (int j = 0; j < NT; ++j) {
        bcol[j] = min(bn0 + 16 * j, bn_last);
        bw[j] = g.B + (long)min(bcol[j] + (lane & 15), N - 1) * g.ldb + koct;      // (a row past N is a repeat of row N - 1: never stored)
    }
    // (m-major B: this wave's fp32 images, behind the partial tiles: [NT column tiles][64 k][16 n])
    float* bimg = part + (size_t)ktiles * MT * NT * 256 + wave * NT * RT_FIMG;

    // what the epilogue will want: wave w < MT * NT runs it for MFMA tile (w / NT, w % NT); the lane holds rows gm0 .. gm0 + 3 of column gn
    const int ei = wave / NT, ej = wave % NT;
    const int gm0 = bm0 + 16 * ei + ((lane >> 4) << 2), gn = bn0 + 16 * ej + (lane & 15);
    const bool live = wave < MT * NT && gn < N && gm0 < M;
    float bias = 0.f, gt[4] = {0.f, 0.f, 0.f, 0.f}, rs[4] = {0.f, 0.f, 0.f, 0.f};
    DropKey dkey = {};
    auto epilogue_loads = [&]() {
        if (!live) return;
        if (g.bias) bias = g.bias[gn];
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int gm = gm0 + r < M ? gm0 + r : gm0;
            if (g.gate) gt[r] = g.gate[(long)gm * g.ldg + gn];
            if (g.resid) rs[r] = g.resid[(long)gm * g.ldr + gn];
        }
        if (g.drop_p > 0.f) dkey = dropout_key(g.rng, g.drop_site);
    };

    for (int t = wave; t < ktiles; t += RT_WAVES) {
        bf16x8 fa[2][MT], la[2][MT], fb[2][NT], lb[2][NT];
        if (!BK) {
            if (t != wave) asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");      // (the images' last fragment reads: LDS operations of a wave retire in order)
#pragma unroll
            for (int j = 0; j < NT; ++j) rows_dma_image_f32(g.B, g.ldb, t * 64, bcol[j], N, bimg + j * RT_FIMG, lane);
        }
#pragma unroll
        for (int kk = 0; kk < 2; ++kk) {
            const int k = t * 64 + kk * 32;
            if (BK) {
#pragma unroll
                for (int j = 0; j < NT; ++j) {
                    float x[8];
                    rows_load8(bw[j] + k, x);
                    rows_split8<NSPLIT>(x, fb[kk][j], lb[kk][j]);
                }
            }
#pragma unroll
            for (int i = 0; i < MT; ++i) {
                fa[kk][i] = *reinterpret_cast<const bf16x8*>(ah[i] + k);
                if (NSPLIT == 3) la[kk][i] = *reinterpret_cast<const bf16x8*>(al[i] + k);
            }
        }
        // (requested behind the first tile's operands, in front of its MFMAs: vector-memory operations retire in order, so a slow
        //  residual line in FRONT of the operands would hold the first MFMA's counted wait -- 0.4 us on gemm.hip's 16-wide tile)
        if (t == wave) epilogue_loads();
        if (!BK) {
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");         // this wave's images have landed
#pragma unroll
            for (int kk = 0; kk < 2; ++kk)
#pragma unroll
                for (int j = 0; j < NT; ++j) {
                    float x[8];
                    rows_img_col8(bimg + j * RT_FIMG, kk, lane, x);
                    rows_split8<NSPLIT>(x, fb[kk][j], lb[kk][j]);
                }
        }
#if SLNLP_PROBE_FENCES == 256
        if (t == 0) { asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); RTS_MARK(1); }
#endif
        f32x4 acc[MT][NT];
#pragma unroll
        for (int i = 0; i < MT; ++i)
#pragma unroll
            for (int j = 0; j < NT; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int kk = 0; kk < 2; ++kk)
#pragma unroll
            for (int i = 0; i < MT; ++i)
#pragma unroll
                for (int j = 0; j < NT; ++j) {
                    if (NSPLIT == 3) {
                        acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(la[kk][i], fb[kk][j], acc[i][j], 0, 0, 0);
                        acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fa[kk][i], lb[kk][j], acc[i][j], 0, 0, 0);
                    }
                    acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fa[kk][i], fb[kk][j], acc[i][j], 0, 0, 0);
                }
#pragma unroll
        for (int i = 0; i < MT; ++i)
#pragma unroll
            for (int j = 0; j < NT; ++j) *reinterpret_cast<f32x4*>(part + (((t * MT + i) * NT + j) * 64 + lane) * 4) = acc[i][j];
    }
    if (wave >= ktiles) epilogue_loads();          // (a wave without a K tile still owes its epilogue requests)
    RTS_MARK(2);
    __syncthreads();
    if (wave >= MT * NT) return;
    // the K sum of this wave's MFMA tile, in tile order
    f32x4 acc = *reinterpret_cast<const f32x4*>(part + (wave * 64 + lane) * 4);
    for (int t = 1; t < ktiles; ++t) acc += *reinterpret_cast<const f32x4*>(part + ((t * MT * NT + wave) * 64 + lane) * 4);
    RTS_MARK(3);
    if (!live) return;

    // ---- epilogue in the accumulator layout
    unsigned lot[4] = {0u, 0u, 0u, 0u};
    if (g.drop_p > 0.f) {
        if (g.drop_head_dim == 0) {
            const uint4 bits = dropout_bits8(dkey, (unsigned)gm0 >> 2, drop_cc((unsigned)gn));
            const int h = drop_half((unsigned)gn);
#pragma unroll
            for (int r = 0; r < 4; ++r) lot[r] = pick_lot(bits, h, r);
        } else {                                  // one keep / drop decision per (row, head), see slnlp.h
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const unsigned rh = (unsigned)(gm0 + r) * (unsigned)(N / g.drop_head_dim) + (unsigned)(gn / g.drop_head_dim);
                lot[r] = pick_lot(dropout_bits8(dkey, rh >> 2, 0u), 0, (int)(rh & 3u));
            }
        }
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int gm = gm0 + r;
        if (gm >= M) break;
        float v = acc[r] + bias;
        if (g.relu == 1) v = fmaxf(v, 0.f);
        else if (g.relu == 2) v = tanhf(v);
        if (g.gate) v = g.gate_mode == 1 ? v * (1.f - gt[r] * gt[r]) : (gt[r] > 0.f ? v * g.gate_scale : 0.f);
        if (g.drop_p > 0.f) v = (lot[r] >= p.drop_thr) ? v * p.drop_scale : 0.f;
        if (g.resid) v += rs[r];
        if (g.C) g.C[(long)gm * g.ldc + gn] = v;
        if (g.C_hi) {
            unsigned short h, l;
            split_bf16(v, h, l);
            g.C_hi[(long)gm * g.ldc_p + gn] = h;
            if (g.C_lo) g.C_lo[(long)gm * g.ldc_p + gn] = l;
        }
    }
}

// One weight-gradient unit: dW[16 WM m x 128 n] = dY^T x over the batch rows -- A = dY planes [k = row][m], B = x planes [k = row][n],
// both m-major; WAVE w computes the WM 16 x 16 tiles of columns n0 + 16 w.  The WM dY images are staged ONCE per workgroup (the waves
// share the DMA instructions; one barrier), each wave stages its own x image.  K = the batch rows (one 64-k tile at the headline
// batch of 50; more tiles: partials added in tile order, as everywhere in this file).  rowsum_a (the bias gradient: sum over the rows
// of dY[., m]) is the same dY fragments times an all-ones fragment, by the first column unit's wave 0.  WM = 1 for a solo fit's launch (128 units of
// 36 KB for a 512 x 512 gradient), 4 for merged lockstep launches (a quarter of the x-image reads).
template <int NSPLIT, int WM>
__device__ __forceinline__ void rows_wgrad_unit(const slnlp_gemm_args& g, int unit, unsigned short* smem) {
    constexpr int NP = NSPLIT == 3 ? 2 : 1;
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int M = g.M, N = g.N, ktiles = (g.K + 63) >> 6;
    const int units_n = (N + 127) / 128, um = unit / units_n, un = unit - um * units_n;
    const int m0 = um * 16 * WM, n0 = un * 128 + wave * 16, m_last = ((M + 15) / 16 - 1) * 16;
    const bool active = n0 < N;                          // (a wave past the last column tile only keeps the barriers company)
    unsigned short* aimg = smem;                          // [WM][hi, lo][64 k][16 m]: the workgroup's
    unsigned short* bimg = smem + WM * 2 * RT_IMG + wave * 2 * RT_IMG;   // [hi, lo][64 k][16 n]: this wave's
    f32x4 total[WM], rsum[WM];
#pragma unroll
    for (int i = 0; i < WM; ++i) { total[i] = f32x4{0.f, 0.f, 0.f, 0.f}; rsum[i] = f32x4{0.f, 0.f, 0.f, 0.f}; }
    // the bias gradient is one more product of the same dY fragments: dY^T 1 (an all-ones B fragment, exact in bf16), hi and lo -- two
    // MFMAs per fragment instead of a lane-serial walk over the image (16 lanes x 64 k x WM dependent LDS reads: 17 us of a 20 us unit
    // at batch 256, r05 timeline).  Every column of the result tile holds the row sums; column 0's lanes store them.
    const bool do_rs = g.rowsum_a != nullptr && un == 0 && wave == 0;      // (wave-uniform)
    bf16x8 ones;
#pragma unroll
    for (int e = 0; e < 8; ++e) ones[e] = (__bf16)1.0f;
#if SLNLP_PROBE_FENCES == 256
    // (probe build: entry, first tile's images landed, first tile's MFMAs issued, K loop done, end; bit 31 of the block word = a weight-gradient unit,
    //  bit 30 = one that also sums the rows of dY)
    unsigned long long rts[RTS_W] = {0, 0, 0, 0, 0, 0};
    struct RtsFlushW {
        unsigned long long* t;
        unsigned tag;
        __device__ ~RtsFlushW() {
            if (threadIdx.x == 0) {
                t[4] = __builtin_amdgcn_s_memrealtime();
                t[5] = ((unsigned long long)(gridDim.x * gridDim.y) << 32) | tag | (unsigned)(blockIdx.y * gridDim.x + blockIdx.x);
                const unsigned i = atomicAdd(&g_rts_n, 1u) & (unsigned)(RTS_MAX - 1);
                for (int k = 0; k < RTS_W; ++k) g_rts[i][k] = t[k];
            }
        }
    } rts_flush{rts, 0x80000000u | (g.rowsum_a != nullptr && un == 0 ? 0x40000000u : 0u)};
    RTS_MARK(0);
#endif
    for (int t = 0; t < ktiles; ++t) {
        if (t) {                                          // every wave is done with the previous tile's images
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
            __syncthreads();
        }
        for (int im = wave; im < WM * NP; im += RT_WAVES) {
            const int i = im / NP, pl = im - i * NP;
            rows_dma_image(pl ? g.A_lo : g.A_hi, g.lda_p, t * 64, min(m0 + 16 * i, m_last), aimg + (2 * i + pl) * RT_IMG, lane);
        }
        if (active) {
            rows_dma_image(g.B_hi, g.ldb_p, t * 64, n0, bimg, lane);
            if (NSPLIT == 3) rows_dma_image(g.B_lo, g.ldb_p, t * 64, n0, bimg + RT_IMG, lane);
        }
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();
#if SLNLP_PROBE_FENCES == 256
        if (t == 0) RTS_MARK(1);
#endif
        if (active) {
            bf16x8 fb[2], lb[2];
#pragma unroll
            for (int kk = 0; kk < 2; ++kk) {
                fb[kk] = rows_tr_frag(bimg, kk, lane);
                if (NSPLIT == 3) lb[kk] = rows_tr_frag(bimg + RT_IMG, kk, lane);
            }
#pragma unroll
            for (int i = 0; i < WM; ++i) {
                f32x4 acc = f32x4{0.f, 0.f, 0.f, 0.f}, rs = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
                for (int kk = 0; kk < 2; ++kk) {
                    const bf16x8 fa = rows_tr_frag(aimg + (2 * i) * RT_IMG, kk, lane);
                    if (NSPLIT == 3) {
                        const bf16x8 la = rows_tr_frag(aimg + (2 * i + 1) * RT_IMG, kk, lane);
                        acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(la, fb[kk], acc, 0, 0, 0);
                        acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fa, lb[kk], acc, 0, 0, 0);
                        if (do_rs) rs = __builtin_amdgcn_mfma_f32_16x16x32_bf16(la, ones, rs, 0, 0, 0);
                    }
                    acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fa, fb[kk], acc, 0, 0, 0);
                    if (do_rs) rs = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fa, ones, rs, 0, 0, 0);
                }
                total[i] = t == 0 ? acc : total[i] + acc;
                if (do_rs) rsum[i] = t == 0 ? rs : rsum[i] + rs;
            }
        }
#if SLNLP_PROBE_FENCES == 256
        if (t == 0) RTS_MARK(2);
#endif
    }
    RTS_MARK(3);
    if (!active) return;
    const int gn = n0 + (lane & 15);
#pragma unroll
    for (int i = 0; i < WM; ++i) {
        const int gm0 = m0 + 16 * i + ((lane >> 4) << 2);
        if (gn < N) {
#pragma unroll
            for (int r = 0; r < 4; ++r)
                if (gm0 + r < M) g.C[(long)(gm0 + r) * g.ldc + gn] = total[i][r];
        }
        if (do_rs && (lane & 15) == 0) {
#pragma unroll
            for (int r = 0; r < 4; ++r)
                if (gm0 + r < M) g.rowsum_a[gm0 + r] = rsum[i][r];
        }
    }
}

template <int NSPLIT, int MT, int NT>
__device__ __forceinline__ void gemm_rows_body(RowsParams p) {
    extern __shared__ __attribute__((aligned(16))) float part[];      // [ktiles][MT x NT tiles][64 lanes][4]
    rows_tile<NSPLIT, MT, NT, true>(p, blockIdx.x, blockIdx.y, part);
}

// ---- The forward product whose operand is the output of a LayerNorm that has not run yet (the decoder's norm1 / norm2 / norm3 and
// final norm each feed exactly one B-row product on the chain: 4.6 us of launch for 13 workgroups of work).  A kernel of its own for
// the 16 x 16 tile of a solo fit's launch -- the kernels above, which merged lockstep launches also take, keep their registers.
// The workgroup takes UN-NORMALISED fp32 rows where rows_tile takes planes: wave w normalises rows 2 w and 2 w + 1 of its 16 with
// layernorm_row -- the stand-alone kernel's lane-to-column mapping and reductions, hence its bits -- splits them (split_bf16: the
// bits LayerNorm's plane output holds) into an LDS image, and after one barrier every wave reads the A fragments of its K tiles
// from that image; weight fragments, MFMA order, K sum and epilogue are rows_tile's.  The weight fragments of the wave's first
// tile and the epilogue's operands are requested in front of the arithmetic: one memory round trip covers all of them.
// The workgroups of column tile 0 also store what the LayerNorm launch stored (y, its planes, (mean, rstd); rows < M only), as
// each wave's last instructions.  Measured at the bench shape: 7.4 us per launch against 6.0 + 3.9 for the two it replaces.
struct RowsLnParams {
    RowsParams r;
    RowsLn ln;
};
__device__ __forceinline__ RowsLnParams as_global(RowsLnParams p) {
    launder(p.r.a);
    p.ln.x = as_global(p.ln.x); p.ln.gamma = as_global(p.ln.gamma); p.ln.beta = as_global(p.ln.beta);
    p.ln.y = as_global(p.ln.y); p.ln.stats = as_global(p.ln.stats); p.ln.y_hi = as_global(p.ln.y_hi); p.ln.y_lo = as_global(p.ln.y_lo);
    return p;
}
// The image: [16 rows][K] bf16 per plane, rows unpadded, the 16-byte slots of a row XOR-ed with the row number.  A fragment read
// is ds_read_b128 by lane (row l & 15, k-octet l >> 4): banks (a / 4) % 64, i.e. 16 slots per 256 bytes, and each of its 16-lane
// groups holds 8 rows at one octet and the other 8 at the next ({0-3, 12-15, 20-27}, ...).  Unswizzled, a 1024-byte row puts
// all 16 rows on one slot; no padding separates them all (rows r, r' at octets o, o + 1 meet whenever (r' - r) stride = 1 in
// slots mod 16, and every difference occurs); slot ^ row maps a group onto 16 different slots.  (K not a multiple of 128: rows
// of 8 n slots, XOR with 3 bits of the row, 2-way.)  Returns the element offset of columns c .. c + 7, c a multiple of 8.
__device__ __forceinline__ int rows_ln_off(int r, int c, int K) { return r * K + (((c >> 3) ^ (r & ((K & 127) ? 7 : 15))) << 3); }

template <int NSPLIT>
__device__ __forceinline__ void gemm_rows_ln_body(RowsLnParams p) {
    extern __shared__ __attribute__((aligned(16))) float part[];      // [ktiles][64 lanes][4] | the image [hi, lo][16 rows][K]
    const slnlp_gemm_args& g = p.r.a;
    const RowsLn& n = p.ln;
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int bx = blockIdx.x, bn0 = bx * 16, bm0 = blockIdx.y * 16;
    const int M = g.M, N = g.N, K = g.K, ktiles = K >> 6;
    unsigned short* img = reinterpret_cast<unsigned short*>(part + ktiles * 256);
    const int koct = 8 * (lane >> 4);

    // requests first, every one of them, then one wait: this wave's two rows, gamma and beta ...  No lane-dependent control
    // flow around a load and nothing that reads a loaded value between them: a slot past K reads the row's last float4 and a
    // row past M repeats row M - 1 (zeros are selected in below; such a row is normalised like any other and never stored).
    const int r0 = bm0 + 2 * wave;
    const float4 zero4 = make_float4(0.f, 0.f, 0.f, 0.f);
    float4 v[2][LN_MAXU], ga[LN_MAXU], bt[LN_MAXU];
#pragma unroll
    for (int u = 0; u < LN_MAXU; ++u) {
        v[0][u] = v[1][u] = ga[u] = bt[u] = zero4;
        if (u * 256 < K) {                                   // (wave-uniform)
            const int cl = min(lane * 4 + u * 256, K - 4);
#pragma unroll
            for (int i = 0; i < 2; ++i) v[i][u] = *reinterpret_cast<const float4*>(n.x + (long)min(r0 + i, M - 1) * n.ldx + cl);
            ga[u] = *reinterpret_cast<const float4*>(n.gamma + cl);
            bt[u] = *reinterpret_cast<const float4*>(n.beta + cl);
        }
    }
    // ... the weight fragments of its first K tile (a row past N is a repeat of row N - 1: never stored; a wave without a tile
    // repeats the last one's) ...
    const float* bw = g.B + (long)min(bn0 + (lane & 15), N - 1) * g.ldb + koct;
    float xb[2][8];
#pragma unroll
    for (int kk = 0; kk < 2; ++kk) rows_load8(bw + min(wave, ktiles - 1) * 64 + kk * 32, xb[kk]);
    // ... and what the epilogue wants (wave 0 runs it: the lane holds rows gm0 .. gm0 + 3 of column gn)
    const int gm0 = bm0 + ((lane >> 4) << 2), gn = bn0 + (lane & 15);
    const bool live = wave == 0 && gn < N && gm0 < M;
    RowsEpi epi;
    if (live) rows_epilogue_loads(g, gm0, gn, epi);

    // everything has been requested: zeros into the slots past K, and the first tile's weight fragments split
#pragma unroll
    for (int u = 0; u < LN_MAXU; ++u)
        if (lane * 4 + u * 256 >= K) v[0][u] = v[1][u] = ga[u] = bt[u] = zero4;
    bf16x8 fb0[2], lb0[2];
#pragma unroll
    for (int kk = 0; kk < 2; ++kk) rows_split8<NSPLIT>(xb[kk], fb0[kk], lb0[kk]);

    // the prologue: rows 2 w, 2 w + 1 -> the image.  What column tile 0 owes memory (y, its planes, the statistics) stays in
    // registers until the wave's last instruction: a store in front of a counted wait is waited for with the loads
    float4 on[2][LN_MAXU];
    float mean[2], rstd[2];
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        const int rl = 2 * wave + i;
        layernorm_row(v[i], ga, bt, K, n.eps, lane, mean[i], rstd[i], [&](int u, int c, const float4& o) {
            unsigned short h[4], l[4];
            split_bf16(o.x, h[0], l[0]); split_bf16(o.y, h[1], l[1]); split_bf16(o.z, h[2], l[2]); split_bf16(o.w, h[3], l[3]);
            const int off = rows_ln_off(rl, c & ~7, K) + (c & 4);
            *reinterpret_cast<uint2*>(img + off) = make_uint2(h[0] | ((unsigned)h[1] << 16), h[2] | ((unsigned)h[3] << 16));
            if (NSPLIT == 3) *reinterpret_cast<uint2*>(img + 16 * K + off) = make_uint2(l[0] | ((unsigned)l[1] << 16), l[2] | ((unsigned)l[3] << 16));
            on[i][u] = o;
        });
    }
    auto store_rows = [&]() {
        if (bx != 0) return;
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            const int row = r0 + i;
            if (row >= M) break;
#pragma unroll
            for (int u = 0; u < LN_MAXU; ++u) {
                const int c = lane * 4 + u * 256;
                if (c < K) {
                    *reinterpret_cast<float4*>(n.y + (long)row * K + c) = on[i][u];
                    store_planes4(PlaneOut{n.y_hi, n.y_lo, nullptr}, (long)row * n.ldp + c, on[i][u]);
                }
            }
            if (lane == 0 && n.stats) {
                n.stats[2 * row] = mean[i];
                n.stats[2 * row + 1] = rstd[i];
            }
        }
    };
    __syncthreads();

    for (int t = wave; t < ktiles; t += RT_WAVES) {
        bf16x8 fa[2], la[2], fb[2], lb[2];
#pragma unroll
        for (int kk = 0; kk < 2; ++kk) {
            const int k = t * 64 + kk * 32;
            if (t != wave) {
                rows_load8(bw + k, xb[kk]);
                rows_split8<NSPLIT>(xb[kk], fb[kk], lb[kk]);
            } else {
                fb[kk] = fb0[kk];
                if (NSPLIT == 3) lb[kk] = lb0[kk];
            }
            const int off = rows_ln_off(lane & 15, k + koct, K);
            fa[kk] = *reinterpret_cast<const bf16x8*>(img + off);
            if (NSPLIT == 3) la[kk] = *reinterpret_cast<const bf16x8*>(img + 16 * K + off);
        }
        f32x4 acc = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int kk = 0; kk < 2; ++kk) {                      // (rows_tile's order)
            if (NSPLIT == 3) {
                acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(la[kk], fb[kk], acc, 0, 0, 0);
                acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fa[kk], lb[kk], acc, 0, 0, 0);
            }
            acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fa[kk], fb[kk], acc, 0, 0, 0);
        }
        *reinterpret_cast<f32x4*>(part + (t * 64 + lane) * 4) = acc;
    }
    __syncthreads();
    if (wave == 0) {
        // the K sum in tile order, then the epilogue
        f32x4 acc = *reinterpret_cast<const f32x4*>(part + lane * 4);
        for (int t = 1; t < ktiles; ++t) acc += *reinterpret_cast<const f32x4*>(part + (t * 64 + lane) * 4);
        if (live) rows_epilogue(p.r, acc, gm0, gn, epi);
    }
    store_rows();
}
__device__ __forceinline__ void gemm_rows_ln_body_3(RowsLnParams p) { gemm_rows_ln_body<3>(p); }
__device__ __forceinline__ void gemm_rows_ln_body_1(RowsLnParams p) { gemm_rows_ln_body<1>(p); }
SLNLP_ZKERNEL(gemm_rows_ln_kernel_3, RT_THREADS, gemm_rows_ln_body_3)
SLNLP_ZKERNEL(gemm_rows_ln_kernel_1, RT_THREADS, gemm_rows_ln_body_1)

// The backward pair of one dY in ONE launch: blocks [0, nd) are the data gradient's tiles (dX = dY W, W m-major), the rest the weight
// gradient's units (dW = dY^T x, db = column sums of dY).  Both read the same dY planes.
struct RowsBwdParams {
    RowsParams d;
    slnlp_gemm_args w;
};
__device__ __forceinline__ RowsBwdParams as_global(RowsBwdParams p) {
    launder(p.d.a);
    launder(p.w);
    return p;
}
template <int NSPLIT, int MT, int NT>
__device__ __forceinline__ void gemm_rows_bwd_body(RowsBwdParams p) {
    extern __shared__ __attribute__((aligned(16))) float part[];
    const int gx = (p.d.a.N + 16 * NT - 1) / (16 * NT), gy = (p.d.a.M + 16 * MT - 1) / (16 * MT), nd = gx * gy;
    const int id = blockIdx.x;
    if (id < nd) rows_tile<NSPLIT, MT, NT, false>(p.d, id % gx, id / gx, part);
    else rows_wgrad_unit<NSPLIT, MT>(p.w, id - nd, reinterpret_cast<unsigned short*>(part));      // (16 MT gradient rows per unit)
}

// geometries: MFMA tiles per workgroup
struct RowsGeo { int mt, nt; };
constexpr int RT_NGEO = 3;
constexpr RowsGeo RT_GEO[RT_NGEO] = {{1, 1}, {4, 1}, {4, 2}};
#define SLNLP_ROWS_KERNEL(NS, G)                                                                                          \
    __device__ __forceinline__ void gemm_rows_body_##NS##_##G(RowsParams p) { gemm_rows_body<NS, RT_GEO[G].mt, RT_GEO[G].nt>(p); } \
    SLNLP_ZKERNEL(gemm_rows_kernel_##NS##_##G, RT_THREADS, gemm_rows_body_##NS##_##G)                                     \
    __device__ __forceinline__ void gemm_rows_bwd_body_##NS##_##G(RowsBwdParams p) { gemm_rows_bwd_body<NS, RT_GEO[G].mt, RT_GEO[G].nt>(p); } \
    SLNLP_ZKERNEL(gemm_rows_bwd_kernel_##NS##_##G, RT_THREADS, gemm_rows_bwd_body_##NS##_##G)
SLNLP_ROWS_KERNEL(3, 0)
SLNLP_ROWS_KERNEL(3, 1)
SLNLP_ROWS_KERNEL(3, 2)
SLNLP_ROWS_KERNEL(1, 0)
SLNLP_ROWS_KERNEL(1, 1)
SLNLP_ROWS_KERNEL(1, 2)

using RowsKernel = void (*)(Pack<RowsParams>, const Pack<RowsParams>*);
using RowsBwdKernel = void (*)(Pack<RowsBwdParams>, const Pack<RowsBwdParams>*);
static RowsKernel rows_kernel(int precision, int geo) {
    if (precision == 3) return geo == 0 ? gemm_rows_kernel_3_0 : geo == 1 ? gemm_rows_kernel_3_1 : gemm_rows_kernel_3_2;
    return geo == 0 ? gemm_rows_kernel_1_0 : geo == 1 ? gemm_rows_kernel_1_1 : gemm_rows_kernel_1_2;
}
static RowsBwdKernel rows_bwd_kernel(int precision, int geo) {
    if (precision == 3) return geo == 0 ? gemm_rows_bwd_kernel_3_0 : geo == 1 ? gemm_rows_bwd_kernel_3_1 : gemm_rows_bwd_kernel_3_2;
    return geo == 0 ? gemm_rows_bwd_kernel_1_0 : geo == 1 ? gemm_rows_bwd_kernel_1_1 : gemm_rows_bwd_kernel_1_2;
}
static size_t rows_lds(int geo, int K) { return (size_t)ceil_div(K, 64) * RT_GEO[geo].mt * RT_GEO[geo].nt * 64 * 4 * sizeof(float); }
// backward launches: the data gradient's partial tiles + its waves' W images, or the weight gradient's four images per wave
static size_t rows_bwd_lds(int geo, int K) {
    const size_t d = rows_lds(geo, K) + (size_t)RT_WAVES * RT_GEO[geo].nt * RT_FIMG * sizeof(float);
    const size_t w = (size_t)(RT_GEO[geo].mt + RT_WAVES) * 2 * RT_IMG * sizeof(unsigned short);      // the workgroup's dY images + the waves' x images
    return d > w ? d : w;
}
// the LayerNorm-prologue kernel: the partial tiles + the image of the 16 normalised rows, hi and lo (K = 512: 8 + 32 KiB; 1024: 16 + 64)
static size_t rows_ln_lds(int K) { return rows_lds(0, K) + (size_t)2 * 16 * K * sizeof(unsigned short); }
static dim3 rows_grid(int geo, int M, int N) { return dim3(ceil_div(N, 16 * RT_GEO[geo].nt), ceil_div(M, 16 * RT_GEO[geo].mt)); }
static int rows_wgrad_units(const slnlp_gemm_args& w, int geo) { return ceil_div(w.M, 16 * RT_GEO[geo].mt) * ceil_div(w.N, 128); }

// -1 = automatic; 0 .. RT_NGEO-1 forced (slnlp_set_rows_tile: tests, tuning)
static std::atomic<int> g_rows_geo{[] { const char* e = getenv("SLNLP_ROWS_TILE"); const int v = e ? atoi(e) : -1; return v >= 0 && v < RT_NGEO ? v : -1; }()};
// Which tile a launch of `fits` products [M x N x K] takes: rounds of workgroups over the 256 compute units x the panel bytes one
// workgroup loads (a compute unit's load rate is the limit, see gemm_rows_body) -- the small tile while the launch fits the chip
// about once (one fit: 128 workgroups of 64 KB), the wide ones when K fits in lockstep fill it many times over.
constexpr size_t RT_LDS_MAX = 160 * 1024;    // per workgroup (MI355X: 160 KiB per compute unit)
static int rows_geo(int M, int N, int K, int fits, bool bwd) {
    const int forced = g_rows_geo.load(std::memory_order_relaxed);
    auto fits_lds = [&](int geo) { return (bwd ? rows_bwd_lds(geo, K) : rows_lds(geo, K)) <= RT_LDS_MAX; };
    if (forced >= 0 && fits_lds(forced)) return forced;
    int best = 0;
    long best_cost = -1;
    for (int geo = 0; geo < RT_NGEO; ++geo) {
        if (!fits_lds(geo)) continue;
        const dim3 gr = rows_grid(geo, M, N);
        // (a backward launch also carries the weight gradient's units: dW [K x N] in pieces of 16 mt x 128)
        const long wunits = bwd ? (long)ceil_div(K, 16 * RT_GEO[geo].mt) * ceil_div(N, 128) : 0;
        const long units = ((long)gr.x * gr.y + wunits) * fits, rounds = (units + 255) / 256;
        const long cost = rounds * (16L * (RT_GEO[geo].mt + RT_GEO[geo].nt) * K * 4 + 16384);     // (+ a fixed cost per round)
        if (best_cost < 0 || cost < best_cost) { best_cost = cost; best = geo; }
    }
    return best;
}

static int rows_init() {
    static DeviceOnce once;
    return once.run([]() -> int {
        bool ok = true;
        for (int prec = 1; prec <= 3; prec += 2)
            for (int geo = 0; geo < RT_NGEO; ++geo)
                ok = ok && hipFuncSetAttribute((const void*)rows_kernel(prec, geo), hipFuncAttributeMaxDynamicSharedMemorySize,
                                               (int)std::min(rows_lds(geo, 64 * RT_MAX_KTILES), RT_LDS_MAX)) == hipSuccess &&
                     hipFuncSetAttribute((const void*)rows_bwd_kernel(prec, geo), hipFuncAttributeMaxDynamicSharedMemorySize,
                                         (int)std::min(rows_bwd_lds(geo, 64 * RT_MAX_KTILES), RT_LDS_MAX)) == hipSuccess;
        ok = ok && hipFuncSetAttribute((const void*)gemm_rows_ln_kernel_3, hipFuncAttributeMaxDynamicSharedMemorySize, (int)rows_ln_lds(64 * RT_MAX_KTILES)) == hipSuccess &&
             hipFuncSetAttribute((const void*)gemm_rows_ln_kernel_1, hipFuncAttributeMaxDynamicSharedMemorySize, (int)rows_ln_lds(64 * RT_MAX_KTILES)) == hipSuccess;
        if (!ok) {
            set_error("gemm_rows: cannot raise dynamic LDS limit: %s", hipGetErrorString(hipGetLastError()));
            return SLNLP_ERR_LAUNCH;
        }
        return 0;
    });
}

// A merged (lockstep) launch of K fits' recorded gemm_rows call sites picks its tile again for K products (lockstep.hip): returns the
// kernel to launch and its grid / LDS, or nullptr when `fn` is not a gemm_rows kernel.  Results do not depend on the tile.
const void* gemm_rows_for_fits(const void* fn, const void* recorded_args, int fits, dim3* grid, size_t* lds) {
    int prec = 0;
    bool bwd = false;
    for (int geo = 0; geo < RT_NGEO; ++geo) {
        if (fn == (const void*)rows_kernel(3, geo)) prec = 3;
        if (fn == (const void*)rows_kernel(1, geo)) prec = 1;
        if (fn == (const void*)rows_bwd_kernel(3, geo)) { prec = 3; bwd = true; }
        if (fn == (const void*)rows_bwd_kernel(1, geo)) { prec = 1; bwd = true; }
    }
    if (!prec) return nullptr;
    if (bwd) {
        const RowsBwdParams& P = *reinterpret_cast<const RowsBwdParams*>(recorded_args);
        const int geo = rows_geo(P.d.a.M, P.d.a.N, P.d.a.K, fits, true);
        const dim3 gr = rows_grid(geo, P.d.a.M, P.d.a.N);
        *grid = dim3(gr.x * gr.y + rows_wgrad_units(P.w, geo));
        *lds = rows_bwd_lds(geo, P.d.a.K);
        return (const void*)rows_bwd_kernel(prec, geo);
    }
    const slnlp_gemm_args& a = reinterpret_cast<const RowsParams*>(recorded_args)->a;
    const int geo = rows_geo(a.M, a.N, a.K, fits, false);
    *grid = rows_grid(geo, a.M, a.N);
    *lds = rows_lds(geo, a.K);
    return (const void*)rows_kernel(prec, geo);
}

static int check_rows_job(const slnlp_gemm_args& a, bool b_kmajor, const char* who) {
    SLNLP_CHECK_ARG(a.A_hi && a.B, "%s: A as bf16 planes (A_hi / A_lo / lda_p) and the weight B as fp32 (B / ldb) required", who);
    SLNLP_CHECK_ARG(a.a_kmajor && (a.b_kmajor != 0) == b_kmajor, "%s: operand layouts (A k-major; B k-major for a forward product, m-major for a data gradient)", who);
    SLNLP_CHECK_ARG(a.C || a.C_hi, "%s: no output", who);
    SLNLP_CHECK_ARG(a.M > 0 && a.N > 0 && a.K > 0, "%s: bad shape M=%d N=%d K=%d", who, a.M, a.N, a.K);
    SLNLP_CHECK_ARG(a.precision == 1 || (a.precision == 3 && a.A_lo), "%s: precision 1, or 3 with A's lo plane", who);
    SLNLP_CHECK_ARG(a.lda_p % 64 == 0 && a.lda_p >= a.K, "%s: A's plane row stride must be a multiple of 64 and cover K (zero-padded)", who);
    SLNLP_CHECK_ARG(a.K % 64 == 0 && a.ldb % 4 == 0 && a.ldb >= (b_kmajor ? a.K : a.N) && (b_kmajor || a.N % 4 == 0),
                    "%s: K must be a multiple of 64 (the fp32 weight has no padding), ldb a multiple of 4 that covers a row", who);
    SLNLP_CHECK_ARG((((uintptr_t)a.A_hi | (uintptr_t)a.A_lo | (uintptr_t)a.B) & 15) == 0, "%s: operands must be 16-byte aligned", who);
    SLNLP_CHECK_ARG(!a.C || a.ldc >= a.N, "%s: ldc < N", who);
    SLNLP_CHECK_ARG(!a.C_hi || a.ldc_p >= a.N, "%s: ldc_p < N", who);
    SLNLP_CHECK_ARG(a.drop_p >= 0.f && a.drop_p < 1.f && (a.drop_p == 0.f || a.rng), "%s: bad dropout args", who);
    SLNLP_CHECK_ARG(!a.gate || a.ldg >= a.N, "%s: ldg too small", who);
    SLNLP_CHECK_ARG(!a.resid || a.ldr >= a.N, "%s: ldr too small", who);
    SLNLP_CHECK_ARG(!a.rowsum_a && a.batch <= 1, "%s: no row sums, no batched jobs", who);
    SLNLP_CHECK_ARG(a.drop_head_dim >= 0 && (a.drop_head_dim == 0 || a.N % a.drop_head_dim == 0), "%s: drop_head_dim %d does not divide N %d", who,
                    a.drop_head_dim, a.N);
    SLNLP_CHECK_ARG(ceil_div(a.K, 64) <= RT_MAX_KTILES, "%s: K = %d > %d (the workgroup's partial tiles live in LDS)", who, a.K, 64 * RT_MAX_KTILES);
    return 0;
}

// dX = dY W (+ epilogue) and dW = dY^T x, db = colsum(dY) in one launch (gemm_rows_bwd_body).  dgrad: A = dY planes k-major, B = W planes
// m-major; wgrad: A = dY planes, B = x planes, both m-major, K = the batch rows (planes zero beyond them), C = dW fp32, rowsum_a = db or null.
int gemm_rows_bwd(const slnlp_gemm_args& dgrad, const slnlp_gemm_args& wgrad, hipStream_t st) {
    SLNLP_TRY(check_rows_job(dgrad, false, "gemm_rows_bwd (dgrad)"));
    const slnlp_gemm_args& w = wgrad;
    SLNLP_CHECK_ARG(w.A_hi && w.B_hi && w.C && !w.a_kmajor && !w.b_kmajor, "gemm_rows_bwd (wgrad): m-major operand planes and an fp32 output required");
    SLNLP_CHECK_ARG(w.precision == dgrad.precision && (w.precision == 1 || (w.A_lo && w.B_lo)), "gemm_rows_bwd (wgrad): same precision as the dgrad, lo planes for 3");
    SLNLP_CHECK_ARG(w.M > 0 && w.N > 0 && w.K > 0 && w.lda_p % 64 == 0 && w.ldb_p % 64 == 0 && w.lda_p >= w.M && w.ldb_p >= w.N && w.ldc >= w.N,
                    "gemm_rows_bwd (wgrad): bad shape / strides");
    SLNLP_CHECK_ARG((((uintptr_t)w.A_hi | (uintptr_t)w.B_hi | (uintptr_t)w.A_lo | (uintptr_t)w.B_lo) & 15) == 0, "gemm_rows_bwd (wgrad): planes must be 16-byte aligned");
    SLNLP_CHECK_ARG(!w.bias && !w.gate && !w.resid && w.drop_p == 0.f && !w.C_hi && w.relu == 0 && w.batch <= 1, "gemm_rows_bwd (wgrad): no epilogue");
    RowsBwdParams p;
    p.d.a = dgrad;
    p.d.drop_thr = dropout_threshold(dgrad.drop_p);
    p.d.drop_scale = 1.f / (1.f - dgrad.drop_p);
    p.w = wgrad;
    SLNLP_TRY(rows_init());
    const int geo = rows_geo(dgrad.M, dgrad.N, dgrad.K, 1, true);
    const dim3 gr = rows_grid(geo, dgrad.M, dgrad.N);
    return zlaunch(rows_bwd_kernel(dgrad.precision, geo), dim3(gr.x * gr.y + rows_wgrad_units(wgrad, geo)), RT_THREADS, rows_bwd_lds(geo, dgrad.K), st,
                   "gemm_rows_bwd", p);
}

int gemm_rows(const slnlp_gemm_args& a, hipStream_t st) {
    SLNLP_TRY(check_rows_job(a, true, "gemm_rows"));
    RowsParams p;
    p.a = a;
    p.drop_thr = dropout_threshold(a.drop_p);
    p.drop_scale = 1.f / (1.f - a.drop_p);
    SLNLP_TRY(rows_init());
    const int geo = rows_geo(a.M, a.N, a.K, 1, false);
    return zlaunch(rows_kernel(a.precision, geo), rows_grid(geo, a.M, a.N), RT_THREADS, rows_lds(geo, a.K), st, "gemm_rows", p);
}

// whether a solo launch of this product takes the 16 x 16 tile, the only one the LayerNorm prologue is built for (a forced
// SLNLP_ROWS_TILE other than 0 says no), and the row fits the prologue's registers
bool gemm_rows_ln_covers(int M, int N, int K) {
    return K % 64 == 0 && K <= LN_MAXU * 256 && ceil_div(K, 64) <= RT_MAX_KTILES && rows_geo(M, N, K, 1, false) == 0;
}

// C = epilogue( LayerNorm(x) W^T ) in one launch (gemm_rows_ln_body): `a` as for gemm_rows without its A operand, which is ln.x here
int gemm_rows_ln(const slnlp_gemm_args& a, const RowsLn& ln, hipStream_t st) {
    SLNLP_CHECK_ARG(!recording(), "gemm_rows_ln: a solo launch only (a lockstep program keeps layernorm_fwd and gemm_rows)");
    SLNLP_CHECK_ARG(ln.x && ln.gamma && ln.beta && ln.y, "gemm_rows_ln: null pointer (x, gamma, beta and y are required)");
    SLNLP_CHECK_ARG((ln.y_hi == nullptr) == (ln.y_lo == nullptr), "gemm_rows_ln: y's planes come as a pair (hi and lo), or not at all");
    slnlp_gemm_args c = a;                                   // (the shared checks see x in the A operand's place)
    c.A_hi = c.A_lo = reinterpret_cast<const uint16_t*>(ln.x);
    c.lda_p = a.K;
    SLNLP_TRY(check_rows_job(c, true, "gemm_rows_ln"));
    SLNLP_CHECK_ARG(gemm_rows_ln_covers(a.M, a.N, a.K), "gemm_rows_ln: M=%d N=%d K=%d is not a 16 x 16-tile launch with K <= %d (or another tile is forced)",
                    a.M, a.N, a.K, LN_MAXU * 256);
    SLNLP_CHECK_ARG(ln.ldx >= a.K && ln.ldx % 4 == 0 && (!ln.y_hi || (ln.ldp >= a.K && ln.ldp % 4 == 0)), "gemm_rows_ln: row strides must cover K and be multiples of 4");
    SLNLP_CHECK_ARG((((uintptr_t)ln.x | (uintptr_t)ln.gamma | (uintptr_t)ln.beta | (uintptr_t)ln.y) & 15) == 0 &&
                        (((uintptr_t)ln.y_hi | (uintptr_t)ln.y_lo) & 7) == 0,
                    "gemm_rows_ln: x, gamma, beta and y must be 16-byte aligned, y's planes 8-byte aligned");
    // other workgroups of the launch still read x (and the epilogue's operands) while the first column tile's write y
    const Span y = {ln.y, matrix_bytes(a.M, a.K, a.K), "y"};
    const Span read[3] = {{ln.x, matrix_bytes(a.M, ln.ldx, a.K), "x"}, {a.resid, matrix_bytes(a.M, a.ldr, a.N), "resid"},
                          {a.gate, matrix_bytes(a.M, a.ldg, a.N), "gate"}};
    for (const Span& s : read) SLNLP_CHECK_ARG(!spans_overlap(s, y), "gemm_rows_ln: %s and y overlap", s.name);
    RowsLnParams p;
    p.r.a = a;
    p.r.a.A_hi = p.r.a.A_lo = nullptr;
    p.r.drop_thr = dropout_threshold(a.drop_p);
    p.r.drop_scale = 1.f / (1.f - a.drop_p);
    p.ln = ln;
    SLNLP_TRY(rows_init());
    return zlaunch(a.precision == 3 ? gemm_rows_ln_kernel_3 : gemm_rows_ln_kernel_1, rows_grid(0, a.M, a.N), RT_THREADS, rows_ln_lds(a.K), st, "gemm_rows_ln", p);
}

}  // namespace slnlp

#if SLNLP_PROBE_FENCES == 256
// probe build only: copy the recorded workgroup timelines to the host and reset the recorder; returns the number recorded
extern "C" int slnlp_probe_rows_ts(unsigned long long* dst, int max_entries) {
    unsigned n = 0;
    if (hipDeviceSynchronize() != hipSuccess) return -1;
    if (hipMemcpyFromSymbol(&n, HIP_SYMBOL(slnlp::g_rts_n), sizeof(n)) != hipSuccess) return -1;
    if (n > (unsigned)slnlp::RTS_MAX) n = slnlp::RTS_MAX;
    if ((int)n > max_entries) n = max_entries;
    if (n && hipMemcpyFromSymbol(dst, HIP_SYMBOL(slnlp::g_rts), (size_t)n * slnlp::RTS_W * sizeof(unsigned long long)) != hipSuccess) return -1;
    const unsigned zero = 0;
    if (hipMemcpyToSymbol(HIP_SYMBOL(slnlp::g_rts_n), &zero, sizeof(zero)) != hipSuccess) return -1;
    return (int)n;
}
#endif

extern "C" int slnlp_gemm_rows_bwd(const slnlp_gemm_args* dgrad, const slnlp_gemm_args* wgrad, void* stream) {
    if (!dgrad || !wgrad) {
        slnlp::set_error("gemm_rows_bwd: null args");
        return SLNLP_ERR_INVALID_ARG;
    }
    return slnlp::gemm_rows_bwd(*dgrad, *wgrad, (hipStream_t)stream);
}

extern "C" int slnlp_set_rows_tile(int tile) {
    if (tile < -1 || tile >= slnlp::RT_NGEO) {
        slnlp::set_error("set_rows_tile: %d (-1 = automatic, 0 = 16 x 16, 1 = 64 x 16, 2 = 64 x 32 outputs per workgroup)", tile);
        return SLNLP_ERR_INVALID_ARG;
    }
    slnlp::g_rows_geo.store(tile, std::memory_order_relaxed);
    return 0;
}

extern "C" int slnlp_gemm_rows_ln(const slnlp_gemm_args* args, const float* x, int64_t ldx, const float* gamma, const float* beta, float eps, float* y,
                                  float* stats, uint16_t* y_hi, uint16_t* y_lo, int64_t ldp, void* stream) {
    if (!args) {
        slnlp::set_error("gemm_rows_ln: null args");
        return SLNLP_ERR_INVALID_ARG;
    }
    slnlp::RowsLn ln;
    ln.x = x; ln.ldx = ldx; ln.gamma = gamma; ln.beta = beta; ln.eps = eps; ln.y = y; ln.stats = stats; ln.y_hi = y_hi; ln.y_lo = y_lo; ln.ldp = ldp;
    return slnlp::gemm_rows_ln(*args, ln, (hipStream_t)stream);
}

extern "C" int slnlp_gemm_rows(const slnlp_gemm_args* args, void* stream) {
    if (!args) {
        slnlp::set_error("gemm_rows: null args");
        return SLNLP_ERR_INVALID_ARG;
    }
    return slnlp::gemm_rows(*args, (hipStream_t)stream);
}
