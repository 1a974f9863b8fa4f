// gemm.hip -- split-bf16 MFMA GEMM for gfx950 (MI355X).
//
//   C[M,N] = epilogue( sum_k A(m,k) * B(n,k) )
//
// All tensors are fp32 in HBM.  Tiles are converted to bf16 on the way into
// LDS; with precision 3 each fp32 value x is split into hi = bf16(x) and
// lo = bf16(x - hi) and the product is accumulated as Alo*Bhi + Ahi*Blo +
// Ahi*Bhi on v_mfma_f32_16x16x32_bf16 with fp32 accumulators (~2e-5 relative
// error: what the reference-parity bar of 1e-3 on logits needs; a single bf16
// pass measures 5e-3 and flips argmaxes).
//
// Shapes here are small (M = 2400 or 50 tokens, K,N <= 1536) and every launch
// sits on a dependent chain, so the kernel is built for per-block LATENCY:
//  * 64 x BN tile (BN = 64, or 16 to spread a skinny problem over more CUs),
//    K-step 64: K = 512 is 8 steps;
//  * the fp32 tiles of steps t+1 AND t+2 are in flight in registers while step
//    t is consumed from LDS (HBM/L2 latency is ~1 us, a step's MFMA work ~0.1 us);
//  * k-major operands are stored [row][k] and read as 16-byte fragments;
//    m-major operands (dgrad's W, both wgrad operands) are stored [k][row]
//    with 8-byte vector writes and read with ds_read_b64_tr_b16, the CDNA4
//    transposing LDS read -- no 2-byte scatter, no transposed copies in HBM.
//
// Replaces the matmuls inside nn.Linear / MultiheadAttention in/out
// projections / nn.LSTM / nn.GRU that the reference reaches at
// /root/reference/model/transformer.py:40-48 and
// /root/reference/model/base/encoder_decoder_attn_bkp.py:95-100,186-200.
#include <atomic>
#include <type_traits>

#include "common.hpp"
#include "gemm_jobs.hpp"
#include "mfma_tile.hpp"

namespace slnlp {

#if SLNLP_PROBE_FENCES == 256
// timeline probe build (tools/probes/probe_gemm_timeline.py): every workgroup records 100 MHz timestamps of its phases
constexpr int GTS_MAX = 1 << 14, GTS_W = 6;   // words: entry, first K tile in LDS, K loop done, image written, end, {grid, block}
__device__ unsigned long long g_gts[GTS_MAX][GTS_W];
__device__ unsigned g_gts_n;
#define GTS_MARK(slot) do { if (threadIdx.x == 0) gts[slot] = __builtin_amdgcn_s_memrealtime(); } while (0)
#else
#define GTS_MARK(slot) do { } while (0)
#endif

// LDS of one tile job: A planes, B planes, 4 x 64 row-sum scratch
template <int NSPLIT, bool AK, bool BK, int BNT>
constexpr int tile_lds_elems() {
    return (NSPLIT == 3 ? 2 : 1) * (TileIO<AK, BM>::PLANE + TileIO<BK, BNT>::PLANE) + 4 * BM * 2;
}

// One workgroup's tile: block (bid_x, bid_y) of a (grid_x, grid_y) grid over C.
// The K sum of every output element is DEFINED as two halves -- K tiles [0, T) and [T, ktiles), T = ceil(ktiles / 2), each
// accumulated in tile order from zero -- added at the end (first + second).  How the halves are computed is then a scheduling
// choice that does not touch the result:
//   KS = 2: the workgroup has two groups of 256 threads; group g runs the K loop over its own half of the K tiles with its own
//           stage images (all loads of both halves are in flight together, the dependent chain of K steps is half as long),
//           group 1 hands its accumulators over through LDS and group 0 adds them and runs the epilogue.  For launches that
//           cannot fill the chip anyway (the decoder's 50-row GEMMs: 32 ... 96 workgroups of 8 K tiles, whose duration IS the
//           K chain);
//   KS = 1: one group walks both halves and parks the first half's accumulators when it reaches tile T -- half the threads and a
//           quarter less registers per workgroup: the merged launches of a lockstep group (throughput-bound), which therefore
//           need not run the kernel a solo fit runs to return its bits.
template <int NSPLIT, bool AK, bool BK, int BNT, bool VEC, int KS = 1>
__device__ __forceinline__ void gemm_tile(const GemmParams& p, int bid_x, int bid_y, int grid_x, int grid_y,
                                          unsigned short* __restrict__ smem_base) {
#if SLNLP_PROBE_FENCES == 256
    unsigned long long gts[GTS_W] = {0, 0, 0, 0, 0, 0};
    struct GtsFlush {
        unsigned long long* t; int gx, bx;
        __device__ ~GtsFlush() {
            if (threadIdx.x == 0) {
                t[4] = __builtin_amdgcn_s_memrealtime();
                t[5] = ((unsigned long long)gx << 32) | (unsigned)bx;
                const unsigned i = atomicAdd(&g_gts_n, 1u) & (unsigned)(GTS_MAX - 1);
                for (int k = 0; k < GTS_W; ++k) g_gts[i][k] = t[k];
            }
        }
    } gts_flush{gts, grid_x * grid_y, bid_y * grid_x + bid_x};
    GTS_MARK(0);
#endif
    const int grp = KS == 2 ? (int)(threadIdx.x >> 8) : 0;
    unsigned short* __restrict__ smem = smem_base + grp * tile_lds_elems<NSPLIT, AK, BK, BNT>();
    using TA = TileIO<AK, BM>;
    using TB = TileIO<BK, BNT>;
    constexpr int NP = (NSPLIT == 3) ? 2 : 1;
    constexpr int MT = (BNT == 16) ? 1 : 2;  // 16x16 tiles per wave along M
    constexpr int NT = (BNT == 64) ? 2 : 1;  // ... along N
    unsigned short* As = smem;
    unsigned short* Bs = smem + NP * TA::PLANE;
    float (*rsum)[BM] = reinterpret_cast<float (*)[BM]>(smem + NP * (TA::PLANE + TB::PLANE));

    const slnlp_gemm_args& g = p.a;
    const int tid = threadIdx.x & 255, lane = tid & 63, wave = tid >> 6;
    // BNT=64: waves 2x2, each 32x32.  BNT=32: waves 2x2, each 32x16.  BNT=16: waves 4x1, each 16x16.
    const int wm0 = (BNT == 16) ? wave * 16 : (wave >> 1) * 32;
    const int wn0 = (BNT == 64) ? (wave & 1) * 32 : (BNT == 32) ? (wave & 1) * 16 : 0;
    // XCD-aware tile order: workgroups are dealt round-robin over the 8 XCDs (private 4 MiB L2 each);
    // remap so each XCD owns a contiguous run of tiles (all column blocks of a few row blocks): its
    // L2 then holds the whole B operand plus a few A panels instead of every panel of both.
    int bx, by;
    {
        const int nwg = grid_x * grid_y, id = bid_y * grid_x + bid_x;
        const int xcd = id & 7, q = nwg >> 3, r = nwg & 7;
        const int t = (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + (id >> 3);
        by = t / grid_x;
        bx = t - by * grid_x;
    }
    const int bm0 = by * BM, bn0 = bx * BNT;
    const int M = g.M, N = g.N, K = g.K;

    f32x4 acc[MT][NT];
#pragma unroll
    for (int i = 0; i < MT; ++i)
#pragma unroll
        for (int j = 0; j < NT; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

    const bool do_rowsum = (g.rowsum_a != nullptr) && (bx == 0);
    float rowsum = 0.f;

    const int ktiles = (K + BKT - 1) / BKT;
    // this group's K tiles [k0, k1); both groups make `trips` K steps (the barriers are the workgroup's), group 1 idles in its
    // last one when the number of tiles is odd
    const int half = (ktiles + 1) / 2;           // T: the second half of the K sum starts at this tile
    const int trips = KS == 2 ? half : ktiles;
    const int k0 = grp * trips, k1 = (KS == 2 && grp == 0) ? trips : ktiles;
    f32x4 acc_first[MT][NT];                     // KS = 1: the first half's sums, parked at tile T
    float rowsum_first = 0.f;
#pragma unroll
    for (int i = 0; i < MT; ++i)
#pragma unroll
        for (int j = 0; j < NT; ++j) acc_first[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
    // DEPTH K tiles in flight in registers.  (Four for the 16-wide tile of the decoder's 50-row products -- with KS = 2 all eight
    // tiles of a K = 512 product requested at kernel entry -- was measured with per-workgroup timelines, tools/probes/
    // probe_gemm_timeline.py: the K loop of 4 steps stayed at 2.6 us, it is the steps' own convert / barrier / MFMA chain and not a
    // wait for loads, and the first tile arrived 0.6 us (warm) to 1.5 us (cold) LATER behind the twenty requests.)
    // Prefetches are UNCONDITIONAL (past-the-end tiles read a clamped, valid address and are never
    // stashed): a guard would add a join point and make hipcc fall back to conservative vmcnt counts.
    constexpr int DEPTH = 2;
    // (Requesting the 16-wide tile's bias / gate / residual values here, in front of the K tiles, was measured too: the epilogue got
    // 0.15 - 0.3 us shorter and the first tile arrived 0.4 us later behind the nine extra requests -- a net loss.)
    float4 ra[DEPTH][TA::NV], rb[DEPTH][TB::NV];
#pragma unroll
    for (int d = 0; d < DEPTH; ++d) {
        TA::template fetch<VEC>(g.A, g.lda, bm0, M, (k0 + d) * BKT, K, tid, ra[d]);
        TB::template fetch<VEC>(g.B, g.ldb, bn0, N, (k0 + d) * BKT, K, tid, rb[d]);
    }

    auto consume = [&]() {
#pragma unroll
        for (int kk = 0; kk < 2; ++kk) {
            bf16x8 ah[MT], al[MT], bh[NT], bl[NT];
#pragma unroll
            for (int i = 0; i < MT; ++i) {
                ah[i] = TA::frag(As, wm0 + 16 * i, kk, lane);
                if (NSPLIT == 3) al[i] = TA::frag(As + TA::PLANE, wm0 + 16 * i, kk, lane);
            }
#pragma unroll
            for (int j = 0; j < NT; ++j) {
                bh[j] = TB::frag(Bs, wn0 + 16 * j, kk, lane);
                if (NSPLIT == 3) bl[j] = TB::frag(Bs + TB::PLANE, wn0 + 16 * j, kk, lane);
            }
#pragma unroll
            for (int i = 0; i < MT; ++i)
#pragma unroll
                for (int j = 0; j < NT; ++j) {
                    if (NSPLIT == 3) {
                        acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(al[i], bh[j], acc[i][j], 0, 0, 0);
                        acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ah[i], bl[j], acc[i][j], 0, 0, 0);
                    }
                    acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ah[i], bh[j], acc[i][j], 0, 0, 0);
                }
        }
        if (do_rowsum) {  // thread owns row (tid & 63), k-quarter (tid >> 6)
            const int row = tid & 63, kq = (tid >> 6) * 16;
            float s = 0.f;
#pragma unroll
            for (int k = 0; k < 16; ++k) s += TA::template value<NSPLIT>(As, row, kq + k);
            rowsum += s;
        }
    };

    // DEPTH K-steps per trip so the prefetch registers keep compile-time names
    auto mainloop = [&](auto edge_tag) {
        constexpr bool EDGE = decltype(edge_tag)::value;
        for (int it = 0; it < trips; it += DEPTH) {
#pragma unroll
            for (int d = 0; d < DEPTH; ++d) {
                if (d > 0 && it + d >= trips) break;
                const int kt = k0 + it + d;
                if (KS == 1 && kt == half) {     // (block-uniform; never taken when there is one tile)
#pragma unroll
                    for (int i = 0; i < MT; ++i)
#pragma unroll
                        for (int j = 0; j < NT; ++j) { acc_first[i][j] = acc[i][j]; acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f}; }
                    rowsum_first = rowsum;
                    rowsum = 0.f;
                }
                lds_barrier();
                if (KS == 1 || kt < k1) {
                    TA::template stash<NSPLIT, EDGE>(As, tid, ra[d], bm0, M, kt * BKT, K);
                    TB::template stash<NSPLIT, EDGE>(Bs, tid, rb[d], bn0, N, kt * BKT, K);
                }
                lds_barrier();
#if SLNLP_PROBE_FENCES == 256
                if (it + d == 0) GTS_MARK(1);
#endif
                TA::template fetch<VEC>(g.A, g.lda, bm0, M, (kt + DEPTH) * BKT, K, tid, ra[d]);
                TB::template fetch<VEC>(g.B, g.ldb, bn0, N, (kt + DEPTH) * BKT, K, tid, rb[d]);
                if (KS == 1 || kt < k1) consume();
            }
        }
    };
    // interior tile (block-uniform): no bounds masks in the conversion
    if (bm0 + BM <= M && bn0 + BNT <= N && (K % BKT) == 0) mainloop(std::false_type{});
    else mainloop(std::true_type{});
    GTS_MARK(2);
    if (KS == 1 && ktiles <= half) {             // a single tile: it IS the first half (the loop never reached tile T)
#pragma unroll
        for (int i = 0; i < MT; ++i)
#pragma unroll
            for (int j = 0; j < NT; ++j) { acc_first[i][j] = acc[i][j]; acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f}; }
        rowsum_first = rowsum;
        rowsum = 0.f;
    }
    if (do_rowsum) {
        // row sums of A: per half the four k-quarters of the threads, (q0 + q1) + (q2 + q3); first half + second half
        if (KS == 2) {
            rsum[tid >> 6][tid & 63] = rowsum;
            __syncthreads();
            float (*rs1)[BM] = reinterpret_cast<float (*)[BM]>(smem_base + tile_lds_elems<NSPLIT, AK, BK, BNT>() + NP * (TA::PLANE + TB::PLANE));
            float (*rs0)[BM] = reinterpret_cast<float (*)[BM]>(smem_base + NP * (TA::PLANE + TB::PLANE));
            if (grp == 0 && tid < 64 && bm0 + tid < M)
                g.rowsum_a[bm0 + tid] = ((rs0[0][tid] + rs0[1][tid]) + (rs0[2][tid] + rs0[3][tid])) + ((rs1[0][tid] + rs1[1][tid]) + (rs1[2][tid] + rs1[3][tid]));
        } else {
            lds_barrier();                       // (the last K step's fragment reads: rsum may overlap nothing, but keep the phases apart)
            rsum[tid >> 6][tid & 63] = rowsum_first;
            __syncthreads();
            float s_first = 0.f;
            if (tid < 64) s_first = (rsum[0][tid] + rsum[1][tid]) + (rsum[2][tid] + rsum[3][tid]);
            __syncthreads();
            rsum[tid >> 6][tid & 63] = rowsum;
            __syncthreads();
            if (tid < 64 && bm0 + tid < M) g.rowsum_a[bm0 + tid] = s_first + ((rsum[0][tid] + rsum[1][tid]) + (rsum[2][tid] + rsum[3][tid]));
        }
    }
    if (KS == 1) {
#pragma unroll
        for (int i = 0; i < MT; ++i)
#pragma unroll
            for (int j = 0; j < NT; ++j) acc[i][j] = acc_first[i][j] + acc[i][j];
    }
    if (KS == 2) {   // group 1's half of the K sum -> LDS -> group 0 (its stage images are free now)
        float* red = reinterpret_cast<float*>(smem_base + tile_lds_elems<NSPLIT, AK, BK, BNT>());
        __syncthreads();
        if (grp == 1) {
#pragma unroll
            for (int i = 0; i < MT; ++i)
#pragma unroll
                for (int j = 0; j < NT; ++j)
#pragma unroll
                    for (int r = 0; r < 4; ++r) red[((i * NT + j) * 4 + r) * 256 + tid] = acc[i][j][r];
        }
        __syncthreads();
        if (grp == 1) return;
#pragma unroll
        for (int i = 0; i < MT; ++i)
#pragma unroll
            for (int j = 0; j < NT; ++j)
#pragma unroll
                for (int r = 0; r < 4; ++r) acc[i][j][r] += red[((i * NT + j) * 4 + r) * 256 + tid];
    }

    // ---- epilogue: +bias -> relu -> gate -> dropout -> +resid, through an fp32 image of the tile in LDS (the stage images are free).
    // Straight out of the accumulator layout -- MT x NT tiles x 4 rows unrolled, a Philox per tile (per ROW with per-head dropout) and
    // a tanh per element inlined 16 times -- the epilogue was three quarters of this kernel's code (5100 of 6900 instructions at the
    // 64-wide tile): straight-line code every workgroup walks once, cold in the instruction cache.  Now the accumulators go to the
    // image as they are and ONE rolled loop takes "quads" -- 4 consecutive rows x 1 column, the unit one Philox call serves -- through
    // the chain; consecutive lanes hold consecutive columns, so the stores are whole 64-float rows instead of 16-float segments.
    // Same operations in the same order per element: the bits do not change.
    constexpr int ILD = BNT + 4;
    static_assert(tile_lds_elems<NSPLIT, AK, BK, BNT>() * 2 >= BM * ILD * 4, "the tile's image must fit the stage memory");
    float* img = reinterpret_cast<float*>(smem_base);
    if (KS == 1) lds_barrier();                  // (KS = 2: the hand-over above already put a barrier behind every wave's last fragment read)
    {
        const int crow = (lane >> 4) << 2, ccol = lane & 15;
#pragma unroll
        for (int i = 0; i < MT; ++i)
#pragma unroll
            for (int j = 0; j < NT; ++j)
#pragma unroll
                for (int r = 0; r < 4; ++r) img[(wm0 + i * 16 + crow + r) * ILD + wn0 + j * 16 + ccol] = acc[i][j][r];
    }
    lds_barrier();                               // (group 1 of a KS = 2 workgroup has ended: the barrier counts the waves that are left)
    GTS_MARK(3);
    const bool per_head = g.drop_head_dim > 0;
    DropKey dkey = {};                           // the step's Threefry key, made ONCE in front of the loop (common.hpp: dropout_key)
    if (g.drop_p > 0.f) dkey = dropout_key(g.rng, g.drop_site);
#pragma unroll 1
    for (int q = tid; q < (BM / 4) * BNT; q += 256) {
        const int col = q % BNT, gm0 = bm0 + 4 * (q / BNT), gn = bn0 + col;
        if (gn >= N || gm0 >= M) continue;
        const float bias = g.bias ? g.bias[gn] : 0.f;
        unsigned lot[4] = {0u, 0u, 0u, 0u};       // the quad's four 16-bit lots (common.hpp: one call serves 4 rows x columns {c, c ^ 16})
        if (g.drop_p > 0.f) {
            if (!per_head) {
                const uint4 bits = dropout_bits8(dkey, (unsigned)gm0 >> 2, drop_cc((unsigned)gn));
                const int half = drop_half((unsigned)gn);
#pragma unroll
                for (int r = 0; r < 4; ++r) lot[r] = pick_lot(bits, half, r);
            } else {                              // one keep/drop decision per (row, head), see slnlp.h
#pragma unroll 1
                for (int r = 0; r < 4; ++r) {
                    const unsigned rh = (unsigned)(gm0 + r) * (unsigned)(N / g.drop_head_dim) + (unsigned)(gn / g.drop_head_dim);
                    const uint4 hb = dropout_bits8(dkey, rh >> 2, 0u);
                    const unsigned wsel = pick_lot(hb, 0, (int)(rh & 3u));
                    if (r == 0) lot[0] = wsel; else if (r == 1) lot[1] = wsel; else if (r == 2) lot[2] = wsel; else lot[3] = wsel;
                }
            }
        }
        const float* src = img + (gm0 - bm0) * ILD + col;
        // the quad's gate and residual values are requested before its first store: resid may alias C (an in-place add), so a load
        // written behind a store has to stay there -- four dependent round trips per quad instead of one
        float gt[4], rs[4];
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int gm = gm0 + r;
            gt[r] = (g.gate && gm < M) ? g.gate[(long)gm * g.ldg + gn] : 0.f;
            rs[r] = (g.resid && gm < M) ? g.resid[(long)gm * g.ldr + gn] : 0.f;
        }
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int gm = gm0 + r;
            if (gm >= M) break;
            float v = src[r * ILD] + bias;
            if (g.relu == 1) v = fmaxf(v, 0.f);
            else if (g.relu == 2) v = tanhf(v);
            if (g.gate) v = g.gate_mode == 1 ? v * (1.f - gt[r] * gt[r]) : (gt[r] > 0.f ? v * g.gate_scale : 0.f);
            if (g.drop_p > 0.f) v = (lot[r] >= p.drop_thr) ? v * p.drop_scale : 0.f;
            if (g.resid) v += rs[r];
            g.C[(long)gm * g.ldc + gn] = v;
            if (g.C_hi) {                        // also as planes: the operand of a B-row product (gemm_rows.hip)
                unsigned short hh, ll;
                split_bf16(v, hh, ll);
                g.C_hi[(long)gm * g.ldc_p + gn] = hh;
                if (g.C_lo) g.C_lo[(long)gm * g.ldc_p + gn] = ll;
            }
        }
    }
}

// (two 256-thread workgroups per CU must fit: at most 256 registers a lane -- the scalar-load build of the 64-wide tile sits at the edge)
template <int NSPLIT, bool AK, bool BK, int BNT, bool VEC, int KS = 1>
__global__ __launch_bounds__(256 * KS, KS == 1 ? 2 : 1) void gemm_kernel(const GemmParams p) {
    __shared__ __attribute__((aligned(16))) unsigned short smem[KS * tile_lds_elems<NSPLIT, AK, BK, BNT>()];
    probe_kernel_begin();
    gemm_tile<NSPLIT, AK, BK, BNT, VEC, KS>(p, blockIdx.x, blockIdx.y, gridDim.x, gridDim.y, smem);
    probe_kernel_end();
}

// Several independent fp32-operand GEMMs in ONE launch (e.g. the data- and weight-gradient of one dY in the
// decoder, whose B-row GEMMs are pure launch latency): workgroups [block_begin, block_begin + gx*gy) run job j.
// `tab` != nullptr: a merged (lockstep) launch -- the jobs of K fits in a device-resident table, blockmap[block] = job
template <int NSPLIT, int KS>
__global__ __launch_bounds__(256 * KS) void gemm_group_kernel(const GemmGroupParams P, const GemmJob* __restrict__ tab,
                                                              const int* __restrict__ blockmap) {
    __shared__ __attribute__((aligned(16))) unsigned short smem[KS * tile_lds_elems<NSPLIT, false, false, 64>()];   // the largest variant
    GemmParams p;
    int variant, gx, gy, lid;
    if (tab) {
        const GemmJob& J = tab[blockmap[blockIdx.x]];
        p = J.p; variant = J.variant; gx = J.gx; gy = J.gy; lid = blockIdx.x - J.block_begin;
    } else {
        int j = 0;
        for (int t = 1; t < P.njobs; ++t)
            if ((int)blockIdx.x >= P.block_begin[t]) j = t;
        p = P.job[j]; variant = P.variant[j]; gx = P.gx[j]; gy = P.gy[j]; lid = blockIdx.x - P.block_begin[j];
    }
    launder(p.a);
    if (p.a.batch > 1) {                    // `batch` GEMMs of one shape: this block belongs to GEMM z
        const int z = lid / (gx * gy);
        lid -= z * gx * gy;
        p.a.A += (long)z * p.a.batch_stride_a;
        p.a.B += (long)z * p.a.batch_stride_b;
        p.a.C += (long)z * p.a.batch_stride_c;
        if (p.a.resid) p.a.resid += (long)z * p.a.batch_stride_c;
        if (p.a.C_hi) p.a.C_hi += (long)z * p.a.batch_stride_c;     // (plane outputs share C's column layout: ldc_p = ldc)
        if (p.a.C_lo) p.a.C_lo += (long)z * p.a.batch_stride_c;
    }
    const int bx = lid % gx, by = lid / gx;
    probe_kernel_begin();
    switch (variant) {
        case 0: gemm_tile<NSPLIT, true, true, 64, true, KS>(p, bx, by, gx, gy, smem); break;
        case 1: gemm_tile<NSPLIT, true, true, 16, true, KS>(p, bx, by, gx, gy, smem); break;
        case 2: gemm_tile<NSPLIT, true, false, 64, true, KS>(p, bx, by, gx, gy, smem); break;
        case 3: gemm_tile<NSPLIT, true, false, 16, true, KS>(p, bx, by, gx, gy, smem); break;
        case 4: gemm_tile<NSPLIT, false, false, 64, true, KS>(p, bx, by, gx, gy, smem); break;
        default: gemm_tile<NSPLIT, false, false, 16, true, KS>(p, bx, by, gx, gy, smem); break;
    }
    probe_kernel_end();
}

// KS = 2 (the two K halves on two thread groups) for launches that cannot fill the chip and whose duration is the chain of K steps.
// Results do not depend on KS (gemm_tile: the K sum is two halves either way), so the rule may look at whatever it likes -- a merged
// lockstep launch picks again for its own size (gemm_group_ks, lockstep.hip).  -1 = automatic; 1 / 2 forced (slnlp_set_gemm_ks: tests).
static std::atomic<int> g_gemm_ks{[] { const char* e = getenv("SLNLP_GEMM_KS"); const int v = e ? atoi(e) : 0; return v == 1 || v == 2 ? v : -1; }()};
int gemm_group_ks(int blocks, int longest_ktiles) {
    const int forced = g_gemm_ks.load(std::memory_order_relaxed);
    if (forced > 0) return forced;
    // <= 256 workgroups: the decoder's 50-row products (32 ... 128) and the RNN's recurrent data-gradient group (256: a solo LSTM step
    // gains 2.6 %); a merged launch of 4 Transformer fits is past that and throughput-bound (two thread groups per workgroup cost
    // it 3 %, 15 fits 2 %, 16 LSTM fits 15 %).  The longest K loop decides: a decoder weight gradient (K = the batch's 50 rows, one
    // tile -- its second thread group idles) shares its launch with the data gradient (K = 512: 8 steps -> 4), and the launch lasts
    // as long as that chain (cfg2 step 2.78 -> 2.75 ms).
    return blocks <= 256 && longest_ktiles >= 4 ? 2 : 1;
}
static int pick_ks(const slnlp_gemm_args* jobs, int njobs, int blocks) {
    int longest = 0;
    for (int i = 0; i < njobs; ++i) longest = std::max(longest, ceil_div(jobs[i].K, BKT));
    return gemm_group_ks(blocks, longest);
}

template <int NSPLIT, bool AK, bool BK, bool VEC>
static void launch2(const GemmParams& p, hipStream_t s) {
    // Skinny problems (one row-block) get 16-column tiles: 4x the workgroups, so a
    // [50 x 512] x [512 x 512] decoder GEMM runs on 32 CUs instead of 8.
    const bool narrow = p.a.M <= BM && p.a.rowsum_a == nullptr;
    const dim3 grid(ceil_div(p.a.N, narrow ? 16 : 64), ceil_div(p.a.M, BM));
    const int ks = VEC ? pick_ks(&p.a, 1, (int)(grid.x * grid.y)) : 1;
    if (narrow) {
        if (ks == 2) hipLaunchKernelGGL((gemm_kernel<NSPLIT, AK, BK, 16, VEC, VEC ? 2 : 1>), grid, dim3(VEC ? 512 : 256), 0, s, p);
        else hipLaunchKernelGGL((gemm_kernel<NSPLIT, AK, BK, 16, VEC>), grid, dim3(256), 0, s, p);
    } else {   // (64x32 tiles for ~1-block-per-CU grids were measured: no gain, 17.6 vs 16.0 us)
        if (ks == 2) hipLaunchKernelGGL((gemm_kernel<NSPLIT, AK, BK, 64, VEC, VEC ? 2 : 1>), grid, dim3(VEC ? 512 : 256), 0, s, p);
        else hipLaunchKernelGGL((gemm_kernel<NSPLIT, AK, BK, 64, VEC>), grid, dim3(256), 0, s, p);
    }
}

template <int NSPLIT, bool AK, bool BK>
static void launch(const GemmParams& p, hipStream_t s) {
    // 16-byte vector loads need both operands 16-B aligned with ld % 4 == 0; anything else
    // (e.g. an unpadded [B, 202] matrix) takes the scalar-load build of the same kernel.
    if (p.a_vec && p.b_vec) launch2<NSPLIT, AK, BK, true>(p, s);
    else launch2<NSPLIT, AK, BK, false>(p, s);
}

static int fill_params(const slnlp_gemm_args& a, GemmParams& p) {
    SLNLP_CHECK_ARG(a.A && a.B && a.C, "gemm: null operand");
    SLNLP_CHECK_ARG(a.M > 0 && a.N > 0 && a.K > 0, "gemm: bad shape M=%d N=%d K=%d", a.M, a.N, a.K);
    SLNLP_CHECK_ARG(a.precision == 1 || a.precision == 3, "gemm: precision must be 1 or 3, got %d", a.precision);
    SLNLP_CHECK_ARG(a.lda >= (a.a_kmajor ? a.K : a.M), "gemm: lda %ld too small", (long)a.lda);
    SLNLP_CHECK_ARG(a.ldb >= (a.b_kmajor ? a.K : a.N), "gemm: ldb %ld too small", (long)a.ldb);
    SLNLP_CHECK_ARG(a.ldc >= a.N, "gemm: ldc %ld < N %d", (long)a.ldc, a.N);
    SLNLP_CHECK_ARG(a.drop_p >= 0.f && a.drop_p < 1.f, "gemm: dropout p=%f out of [0,1)", a.drop_p);
    SLNLP_CHECK_ARG(a.drop_p == 0.f || a.rng, "gemm: dropout needs rng state");
    SLNLP_CHECK_ARG(!a.gate || a.ldg >= a.N, "gemm: ldg too small");
    SLNLP_CHECK_ARG(!a.resid || a.ldr >= a.N, "gemm: ldr too small");
    SLNLP_CHECK_ARG(!(a.a_kmajor == 0 && a.b_kmajor != 0), "gemm: layout (A m-major, B k-major) not built");
    SLNLP_CHECK_ARG(a.drop_head_dim >= 0 && (a.drop_head_dim == 0 || a.N % a.drop_head_dim == 0),
                    "gemm: drop_head_dim %d does not divide N %d", a.drop_head_dim, a.N);
    SLNLP_CHECK_ARG(!a.C_hi || a.ldc_p >= a.N, "gemm: ldc_p < N");
    p.a = a;
    p.drop_thr = dropout_threshold(a.drop_p);
    p.drop_scale = 1.f / (1.f - a.drop_p);
    p.a_vec = vec_ok(a.A, a.lda);
    p.b_vec = vec_ok(a.B, a.ldb);
    return 0;
}

int gemm(const slnlp_gemm_args& a, hipStream_t s) {
    if (a.A_hi || a.B_hi) return gemm_planes(a, s);   // pre-split operands: LDS-DMA kernel (gemm_planes.hip)
    if (recording()) return gemm_group(&a, 1, s);     // lockstep: every GEMM is a job of a grouped launch (same tile code)
    GemmParams p;
    SLNLP_TRY(fill_params(a, p));
    const bool ak = a.a_kmajor != 0, bk = a.b_kmajor != 0;
    if (a.precision == 3) {
        if (ak && bk) launch<3, true, true>(p, s);
        else if (ak) launch<3, true, false>(p, s);
        else launch<3, false, false>(p, s);
    } else {
        if (ak && bk) launch<1, true, true>(p, s);
        else if (ak) launch<1, true, false>(p, s);
        else launch<1, false, false>(p, s);
    }
    SLNLP_CHECK_LAUNCH("gemm");
    return SLNLP_OK;
}

// fp32-operand jobs in one launch; a job with operands that cannot take 16-B vector loads makes the whole group
// fall back to one launch per job (same results, just not fused)
// wide_mask bit i: job i takes 64-column tiles although it has one block of rows (16-column tiles spread a skinny product over 4 x
// the CUs, which pays while its K loop is long; a product cut into short K-slices has its workgroups from the slices, and wide tiles
// quarter the re-reads of its A rows).  Same K order: same bits either way.
int gemm_group(const slnlp_gemm_args* jobs, int njobs, hipStream_t s, unsigned wide_mask) {
    SLNLP_CHECK_ARG(jobs && njobs >= 1 && njobs <= GEMM_GROUP_MAX, "gemm_group: 1..%d jobs", GEMM_GROUP_MAX);
    GemmGroupParams P;
    P.njobs = njobs;
    int blocks = 0;
    bool fusable = true;
    for (int i = 0; i < njobs; ++i) {
        const slnlp_gemm_args& a = jobs[i];
        SLNLP_CHECK_ARG(!a.A_hi && !a.B_hi, "gemm_group: fp32 and pre-split jobs cannot share a launch");
        SLNLP_CHECK_ARG(a.precision == jobs[0].precision, "gemm_group: jobs of one launch share the precision");
        SLNLP_TRY(fill_params(a, P.job[i]));
        fusable = fusable && P.job[i].a_vec && P.job[i].b_vec;
        const bool narrow = a.M <= BM && a.rowsum_a == nullptr && !((wide_mask >> i) & 1u);
        P.variant[i] = (a.a_kmajor && a.b_kmajor ? 0 : a.a_kmajor ? 2 : 4) + (narrow ? 1 : 0);
        P.gx[i] = ceil_div(a.N, narrow ? 16 : 64);
        P.gy[i] = ceil_div(a.M, BM);
        P.block_begin[i] = blocks;
        const int nb = a.batch > 1 ? a.batch : 1;
        SLNLP_CHECK_ARG(nb == 1 || (!a.bias && !a.gate && !a.rowsum_a && a.drop_p == 0.f), "gemm_group: a batched job takes a residual only");
        SLNLP_CHECK_ARG(nb == 1 || (a.batch_stride_a % 4 == 0 && a.batch_stride_b % 4 == 0), "gemm_group: batch strides must keep 16-byte alignment");
        blocks += P.gx[i] * P.gy[i] * nb;
    }
    const int ks = pick_ks(jobs, njobs, blocks);
    if (recording()) {
        SLNLP_CHECK_ARG(fusable, "gemm_group: an operand that cannot take 16-byte loads cannot join a lockstep launch");
        return record_op(gemm_group_kernel_ptr(jobs[0].precision, ks), dim3(blocks), dim3(256 * ks), 0, REC_GEMM_GROUP, &P, sizeof(P), "gemm_group");
    }
    bool batched = false;
    for (int i = 0; i < njobs; ++i) batched = batched || jobs[i].batch > 1;
    if (!fusable || (njobs == 1 && !batched)) {
        for (int i = 0; i < njobs; ++i) {
            const int nb = jobs[i].batch > 1 ? jobs[i].batch : 1;
            for (int z = 0; z < nb; ++z) {                     // (operands without 16-byte alignment: one launch per GEMM)
                slnlp_gemm_args a = jobs[i];
                a.batch = 0;
                a.A += (long)z * jobs[i].batch_stride_a; a.B += (long)z * jobs[i].batch_stride_b; a.C += (long)z * jobs[i].batch_stride_c;
                if (a.resid) a.resid += (long)z * jobs[i].batch_stride_c;
                if (a.C_hi) a.C_hi += (long)z * jobs[i].batch_stride_c;
                if (a.C_lo) a.C_lo += (long)z * jobs[i].batch_stride_c;
                SLNLP_TRY(gemm(a, s));
            }
        }
        return SLNLP_OK;
    }
    void* args[3] = {(void*)&P, nullptr, nullptr};
    const GemmJob* no_tab = nullptr;
    const int* no_map = nullptr;
    args[1] = (void*)&no_tab; args[2] = (void*)&no_map;
    if (hipLaunchKernel(gemm_group_kernel_ptr(jobs[0].precision, ks), dim3(blocks), dim3(256 * ks), args, 0, s) != hipSuccess) {
        set_error("gemm_group: launch failed: %s", hipGetErrorString(hipGetLastError()));
        return SLNLP_ERR_LAUNCH;
    }
    SLNLP_CHECK_LAUNCH("gemm_group");
    return SLNLP_OK;
}

const void* gemm_group_kernel_ptr(int precision, int ks) {
    if (precision == 3) return ks == 2 ? (const void*)gemm_group_kernel<3, 2> : (const void*)gemm_group_kernel<3, 1>;
    return ks == 2 ? (const void*)gemm_group_kernel<1, 2> : (const void*)gemm_group_kernel<1, 1>;
}

}  // namespace slnlp

extern "C" int slnlp_gemm(const slnlp_gemm_args* args, void* stream) {
    if (!args) {
        slnlp::set_error("slnlp_gemm: null args");
        return SLNLP_ERR_INVALID_ARG;
    }
    return slnlp::gemm(*args, (hipStream_t)stream);
}

#if SLNLP_PROBE_FENCES == 256
// probe build only: copy the recorded workgroup timelines to the host and reset the recorder; returns the number recorded
extern "C" int slnlp_probe_gemm_ts(unsigned long long* dst, int max_entries) {
    unsigned n = 0;
    if (hipDeviceSynchronize() != hipSuccess) return -1;
    if (hipMemcpyFromSymbol(&n, HIP_SYMBOL(slnlp::g_gts_n), sizeof(n)) != hipSuccess) return -1;
    if (n > (unsigned)slnlp::GTS_MAX) n = slnlp::GTS_MAX;
    if ((int)n > max_entries) n = max_entries;
    if (n && hipMemcpyFromSymbol(dst, HIP_SYMBOL(slnlp::g_gts), (size_t)n * slnlp::GTS_W * sizeof(unsigned long long)) != hipSuccess) return -1;
    const unsigned zero = 0;
    if (hipMemcpyToSymbol(HIP_SYMBOL(slnlp::g_gts_n), &zero, sizeof(zero)) != hipSuccess) return -1;
    return (int)n;
}
#endif

extern "C" int slnlp_set_gemm_ks(int ks) {
    if (ks != 0 && ks != 1 && ks != 2) {
        slnlp::set_error("set_gemm_ks: %d (0 = automatic, 1 or 2 thread groups per workgroup)", ks);
        return SLNLP_ERR_INVALID_ARG;
    }
    slnlp::g_gemm_ks.store(ks == 0 ? -1 : ks, std::memory_order_relaxed);
    return 0;
}
