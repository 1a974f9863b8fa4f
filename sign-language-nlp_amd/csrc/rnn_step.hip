// rnn_step.hip -- the recurrent MFMA kernels of the LSTM / GRU path: the fused forward timestep (recurrent GEMM + cell in one
// launch, on two tilings), the fused backward timestep, and the opt-in persistent layer kernel (all timesteps in one launch).
// They are built from the tile toolkit of the fp32-operand GEMM (mfma_tile.hpp: same images, same split-bf16 product order),
// walk K in gemm_tile's two halves (k_halves below) and apply the one cell arithmetic of rnn_cell.hpp, so each of them
// returns the bits of GEMM (gemm.hip) + point-wise cell (rnn.hip).
#include <atomic>

#include "common.hpp"
#include "gemm_jobs.hpp"
#include "mfma_tile.hpp"
#include "rnn_cell.hpp"

namespace slnlp {

// ------------------------------------------------------------- fused recurrent step ---
// One forward timestep of an LSTM / GRU layer (up to two directions) in ONE launch: the recurrent GEMM
// h_{t-1} W_hh^T and the point-wise cell (rnn_cell.hpp, rnn_cell_fwd_elem) that consumes it.  A workgroup owns 16 hidden
// units: it computes their G gate pre-activations for all B rows (G B-tiles of 16 weight rows, one shared A tile per
// K-step, same split-bf16 K order as gemm_tile, so results are bit-identical to GEMM + cell) and applies the cell in
// the accumulator layout -- every lane holds all G gates of its (row, unit) pairs.  The new state goes to a DIFFERENT
// buffer than the one read (other workgroups still read h_{t-1}): the caller chains the per-timestep `hprev` slots.
struct RnnStepParams {
    slnlp_rnn_step_dir d[2];
    int B, Hd, ndir;
    const long* lengths;
    float fill;
    long ld_out;
    float drop_p;
    unsigned drop_thr;
    int drop_site;
    const unsigned long long* rng;
};

__device__ __forceinline__ slnlp_rnn_step_dir as_global(slnlp_rnn_step_dir d) {
    d.h_in = as_global(d.h_in); d.h_out = as_global(d.h_out); d.w_hh = as_global(d.w_hh); d.b_hh = as_global(d.b_hh);
    d.xproj = as_global(d.xproj); d.c = as_global(d.c); d.cprev_save = as_global(d.cprev_save); d.acts = as_global(d.acts);
    d.hn_save = as_global(d.hn_save); d.out = as_global(d.out);
    return d;
}

// The cell of element (row b, unit j) of a forward timestep and its stores, for both tilings (hp = accumulator + b_hh)
template <bool LSTM>
__device__ __forceinline__ void rnn_step_cell(const RnnStepParams& P, const slnlp_rnn_step_dir& d, int b, int j, const float (&xp)[LSTM ? 4 : 3],
                                              const float (&hp)[LSTM ? 4 : 3], float hprev, float cprev) {
    constexpr int G = LSTM ? 4 : 3;
    const int Hd = P.Hd;
    const long idx = (long)b * Hd + j;
    const bool valid = P.lengths ? (d.t < P.lengths[b]) : true;
    const RnnCellFwd<LSTM> o = rnn_cell_fwd_elem<LSTM>(xp, hp, hprev, cprev);
    float* a = d.acts + (long)b * G * Hd;
#pragma unroll
    for (int g = 0; g < G; ++g) a[g * Hd + j] = o.act[g];
    if constexpr (LSTM) {
        d.cprev_save[idx] = cprev;
        d.c[idx] = valid ? o.cnew : cprev;
    } else {
        d.hn_save[idx] = o.hn;
    }
    d.h_out[idx] = valid ? o.hnew : hprev;
    if (d.out)
        d.out[(long)b * P.ld_out + j] = rnn_cell_out(valid, o.hnew, P.fill, P.drop_p, P.drop_thr, P.drop_site, P.rng,
                                                     (unsigned)(d.out_row0 + b), (unsigned)(d.out_col0 + j));
}

// The K walk of the forward kernels: gemm_tile's loop (gemm.hip) without its row sums and probes.  The K sum is DEFINED as two
// halves, tiles [0, T) and [T, ktiles), T = ceil(ktiles / 2), each summed in tile order from zero, then first + second; how
// they are scheduled does not touch the bits:
//   KS = 1: one thread group walks all tiles and calls park() at tile T (behind the loop when there is one tile: it IS the
//           first half) -- park moves the accumulators aside and zeroes them; the caller adds parked + live;
//   KS = 2: group `grp` walks its own half; both make T trips (the barriers are the workgroup's), group 1 idles in its last
//           one when the tile count is odd; the caller hands group 1's sums to group 0 through LDS and adds them there.
// Two tiles are in flight in registers: fetch(kt, slot) requests tile kt into slot 0 / 1 (past-the-end tiles read a clamped,
// valid address and are never stashed), stash(kt, slot) converts the slot into the stage image, consume(kt) multiplies it.
template <int KS, class Fetch, class Stash, class Consume, class Park>
__device__ __forceinline__ void k_halves(int ktiles, int grp, const Fetch& fetch, const Stash& stash, const Consume& consume,
                                         const Park& park) {
    const int half = (ktiles + 1) / 2, trips = KS == 2 ? half : ktiles;
    const int k0 = grp * trips, k1 = (KS == 2 && grp == 0) ? trips : ktiles;      // this group's tiles [k0, k1)
    fetch(k0, 0);
    fetch(k0 + 1, 1);
    for (int it = 0; it < trips; it += 2) {
#pragma unroll
        for (int slot = 0; slot < 2; ++slot) {      // two K steps per trip so the prefetch registers keep compile-time names
            if (slot > 0 && it + slot >= trips) break;
            const int kt = k0 + it + slot;
            if (KS == 1 && kt == half) park();
            lds_barrier();
            if (KS == 1 || kt < k1) stash(kt, slot);
            lds_barrier();
            fetch(kt + 2, slot);
            if (KS == 1 || kt < k1) consume(kt);
        }
    }
    if (KS == 1 && ktiles <= half) park();
}

// ------------------------------------------------------------------------------------------ fused backward timestep ---
// One launch per backward timestep (rounds 1-3: a cell kernel + a grouped K-sliced GEMM launch, 192 + 192 launches per cfg3 step):
//   dh(t) = dgh(t+1) W_hh + carry(t+1)            [B, Hd]     recurrent data gradient of the step processed just before
//   cell backward of step t (rnn_cell.hpp, rnn_cell_bwd_elem)  ->  dgx(t), dgh(t), dc, carry(t)
// A workgroup owns 16 hidden units (output columns of the GEMM) of one direction and 64 batch rows.  The contraction runs over
// the G * Hd gate columns: G groups of 256 threads, group g contracting gate g's Hd columns with its own stage images (all G K
// loops in flight together: the dependent chain is Hd / 64 steps, as in the K-sliced launch it replaces); the groups' partial
// sums meet in LDS and are added in gate order -- ((P0 + carry) + P1) + P2 (+ P3), the order of the unfused path -- and group 0
// applies the cell in the accumulator layout.  dgh_next == NULL: first step of a layer, dh = dh_state (no product).
struct RnnStepBwdParams {
    slnlp_rnn_step_bwd_dir d[2];
    int B, Hd, ndir;
    const long* lengths;
    long ld_dout;
    float drop_p;
    unsigned drop_thr;
    int drop_site;
    const unsigned long long* rng;
};
__device__ __forceinline__ slnlp_rnn_step_bwd_dir as_global(slnlp_rnn_step_bwd_dir d) {
    d.cell = as_global(d.cell);
    d.dgh_next = as_global(d.dgh_next); d.w_hh = as_global(d.w_hh);
    return d;
}
template <int NSPLIT, bool LSTM>
constexpr int rnn_step_bwd_group_elems() {
    return (NSPLIT == 3 ? 2 : 1) * (TileIO<true, BM>::PLANE + TileIO<false, 16>::PLANE);
}
template <int NSPLIT, bool LSTM>
constexpr size_t rnn_step_bwd_lds() {
    constexpr int G = LSTM ? 4 : 3;
    return (size_t)G * rnn_step_bwd_group_elems<NSPLIT, LSTM>() * sizeof(unsigned short) + (size_t)(G - 1) * 256 * sizeof(f32x4);
}

template <int NSPLIT, bool LSTM>
__global__ __launch_bounds__(LSTM ? 1024 : 768) void rnn_step_bwd_kernel(const RnnStepBwdParams P0, const RnnStepBwdParams* __restrict__ tab) {
    extern __shared__ __attribute__((aligned(16))) unsigned short bsm[];
    RnnStepBwdParams P;
    if (tab) P = tab[blockIdx.z];
    else P = P0;
    P.lengths = as_global(P.lengths);
    P.rng = as_global(P.rng);
    constexpr int G = LSTM ? 4 : 3;
    constexpr int NP = NSPLIT == 3 ? 2 : 1;
    using TA = TileIO<true, BM>;
    using TB = TileIO<false, 16>;
    const int grp = threadIdx.x >> 8, tid = threadIdx.x & 255, lane = tid & 63, wave = tid >> 6;
    unsigned short* As = bsm + grp * rnn_step_bwd_group_elems<NSPLIT, LSTM>();
    unsigned short* Bs = As + NP * TA::PLANE;
    f32x4* red = reinterpret_cast<f32x4*>(bsm + G * rnn_step_bwd_group_elems<NSPLIT, LSTM>());
    const int dir = blockIdx.y % P.ndir;
    const slnlp_rnn_step_bwd_dir sd = as_global(dir == 0 ? P.d[0] : P.d[1]);
    const slnlp_rnn_cell_bwd_dir& d = sd.cell;
    const int B = P.B, Hd = P.Hd, GH = G * Hd, j0 = blockIdx.x * 16, bm0 = (blockIdx.y / P.ndir) * BM;
    const bool product = sd.dgh_next != nullptr;       // (launch-uniform per direction)

    f32x4 acc = f32x4{0.f, 0.f, 0.f, 0.f};
    if (product) {
        const int ktiles = Hd / BKT, kg = grp * Hd;    // this group's gate columns [kg, kg + Hd)
        float4 ra0[TA::NV], ra1[TA::NV], rb0[TB::NV], rb1[TB::NV];
        auto fetch = [&](int kt, float4 (&ra)[TA::NV], float4 (&rb)[TB::NV]) {
            const int kc = kt < ktiles ? kt : 0;           // past-the-end prefetch: a valid tile, never stashed
            TA::template fetch<true>(sd.dgh_next, GH, bm0, B, kg + kc * BKT, GH, tid, ra);
            TB::template fetch<true>(sd.w_hh, Hd, j0, Hd, kg + kc * BKT, GH, tid, rb);
        };
        auto stash = [&](int kt, const float4 (&ra)[TA::NV], const float4 (&rb)[TB::NV]) {
            // rows >= B hold a clamped row's data and only feed accumulator rows that are never used (no masks: Hd % 64 == 0)
            TA::template stash<NSPLIT, false>(As, tid, ra, bm0, B, kg + kt * BKT, GH);
            TB::template stash<NSPLIT, false>(Bs, tid, rb, j0, Hd, kg + kt * BKT, GH);
        };
        auto consume = [&]() {
#pragma unroll
            for (int kk = 0; kk < 2; ++kk) {
                const bf16x8 ah = TA::frag(As, wave * 16, kk, lane);
                const bf16x8 bh = TB::frag(Bs, 0, kk, lane);
                bf16x8 al = ah, bl = bh;
                if (NSPLIT == 3) {
                    al = TA::frag(As + TA::PLANE, wave * 16, kk, lane);
                    bl = TB::frag(Bs + TB::PLANE, 0, kk, lane);
                }
                acc = mfma_split<NSPLIT>(ah, al, bh, bl, acc);
            }
        };
        fetch(0, ra0, rb0);
        fetch(1, ra1, rb1);
        for (int kt = 0; kt < ktiles; kt += 2) {
            lds_barrier();
            stash(kt, ra0, rb0);
            lds_barrier();
            fetch(kt + 2, ra0, rb0);
            consume();
            if (kt + 1 >= ktiles) break;
            lds_barrier();
            stash(kt + 1, ra1, rb1);
            lds_barrier();
            fetch(kt + 3, ra1, rb1);
            consume();
        }
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");     // the dummy prefetches
        if (grp > 0) red[(grp - 1) * 256 + tid] = acc;
        __syncthreads();
    }
    if (grp != 0) return;

    // ---- the cell backward of this timestep in the accumulator layout
    const int j = j0 + (lane & 15);
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int b = bm0 + wave * 16 + ((lane >> 4) << 2) + r;
        if (b >= B) break;
        const long idx = (long)b * Hd + j;
        const bool valid = P.lengths ? (d.t < P.lengths[b]) : true;
        float dh;
        if (product) {
            dh = acc[r] + d.carry[idx];                      // (the unfused path adds carry as the first job's residual)
#pragma unroll
            for (int e = 0; e < G - 1; ++e) dh += red[e * 256 + tid][r];
        } else {
            dh = d.dh_state[idx];
        }
        float* gx = d.dgx + (long)b * GH;
        float* gh = LSTM ? gx : d.dgh + (long)b * GH;
        if (!valid) {
#pragma unroll
            for (int g = 0; g < G; ++g) {
                gx[g * Hd + j] = 0.f;
                if (!LSTM) gh[g * Hd + j] = 0.f;
            }
            d.carry[idx] = dh;
            continue;
        }
        if (d.dout) {
            float g = d.dout[(long)b * P.ld_dout + j];
            if (P.drop_p > 0.f)
                g = dropout_keep(P.rng, P.drop_site, (unsigned)(d.out_row0 + b), (unsigned)(d.out_col0 + j), P.drop_thr)
                        ? g / (1.f - P.drop_p) : 0.f;
            dh += g;
        }
        const float* a = d.acts + (long)b * GH;
        const float s0 = LSTM ? d.cprev_save[idx] : d.hprev_save[idx], s1 = LSTM ? d.dc_state[idx] : d.hn_save[idx];
        const RnnCellBwd<LSTM> o = rnn_cell_bwd_elem<LSTM>(dh, a[j], a[Hd + j], a[2 * Hd + j], LSTM ? a[3 * Hd + j] : 0.f, s0, s1);
#pragma unroll
        for (int g = 0; g < G; ++g) gx[g * Hd + j] = o.dg[g];
        if constexpr (LSTM) {
            d.dc_state[idx] = o.dc_state;
        } else {
            gh[j] = o.dg[0]; gh[Hd + j] = o.dg[1]; gh[2 * Hd + j] = o.dgh_n;
        }
        d.carry[idx] = o.carry;
    }
}

// the four builds and their dynamic LDS: [precision 3 ? 2 : 0] + [LSTM]
struct RnnStepBwdBuild { const void* fn; size_t lds; };
static const RnnStepBwdBuild* rnn_step_bwd_builds() {
#define SLNLP_RB(NS, L) {(const void*)rnn_step_bwd_kernel<NS, L>, rnn_step_bwd_lds<NS, L>()}
    static const RnnStepBwdBuild tab[4] = {SLNLP_RB(1, false), SLNLP_RB(1, true), SLNLP_RB(3, false), SLNLP_RB(3, true)};
#undef SLNLP_RB
    return tab;
}

// raise the kernels' dynamic LDS limit once per device (plan creation: never inside a graph capture)
int rnn_step_bwd_init() {
    static DeviceOnce once;
    return once.run([]() -> int {
        for (int i = 0; i < 4; ++i) {
            const RnnStepBwdBuild& k = rnn_step_bwd_builds()[i];
            if (hipFuncSetAttribute(k.fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)k.lds) != hipSuccess) {
                set_error("rnn_step_bwd_init: cannot raise dynamic LDS limit: %s", hipGetErrorString(hipGetLastError()));
                return SLNLP_ERR_LAUNCH;
            }
        }
        return 0;
    });
}

bool rnn_step_bwd_covers(int B, int Hd) { return Hd % 64 == 0 && B > 0; }

int rnn_step_bwd(int lstm, const slnlp_rnn_step_bwd_dir* dirs, int ndir, int B, int Hd, const int64_t* lengths, int64_t ld_dout,
                 float drop_p, int drop_site, const unsigned long long* rng, int precision, hipStream_t st) {
    SLNLP_CHECK_ARG(dirs && (ndir == 1 || ndir == 2) && rnn_step_bwd_covers(B, Hd), "rnn_step_bwd: bad args (Hd %% 64 == 0)");
    SLNLP_CHECK_ARG(precision == 1 || precision == 3, "rnn_step_bwd: precision must be 1 or 3");
    SLNLP_CHECK_ARG(drop_p >= 0.f && drop_p < 1.f && (drop_p == 0.f || rng), "rnn_step_bwd: bad dropout args");
    const int G = lstm ? 4 : 3;
    RnnStepBwdParams P;
    for (int k = 0; k < ndir; ++k) {
        const slnlp_rnn_step_bwd_dir& d = dirs[k];
        SLNLP_CHECK_ARG(d.cell.dc_state || !lstm, "rnn_step_bwd: dc_state missing in direction %d", k);
        SLNLP_CHECK_ARG(d.cell.acts && d.cell.dgx && d.cell.carry && (lstm ? d.cell.cprev_save != nullptr : (d.cell.hprev_save && d.cell.hn_save && d.cell.dgh)),
                        "rnn_step_bwd: null pointer in direction %d", k);
        SLNLP_CHECK_ARG(d.dgh_next ? (d.w_hh && vec_ok(d.dgh_next, (long)G * Hd) && vec_ok(d.w_hh, Hd)) : d.cell.dh_state != nullptr,
                        "rnn_step_bwd: direction %d needs {dgh_next, w_hh} (16-byte aligned) or dh_state", k);
        SLNLP_CHECK_ARG((dirs[0].dgh_next != nullptr) == (d.dgh_next != nullptr), "rnn_step_bwd: the directions of a launch are both first steps or both not");
        P.d[k] = d;
    }
    if (ndir == 1) P.d[1] = P.d[0];
    P.B = B; P.Hd = Hd; P.ndir = ndir; P.lengths = (const long*)lengths; P.ld_dout = ld_dout;
    P.drop_p = drop_p; P.drop_thr = dropout_threshold(drop_p); P.drop_site = drop_site; P.rng = rng;
    SLNLP_TRY(rnn_step_bwd_init());
    const dim3 grid(Hd / 16, ndir * ceil_div(B, BM));
    const dim3 block(G * 256);
    const RnnStepBwdBuild& k = rnn_step_bwd_builds()[(precision == 3 ? 2 : 0) + (lstm ? 1 : 0)];
    const void* fn = k.fn;
    const size_t lds = k.lds;
    if (recording()) return record_op(fn, grid, block, lds, REC_Z, &P, sizeof(P), "rnn_step_bwd");
    const RnnStepBwdParams* tab = nullptr;
    void* args[2] = {&P, &tab};
    if (hipLaunchKernel(fn, grid, block, args, lds, st) != hipSuccess) {
        set_error("rnn_step_bwd: %s", hipGetErrorString(hipGetLastError()));
        return SLNLP_ERR_LAUNCH;
    }
    return SLNLP_OK;
}

// grid (Hd / 16, ndir x row tiles, fit): `tab` != nullptr is a lockstep launch, fit z takes tab[z] (launch.hpp)
// KS = 2: two groups of 256 threads, one half of the K tiles each (gemm_tile's scheme: the K sum is two halves by definition, so the
// bits do not depend on KS) -- a solo fit's 64-workgroup launch is a chain of 8 K steps, a merged lockstep launch takes KS = 1.
template <int NSPLIT, bool LSTM, bool EDGE, int KS = 1>
__global__ __launch_bounds__(256 * KS) void rnn_step_fwd_kernel(const RnnStepParams P0, const RnnStepParams* __restrict__ tab) {
    RnnStepParams P;
    if (tab) P = tab[blockIdx.z];
    else P = P0;
    P.lengths = as_global(P.lengths);
    P.rng = as_global(P.rng);
    constexpr int G = LSTM ? 4 : 3;
    constexpr int NP = NSPLIT == 3 ? 2 : 1;
    using TA = TileIO<true, BM>;
    using TB = TileIO<true, 16>;
    __shared__ __attribute__((aligned(16))) unsigned short As_all[KS * NP * TA::PLANE];
    __shared__ __attribute__((aligned(16))) unsigned short Bs_all[KS * G * NP * TB::PLANE];
    __shared__ f32x4 red[KS == 2 ? G * 256 : 1];               // group 1's half of the K sum on its way to group 0
    const int grp = KS == 2 ? (int)(threadIdx.x >> 8) : 0;
    unsigned short* As = As_all + grp * NP * TA::PLANE;
    unsigned short* Bs = Bs_all + grp * G * NP * TB::PLANE;
    const int dir = blockIdx.y % P.ndir;
    const slnlp_rnn_step_dir d = as_global(dir == 0 ? P.d[0] : P.d[1]);
    const int tid = threadIdx.x & 255, lane = tid & 63, wave = tid >> 6;
    const int B = P.B, Hd = P.Hd, j0 = blockIdx.x * 16, bm0 = (blockIdx.y / P.ndir) * BM;
    const int K = Hd, ktiles = (K + BKT - 1) / BKT;

    f32x4 acc[G];
#pragma unroll
    for (int g = 0; g < G; ++g) acc[g] = f32x4{0.f, 0.f, 0.f, 0.f};
    float4 ra[2][TA::NV], rb[2][G][TB::NV];
    auto fetch = [&](int kt, int slot) {
        TA::template fetch<true>(d.h_in, Hd, bm0, B, kt * BKT, K, tid, ra[slot]);
#pragma unroll
        for (int g = 0; g < G; ++g) TB::template fetch<true>(d.w_hh + (long)g * Hd * Hd, Hd, j0, Hd, kt * BKT, K, tid, rb[slot][g]);
    };
    auto stash = [&](int kt, int slot) {
        // EDGE = false (Hd % 64 == 0): no masks at all -- rows >= B hold a clamped row's data and only feed accumulator
        // rows that are never stored
        TA::template stash<NSPLIT, EDGE>(As, tid, ra[slot], bm0, B, kt * BKT, K);
#pragma unroll
        for (int g = 0; g < G; ++g) TB::template stash<NSPLIT, EDGE>(Bs + g * NP * TB::PLANE, tid, rb[slot][g], j0, Hd, kt * BKT, K);
    };
    auto consume = [&](int) {
#pragma unroll
        for (int kk = 0; kk < 2; ++kk) {
            const bf16x8 ah = TA::frag(As, wave * 16, kk, lane);
            bf16x8 al = ah;
            if (NSPLIT == 3) al = TA::frag(As + TA::PLANE, wave * 16, kk, lane);
#pragma unroll
            for (int g = 0; g < G; ++g) {
                const unsigned short* bt = Bs + g * NP * TB::PLANE;
                const bf16x8 bh = TB::frag(bt, 0, kk, lane);
                bf16x8 bl = bh;
                if (NSPLIT == 3) bl = TB::frag(bt + TB::PLANE, 0, kk, lane);
                acc[g] = mfma_split<NSPLIT>(ah, al, bh, bl, acc[g]);
            }
        }
    };
    // the cell's own operands are requested first, so their latency hides behind the K loop
    const int j = j0 + (lane & 15), jj = j < Hd ? j : 0;
    float bh[G], xpv[4][G], hpv[4], cpv[4];
#pragma unroll
    for (int g = 0; g < G; ++g) bh[g] = d.b_hh ? d.b_hh[g * Hd + jj] : 0.f;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int b = bm0 + wave * 16 + ((lane >> 4) << 2) + r, bb = b < B ? b : 0;
#pragma unroll
        for (int g = 0; g < G; ++g) xpv[r][g] = d.xproj[(long)bb * G * Hd + g * Hd + jj];
        hpv[r] = d.h_in[(long)bb * Hd + jj];
        cpv[r] = LSTM ? d.c[(long)bb * Hd + jj] : 0.f;
    }
    f32x4 acc_first[G];
    auto park = [&]() {
#pragma unroll
        for (int g = 0; g < G; ++g) { acc_first[g] = acc[g]; acc[g] = f32x4{0.f, 0.f, 0.f, 0.f}; }
    };
    k_halves<KS>(ktiles, grp, fetch, stash, consume, park);
    if constexpr (KS == 1) {
#pragma unroll
        for (int g = 0; g < G; ++g) acc[g] = acc_first[g] + acc[g];
    } else {
        if (grp == 1) {
#pragma unroll
            for (int g = 0; g < G; ++g) red[g * 256 + tid] = acc[g];
        }
        __syncthreads();
        if (grp == 1) return;
#pragma unroll
        for (int g = 0; g < G; ++g) acc[g] = acc[g] + red[g * 256 + tid];
    }

    // ---- cell (rnn_cell.hpp) in the accumulator layout: every lane holds all G gates of its (row, unit) pairs
    if (j >= Hd) return;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int b = bm0 + wave * 16 + ((lane >> 4) << 2) + r;
        if (b >= B) break;
        float hp[G];
#pragma unroll
        for (int g = 0; g < G; ++g) hp[g] = acc[g][r] + bh[g];
        rnn_step_cell<LSTM>(P, d, b, j, xpv[r], hp, hpv[r], cpv[r]);
    }
}

// The same timestep RE-TILED for a solo fit's launch: a workgroup owns 16 batch rows x 16 hidden units x all G gates (grid Hd / 16 x
// ndir x row tiles of 16: 256 workgroups at B = 50, Hd = 512, two directions -- every CU -- instead of 64), WAVE g computes gate g's
// 16 x 16 tile, and wave 0 applies the cell once the gates have met in LDS.  Why: such a launch lasts as long as one workgroup takes
// to LOAD its operands (gemm_rows.hip measured the same for the decoder's products: ~33 GB/s per compute unit), and the 64-row
// tile above pulls 128 KB of h beside its 128 KB of W_hh per workgroup where this one pulls 32 + 128.  Same K order, same halves,
// same cell arithmetic per element: bit-identical to rnn_step_fwd_kernel (tests/test_rnn_gpu.py), so a merged lockstep launch --
// which pays for total bytes, not for one workgroup's -- keeps the 64-row kernel (rnn_step_fwd_for_blocks).
template <int NSPLIT, bool LSTM, bool EDGE, int KS = 1>
__global__ __launch_bounds__(256 * KS) void rnn_step_fwd_rt_kernel(const RnnStepParams P0, const RnnStepParams* __restrict__ tab) {
    RnnStepParams P;
    if (tab) P = tab[blockIdx.z];
    else P = P0;
    P.lengths = as_global(P.lengths);
    P.rng = as_global(P.rng);
    constexpr int G = LSTM ? 4 : 3;
    constexpr int NP = NSPLIT == 3 ? 2 : 1;
    using TA = TileIO<true, 16>;
    using TB = TileIO<true, 16>;
    __shared__ __attribute__((aligned(16))) unsigned short As_all[KS * NP * TA::PLANE];
    __shared__ __attribute__((aligned(16))) unsigned short Bs_all[KS * G * NP * TB::PLANE];
    __shared__ f32x4 red[(KS == 2 ? 4 : 0) * 64 + 4 * 64];     // group 1's half of the K sum; then the gates on their way to wave 0
    const int grp = KS == 2 ? (int)(threadIdx.x >> 8) : 0;
    unsigned short* As = As_all + grp * NP * TA::PLANE;
    unsigned short* Bs = Bs_all + grp * G * NP * TB::PLANE;
    const int dir = blockIdx.y % P.ndir;
    const slnlp_rnn_step_dir d = as_global(dir == 0 ? P.d[0] : P.d[1]);
    const int tid = threadIdx.x & 255, lane = tid & 63, wave = tid >> 6;      // wave = gate
    const int B = P.B, Hd = P.Hd, j0 = blockIdx.x * 16, bm0 = (blockIdx.y / P.ndir) * 16;
    const int K = Hd, ktiles = (K + BKT - 1) / BKT;

    f32x4 acc = f32x4{0.f, 0.f, 0.f, 0.f};
    float4 ra[2][TA::NV], rb[2][G][TB::NV];
    auto fetch = [&](int kt, int slot) {
        TA::template fetch<true>(d.h_in, Hd, bm0, B, kt * BKT, K, tid, ra[slot]);
#pragma unroll
        for (int g = 0; g < G; ++g) TB::template fetch<true>(d.w_hh + (long)g * Hd * Hd, Hd, j0, Hd, kt * BKT, K, tid, rb[slot][g]);
    };
    auto stash = [&](int kt, int slot) {
        TA::template stash<NSPLIT, EDGE>(As, tid, ra[slot], bm0, B, kt * BKT, K);
#pragma unroll
        for (int g = 0; g < G; ++g) TB::template stash<NSPLIT, EDGE>(Bs + g * NP * TB::PLANE, tid, rb[slot][g], j0, Hd, kt * BKT, K);
    };
    auto consume = [&](int) {
        if (wave >= G) return;                                     // (GRU: three gates, the fourth wave only stages)
#pragma unroll
        for (int kk = 0; kk < 2; ++kk) {
            const bf16x8 ah = TA::frag(As, 0, kk, lane);
            bf16x8 al = ah;
            if (NSPLIT == 3) al = TA::frag(As + TA::PLANE, 0, kk, lane);
            const unsigned short* bt = Bs + wave * NP * TB::PLANE;
            const bf16x8 bh = TB::frag(bt, 0, kk, lane);
            bf16x8 bl = bh;
            if (NSPLIT == 3) bl = TB::frag(bt + TB::PLANE, 0, kk, lane);
            acc = mfma_split<NSPLIT>(ah, al, bh, bl, acc);
        }
    };
    // the cell's own operands are requested first (by the wave that will apply it), so their latency hides behind the K loop
    const int j = j0 + (lane & 15), jj = j < Hd ? j : 0;
    float bh[G], xpv[4][G], hpv[4], cpv[4];
    if (grp == 0 && wave == 0) {
#pragma unroll
        for (int g = 0; g < G; ++g) bh[g] = d.b_hh ? d.b_hh[g * Hd + jj] : 0.f;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int b = bm0 + ((lane >> 4) << 2) + r, bb = b < B ? b : 0;
#pragma unroll
            for (int g = 0; g < G; ++g) xpv[r][g] = d.xproj[(long)bb * G * Hd + g * Hd + jj];
            hpv[r] = d.h_in[(long)bb * Hd + jj];
            cpv[r] = LSTM ? d.c[(long)bb * Hd + jj] : 0.f;
        }
    }
    f32x4 acc_first = f32x4{0.f, 0.f, 0.f, 0.f};
    auto park = [&]() { acc_first = acc; acc = f32x4{0.f, 0.f, 0.f, 0.f}; };
    k_halves<KS>(ktiles, grp, fetch, stash, consume, park);
    if constexpr (KS == 1) {
        acc = acc_first + acc;
    } else {
        if (grp == 1) red[4 * 64 + wave * 64 + lane] = acc;
        __syncthreads();
        if (grp == 1) return;
        acc = acc + red[4 * 64 + wave * 64 + lane];
    }
    // the gates meet: wave g -> LDS -> wave 0
    red[wave * 64 + lane] = acc;
    lds_barrier();                                 // (KS = 2: group 1 has left; the barrier counts the waves that remain)
    if (wave != 0) return;
    f32x4 ga[G];
#pragma unroll
    for (int g = 0; g < G; ++g) ga[g] = red[g * 64 + lane];

    // ---- cell (rnn_cell.hpp)
    if (j >= Hd) return;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int b = bm0 + ((lane >> 4) << 2) + r;
        if (b >= B) break;
        float hp[G];
#pragma unroll
        for (int g = 0; g < G; ++g) hp[g] = ga[g][r] + bh[g];
        rnn_step_cell<LSTM>(P, d, b, j, xpv[r], hp, hpv[r], cpv[r]);
    }
}

// Every forward-step build, four per (precision, cell, EDGE): {64-row, 16-row re-tiled} x {KS 1, 2}
static const void* const* rnn_step_kernels() {
#define SLNLP_RS(NS, L, E) (const void*)rnn_step_fwd_kernel<NS, L, E, 1>, (const void*)rnn_step_fwd_kernel<NS, L, E, 2>, \
                           (const void*)rnn_step_fwd_rt_kernel<NS, L, E, 1>, (const void*)rnn_step_fwd_rt_kernel<NS, L, E, 2>
    static const void* const tab[32] = {SLNLP_RS(1, false, false), SLNLP_RS(1, false, true), SLNLP_RS(1, true, false), SLNLP_RS(1, true, true),
                                        SLNLP_RS(3, false, false), SLNLP_RS(3, false, true), SLNLP_RS(3, true, false), SLNLP_RS(3, true, true)};
#undef SLNLP_RS
    return tab;
}
static const void* rnn_step_kernel(int ns, bool lstm, bool edge, bool rt, int ks) {
    return rnn_step_kernels()[(ns == 3 ? 16 : 0) + (lstm ? 8 : 0) + (edge ? 4 : 0) + (rt ? 2 : 0) + (ks - 1)];
}
// slnlp_set_rnn_step_tile / SLNLP_RNN_STEP_RT=0: the 64-row tile for solo launches too (tests, A / B measurements; same bits)
static std::atomic<int> g_rnn_step_rt{[] { const char* e = getenv("SLNLP_RNN_STEP_RT"); return (e && atoi(e) == 0) ? 0 : 1; }()};
static bool rnn_step_rt_enabled() { return g_rnn_step_rt.load(std::memory_order_relaxed) != 0; }
// which tiling / thread groups a launch of `fits` timesteps [B x Hd, ndir directions] takes: the 16-row tile while it still fits the
// chip about twice over (a launch-latency chain: one fit), the 64-row tile (a third of the operand bytes in total) beyond
static void rnn_step_shape(int B, int Hd, int ndir, int fits, bool* rt, int* ks, dim3* grid) {
    const int gx = ceil_div(Hd, 16), rt_blocks = gx * ndir * ceil_div(B, 16) * fits;
    *rt = rnn_step_rt_enabled() && B > 16 && rt_blocks <= 512;
    *grid = dim3(gx, ndir * ceil_div(B, *rt ? 16 : BM));
    *ks = gemm_group_ks((int)(grid->x * grid->y) * fits, ceil_div(Hd, BKT));
}
// The kernel a MERGED launch of `fits` fits runs in place of the recorded forward-step kernel `fn` (nullptr: `fn` is not one of them):
// same results, the tiling and thread-group count of the merged size.  `grid`: in = the recorded (x, y), out = the merged one.
const void* rnn_step_fwd_for_blocks(const void* fn, const void* recorded_args, int fits, int* threads, dim3* grid) {
    for (int i = 0; i < 32; ++i)
        if (fn == rnn_step_kernels()[i]) {
            const RnnStepParams& P = *static_cast<const RnnStepParams*>(recorded_args);
            bool mrt;
            int mks;
            rnn_step_shape(P.B, P.Hd, P.ndir, fits, &mrt, &mks, grid);
            *threads = 256 * mks;
            return rnn_step_kernels()[(i & ~3) + (mrt ? 2 : 0) + (mks - 1)];     // same precision, cell and EDGE
        }
    return nullptr;
}

int rnn_step_fwd(int lstm, const slnlp_rnn_step_dir* dirs, int ndir, int B, int Hd, const int64_t* lengths, float fill,
                 int64_t ld_out, float drop_p, int drop_site, const unsigned long long* rng, int precision, hipStream_t st) {
    SLNLP_CHECK_ARG(dirs && (ndir == 1 || ndir == 2) && B > 0 && Hd > 0 && Hd % 4 == 0, "rnn_step_fwd: bad args (Hd %% 4 == 0)");
    SLNLP_CHECK_ARG(precision == 1 || precision == 3, "rnn_step_fwd: precision must be 1 or 3");
    SLNLP_CHECK_ARG(drop_p >= 0.f && drop_p < 1.f && (drop_p == 0.f || rng), "rnn_step_fwd: bad dropout args");
    RnnStepParams P;
    for (int k = 0; k < ndir; ++k) {
        const slnlp_rnn_step_dir& d = dirs[k];
        SLNLP_CHECK_ARG(d.h_in && d.h_out && d.h_in != d.h_out && d.w_hh && d.xproj && d.acts &&
                            (lstm ? (d.c && d.cprev_save) : (d.hn_save != nullptr)),
                        "rnn_step_fwd: null pointer (or h_in == h_out) in direction %d", k);
        SLNLP_CHECK_ARG(vec_ok(d.h_in, Hd) && vec_ok(d.w_hh, Hd), "rnn_step_fwd: h_in / w_hh must be 16-byte aligned");
        P.d[k] = d;
    }
    if (ndir == 1) P.d[1] = P.d[0];
    P.B = B; P.Hd = Hd; P.ndir = ndir; P.lengths = (const long*)lengths; P.fill = fill; P.ld_out = ld_out;
    P.drop_p = drop_p; P.drop_thr = dropout_threshold(drop_p); P.drop_site = drop_site; P.rng = rng;
    const bool edge = (Hd % BKT) != 0;
    // tile and thread groups for ONE fit's launch (a merged lockstep launch picks again for its size: rnn_step_fwd_for_blocks)
    bool rt;
    int ks;
    dim3 grid;
    rnn_step_shape(B, Hd, ndir, 1, &rt, &ks, &grid);
    const void* fn = rnn_step_kernel(precision, lstm != 0, edge, rt, ks);
    if (recording()) return record_op(fn, grid, dim3(256 * ks), 0, REC_Z, &P, sizeof(P), "rnn_step_fwd");
    const RnnStepParams* no_tab = nullptr;
    void* args[2] = {&P, &no_tab};
    if (hipLaunchKernel(fn, grid, dim3(256 * ks), args, 0, st) != hipSuccess) {
        set_error("rnn_step_fwd: %s", hipGetErrorString(hipGetLastError()));
        return SLNLP_ERR_LAUNCH;
    }
    return SLNLP_OK;
}

// ------------------------------------------------------- persistent recurrent layer ---
// ALL S timesteps of one bidirectional LSTM / GRU layer in ONE launch.  The per-timestep kernel above is ~5 us of
// launch latency plus a K loop that re-reads and re-converts the same W_hh slice 48 times; here a workgroup keeps its
// slice of W_hh (the G x 16 rows of its 16 hidden units, all K) in LDS as bf16 hi/lo for the whole sequence
// (128 KiB at Hd = 512) and only streams h_{t-1} per step.  The Hd/16 x ndir co-resident workgroups meet at a
// device-wide barrier between steps (sense-reversing counter, agent-scope atomics, bounded spin: 1.35 us for 64
// workgroups, tools/micro/grid_barrier.hip); the new state is written with sc1 (write-through) stores and drained
// before the barrier, and every h slot is written once and read only afterwards, so no workgroup can see a stale
// L1 / L2 line -- no fences (an agent-scope fence is a whole-L2 write-back on this part).
// Same K order and split as rnn_step_fwd_kernel -> bit-identical results.
// Measured (round 1): 13.9 us per timestep, no faster than the per-timestep launches (13.4 us) -- with one wave per SIMD
// the K loop (convert h_{t-1}, two block barriers per K tile, LDS fragment reads exposed in front of every MFMA group)
// costs ~8 us, and h_{t-1} arrives from the memory side.  It is therefore OPT-IN (slnlp_rnn_set_persistent); the plan
// for it: 8 waves (two per SIMD, gates split over wave pairs) and the state exchanged as bf16 planes via LDS-DMA.
struct RnnLayerParams {
    slnlp_rnn_layer_dir d[2];
    int B, Hd, S;
    const long* lengths;
    float fill;
    long ld_out;
    float drop_p;
    unsigned drop_thr;
    int drop_site;
    const unsigned long long* rng;
    unsigned* bar;      // {count, generation}
    int* err;
};

__device__ __forceinline__ void grid_barrier_sr(unsigned* bar, int* err, unsigned nblocks) {
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");            // this wave's sc1 stores have reached the memory side
    __syncthreads();
    if (threadIdx.x == 0) {
        const unsigned gen = __hip_atomic_load(bar + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (__hip_atomic_fetch_add(bar, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == nblocks - 1) {
            __hip_atomic_store(bar, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");    // the reset lands before anyone is released
            __hip_atomic_fetch_add(bar + 1, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        } else {
            long spins = 0;
            while (__hip_atomic_load(bar + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == gen) {
                __builtin_amdgcn_s_sleep(1);
                if (++spins > 4000000) { *err = 1; break; }     // never hang: flag the step as invalid and move on
            }
        }
    }
    __syncthreads();
}

template <int NSPLIT, bool LSTM>
__global__ __launch_bounds__(256) void rnn_layer_fwd_kernel(const RnnLayerParams P) {
    constexpr int G = LSTM ? 4 : 3;
    constexpr int NP = NSPLIT == 3 ? 2 : 1;
    using TA = TileIO<true, BM>;
    using TB = TileIO<true, 16>;
    extern __shared__ __attribute__((aligned(16))) unsigned short lsm[];
    const slnlp_rnn_layer_dir& d = P.d[blockIdx.y];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int B = P.B, Hd = P.Hd, S = P.S, j0 = blockIdx.x * 16, GH = G * Hd;
    const int K = Hd, ktiles = K / BKT;                          // host guarantees Hd % 64 == 0, B <= 64
    unsigned short* Wl = lsm;                                    // [ktile][gate][plane][16 x 64]
    unsigned short* As = lsm + (size_t)ktiles * G * NP * TB::PLANE;
    const unsigned nblocks = gridDim.x * gridDim.y;

    // ---- resident weight slice: rows g*Hd + j0 .. +15 of W_hh, every K tile, split once
    for (int kt = 0; kt < ktiles; ++kt)
#pragma unroll
        for (int g = 0; g < G; ++g) {
            float4 rw[TB::NV];
            TB::template fetch<true>(d.w_hh + (long)g * Hd * Hd, Hd, j0, Hd, kt * BKT, K, tid, rw);
            TB::template stash<NSPLIT, false>(Wl + ((size_t)kt * G + g) * NP * TB::PLANE, tid, rw, j0, Hd, kt * BKT, K);
        }
    const int j = j0 + (lane & 15);
    float bh[G];
#pragma unroll
    for (int g = 0; g < G; ++g) bh[g] = d.b_hh ? d.b_hh[g * Hd + j] : 0.f;
    const bool rev = d.reverse != 0;

    for (int step = 0; step < S; ++step) {
        const int t = rev ? S - 1 - step : step, tn = rev ? t - 1 : t + 1;
        const float* h_in = d.hprev + (long)t * B * Hd;
        float* h_out = step + 1 < S ? d.hprev + (long)tn * B * Hd : d.h_final;
        const float* xproj = d.xproj + (long)t * B * GH;
        // the cell's own operands first: their latency hides behind the K loop
        float xpv[4][G], hpv[4], cpv[4];
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int b = wave * 16 + ((lane >> 4) << 2) + r, bb = b < B ? b : 0;
#pragma unroll
            for (int g = 0; g < G; ++g) xpv[r][g] = xproj[(long)bb * GH + g * Hd + j];
            hpv[r] = h_in[(long)bb * Hd + j];
            cpv[r] = LSTM ? d.c[(long)bb * Hd + j] : 0.f;
        }
        f32x4 acc[G];
#pragma unroll
        for (int g = 0; g < G; ++g) acc[g] = f32x4{0.f, 0.f, 0.f, 0.f};
        float4 ra[2][TA::NV];
        auto fetch = [&](int kt, int slot) { TA::template fetch<true>(h_in, Hd, 0, B, kt * BKT, K, tid, ra[slot]); };
        auto stash = [&](int kt, int slot) { TA::template stash<NSPLIT, false>(As, tid, ra[slot], 0, B, kt * BKT, K); };
        auto consume = [&](int kt) {
#pragma unroll
            for (int kk = 0; kk < 2; ++kk) {
                const bf16x8 ah = TA::frag(As, wave * 16, kk, lane);
                bf16x8 al = ah;
                if (NSPLIT == 3) al = TA::frag(As + TA::PLANE, wave * 16, kk, lane);
#pragma unroll
                for (int g = 0; g < G; ++g) {
                    const unsigned short* bt = Wl + ((size_t)kt * G + g) * NP * TB::PLANE;
                    const bf16x8 bhf = TB::frag(bt, 0, kk, lane);
                    bf16x8 blf = bhf;
                    if (NSPLIT == 3) blf = TB::frag(bt + TB::PLANE, 0, kk, lane);
                    acc[g] = mfma_split<NSPLIT>(ah, al, bhf, blf, acc[g]);
                }
            }
        };
        f32x4 acc_first[G];
        auto park = [&]() {
#pragma unroll
            for (int g = 0; g < G; ++g) { acc_first[g] = acc[g]; acc[g] = f32x4{0.f, 0.f, 0.f, 0.f}; }
        };
        k_halves<1>(ktiles, 0, fetch, stash, consume, park);     // same halves as the per-timestep kernels
#pragma unroll
        for (int g = 0; g < G; ++g) acc[g] = acc_first[g] + acc[g];
        // ---- cell (rnn_cell.hpp)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int b = wave * 16 + ((lane >> 4) << 2) + r;
            if (b >= B) break;
            const long idx = (long)b * Hd + j;
            const bool valid = P.lengths ? (t < P.lengths[b]) : true;
            float hp[G];
#pragma unroll
            for (int g = 0; g < G; ++g) hp[g] = acc[g][r] + bh[g];
            const RnnCellFwd<LSTM> o = rnn_cell_fwd_elem<LSTM>(xpv[r], hp, hpv[r], cpv[r]);
            float* a = d.acts + (long)t * B * GH + (long)b * GH;
#pragma unroll
            for (int g = 0; g < G; ++g) a[g * Hd + j] = o.act[g];
            if constexpr (LSTM) {
                d.cprev[(long)t * B * Hd + idx] = cpv[r];
                d.c[idx] = valid ? o.cnew : cpv[r];
            } else {
                d.hn[(long)t * B * Hd + idx] = o.hn;
            }
            // the next step's workgroups (other XCDs) read this: write-through store
            __hip_atomic_store(h_out + idx, valid ? o.hnew : hpv[r], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            if (d.out)
                d.out[((long)t * B + b) * P.ld_out + j] = rnn_cell_out(valid, o.hnew, P.fill, P.drop_p, P.drop_thr, P.drop_site, P.rng,
                                                                       (unsigned)(t * B + b), (unsigned)(d.out_col0 + j));
        }
        if (step + 1 < S) grid_barrier_sr(P.bar, P.err, nblocks);
    }
}

// one-time opt-in to > 64 KiB dynamic LDS; called from plan creation so it never lands inside a graph capture
int rnn_layer_init() {
    static DeviceOnce once;                     // hipFuncSetAttribute applies per device
    return once.run([]() -> int {
    const int lim = 156 * 1024;
    const bool ok =
        hipFuncSetAttribute((const void*)rnn_layer_fwd_kernel<3, true>, hipFuncAttributeMaxDynamicSharedMemorySize, lim) == hipSuccess &&
        hipFuncSetAttribute((const void*)rnn_layer_fwd_kernel<3, false>, hipFuncAttributeMaxDynamicSharedMemorySize, lim) == hipSuccess &&
        hipFuncSetAttribute((const void*)rnn_layer_fwd_kernel<1, true>, hipFuncAttributeMaxDynamicSharedMemorySize, lim) == hipSuccess &&
        hipFuncSetAttribute((const void*)rnn_layer_fwd_kernel<1, false>, hipFuncAttributeMaxDynamicSharedMemorySize, lim) == hipSuccess;
    if (!ok) {
        set_error("rnn_layer_init: cannot raise dynamic LDS limit: %s", hipGetErrorString(hipGetLastError()));
        return SLNLP_ERR_LAUNCH;
    }
    return 0;
    });
}

static size_t rnn_layer_lds(int G, int Hd, int precision) {
    const int NP = precision == 3 ? 2 : 1;
    return ((size_t)(Hd / BKT) * G * NP * TileIO<true, 16>::PLANE + (size_t)NP * TileIO<true, BM>::PLANE) * sizeof(unsigned short);
}

// 0 = launched; 1 = shape not covered by the persistent kernel (caller uses the per-timestep path)
int rnn_layer_fwd(int lstm, const slnlp_rnn_layer_dir* dirs, int ndir, int B, int Hd, int S, const int64_t* lengths,
                  float fill, int64_t ld_out, float drop_p, int drop_site, const unsigned long long* rng, int precision,
                  unsigned* bar, int* err, int* launched, hipStream_t st) {
    SLNLP_CHECK_ARG(dirs && (ndir == 1 || ndir == 2) && B > 0 && Hd > 0 && S > 0 && bar && err && launched, "rnn_layer_fwd: bad args");
    SLNLP_CHECK_ARG(precision == 1 || precision == 3, "rnn_layer_fwd: precision must be 1 or 3");
    SLNLP_CHECK_ARG(drop_p >= 0.f && drop_p < 1.f && (drop_p == 0.f || rng), "rnn_layer_fwd: bad dropout args");
    const int G = lstm ? 4 : 3;
    const size_t lds = rnn_layer_lds(G, Hd, precision);
    *launched = 0;
    if (B > BM || Hd % BKT != 0 || lds > 156 * 1024 || (Hd / 16) * ndir > 128) return SLNLP_OK;   // not covered
    RnnLayerParams P;
    for (int k = 0; k < ndir; ++k) {
        const slnlp_rnn_layer_dir& d = dirs[k];
        SLNLP_CHECK_ARG(d.hprev && d.h_final && d.w_hh && d.xproj && d.acts && (lstm ? (d.c && d.cprev) : (d.hn != nullptr)),
                        "rnn_layer_fwd: null pointer in direction %d", k);
        SLNLP_CHECK_ARG(vec_ok(d.hprev, Hd) && vec_ok(d.w_hh, Hd) && ((long)B * Hd) % 4 == 0, "rnn_layer_fwd: hprev / w_hh must be 16-byte aligned");
        P.d[k] = d;
    }
    if (ndir == 1) P.d[1] = P.d[0];
    P.B = B; P.Hd = Hd; P.S = S; P.lengths = (const long*)lengths; P.fill = fill; P.ld_out = ld_out;
    P.drop_p = drop_p; P.drop_thr = dropout_threshold(drop_p); P.drop_site = drop_site; P.rng = rng;
    P.bar = bar; P.err = err;
    const dim3 grid(Hd / 16, ndir);
    SLNLP_TRY(rnn_layer_init());
#define SLNLP_LAYER(NS, L) hipLaunchKernelGGL((rnn_layer_fwd_kernel<NS, L>), grid, dim3(256), lds, st, P)
    if (precision == 3) { if (lstm) SLNLP_LAYER(3, true); else SLNLP_LAYER(3, false); }
    else { if (lstm) SLNLP_LAYER(1, true); else SLNLP_LAYER(1, false); }
#undef SLNLP_LAYER
    SLNLP_CHECK_LAUNCH("rnn_layer_fwd");
    *launched = 1;
    return SLNLP_OK;
}

}  // namespace slnlp

extern "C" int slnlp_rnn_layer_fwd(int lstm, const slnlp_rnn_layer_dir* dirs, int ndir, int B, int Hd, int S,
                                   const int64_t* lengths, float fill, int64_t ld_out, float drop_p, int drop_site,
                                   const unsigned long long* rng, int precision, uint32_t* sync, int* launched, void* stream) {
    if (!sync) {
        slnlp::set_error("slnlp_rnn_layer_fwd: sync words required");
        return SLNLP_ERR_INVALID_ARG;
    }
    return slnlp::rnn_layer_fwd(lstm, dirs, ndir, B, Hd, S, lengths, fill, ld_out, drop_p, drop_site, rng, precision, sync,
                                reinterpret_cast<int*>(sync + 2), launched, (hipStream_t)stream);
}

extern "C" int slnlp_rnn_step_bwd(int lstm, const slnlp_rnn_step_bwd_dir* dirs, int ndir, int B, int Hd, const int64_t* lengths,
                                  int64_t ld_dout, float drop_p, int drop_site, const unsigned long long* rng, int precision,
                                  void* stream) {
    return slnlp::rnn_step_bwd(lstm, dirs, ndir, B, Hd, lengths, ld_dout, drop_p, drop_site, rng, precision, (hipStream_t)stream);
}

extern "C" int slnlp_rnn_step_fwd(int lstm, const slnlp_rnn_step_dir* dirs, int ndir, int B, int Hd, const int64_t* lengths,
                                  float fill, int64_t ld_out, float drop_p, int drop_site, const unsigned long long* rng,
                                  int precision, void* stream) {
    return slnlp::rnn_step_fwd(lstm, dirs, ndir, B, Hd, lengths, fill, ld_out, drop_p, drop_site, rng, precision,
                               (hipStream_t)stream);
}

extern "C" int slnlp_set_rnn_step_tile(int rows16) {
    slnlp::g_rnn_step_rt.store(rows16 ? 1 : 0, std::memory_order_relaxed);
    return 0;
}
