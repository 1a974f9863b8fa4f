// mfma_tile.hpp -- the split-bf16 MFMA tile toolkit shared by the fp32-operand GEMM (gemm.hip) and the fused recurrent
// kernels (rnn_step.hip): fp32 tiles go from HBM to registers (fetch), as bf16 hi (+ lo) planes into LDS (stash), and out of
// LDS as v_mfma_f32_16x16x32_bf16 operand fragments (frag).  The layouts and the reasons for them are in gemm.hip's header.
#pragma once
#include "common.hpp"

namespace slnlp {

typedef __attribute__((ext_vector_type(8))) __bf16 bf16x8;
typedef __attribute__((ext_vector_type(4))) short s16x4;
typedef __attribute__((ext_vector_type(8))) short s16x8;
typedef __attribute__((ext_vector_type(4))) float f32x4;

constexpr int BM = 64, BKT = 64;
constexpr int KLD = BKT;      // [row][k] image: 64 bf16 = 128-B rows, 16-B slots XOR-swizzled by (row & 7)

// element offset of (row, k) in the k-major image.  The mixed-row lane groups of ds_read_b128
// ({0-3,12-15,20-27}, ...) hit 16 distinct 16-B slots of the 256-B bank row with this swizzle;
// a padded stride cannot do that (the g=1 slots are the g=0 slots shifted by one).
__device__ __forceinline__ int kmaj_off(int row, int k) { return row * KLD + ((((k >> 3) ^ (row & 7)) << 3) | (k & 7)); }

__device__ __forceinline__ unsigned short f2bf(float x) {
    __bf16 b = (__bf16)x;
    return __builtin_bit_cast(unsigned short, b);
}
__device__ __forceinline__ float bf2f(unsigned short h) { return __uint_as_float(((unsigned)h) << 16); }

// One operand tile = ROWS x 64(k) fp32.  NV float4 per thread.
//  KMAJOR: element (row,k) at P + row*ld + k; float4 runs along k; 16 float4 per row.
// !KMAJOR: element (row,k) at P + k*ld + row; float4 runs along row; ROWS/4 float4 per k.
template <bool KMAJOR, int ROWS>
struct TileIO {
    static constexpr int NV = ROWS * BKT / 4 / 256;       // 4 (ROWS=64), 2 (ROWS=32) or 1 (ROWS=16)
    static constexpr int MLD = ROWS + 8;                  // [k][row] image row stride (bf16)
    static constexpr int PLANE = KMAJOR ? ROWS * KLD : BKT * MLD;

    __device__ static __forceinline__ void coords(int idx, int& row, int& k) {
        if (KMAJOR) { row = idx >> 4; k = (idx & 15) << 2; }
        else { k = idx / (ROWS / 4); row = (idx % (ROWS / 4)) << 2; }
    }

    // Issue the loads of one K-tile.  Branch-free and with NO use of the loaded values: any use here
    // (even zeroing a tail lane) makes hipcc wait vmcnt(0) right behind each load and serialises the
    // whole prefetch.  Out-of-range coordinates are clamped to a valid address; stash() zeroes them.
    template <bool VEC>
    __device__ static __forceinline__ void fetch(const float* __restrict__ P, long ld, int row0, int nrows,
                                                 int k0, int K, int tid, float4 (&r)[NV]) {
#pragma unroll
        for (int u = 0; u < NV; ++u) {
            int row, k;
            coords(tid + 256 * u, row, k);
            row += row0;
            k += k0;
            if (VEC) {   // compile-time: the hot kernel has no control flow around its loads
                const int rc = row < nrows ? row : 0, kc = k < K ? k : 0;
                r[u] = *reinterpret_cast<const float4*>(KMAJOR ? P + (long)rc * ld + kc : P + (long)kc * ld + rc);
            } else {
                float x[4];
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    int rr = KMAJOR ? row : row + e, kk = KMAJOR ? k + e : k;
                    rr = rr < nrows ? rr : 0;
                    kk = kk < K ? kk : 0;
                    x[e] = KMAJOR ? P[(long)rr * ld + kk] : P[(long)kk * ld + rr];
                }
                r[u] = make_float4(x[0], x[1], x[2], x[3]);
            }
        }
    }

    // fp32 -> bf16 hi (+ lo) and store into the LDS image.  hi is the TRUNCATED upper half of the
    // fp32 word (1 VALU op instead of a round-to-nearest convert); x - hi is exact in fp32 and
    // lo = rne_bf16(x - hi) absorbs the truncation, so hi + lo still represents x to ~2^-16.
    // EDGE = false: interior tile, no bounds masks at all.
    template <int NSPLIT, bool EDGE>
    __device__ static __forceinline__ void stash(unsigned short* __restrict__ T, int tid, const float4 (&r)[NV],
                                                 int row0, int nrows, int k0, int K) {
        typedef __attribute__((ext_vector_type(2))) float f32x2;
        typedef __attribute__((ext_vector_type(2))) __bf16 bf16x2;
#pragma unroll
        for (int u = 0; u < NV; ++u) {
            int row, k;
            coords(tid + 256 * u, row, k);
            float x[4] = {r[u].x, r[u].y, r[u].z, r[u].w};
            if (EDGE) {
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const int rr = row0 + (KMAJOR ? row : row + e), kk = k0 + (KMAJOR ? k + e : k);
                    if (!(rr < nrows && kk < K)) x[e] = 0.f;      // edge / K-tail zero fill (v_cndmask)
                }
            }
            const int off = KMAJOR ? kmaj_off(row, k) : k * MLD + row;   // both 8-B aligned
            unsigned ub[4];
#pragma unroll
            for (int e = 0; e < 4; ++e) ub[e] = __float_as_uint(x[e]);
            uint2 w;
            if (NSPLIT == 3) {
                w.x = (ub[0] >> 16) | (ub[1] & 0xFFFF0000u);
                w.y = (ub[2] >> 16) | (ub[3] & 0xFFFF0000u);
                *reinterpret_cast<uint2*>(T + off) = w;
                float lo[4];
#pragma unroll
                for (int e = 0; e < 4; ++e) lo[e] = x[e] - __uint_as_float(ub[e] & 0xFFFF0000u);
                const bf16x2 l01 = __builtin_convertvector(f32x2{lo[0], lo[1]}, bf16x2);
                const bf16x2 l23 = __builtin_convertvector(f32x2{lo[2], lo[3]}, bf16x2);
                w.x = __builtin_bit_cast(unsigned, l01);
                w.y = __builtin_bit_cast(unsigned, l23);
                *reinterpret_cast<uint2*>(T + PLANE + off) = w;
            } else {   // single pass: round to nearest
                const bf16x2 h01 = __builtin_convertvector(f32x2{x[0], x[1]}, bf16x2);
                const bf16x2 h23 = __builtin_convertvector(f32x2{x[2], x[3]}, bf16x2);
                w.x = __builtin_bit_cast(unsigned, h01);
                w.y = __builtin_bit_cast(unsigned, h23);
                *reinterpret_cast<uint2*>(T + off) = w;
            }
        }
    }

    // MFMA 16x16x32 operand fragment of tile rows [r0, r0+16), k in [kk*32, kk*32+32):
    // lane l holds (row r0 + (l&15), k = kk*32 + 8*(l>>4) + j), j = 0..7.
    __device__ static __forceinline__ bf16x8 frag(const unsigned short* __restrict__ T, int r0, int kk, int lane) {
        if (KMAJOR) {
            return *reinterpret_cast<const bf16x8*>(T + kmaj_off(r0 + (lane & 15), kk * 32 + ((lane >> 4) << 3)));
        } else {
            // transposing read: lane (i = l&15; q = i>>2, p = i&3) addresses k-row q, columns 4p..4p+3 of a
            // 4(k) x 16(row) block and receives the 4 k-values of column i.
            const int i = lane & 15, kb = kk * 32 + ((lane >> 4) << 3) + (i >> 2);
            const unsigned short* p0 = T + kb * MLD + r0 + ((i & 3) << 2);
            typedef __attribute__((address_space(3))) s16x4* lds_p;
            const s16x4 v0 = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_p)(p0));
            const s16x4 v1 = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_p)(p0 + 4 * MLD));
            const s16x8 v = {v0[0], v0[1], v0[2], v0[3], v1[0], v1[1], v1[2], v1[3]};
            return __builtin_bit_cast(bf16x8, v);
        }
    }

    // bf16(hi)+bf16(lo) value of tile element (row, k) -- for the fused bias-gradient row sums
    template <int NSPLIT>
    __device__ static __forceinline__ float value(const unsigned short* __restrict__ T, int row, int k) {
        const int off = KMAJOR ? kmaj_off(row, k) : k * MLD + row;
        float v = bf2f(T[off]);
        if (NSPLIT == 3) v += bf2f(T[PLANE + off]);
        return v;
    }
};

// Workgroup barrier that orders LDS traffic only.  __syncthreads() also emits s_waitcnt vmcnt(0),
// which would drain the register prefetch of the next two K-tiles at every step.
__device__ __forceinline__ void lds_barrier() {
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
    asm volatile("" ::: "memory");
}

// acc += A * B on operand fragments held as bf16 hi (+ lo) planes.  The order IS the result: Alo*Bhi, then Ahi*Blo, then
// Ahi*Bhi (NSPLIT == 1: Ahi*Bhi alone; al / bl are not read).  Every kernel that promises the bits of another takes its
// products through here.
template <int NSPLIT>
__device__ __forceinline__ f32x4 mfma_split(bf16x8 ah, bf16x8 al, bf16x8 bh, bf16x8 bl, f32x4 acc) {
    if (NSPLIT == 3) {
        acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(al, bh, acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ah, bl, acc, 0, 0, 0);
    }
    return __builtin_amdgcn_mfma_f32_16x16x32_bf16(ah, bh, acc, 0, 0, 0);
}

// 16-byte vector loads are legal for this operand
static inline bool vec_ok(const float* ptr, long ld) {
    return (ld % 4 == 0) && ((reinterpret_cast<uintptr_t>(ptr) & 15) == 0);
}

}  // namespace slnlp
