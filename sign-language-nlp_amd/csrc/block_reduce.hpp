// block_reduce.hpp -- the fixed binary tree over the 256 threads of a block, in LDS.  The judging kernels'
// "a fixed binary tree adds the 256 threads" is this one loop: level w (128, 64, .. 1) gives thread t < w the combine of cells t and
// t + w, so the order of the combines depends on nothing but the thread index and a sum's bits are a function of the 256 inputs.
#pragma once
#include <hip/hip_runtime.h>

namespace slnlp {

struct TreeSum {
    template <class T>
    __device__ __forceinline__ T operator()(T mine, T other) const { return mine + other; }
};

// red[h][t] holds thread t's input of reduction h (H of them share the levels and their barriers); afterwards red[h][0] = the
// tree's result, the other cells are spent.  op(mine, other) with mine = cell t, other = cell t + w.  BARRIERS INSIDE: one in front
// of the tree (the caller's stores to red need none of their own) and one per level, so the last also covers the caller's read of
// red[h][0]; every thread of the block must reach the call (block-uniform control flow only).  A caller that rewrites red
// afterwards puts its own barrier behind its read.  A one-dimensional `T red[256]` is passed as &red with H = 1.
template <int H, class T, class Op>
__device__ __forceinline__ void block_tree(T (*red)[256], int tid, Op op) {
    __syncthreads();
    for (int w = 128; w >= 1; w >>= 1) {
        if (tid < w) {
#pragma unroll
            for (int h = 0; h < H; ++h) red[h][tid] = op(red[h][tid], red[h][tid + w]);
        }
        __syncthreads();
    }
}

// "thread t adds rows t, t + 256, ... in increasing order, then the tree": f(r, acc) adds row r's terms to acc[0 .. H), and
// red[h][0] is sum h afterwards -- an order that depends on n alone.  block_tree's barriers and rules.
template <int H, class T, class F>
__device__ __forceinline__ void block_sum_rows(T (*red)[256], int tid, long n, F f) {
    T acc[H] = {};
    for (long r = tid; r < n; r += 256) f(r, acc);
#pragma unroll
    for (int h = 0; h < H; ++h) red[h][tid] = acc[h];
    block_tree<H>(red, tid, TreeSum{});
}

}  // namespace slnlp
