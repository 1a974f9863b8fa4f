// bias_calibration.hip -- bias-corrected temperature calibration fitted on the device (the estimator's `calibration` option with
// method "bias_temperature"; include/slnlp.h states the algorithm, tests/bias_calibration_ref.py is its
// numpy restatement, line by line).
//
// theta = (beta, b_0 .. b_{V-1}): the calibrated probabilities are softmax(beta z + b) -- bias-corrected temperature scaling
// (Alexandari, Kundaje and Shrikumar 2020), the map slnlp_shift_logp applies with log_w = b.  With z float32 log-probs [N, ld] (V
// columns used), y int64 [N], M the rows whose label lies in [0, V), n_c their label frequencies, p_i = softmax(beta z_i + b) and
// m_i = sum_c p_ic z_ic, the objective is the MAP estimate under a N(0, bias_sd^2) prior on every bias:
//   F(theta) = mean_i [ logsumexp_c(beta z_ic + b_c) - beta z_iy - b_y ] + (lambda / 2) sum_c b_c^2      lambda = 1 / (bias_sd^2 M)
//   g_beta = mean_i (m_i - z_iy)                     g_b = mean_i p_i - n + lambda b
//   H_beta,beta = mean_i (sum_c p_ic z_ic^2 - m_i^2)   H_beta,b = mean_i p_i (z_i - m_i)   H_bb = diag(mean_i p_i + lambda) - P^T P / M
// F is jointly convex; the penalty also removes the softmax's free constant in b.  slnlp_fit_bias_temperature minimises F by a
// damped Newton iteration on the dense (V + 1) x (V + 1) system.  Everything but z itself is fp64.
//
// HOW IT RUNS.  The call queues a FIXED sequence of 48 evaluations plus the one at the result and never waits for the host.
// Evaluation e is five launches (the last two are not queued behind evaluation 47, the final one has the first three):
//   bias_rows     one wave per row, four rows per block, rows over a grid-stride loop (wave_rows, common.hpp): lanes stride the
//                 columns; the maximum and the sums are wave reductions in a fixed order; the wave writes p_i as fp64 into scratch
//                 [N, Vp] (Vp = V rounded up to 16, the padding zeros) and lane 0 the row terms (f_i, m_i - z_iy, h_i, m_i).  A row
//                 whose label lies outside the columns writes zeros.
//   bias_classes  one block of 256 threads per class c (prior_shift.hip's grid): thread t adds rows t, t + 256, ... in increasing
//                 order, then a fixed binary tree over the 256 partial sums in LDS: sum_i p_ic and sum_i p_ic (z_ic - m_i)
//                 (evaluation 0: n_c too).
//   bias_decide   ONE block: F and g of the evaluated point, the Armijo test, and the accept / halve / stop decision, taken by
//                 one thread and written as flags into `state`.
//   bias_hessian  P^T P over the 16 x 16 tiles of the lower triangle, one wave per tile with v_mfma_f64_16x16x4_f64; the K loop
//                 runs over the rows in increasing order, four per instruction.  Its epilogue writes H_bb into the system
//                 matrix.  Returns at once after a rejected candidate.
//   bias_solve    ONE block: the Cholesky factorisation in global memory (a 203 x 203 fp64 matrix does not fit LDS; panels of 8
//                 columns pass through it), the two triangular solves, g^T d, and the next candidate theta + t d; after a
//                 rejected candidate only t / 2 and the candidate.
// Every later launch reads the decision as a flag in `state`, so every block of every launch sees the same one; once the reason
// is set the launches return at once, the final evaluation always runs.  No atomics, every sum runs in an order that depends on N
// and V alone: the result is a pure function of the arguments.
//
// COST.  The Hessian is the only O(N V^2) work (1.6e8 fp64 FMAs at 4000 x 202); the factorisation is O(V^3 / 3) on one block.
// What is measured (tools/time_bias_calibration.py, profiles/bias_calibration_timing.json) is the whole queued sequence against
// slnlp_fit_temperature's and one valid pass over the same rows, and the Hessian launch alone.
#include <limits.h>
#include <math.h>

#include "block_reduce.hpp"
#include "common.hpp"
#include "fit_state.hpp"
#include "launch.hpp"
#include "spans.hpp"

namespace slnlp {

constexpr int BC_EVALS = 48;           // the evaluation cap (rejected candidates count)
constexpr int BC_FINAL = BC_EVALS;     // the evaluation at the result
constexpr int BC_MAX_V = SLNLP_BIAS_CAL_MAX_V;
constexpr double BC_BETA_MIN = 0.015625, BC_BETA_MAX = 64.0;      // 2^-6, 2^6
constexpr double BC_ARMIJO = 1e-4;
// state (fit_state.hpp; FIT_ITERATIONS counts the evaluations): the iteration's own doubles and words
enum { BC_F = 4, BC_STEP = 5, BC_GTD = 6, BC_LAMBDA = 7 };
enum { BC_NEED_H = 4, BC_HALVINGS = 5, BC_NEWTON = 6 };

typedef double bc_double4 __attribute__((ext_vector_type(4)));

// the slices of scratch, in doubles.  Vp = V rounded up to 16; W = Vp + 16 >= V + 1 is the stride of the vectors and of the system
// matrix, so every slice starts on a multiple of 128 bytes
struct BiasScratch {
    long Vp, W;
    long P, colS, colC, cnt, theta, cand, g, d, A, terms, doubles;
    BiasScratch(long N, long V) {
        Vp = (V + 15) & ~15L;
        W = Vp + 16;
        P = 0;
        colS = P + N * Vp;
        colC = colS + Vp;
        cnt = colC + Vp;
        theta = cnt + Vp;
        cand = theta + W;
        g = cand + W;
        d = g + W;
        A = d + W;
        terms = A + (V + 1) * W;
        doubles = terms + 4 * N;
    }
};

// a maximum that keeps a NaN (from arguments out of contract: the gradient test then fails)
__device__ __forceinline__ double bc_max_nan(double m, double o) { return o > m || o != o ? o : m; }

__device__ __forceinline__ void bias_rows_body(const float* __restrict__ logp, long ld, const int64_t* __restrict__ y, int N, int V, int Vp,
                                               const double* __restrict__ state, const double* __restrict__ cand, double* __restrict__ P,
                                               double* __restrict__ terms, int eval) {
    if (fit_settled(state, eval, 0, BC_FINAL)) return;
    const bool start = eval == 0;                        // the point (1, 0): cand holds nothing yet
    const double beta = start ? 1.0 : cand[0];
    const double* b = cand + 1;
    wave_rows(N, [&](long r, int lane) {
        const float* row = logp + r * ld;
        double* prow = P + r * Vp;
        const int64_t label = y[r];
        if (label < 0 || label >= V) {                   // (wave-uniform) never used as an index: the row adds nothing to any sum
            for (int j = lane; j < Vp; j += 64) prow[j] = 0.0;
            if (lane == 0) *(double4*)(terms + 4 * r) = make_double4(0.0, 0.0, 0.0, 0.0);
            return;
        }
        double amax = -INFINITY;
        for (int j = lane; j < V; j += 64) amax = fmax(amax, beta * (double)row[j] + (start ? 0.0 : b[j]));
        amax = wave_max_d(amax);
        // the columns AT the maximum have e = 1 exactly: counted, not summed, so that log1p keeps a confident row's digits
        double rest = 0.0, at_max = 0.0, s1 = 0.0, s2 = 0.0;
        for (int j = lane; j < V; j += 64) {
            const double z = (double)row[j];
            const double a = beta * z + (start ? 0.0 : b[j]);
            const double e = exp(a - amax);
            if (a == amax) at_max += 1.0; else rest += e;
            s1 += e * z;
            s2 += e * z * z;
            prow[j] = e;
        }
        rest = wave_sum_d(rest) + (wave_sum_d(at_max) - 1.0);
        const double s0 = 1.0 + rest;
        s1 = wave_sum_d(s1);
        s2 = wave_sum_d(s2);
        for (int j = lane; j < Vp; j += 64) prow[j] = j < V ? prow[j] / s0 : 0.0;      // each lane: the columns it wrote itself
        if (lane == 0) {
            const double zy = (double)row[label], mean = s1 / s0;
            const double ay = beta * zy + (start ? 0.0 : b[label]);
            *(double4*)(terms + 4 * r) = make_double4(log1p(rest) - (ay - amax), mean - zy, s2 / s0 - mean * mean, mean);
        }
    });
}
SLNLP_ZKERNEL(bias_rows_kernel, 256, bias_rows_body)

// sum_i p_ic, sum_i p_ic (z_ic - m_i) and, in evaluation 0, n_c: block c
__device__ __forceinline__ void bias_classes_body(const float* __restrict__ logp, long ld, const int64_t* __restrict__ y, int N, int Vp,
                                                  const double* __restrict__ state, const double* __restrict__ P,
                                                  const double* __restrict__ terms, double* __restrict__ colS, double* __restrict__ colC,
                                                  double* __restrict__ cnt, int eval) {
    if (fit_settled(state, eval, 0, BC_FINAL)) return;                 // (every thread reads the same flag: the block returns as one)
    __shared__ double red[3][256];
    const int tid = threadIdx.x;
    const long c = blockIdx.x;
    block_sum_rows<3>(red, tid, N, [&](long r, double* acc) {
        const double p = P[r * Vp + c];
        if (p != 0.0) {                                  // (an excluded row, or a column at -inf)
            acc[0] += p;
            acc[1] += p * ((double)logp[r * ld + c] - terms[4 * r + 3]);
        }
        if (eval == 0) acc[2] += y[r] == c ? 1.0 : 0.0;
    });
    if (tid != 0) return;
    colS[c] = red[0][0];
    colC[c] = red[1][0];
    if (eval == 0) cnt[c] = red[2][0];                   // whole numbers: exact
}
SLNLP_ZKERNEL(bias_classes_kernel, 256, bias_classes_body)

// F and g of the evaluated point, the first column of the system matrix, and the decision
__device__ __forceinline__ void bias_decide_body(const double* __restrict__ terms, const int64_t* __restrict__ y, const double* __restrict__ colS,
                                                 const double* __restrict__ colC, const double* __restrict__ cnt, int N, int V, int W,
                                                 double bias_sd, double tol, double* __restrict__ state, double* cand, double* theta,
                                                 double* __restrict__ g, double* __restrict__ A, double* __restrict__ bias, int eval) {
    if (fit_settled(state, eval, 0, BC_FINAL)) return;
    int64_t* q = fit_words(state);
    __shared__ double red[3][256];
    __shared__ int bad_red[256];
    __shared__ int action;
    const int tid = threadIdx.x;
    const bool start = eval == 0;
    double f = 0.0, gb = 0.0, h = 0.0;
    int bad = 0;
    for (long r = tid; r < N; r += 256) {                // (the first evaluation counts the bad labels along with the sums)
        const double4 t = *(const double4*)(terms + 4 * r);
        f += t.x; gb += t.y; h += t.z;
        if (start) {
            const int64_t label = y[r];
            bad += (label < 0 || label >= V) ? 1 : 0;
        }
    }
    red[0][tid] = f; red[1][tid] = gb; red[2][tid] = h;
    block_tree<3>(red, tid, TreeSum{});
    f = red[0][0]; gb = red[1][0]; h = red[2][0];
    long M;
    if (start) {
        bad_red[tid] = bad;
        block_tree<1>(&bad_red, tid, TreeSum{});
        M = (long)N - bad_red[0];
    } else {
        M = q[FIT_ROWS];
    }
    __syncthreads();                                     // red is rewritten below: every thread has read it
    const double inv = M > 0 ? 1.0 / (double)M : 0.0;
    const double lam = M > 0 ? 1.0 / (bias_sd * bias_sd * (double)M) : 0.0;
    double gm = 0.0, pen = 0.0;
    for (int c = tid; c < V; c += 256) {
        const double bc = start ? 0.0 : cand[1 + c];
        const double gc = (colS[c] * inv - cnt[c] * inv) + lam * bc;
        g[1 + c] = gc;
        A[(long)(1 + c) * W] = colC[c] * inv;            // H_beta,b: read only when this point is accepted
        gm = bc_max_nan(gm, fabs(gc));
        pen += bc * bc;
    }
    red[0][tid] = gm; red[1][tid] = pen;
    block_tree<1>(&red[0], tid, [](double m, double o) { return bc_max_nan(m, o); });
    block_tree<1>(&red[1], tid, TreeSum{});
    // what the block does next -- 0: the candidate is rejected; 1: accepted, the iteration goes on; 2: accepted and the search
    // ends at it; 3: rejected and the search ends at theta; 4: the final evaluation
    if (tid == 0) {
        int act;
        const double nll = f * inv;
        if (eval == BC_FINAL) {
            state[FIT_F_AFTER] = nll;
            act = 4;
        } else {
            const double F = nll + 0.5 * lam * red[1][0], gbeta = gb * inv;
            const double gmax = bc_max_nan(red[0][0], fabs(gbeta));
            g[0] = gbeta;
            A[0] = h * inv;
            if (start) {
                fit_state_reset(state, M, (long)N - M);
                state[FIT_F_BEFORE] = nll;
                state[BC_LAMBDA] = lam;
            }
            if (start && (M == 0 || V == 1)) {           // nothing to fit: (1, 0)
                q[FIT_REASON] = SLNLP_CAL_FLAT;
                act = 2;
            } else {
                q[FIT_ITERATIONS] = eval + 1;
                const bool accept = start || F <= state[BC_F] + BC_ARMIJO * state[BC_STEP] * state[BC_GTD];     // (a NaN is rejected)
                if (accept) {
                    state[BC_F] = F;
                    if (gmax <= tol) { q[FIT_REASON] = SLNLP_CAL_GRADIENT; act = 2; }
                    else if (eval == BC_EVALS - 1) { q[FIT_REASON] = SLNLP_CAL_CAP; act = 2; }
                    else { q[BC_NEED_H] = 1; act = 1; }
                } else {
                    q[BC_HALVINGS] += 1;
                    if (eval == BC_EVALS - 1) { q[FIT_REASON] = SLNLP_CAL_CAP; act = 3; }
                    else { q[BC_NEED_H] = 0; act = 0; }
                }
            }
        }
        action = act;
    }
    __syncthreads();
    const int act = action;
    if (act == 0 || act == 4) return;
    for (int i = tid; i <= V; i += 256) {                // entry i is read and written by one thread
        const double v = act == 3 ? theta[i] : start ? (i == 0 ? 1.0 : 0.0) : cand[i];
        theta[i] = v;
        if (act == 1) continue;
        cand[i] = v;                                     // the final evaluation runs at the result
        fit_result(state, bias, i, v);
    }
}
SLNLP_ZKERNEL(bias_decide_kernel, 256, bias_decide_body)

// tile (I, J), J <= I, of P^T P: one wave.  v_mfma_f64_16x16x4_f64: lane l holds A[row l & 15][k = l >> 4] and B[k = l >> 4][col
// l & 15]; of the four results of a lane, register v is D[row (l >> 4) + 4 v][col l & 15] -- not the other shapes' layout.
__device__ __forceinline__ void bias_hessian_body(const double* __restrict__ P, const double* __restrict__ colS, int N, int V, int Vp, int W,
                                                  const double* __restrict__ state, double* __restrict__ A) {
    const int64_t* q = fit_words(state);
    if (fit_settled(state) || q[BC_NEED_H] == 0) return;
    int I = 0;
    while ((I + 1) * (I + 2) / 2 <= (int)blockIdx.x) ++I;
    const int J = (int)blockIdx.x - I * (I + 1) / 2;
    const int lane = threadIdx.x & 63, k = lane >> 4, cc = lane & 15;
    const double* pa = P + 16 * I + cc;
    const double* pb = P + 16 * J + cc;
    bc_double4 acc = {0.0, 0.0, 0.0, 0.0};
    long r0 = 0;                                         // the rows in increasing order, four per instruction
    for (; r0 + 16 <= N; r0 += 16) {                     // sixteen rows' loads in flight in front of their four instructions
        double a[4], b[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            a[u] = pa[(r0 + 4 * u + k) * Vp];
            b[u] = pb[(r0 + 4 * u + k) * Vp];
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) acc = __builtin_amdgcn_mfma_f64_16x16x4f64(a[u], b[u], acc, 0, 0, 0);
    }
    for (; r0 < N; r0 += 4) {
        const long r = r0 + k;
        const double a = r < N ? pa[r * Vp] : 0.0;
        const double b = r < N ? pb[r * Vp] : 0.0;
        acc = __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, acc, 0, 0, 0);
    }
    const double M = (double)q[FIT_ROWS], inv = 1.0 / M, lam = state[BC_LAMBDA];
#pragma unroll
    for (int v = 0; v < 4; ++v) {
        const int row = 16 * I + k + 4 * v, col = 16 * J + cc;
        if (row < V && col <= row) A[(long)(1 + row) * W + 1 + col] = (row == col ? colS[row] * inv + lam : 0.0) - acc[v] * inv;
    }
}
SLNLP_ZKERNEL(bias_hessian_kernel, 64, bias_hessian_body)

// d = -H^-1 g by Cholesky (after an accepted point) or t / 2 (after a rejected one), then the candidate theta + t d.
// The factorisation is right-looking in panels of BC_NB columns: a panel (the rows below it included) is loaded into LDS, factorised
// there, written back, and the trailing lower triangle takes its rank-BC_NB update in one pass over global memory -- every element
// still receives its subtractions in increasing k, the unblocked algorithm's order, at an eighth of the round trips.
constexpr int BC_NB = 8, BC_PAD = BC_NB + 1, BC_SYS_MAX = BC_MAX_V + 16;      // (the padded row keeps a tile's 16 rows off one bank)
__device__ __forceinline__ void bias_solve_body(double* A, const double* __restrict__ g, const double* theta, double* cand, double* d, int V,
                                                int W, double* __restrict__ state, double* __restrict__ bias) {
    int64_t* q = fit_words(state);
    if (fit_settled(state)) return;
    __shared__ double pan[BC_SYS_MAX * BC_PAD], rhs[BC_SYS_MAX];
    __shared__ double red[256];
    __shared__ double step;
    const int tid = threadIdx.x, tx = tid & 15, ty = tid >> 4;
    const int n = V + 1;
    if (q[BC_NEED_H] != 0) {
        for (int i = tid; i < n; i += 256) rhs[i] = -g[i];
        bool positive = true;
        for (int kb = 0; kb < n && positive; kb += BC_NB) {
            const int nb = min(BC_NB, n - kb), m = n - kb;
            // the panel: rows kb .. n - 1 of columns kb .. kb + nb - 1, on and below the diagonal
            for (int e = tid; e < m * BC_NB; e += 256) {
                const int i = e / BC_NB, c = e % BC_NB;
                if (c < nb && c <= i) pan[i * BC_PAD + c] = A[(long)(kb + i) * W + kb + c];
            }
            __syncthreads();                             // (also: rhs is in place before the first panel reads it)
            for (int c = 0; c < nb; ++c) {               // the forward solve L w = -g rides along
                const double piv = pan[c * BC_PAD + c];  // (every thread reads the same value: the block leaves as one)
                if (!(piv > 0.0)) { positive = false; break; }
                const double l = sqrt(piv);
                for (int i = c + 1 + tid; i < m; i += 256) pan[i * BC_PAD + c] /= l;
                __syncthreads();                         // every thread has read the pivot
                if (tid == 0) {
                    pan[c * BC_PAD + c] = l;
                    rhs[kb + c] = rhs[kb + c] / l;
                }
                __syncthreads();
                const double wk = rhs[kb + c];
                for (int i = c + 1 + tid; i < m; i += 256) {         // row i of the panel belongs to one thread
                    const double li = pan[i * BC_PAD + c];
                    rhs[kb + i] -= li * wk;
                    for (int c2 = c + 1; c2 < nb && c2 <= i; ++c2) pan[i * BC_PAD + c2] -= li * pan[c2 * BC_PAD + c];
                }
                __syncthreads();
            }
            if (!positive) break;
            for (int e = tid; e < m * BC_NB; e += 256) {
                const int i = e / BC_NB, c = e % BC_NB;
                if (c < nb && c <= i) A[(long)(kb + i) * W + kb + c] = pan[i * BC_PAD + c];
            }
            // the trailing lower triangle in 16 x 16 tiles: tx the column, ty the row; four tiles' loads in front of their stores
            // (a panel narrower than BC_NB is the last one: nothing trails it)
            const int base = kb + BC_NB, mt = base < n ? (n - base + 15) >> 4 : 0;
            for (int jt = 0; jt < mt; ++jt) {
                const int j = base + 16 * jt + tx;
                double lj[BC_NB];
#pragma unroll
                for (int c = 0; c < BC_NB; ++c) lj[c] = j < n ? pan[(j - kb) * BC_PAD + c] : 0.0;
                for (int it = jt; it < mt; it += 4) {
                    double v[4];
#pragma unroll
                    for (int u = 0; u < 4; ++u) {
                        const int i = base + 16 * (it + u) + ty;
                        v[u] = (i < n && j <= i) ? A[(long)i * W + j] : 0.0;
                    }
#pragma unroll
                    for (int u = 0; u < 4; ++u) {
                        const int i = base + 16 * (it + u) + ty;
                        if (i < n && j <= i) {
                            double acc = v[u];
#pragma unroll
                            for (int c = 0; c < BC_NB; ++c) acc -= pan[(i - kb) * BC_PAD + c] * lj[c];
                            A[(long)i * W + j] = acc;
                        }
                    }
                }
            }
            __syncthreads();
        }
        if (!positive) {                                 // cannot happen in exact arithmetic: reported, not patched
            for (int i = tid; i <= V; i += 256) {
                const double v = theta[i];
                cand[i] = v;
                fit_result(state, bias, i, v);
                if (i == 0) q[FIT_REASON] = SLNLP_CAL_PIVOT;
            }
            return;
        }
        for (int kb = ((n - 1) / BC_NB) * BC_NB; kb >= 0; kb -= BC_NB) {      // L^T d = w, BC_NB rows of L at a time through LDS
            const int nb = min(BC_NB, n - kb);
            for (int r = 0; r < nb; ++r)
                for (int i = tid; i <= kb + r; i += 256) pan[r * BC_SYS_MAX + i] = A[(long)(kb + r) * W + i];
            __syncthreads();
            for (int c = nb - 1; c >= 0; --c) {
                const int k = kb + c;
                if (tid == 0) rhs[k] = rhs[k] / pan[c * BC_SYS_MAX + k];
                __syncthreads();
                const double dk = rhs[k];
                for (int i = tid; i < k; i += 256) rhs[i] -= pan[c * BC_SYS_MAX + i] * dk;
                __syncthreads();
            }
        }
        double s = 0.0;
        for (int i = tid; i < n; i += 256) {
            d[i] = rhs[i];
            s += g[i] * rhs[i];
        }
        red[tid] = s;
        block_tree<1>(&red, tid, TreeSum{});
        if (tid == 0) {
            state[BC_GTD] = red[0];
            q[BC_NEWTON] += 1;
        }
    } else {
        for (int i = tid; i < n; i += 256) rhs[i] = d[i];
    }
    if (tid == 0) {
        double t = q[BC_NEED_H] != 0 ? 1.0 : 0.5 * state[BC_STEP];
        const double b0 = theta[0], db = rhs[0];
        while (t > 0.0 && !(b0 + t * db >= BC_BETA_MIN && b0 + t * db <= BC_BETA_MAX)) {   // the box costs no evaluation
            t *= 0.5;
            q[BC_HALVINGS] += 1;
        }
        state[BC_STEP] = t;
        step = t;
    }
    __syncthreads();
    const double t = step;
    for (int i = tid; i < n; i += 256) cand[i] = theta[i] + t * rhs[i];
}
SLNLP_ZKERNEL(bias_solve_kernel, 256, bias_solve_body)

int64_t fit_bias_temperature_scratch_bytes(int64_t N, int64_t V) {
    if (N < 1 || N > INT_MAX || V < 1 || V > BC_MAX_V) {
        set_error("fit_bias_temperature_scratch_bytes: N=%ld outside 1..%d or V=%ld outside 1..%d", (long)N, INT_MAX, (long)V, BC_MAX_V);
        return -1;
    }
    return BiasScratch(N, V).doubles * 8;
}

int fit_bias_temperature(const float* logp, int64_t ld, const int64_t* y, int64_t N, int64_t V, double bias_sd, double tol, void* state,
                         double* bias, void* scratch, int64_t scratch_bytes, hipStream_t st) {
    SLNLP_CHECK_ARG(logp && y && state && bias && scratch, "fit_bias_temperature: null pointer");
    Span z;
    SLNLP_TRY(check_logp_matrix("fit_bias_temperature", logp, N, INT_MAX, V, BC_MAX_V, ld, &z));
    SLNLP_CHECK_ARG(bias_sd > 0.0 && bias_sd < INFINITY, "fit_bias_temperature: bias_sd=%g is not a finite number > 0", bias_sd);
    SLNLP_CHECK_ARG(tol >= 0.0 && tol < INFINITY, "fit_bias_temperature: tol=%g is not a finite number >= 0", tol);
    const BiasScratch L(N, V);
    const size_t need = (size_t)L.doubles * 8;
    SLNLP_TRY(check_scratch("fit_bias_temperature", scratch, scratch_bytes, need, N, V, 32));
    SLNLP_CHECK_ARG(((uintptr_t)logp & 3) == 0 && (((uintptr_t)y | (uintptr_t)state | (uintptr_t)bias) & 7) == 0,
                    "fit_bias_temperature: misaligned pointer (logp: 4 bytes; y, state, bias: 8 bytes)");
    const Span out[3] = {{state, SLNLP_CAL_STATE_BYTES, "state"}, {bias, (size_t)V * 8, "bias"}, {scratch, need, "scratch"}};
    const Span in[2] = {z, {y, (size_t)N * 8, "y"}};
    SLNLP_TRY(check_no_overlap("fit_bias_temperature", out, in));
    double* s = (double*)scratch;
    double *P = s + L.P, *colS = s + L.colS, *colC = s + L.colC, *cnt = s + L.cnt, *theta = s + L.theta, *cand = s + L.cand, *g = s + L.g,
           *d = s + L.d, *A = s + L.A, *terms = s + L.terms;
    const int Vp = (int)L.Vp, W = (int)L.W, T = Vp / 16;
    const int blocks = wave_rows_grid(N);
    for (int eval = 0; eval <= BC_FINAL; ++eval) {
        SLNLP_TRY(zlaunch(bias_rows_kernel, dim3(blocks), 256, 0, st, "fit_bias_temperature_rows", logp, (long)ld, y, (int)N, (int)V, Vp,
                          (const double*)state, (const double*)cand, P, terms, eval));
        SLNLP_TRY(zlaunch(bias_classes_kernel, dim3((unsigned)V), 256, 0, st, "fit_bias_temperature_classes", logp, (long)ld, y, (int)N, Vp,
                          (const double*)state, (const double*)P, (const double*)terms, colS, colC, cnt, eval));
        SLNLP_TRY(zlaunch(bias_decide_kernel, dim3(1), 256, 0, st, "fit_bias_temperature_decide", (const double*)terms, y, (const double*)colS,
                          (const double*)colC, (const double*)cnt, (int)N, (int)V, W, bias_sd, tol, (double*)state, cand, theta, g, A, bias,
                          eval));
        if (eval >= BC_EVALS - 1) continue;              // no candidate follows the last evaluation
        SLNLP_TRY(zlaunch(bias_hessian_kernel, dim3((unsigned)(T * (T + 1) / 2)), 64, 0, st, "fit_bias_temperature_hessian", (const double*)P,
                          (const double*)colS, (int)N, (int)V, Vp, W, (const double*)state, A));
        SLNLP_TRY(zlaunch(bias_solve_kernel, dim3(1), 256, 0, st, "fit_bias_temperature_solve", A, (const double*)g, (const double*)theta, cand,
                          d, (int)V, W, (double*)state, bias));
    }
    return 0;
}

}  // namespace slnlp

extern "C" int64_t slnlp_fit_bias_temperature_scratch_bytes(int64_t N, int64_t V) { return slnlp::fit_bias_temperature_scratch_bytes(N, V); }

extern "C" int slnlp_fit_bias_temperature(const float* logp, int64_t ld, const int64_t* y, int64_t N, int64_t V, double bias_sd, double tol,
                                          void* state, double* bias, void* scratch, int64_t scratch_bytes, void* stream) {
    return slnlp::fit_bias_temperature(logp, ld, y, N, V, bias_sd, tol, state, bias, scratch, scratch_bytes, (hipStream_t)stream);
}
