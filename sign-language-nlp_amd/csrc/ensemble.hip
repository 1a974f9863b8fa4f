// ensemble.hip -- K fits' log-probs combined on the device into one set of log-probs, with the per-row uncertainty decomposition
// (slnlp/ops.py's ensemble_rows, slnlp/ensemble.py's VotingEnsemble).
//
// Member k: z_k float32 log-probs [N, ld_k] (V columns used), beta_k = beta_dev[k] ? beta_dev[k][0] : 1 (a calibration state's first
// double, read on the device), w_k > 0 with sum w_k = 1 (normalised on the host in fp64).  Per row, all in fp64 but z itself:
//   member term   scale_logp's expression before its rounding, with a_k and rest_k = sum e - 1 from the row head of logp_row.hpp:
//                 l_kc = (beta_k z_kc - a_k) - log1p(rest_k),  p_kc = exp(l_kc)
//   mixture       m_c = max_k l_kc,  mix_c = m_c + log(sum_k w_k exp(l_kc - m_c)),  -inf when m_c is;  pbar_c = exp(mix_c)
//   SOFT          out_c = (float) mix_c
//   LOG           u_c = sum_k w_k l_kc,  out_c = (float)((u_c - umax) - log(sum_c exp(u_c - umax)))
//   rows[i]       (H_total, H_mean, MI, n_disagree):  H_total = -sum_c pbar_c mix_c,  H_mean = sum_k w_k (-sum_c p_kc l_kc),
//                 MI = sum_k w_k sum_c p_kc (l_kc - mix_c) -- summed DIRECTLY, every term a KL integrand, so a row on which the members
//                 agree gives a small sum of small terms and not the difference of two entropies that share their leading digits --
//                 n_disagree = the members whose own arg-max (the first maximum of their float32 row, score.hip's order; beta > 0
//                 does not move it) is not the first maximum of the float32 out row AS STORED.  Terms with a zero probability are 0.
// A row in which a member holds a NaN or has a maximum that is not finite, or (LOG) whose every u_c is -inf, gets NaN in every out
// column and rows = (NaN, NaN, NaN, -2): reliability.hip's NaN-row convention.  tests/ensemble_ref.py restates all of it.
//
// HOW IT RUNS.  One launch in wave_rows' shape (common.hpp): 256 threads, one wave per row, rows over a grid-stride loop, lane t takes columns
// t, t + 64, ...  The members travel BY VALUE in the kernel's argument struct (K <= 32: no device table, nothing uploaded); at its
// start lane k of every wave picks member k's pointer, stride, beta and weight out of it with 32 STATIC selects, and per row it
// keeps member k's row constants (a_k, the log1p term, the arg-max) -- the loops over k then read lane k with v_readlane, k being
// wave-uniform.  Nothing is indexed by a runtime value in registers (that would go to scratch) and no LDS is used.
// Pass 1, per member: arg-max and maximum (wave_best), then rest_k.  (LOG: umax, a wave maximum.)  Pass 2, per column: m_c, the
// mixture sum, and -- only when rows is given -- the three entropy terms, each re-reading the K values of the column: every column
// is re-read by the lane that uses it, and out may therefore alias no input.  Every sum has a fixed order: a lane's columns
// ascending, the members ascending within a column, then the DPP / v_readlane butterfly of common.hpp.  No atomics: the result is a
// function of the arguments alone.
#include <limits.h>
#include <math.h>

#include "common.hpp"
#include "launch.hpp"
#include "logp_row.hpp"
#include "spans.hpp"

namespace slnlp {

struct EnsMembers {                    // by value in the kernel arguments: 1 KiB
    const float* z[SLNLP_ENSEMBLE_MAX_MEMBERS];
    long ld[SLNLP_ENSEMBLE_MAX_MEMBERS];
    const double* beta[SLNLP_ENSEMBLE_MAX_MEMBERS];   // device pointers, null: beta = 1
    double w[SLNLP_ENSEMBLE_MAX_MEMBERS];             // normalised
};

typedef __attribute__((address_space(1))) const float* ens_gf;
typedef __attribute__((address_space(1))) const double* ens_gd;

__device__ __forceinline__ unsigned long long lane_bcast_u64(unsigned long long v, int lane) {   // `lane` wave-uniform
    const unsigned lo = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)v, lane);
    const unsigned hi = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)(v >> 32), lane);
    return ((unsigned long long)hi << 32) | lo;
}

// what lane k holds of member k for the row in hand; the k loops read it with readlane
struct EnsLane {
    unsigned long long row;            // the member's row, a global address
    double beta, w, a, l1p;
};
// l_kc of column j for the wave-uniform member k
__device__ __forceinline__ double ens_term(const EnsLane& me, int k, int j) {
    const ens_gf row = (ens_gf)lane_bcast_u64(me.row, k);
    return (lane_bcast_d(me.beta, k) * (double)row[j] - lane_bcast_d(me.a, k)) - lane_bcast_d(me.l1p, k);
}
// u_c = sum_k w_k l_kc, k increasing (-inf as soon as one member's term is: w > 0)
__device__ __forceinline__ double ens_log_term(const EnsLane& me, int K, int j) {
    double u = 0.0;
    for (int k = 0; k < K; ++k) u += lane_bcast_d(me.w, k) * ens_term(me, k, j);
    return u;
}

__device__ __forceinline__ void ensemble_rows_body(EnsMembers m, int K, int N, int V, int mode, float* __restrict__ out, long ld_out,
                                                   double* __restrict__ rows) {
    // (wave_rows' loop, written out: through the helper this kernel's register counts change -- profiles/judging_shell_isa.txt)
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane((int)(blockIdx.x * 4 + (threadIdx.x >> 6)));
    const int nwaves = gridDim.x * 4;
    const double qnan = __builtin_bit_cast(double, 0x7ff8000000000000ull);
    const float qnanf = __builtin_bit_cast(float, 0x7fc00000u);
    const bool diag = rows != nullptr;
    const bool log_mode = mode == SLNLP_VOTE_LOG;
    // lane k takes member k: static indices into the argument struct, one select each
    unsigned long long my_z = 0, my_bp = 0;
    long my_ld = 0;
    EnsLane me = {0, 1.0, 0.0, 0.0, 0.0};
#pragma unroll
    for (int k = 0; k < SLNLP_ENSEMBLE_MAX_MEMBERS; ++k) {
        if (lane == k) {
            my_z = (unsigned long long)m.z[k];
            my_ld = m.ld[k];
            my_bp = (unsigned long long)m.beta[k];
            me.w = m.w[k];
        }
    }
    if (lane < K && my_bp != 0) me.beta = ((ens_gd)my_bp)[0];
    for (long r = wave; r < N; r += nwaves) {            // r: the same in every lane, so every lane reaches the reductions
        float* dst = out + r * ld_out;
        me.row = my_z + (unsigned long long)(r * my_ld) * 4ull;      // (lanes >= K: never read)
        int my_arg = -1;
        bool bad = false;
        for (int k = 0; k < K; ++k) {                    // pass 1: member k's maximum, arg-max and logsumexp
            const ens_gf row = (ens_gf)lane_bcast_u64(me.row, k);
            const double beta = lane_bcast_d(me.beta, k);
            const LogpRowMax top = logp_row_argmax(row, V, lane);
            bad = bad || !top.finite;
            const LogpRowSums h = logp_row_sums(row, V, lane, beta, top.zmax);
            const double l1p = log1p(h.rest);
            if (lane == k) { me.a = h.a; me.l1p = l1p; my_arg = top.pred; }
        }
        // from here on the column loops run the same number of rounds in every lane (a lane past the row's end works on column 0
        // and adds nothing), so that every v_readlane of the k loops is issued with the whole wave active
        double umax = 0.0;
        if (log_mode && !bad) {
            umax = -INFINITY;
            for (long j0 = 0; j0 < V; j0 += 64) {             // (long: j0 + 64 may pass INT_MAX)
                const bool act = j0 + lane < V;
                const double u = ens_log_term(me, K, act ? (int)(j0 + lane) : 0);
                if (act) umax = fmax(umax, u);
            }
            umax = wave_max_d(umax);
            bad = !(umax > -INFINITY);                   // every class is impossible for some member
        }
        if (bad) {                                       // wave-uniform: it comes out of wave reductions
            for (int j = lane; j < V; j += 64) dst[j] = qnanf;
            if (diag && lane == 0) *(double4*)(rows + 4 * r) = double4{qnan, qnan, qnan, -2.0};
            continue;
        }
        float bv = -INFINITY;                            // the first maximum of the out row as stored
        int bi = INT_MAX;
        double h_total = 0.0, h_mean = 0.0, mi = 0.0;
        if (!log_mode || diag) {                         // pass 2: the mixture, column by column
            for (long j0 = 0; j0 < V; j0 += 64) {             // (long: j0 + 64 may pass INT_MAX)
                const bool act = j0 + lane < V;
                const int j = act ? (int)(j0 + lane) : 0;
                double mx = -INFINITY;
                for (int k = 0; k < K; ++k) mx = fmax(mx, ens_term(me, k, j));
                const bool some = mx > -INFINITY;        // else: no member gives the class any probability
                double s = 0.0;
                for (int k = 0; k < K; ++k) {
                    const double e = exp(ens_term(me, k, j) - mx);
                    s += lane_bcast_d(me.w, k) * (some ? e : 0.0);
                }
                const double mix = some ? mx + log(s) : -INFINITY;
                if (!log_mode && act) {
                    const float o = (float)mix;
                    dst[j] = o;
                    if (score_beats(o, j, bv, bi)) { bv = o; bi = j; }
                }
                if (diag) {
                    const double pbar = some ? exp(mix) : 0.0;
                    if (act && pbar > 0.0) h_total -= pbar * mix;
                    for (int k = 0; k < K; ++k) {
                        const double l = ens_term(me, k, j), wp = lane_bcast_d(me.w, k) * exp(l);
                        if (act && wp > 0.0) {           // (w > 0: zero exactly when p is)
                            h_mean -= wp * l;
                            mi += wp * (l - mix);
                        }
                    }
                }
            }
        }
        if (log_mode) {
            double s = 0.0;
            for (long j0 = 0; j0 < V; j0 += 64) {             // (long: j0 + 64 may pass INT_MAX)
                const bool act = j0 + lane < V;
                const double e = exp(ens_log_term(me, K, act ? (int)(j0 + lane) : 0) - umax);
                if (act) s += e;
            }
            const double lse = log(wave_sum_d(s));
            for (long j0 = 0; j0 < V; j0 += 64) {             // (long: j0 + 64 may pass INT_MAX)
                const bool act = j0 + lane < V;
                const int j = act ? (int)(j0 + lane) : 0;
                const float o = (float)((ens_log_term(me, K, j) - umax) - lse);
                if (act) {
                    dst[j] = o;
                    if (score_beats(o, j, bv, bi)) { bv = o; bi = j; }
                }
            }
        }
        if (diag) {
            wave_best(bv, bi);
            const double n_dis = (double)__popcll(__ballot(lane < K && my_arg != bi));
            h_total = wave_sum_d(h_total);
            h_mean = wave_sum_d(h_mean);
            mi = wave_sum_d(mi);
            if (lane == 0) *(double4*)(rows + 4 * r) = double4{h_total, h_mean, mi, n_dis};
        }
    }
}
SLNLP_ZKERNEL(ensemble_rows_kernel, 256, ensemble_rows_body)

int ensemble_rows(const float* const* logp, const int64_t* ld, const double* const* beta_dev, const double* weights, int K, int64_t N,
                  int64_t V, int mode, float* out, int64_t ld_out, double* rows, hipStream_t st) {
    SLNLP_CHECK_ARG(logp && ld && out, "ensemble_rows: null pointer");
    SLNLP_CHECK_ARG(K >= 1 && K <= SLNLP_ENSEMBLE_MAX_MEMBERS, "ensemble_rows: K=%d outside 1..%d", K, SLNLP_ENSEMBLE_MAX_MEMBERS);
    SLNLP_CHECK_ARG(N >= 1 && N <= INT_MAX, "ensemble_rows: N=%ld outside 1..%d", (long)N, INT_MAX);
    SLNLP_CHECK_ARG(V >= 1 && V <= INT_MAX, "ensemble_rows: V=%ld outside 1..%d", (long)V, INT_MAX);
    SLNLP_CHECK_ARG(mode == SLNLP_VOTE_SOFT || mode == SLNLP_VOTE_LOG, "ensemble_rows: mode=%d is neither SLNLP_VOTE_SOFT nor SLNLP_VOTE_LOG",
                    mode);
    SLNLP_CHECK_ARG(ld_out >= V, "ensemble_rows: ld_out=%ld is less than V=%ld", (long)ld_out, (long)V);
    SLNLP_CHECK_ARG(ld_out <= INT64_MAX / 8 / N, "ensemble_rows: ld_out=%ld times N=%ld is no addressable matrix", (long)ld_out, (long)N);
    SLNLP_CHECK_ARG(((uintptr_t)out & 3) == 0, "ensemble_rows: out is not 4-byte aligned");
    SLNLP_CHECK_ARG(((uintptr_t)rows & 31) == 0, "ensemble_rows: rows is not 32-byte aligned");
    EnsMembers m;
    memset(&m, 0, sizeof(m));
    double wsum = 0.0;
    for (int k = 0; k < K; ++k) {
        SLNLP_CHECK_ARG(logp[k], "ensemble_rows: member %d is a null pointer", k);
        SLNLP_CHECK_ARG(ld[k] >= V, "ensemble_rows: ld[%d]=%ld is less than V=%ld", k, (long)ld[k], (long)V);
        SLNLP_CHECK_ARG(ld[k] <= INT64_MAX / 8 / N, "ensemble_rows: ld[%d]=%ld times N=%ld is no addressable matrix", k, (long)ld[k], (long)N);
        SLNLP_CHECK_ARG(((uintptr_t)logp[k] & 3) == 0, "ensemble_rows: member %d is not 4-byte aligned", k);
        const double* b = beta_dev ? beta_dev[k] : nullptr;
        SLNLP_CHECK_ARG(((uintptr_t)b & 7) == 0, "ensemble_rows: beta of member %d is not 8-byte aligned", k);
        const double w = weights ? weights[k] : 1.0;
        SLNLP_CHECK_ARG(w > 0.0 && w < INFINITY, "ensemble_rows: weights[%d]=%g is not a finite number above 0", k, w);
        m.z[k] = logp[k];
        m.ld[k] = (long)ld[k];
        m.beta[k] = b;
        m.w[k] = w;
        wsum += w;                                       // in increasing k
    }
    SLNLP_CHECK_ARG(wsum < INFINITY, "ensemble_rows: the weights' sum is not finite");
    for (int k = 0; k < K; ++k) m.w[k] = weights ? m.w[k] / wsum : 1.0 / (double)K;
    const Span outs[2] = {{out, matrix_bytes(N, ld_out, V), "out"}, {rows, (size_t)N * 32, "rows"}};
    for (const Span& o : outs) {                         // its own wording: the inputs are numbered members
        for (int k = 0; k < K; ++k) {
            SLNLP_CHECK_ARG(!spans_overlap(o, Span{m.z[k], matrix_bytes(N, m.ld[k], V), ""}), "ensemble_rows: %s overlaps member %d", o.name, k);
            SLNLP_CHECK_ARG(!spans_overlap(o, Span{m.beta[k], 8, ""}), "ensemble_rows: %s overlaps the beta of member %d", o.name, k);
        }
    }
    SLNLP_CHECK_ARG(!spans_overlap(outs[0], outs[1]), "ensemble_rows: out and rows overlap");
    return zlaunch(ensemble_rows_kernel, dim3(wave_rows_grid(N)), 256, 0, st, "ensemble_rows", m, K, (int)N, (int)V, mode, out, (long)ld_out, rows);
}

}  // namespace slnlp

extern "C" int slnlp_ensemble_rows(const float* const* logp, const int64_t* ld, const double* const* beta_dev, const double* weights, int K,
                                   int64_t N, int64_t V, int mode, float* out, int64_t ld_out, double* rows, void* stream) {
    return slnlp::ensemble_rows(logp, ld, beta_dev, weights, K, N, V, mode, out, ld_out, rows, (hipStream_t)stream);
}
