// logp_row.hpp -- the head of ONE row of float32 log-probs on ONE wave, shared by the kernels that judge a row at an inverse
// temperature beta > 0: reliability_rows (reliability.hip), topk_rows (confusion.hip), conformal_rows (conformal.hip) and, once
// per member, pass 1 of ensemble_rows (ensemble.hip).  All four run the statements below, so the arg-max, the probability of the
// arg-max class 1 / s0 and every exp(beta z_c - a) / s0 have the same bits whichever kernel formed them.
//
// Lanes stride the columns (lane l takes l, l + 64, ...); all 64 lanes must be active and V and beta wave-uniform.  `row` is any
// pointer to float (the ensemble passes an address_space(1) pointer).  Each function reads the V columns once, ascending per lane.
//
// NaN AND NON-FINITE MAXIMA.  score_beats' order puts a NaN before every number, so a NaN anywhere in the row wins: zmax is then
// that NaN (pred its first column).  A row of -inf alone has zmax = -inf, a row holding +inf has zmax = +inf.  logp_row_argmax
// reports all three as finite = false; such a row has no softmax.  logp_row_sums may still be called on it (reliability, top-k and
// the ensemble do, to keep every lane on one path): its sums are then NaN or meaningless, nothing faults, and the caller must
// store its NaN-row result instead of them.
//
// NOT HERE, on purpose:
//   fit_rows / scale_logp (calibration.hip) take the maximum with fmaxf / wave_max: another NaN rule (a NaN is skipped) and no arg-max.
//   fit_rows also evaluates exp for the columns AT the maximum, its s1 and s2 need it: folding it in would change bits.
//   score_rows (score.hip) fuses its arg-max with three other counts in one pass over the row.
//   prior_rows / shift_logp (prior_shift.hip) take logp_row_argmax's `finite` alone from here: their maximum is that of beta z + lw.
#pragma once
#include <limits.h>
#include <math.h>

#include "common.hpp"

namespace slnlp {

// zmax / pred: the first maximum of the row in score_beats' total order on the float32 values (a NaN first, then larger values,
// equal values by ascending column), in every lane.  Any column beats the start: -inf at column j ties and j < INT_MAX.
struct LogpRowMax {
    float zmax;
    int pred;
    bool finite;
};
template <class Row>
__device__ __forceinline__ LogpRowMax logp_row_argmax(Row row, int V, int lane) {
    float zmax = -INFINITY;
    int pred = INT_MAX;
    for (int j = lane; j < V; j += 64) {
        const float x = row[j];
        if (score_beats(x, j, zmax, pred)) { zmax = x; pred = j; }
    }
    wave_best(zmax, pred);
    return {zmax, pred, fabsf(zmax) < INFINITY};
}

// The sums at beta, all in fp64: a = beta zmax (beta > 0: the maximum of beta z), e_c = exp(beta z_c - a).  The n_max columns AT
// the maximum have e = 1 exactly: they are counted (whole numbers, summed exactly; n_max >= 1 for a finite maximum) and the others
// summed, so rest = sum e - 1 -- what log1p takes -- is formed without the 1 ever entering a sum, and s0 = 1 + rest = sum e.
// each(e) is called once per column NOT at the maximum, in the lane's column order, for what a caller accumulates beside them.
struct LogpRowSums {
    double a, n_max, rest, s0;
};
template <class Row, class Each>
__device__ __forceinline__ LogpRowSums logp_row_sums(Row row, int V, int lane, double beta, float zmax, Each&& each) {
    LogpRowSums s;
    s.a = beta * (double)zmax;
    double rest = 0.0, at_max = 0.0;
    for (int j = lane; j < V; j += 64) {
        const float zf = row[j];
        if (zf == zmax) {
            at_max += 1.0;
        } else {
            const double e = exp(beta * (double)zf - s.a);
            rest += e;
            each(e);
        }
    }
    s.n_max = wave_sum_d(at_max);
    s.rest = wave_sum_d(rest) + (s.n_max - 1.0);
    s.s0 = 1.0 + s.rest;
    return s;
}
template <class Row>
__device__ __forceinline__ LogpRowSums logp_row_sums(Row row, int V, int lane, double beta, float zmax) {
    return logp_row_sums(row, V, lane, beta, zmax, [](double) {});
}

}  // namespace slnlp
