// scale_row.hpp -- the calibrated log-probs of ONE row on ONE wave: dst[c] = beta z_c - logsumexp_c'(beta z_c'), rounded once to
// float32.  scale_logp (calibration.hip) and scatter_logp (label_audit.hip) both run these statements, so a row has the same bits
// whichever of the two wrote it.
//
// Lanes stride the columns; all 64 lanes must be active and V and beta wave-uniform.  The maximum is fmaxf's (a NaN is skipped:
// calibration.hip's rule, not logp_row.hpp's); the columns AT the maximum are counted and not summed, so sum e - 1 is formed
// without the 1 ever entering a sum.  dst may be row itself: a lane re-reads each of its columns right before it stores that
// column, no other lane touches it, and the row's reductions -- data-dependent on every load of the row -- are complete before
// the first store.
#pragma once
#include <math.h>

#include "common.hpp"

namespace slnlp {

// (no __restrict__: dst may be row itself)
__device__ __forceinline__ void scale_logp_row(const float* row, float* dst, int V, int lane, double beta) {
    float zmax = -INFINITY;
    for (int j = lane; j < V; j += 64) zmax = fmaxf(zmax, row[j]);
    zmax = wave_max(zmax);
    const double a = beta * (double)zmax;
    double rest = 0.0, at_max = 0.0;                 // as in fit_rows: sum e - 1 without the 1 ever entering a sum
    for (int j = lane; j < V; j += 64) {
        const float zf = row[j];
        if (zf == zmax) at_max += 1.0; else rest += exp(beta * (double)zf - a);
    }
    // lse - a; it depends on every load of the row: none is outstanding past here
    const double l = log1p(wave_sum_d(rest) + (wave_sum_d(at_max) - 1.0));
    for (int j = lane; j < V; j += 64) dst[j] = (float)((beta * (double)row[j] - a) - l);   // re-read, then stored, by its own lane
}

}  // namespace slnlp
