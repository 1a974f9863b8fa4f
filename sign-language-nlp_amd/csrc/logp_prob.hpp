// logp_prob.hpp -- the probability of ONE column of a row of float32 log-probs, given the row head (zmax, a, s0) of logp_row.hpp:
// the statement label_audit.hip's passes 1 and 3 and train_dynamics.hip's visit pass share, so the same (row, column) has the same
// bits in each of them.
//
// INCLUDE IT IN FRONT OF a file's `#pragma clang fp contract(off)`: topk_rows forms `exp(beta * (double)v - a) / s0` under the
// compiler's default contraction, and this is that expression under that setting (tests/test_label_audit_gpu.py compares the bits).
#pragma once
#include <math.h>

#include "common.hpp"

namespace slnlp {

__device__ __forceinline__ double audit_prob(float zf, float zmax, double beta, double a, double s0) {
    return zf == zmax ? 1.0 / s0 : exp(beta * (double)zf - a) / s0;
}

}  // namespace slnlp
