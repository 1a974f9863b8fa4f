// train_dynamics.hip -- what happened to every train row DURING a fit, kept on the device epoch by epoch: dataset cartography
// (Swayamdipta et al. 2020: confidence, variability, correctness), forgetting events (Toneva et al. 2019) and the area under the
// margin (Pleiss et al. 2020) (NeuralNetClassifier(train_dynamics=True); slnlp/metrics.py's train_dynamics_report; DESIGN.md
// section 4).  include/slnlp.h states the definitions and the byte layout; tests/train_dynamics_ref.py restates them in numpy, line
// by line.
//
// z float32 log-probs of ONE epoch's train pass [n_visit, ld] (V columns used) in VISIT order, y int64 [n_visit] the labels in visit
// order, order int64 [n_visit] the dataset row of every visit (null: visit i is row i).  ALL PER-ROW STATE IS INTEGER: a
// probability enters as q = rint(min(p, 1) 2^20), a margin as mq = rint(clamp(z_y - z_other, +-1024) 2^20), and rows collect them
// with integer atomics -- under a balanced resample a row is visited several times per epoch and its visits do collide.  Integer
// sums do not depend on the order of arrival, so the state is a pure function of the arguments: no floating-point atomics, nothing
// depends on the grid or on timing.
//
// slnlp_train_dynamics_epoch queues a FIXED sequence of two launches and never waits for the host:
//   dyn_visits   one wave per visit position, four per block, positions over a grid-stride loop (wave_rows, common.hpp): the code,
//                pred / correct from logp_row_argmax (slnlp_score_rows' pred), q from audit_prob (logp_prob.hpp) on the row head
//                at beta = 1 (label_audit's self-confidence, bit for bit), mq from the first column other than the label in
//                score_beats' order (audit_rows' loop); all five to the per-visit scratch, and for a usable visit the adds into
//                row r: v_e += 1, c_e += correct (the epoch's scratch), sum_q += q, sum_q2 += q q, sum_mq += mq (cumulative).
//   dyn_fold     one thread per dataset row and per visit position: a row with v_e > 0 folds the epoch into its counts
//                (a = "right at every visit of the epoch"; a forgetting event is last == 1 and not a) and clears v_e / c_e; the
//                block's integer sums over a fixed tree -- visits by code, rows seen for the first time, rows at the visit
//                limit -- go to the head with one integer atomic per block and count.
// slnlp_train_dynamics_reset is one launch of this library's own (as confusion.hip zeroes its counts): no torch fill kernel
// joins a fused fit's stream.
#include <limits.h>
#include <math.h>

#include "block_reduce.hpp"
#include "common.hpp"
#include "launch.hpp"
#include "logp_prob.hpp"
#include "logp_row.hpp"
#include "spans.hpp"

// this file's own arithmetic (the margin, the two scalings) is rounded operation by operation, as the restatement's numpy
// expressions are
#pragma clang fp contract(off)

namespace slnlp {

typedef unsigned long long dyn_u64;

enum { DYN_EPOCHS = 0, DYN_USABLE = 1, DYN_BAD_LABELS = 2, DYN_NAN_ROWS = 3, DYN_BAD_ROWS = 4, DYN_SEEN = 5, DYN_OVERFLOW = 6 };
constexpr unsigned DYN_MAX_VISITS = 1u << SLNLP_DYN_VISIT_BITS;      // a row at this many visits sets the overflow flag
constexpr double DYN_SCALE = (double)(1 << SLNLP_DYN_FRAC_BITS);     // 2^20
constexpr double DYN_MARGIN_MAX = 1024.0;
constexpr int DYN_MAX_BLOCKS = 2048;                                 // x 256 entries (reset / fold): larger inputs wrap the stride loops

// the pieces of the state and of the per-visit scratch in bytes from their starts (include/slnlp.h documents them); every piece
// is 8-byte aligned
static size_t dyn_even(size_t ints) { return (ints + (ints & 1)) * 4; }
struct DynLayout {
    size_t sum_q, sum_q2, sum_mq, visits, correct_visits, epochs_seen, epochs_correct, forgetting, first_learned, last, v_e, c_e, total;
};
static DynLayout dyn_layout(int64_t N) {
    const size_t n = (size_t)N;
    DynLayout L;
    size_t at = SLNLP_DYN_HEAD_BYTES;
    L.sum_q = at;          at += n * 8;
    L.sum_q2 = at;         at += n * 8;
    L.sum_mq = at;         at += n * 8;
    L.visits = at;         at += dyn_even(n);
    L.correct_visits = at; at += dyn_even(n);
    L.epochs_seen = at;    at += dyn_even(n);
    L.epochs_correct = at; at += dyn_even(n);
    L.forgetting = at;     at += dyn_even(n);
    L.first_learned = at;  at += dyn_even(n);
    L.last = at;           at += dyn_even(n);
    L.v_e = at;            at += dyn_even(n);
    L.c_e = at;            at += dyn_even(n);
    L.total = at;
    return L;
}
struct DynVisits {
    size_t q, mq, code, correct, pred, total;
};
static DynVisits dyn_visits_layout(int64_t n_visit) {
    const size_t n = (size_t)n_visit;
    DynVisits L;
    size_t at = 0;
    L.q = at;       at += n * 8;
    L.mq = at;      at += n * 8;
    L.code = at;    at += dyn_even(n);
    L.correct = at; at += dyn_even(n);
    L.pred = at;    at += dyn_even(n);
    L.total = at;
    return L;
}

// ----------------------------------------------------------------------------------------------------------- reset ----
// everything 0 but first_learned and last, which start at -1 ("never"); words: the 4-byte words of the state behind its head
__device__ __forceinline__ void dyn_reset_body(int64_t* __restrict__ head, int* __restrict__ words, long n_words, long minus_begin,
                                               long minus_end) {
    const long t0 = blockIdx.x * 256L + threadIdx.x;
    if (t0 < 8) head[t0] = 0;
    for (long i = t0; i < n_words; i += gridDim.x * 256L) words[i] = (i >= minus_begin && i < minus_end) ? -1 : 0;
}
SLNLP_ZKERNEL(dyn_reset_kernel, 256, dyn_reset_body)

// ---------------------------------------------------------------------------------------------------------- visits ----
__device__ __forceinline__ void dyn_visits_body(const float* __restrict__ logp, long ld, const int64_t* __restrict__ y,
                                                const int64_t* __restrict__ order, int n_visit, int V, int N, dyn_u64* __restrict__ q,
                                                long long* __restrict__ mq, int* __restrict__ code, int* __restrict__ correct,
                                                int* __restrict__ pred, unsigned* __restrict__ v_e, unsigned* __restrict__ c_e,
                                                dyn_u64* __restrict__ sum_q, dyn_u64* __restrict__ sum_q2, dyn_u64* __restrict__ sum_mq) {
    wave_rows(n_visit, [&](long i, int lane) {
        const float* row = logp + i * ld;
        const int64_t r = order ? order[i] : (int64_t)i;     // one address for the wave: r is wave-uniform
        const int64_t label = y[i];
        const LogpRowMax top = logp_row_argmax(row, V, lane);
        // the row index first (never used as an address), then the row's softmax (looked at before the label, as in audit_rows)
        const int cd = (r < 0 || r >= N) ? -3 : !top.finite ? -2 : (label < 0 || label >= V) ? -1 : 0;
        if (cd != 0) {                                       // wave-uniform
            if (lane == 0) { q[i] = 0; mq[i] = 0; code[i] = cd; correct[i] = 0; pred[i] = top.pred; }
            return;
        }
        const float zmax = top.zmax;
        const LogpRowSums h = logp_row_sums(row, V, lane, 1.0, zmax);
        const int lab = (int)label;
        float bv = -INFINITY;                                // the first column other than the label (V = 1: none, INT_MAX stays)
        int bi = INT_MAX;
        for (int j = lane; j < V; j += 64) {
            if (j == lab) continue;
            const float x = row[j];
            if (score_beats(x, j, bv, bi)) { bv = x; bi = j; }
        }
        wave_best(bv, bi);
        if (lane == 0) {
            const float zy = row[lab];
            const double p = audit_prob(zy, zmax, 1.0, h.a, h.s0);
            const dyn_u64 qi = (dyn_u64)rint(fmin(p, 1.0) * DYN_SCALE);
            // both operands are float32: the difference is exact in fp64 (-inf - x and x - -inf are the infinities the clamp takes)
            const double margin = bi == INT_MAX ? 0.0 : (double)zy - (double)bv;
            const long long mi = (long long)rint(fmin(fmax(margin, -DYN_MARGIN_MAX), DYN_MARGIN_MAX) * DYN_SCALE);
            const int ok = top.pred == lab ? 1 : 0;
            q[i] = qi; mq[i] = mi; code[i] = 0; correct[i] = ok; pred[i] = top.pred;
            atomicAdd(&v_e[r], 1u);
            if (ok) atomicAdd(&c_e[r], 1u);
            atomicAdd(&sum_q[r], qi);
            atomicAdd(&sum_q2[r], qi * qi);
            atomicAdd(&sum_mq[r], (dyn_u64)mi);              // two's complement: the wrap-around add is the signed one
        }
    });
}
SLNLP_ZKERNEL(dyn_visits_kernel, 256, dyn_visits_body)

// ------------------------------------------------------------------------------------------------------------ fold ----
enum { FOLD_USABLE = 0, FOLD_BAD_LABELS = 1, FOLD_NAN_ROWS = 2, FOLD_BAD_ROWS = 3, FOLD_SEEN = 4, FOLD_OVERFLOW = 5, FOLD_COUNTS = 6 };

__device__ __forceinline__ void dyn_fold_body(const int* __restrict__ code, int n_visit, int N, int epoch, unsigned* __restrict__ v_e,
                                              unsigned* __restrict__ c_e, unsigned* __restrict__ visits, unsigned* __restrict__ correct_visits,
                                              int* __restrict__ epochs_seen, int* __restrict__ epochs_correct, int* __restrict__ forgetting,
                                              int* __restrict__ first_learned, int* __restrict__ last, int64_t* __restrict__ head) {
    __shared__ int part[FOLD_COUNTS][256];
    const int tid = threadIdx.x;
    const long top = n_visit > N ? n_visit : N;
    int c[FOLD_COUNTS] = {0, 0, 0, 0, 0, 0};
    for (long t = blockIdx.x * 256L + tid; t < top; t += gridDim.x * 256L) {
        if (t < n_visit) {
            const int cd = code[t];
            ++c[cd == 0 ? FOLD_USABLE : cd == -1 ? FOLD_BAD_LABELS : cd == -2 ? FOLD_NAN_ROWS : FOLD_BAD_ROWS];
        }
        if (t < N) {
            const unsigned ve = v_e[t];
            if (ve > 0) {
                const unsigned ce = c_e[t];
                const int a = ce == ve ? 1 : 0;              // right at every visit of the epoch
                const int was = last[t];
                const unsigned vis = visits[t] + ve;
                visits[t] = vis;
                correct_visits[t] += ce;
                epochs_seen[t] += 1;
                epochs_correct[t] += a;
                if (was == 1 && !a) forgetting[t] += 1;
                if (a && first_learned[t] == -1) first_learned[t] = epoch;
                last[t] = a;
                v_e[t] = 0;
                c_e[t] = 0;
                c[FOLD_SEEN] += was == -1 ? 1 : 0;
                c[FOLD_OVERFLOW] += vis >= DYN_MAX_VISITS ? 1 : 0;
            }
        }
    }
#pragma unroll
    for (int k = 0; k < FOLD_COUNTS; ++k) part[k][tid] = c[k];
    block_tree<FOLD_COUNTS>(part, tid, TreeSum{});
    if (tid < FOLD_COUNTS) {
        const int sum = part[tid][0];
        dyn_u64* h = (dyn_u64*)head;
        if (tid == FOLD_OVERFLOW) {
            if (sum > 0) atomicOr(&h[DYN_OVERFLOW], 1ull);
        } else if (sum > 0) {
            atomicAdd(&h[DYN_USABLE + tid], (dyn_u64)sum);   // FOLD_* and DYN_* list the five counts in one order
        }
    }
    if (blockIdx.x == 0 && tid == 0) atomicAdd((dyn_u64*)head + DYN_EPOCHS, 1ull);
}
SLNLP_ZKERNEL(dyn_fold_kernel, 256, dyn_fold_body)

static inline int dyn_blocks(int64_t n) { return (int)((n + 255) / 256 < DYN_MAX_BLOCKS ? (n + 255) / 256 : DYN_MAX_BLOCKS); }

// ------------------------------------------------------------------------------------------------------- host side ----
static int dyn_check_state(const char* what, const void* state, int64_t state_bytes, int64_t N, DynLayout* L) {
    SLNLP_CHECK_ARG(state, "%s: null pointer", what);
    SLNLP_CHECK_ARG(N >= 1 && N <= INT_MAX, "%s: N=%ld outside 1..%d", what, (long)N, INT_MAX);
    *L = dyn_layout(N);
    SLNLP_CHECK_ARG(state_bytes >= 0 && (size_t)state_bytes >= L->total, "%s: state of %ld bytes is too small, %ld rows need %ld", what,
                    (long)state_bytes, (long)N, (long)L->total);
    SLNLP_CHECK_ARG(((uintptr_t)state & 7) == 0, "%s: state is not 8-byte aligned", what);
    return 0;
}

int train_dynamics_reset(void* state, int64_t state_bytes, int64_t N, hipStream_t st) {
    DynLayout L;
    SLNLP_TRY(dyn_check_state("train_dynamics_reset", state, state_bytes, N, &L));
    char* b = (char*)state;
    const long words = (long)((L.total - SLNLP_DYN_HEAD_BYTES) / 4);
    const long minus_begin = (long)((L.first_learned - SLNLP_DYN_HEAD_BYTES) / 4), minus_end = (long)((L.v_e - SLNLP_DYN_HEAD_BYTES) / 4);
    return zlaunch(dyn_reset_kernel, dim3(dyn_blocks(words)), 256, 0, st, "train_dynamics_reset", (int64_t*)state,
                   (int*)(b + SLNLP_DYN_HEAD_BYTES), words, minus_begin, minus_end);
}

int train_dynamics_epoch(const float* logp, int64_t ld, const int64_t* y, const int64_t* order, int64_t n_visit, int64_t V, int64_t N,
                         int64_t epoch, void* state, int64_t state_bytes, void* visits, int64_t visits_bytes, hipStream_t st) {
    const char* what = "train_dynamics_epoch";
    SLNLP_CHECK_ARG(logp && y && state && visits, "%s: null pointer", what);
    SLNLP_CHECK_ARG(n_visit >= 1 && n_visit <= INT_MAX, "%s: n_visit=%ld outside 1..%d", what, (long)n_visit, INT_MAX);
    DynLayout L;
    SLNLP_TRY(dyn_check_state(what, state, state_bytes, N, &L));
    Span z;
    SLNLP_TRY(check_logp_matrix(what, logp, n_visit, INT_MAX, V, INT_MAX, ld, &z));
    SLNLP_CHECK_ARG(epoch >= 1 && epoch <= INT_MAX, "%s: epoch=%ld outside 1..%d", what, (long)epoch, INT_MAX);
    const DynVisits W = dyn_visits_layout(n_visit);
    SLNLP_CHECK_ARG(visits_bytes >= 0 && (size_t)visits_bytes >= W.total, "%s: visits of %ld bytes is too small, %ld visits need %ld", what,
                    (long)visits_bytes, (long)n_visit, (long)W.total);
    SLNLP_CHECK_ARG(((uintptr_t)logp & 3) == 0 && (((uintptr_t)y | (uintptr_t)order | (uintptr_t)visits) & 7) == 0,
                    "%s: misaligned pointer (logp: 4 bytes; y, order, state, visits: 8 bytes)", what);
    const Span in[3] = {z, {y, (size_t)n_visit * 8, "y"}, {order, (size_t)n_visit * 8, "order"}};
    const Span out[2] = {{state, L.total, "state"}, {visits, W.total, "visits"}};
    SLNLP_TRY(check_no_overlap(what, out, in));
    char* b = (char*)state;
    char* w = (char*)visits;
    unsigned* v_e = (unsigned*)(b + L.v_e);
    unsigned* c_e = (unsigned*)(b + L.c_e);
    int* code = (int*)(w + W.code);
    SLNLP_TRY(zlaunch(dyn_visits_kernel, dim3(wave_rows_grid(n_visit)), 256, 0, st, "train_dynamics_visits", logp, (long)ld, y, order, (int)n_visit,
                      (int)V, (int)N, (dyn_u64*)(w + W.q), (long long*)(w + W.mq), code, (int*)(w + W.correct), (int*)(w + W.pred), v_e, c_e,
                      (dyn_u64*)(b + L.sum_q), (dyn_u64*)(b + L.sum_q2), (dyn_u64*)(b + L.sum_mq)));
    return zlaunch(dyn_fold_kernel, dim3(dyn_blocks(n_visit > N ? n_visit : N)), 256, 0, st, "train_dynamics_fold", (const int*)code, (int)n_visit,
                   (int)N, (int)epoch, v_e, c_e, (unsigned*)(b + L.visits), (unsigned*)(b + L.correct_visits), (int*)(b + L.epochs_seen),
                   (int*)(b + L.epochs_correct), (int*)(b + L.forgetting), (int*)(b + L.first_learned), (int*)(b + L.last), (int64_t*)state);
}

}  // namespace slnlp

extern "C" int64_t slnlp_train_dynamics_state_bytes(int64_t N) {
    if (N < 1 || N > INT_MAX) {
        slnlp::set_error("train_dynamics_state_bytes: N=%ld outside 1..%d", (long)N, INT_MAX);
        return -1;
    }
    return (int64_t)slnlp::dyn_layout(N).total;
}
extern "C" int slnlp_train_dynamics_reset(void* state, int64_t state_bytes, int64_t N, void* stream) {
    return slnlp::train_dynamics_reset(state, state_bytes, N, (hipStream_t)stream);
}
extern "C" int slnlp_train_dynamics_epoch(const float* logp, int64_t ld, const int64_t* y, const int64_t* order, int64_t n_visit, int64_t V,
                                          int64_t N, int64_t epoch, void* state, int64_t state_bytes, void* visits, int64_t visits_bytes,
                                          void* stream) {
    return slnlp::train_dynamics_epoch(logp, ld, y, order, n_visit, V, N, epoch, state, state_bytes, visits, visits_bytes, (hipStream_t)stream);
}
