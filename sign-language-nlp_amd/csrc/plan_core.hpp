// plan_core.hpp -- the part of a plan that is not the model.  The Transformer plan (tf_plan.hpp) and the LSTM / GRU
// encoder-decoder plan (rnn_plan.hip) differ in layout, workspace, forward and backward; the criterion / update / param-group
// settings, the clip + SGD / Adam update call, graph capture and replay, the destroy rule and what the lockstep driver
// (lockstep.hip) needs from a fit are the same code: they live here, once.  The model-specific pieces are a handful of
// virtual methods, called a few times per step on the host, never per launch.
#pragma once
#include <map>
#include <string>
#include <vector>

#include "common.hpp"
#include "launch.hpp"

namespace slnlp {

static inline long align_up(long v, long a) { return (v + a - 1) / a * a; }

// ---- what both plan types lay out the same way
// one tensor of the flat parameter arena (names / shapes = the reference state_dict)
struct ParamEnt {
    std::string name;
    int64_t shape[2];
    int ndim;
    int64_t off, numel;
};
// the body of slnlp_{tf,rnn}_param_info; `what` is the entry point's name, the prefix of its error text
static inline int param_info(const std::vector<ParamEnt>& ents, int i, const char* what, char* name, int64_t shape[2], int* ndim, int64_t* offset) {
    SLNLP_CHECK_ARG(i >= 0 && i < (int)ents.size(), "%s: index %d out of range", what, i);
    const ParamEnt& e = ents[i];
    if (name) {
        strncpy(name, e.name.c_str(), 127);
        name[127] = 0;
    }
    if (shape) {
        shape[0] = e.shape[0];
        shape[1] = e.shape[1];
    }
    if (ndim) *ndim = e.ndim;
    if (offset) *offset = e.off;
    return 0;
}
// the workspace carver: every buffer on a 256-byte boundary
struct Bump {
    char* base;
    size_t cur = 0;
    explicit Bump(void* b) : base((char*)b) {}
    template <typename T>
    T* take(size_t n) {
        cur = (cur + 255) & ~(size_t)255;
        T* p = (T*)(base + cur);
        cur += n * sizeof(T);
        return p;
    }
};
// bf16 hi/lo planes of a GEMM operand (same logical shape / row stride as its fp32 twin, rows
// zero-padded to a multiple of 64): written once by the producer, read by gemm_planes.hip
struct PP {
    unsigned short *hi = nullptr, *lo = nullptr;
    unsigned char* q8 = nullptr;        // precision 8: forward operands also as an e4m3 plane
    PlaneOut out() const { PlaneOut o; o.hi = hi; o.lo = lo; o.q8 = q8; return o; }
    PP at(long off) const { PP q; q.hi = hi + off; q.lo = lo + off; return q; }    // planes of a whole arena: the tensor at float offset `off`
};

struct PlanCore {
    slnlp_tf_buffers buf{};
    TrainOpts opts;                         // slnlp_*_set_criterion / _set_update / _set_param_groups
    std::map<int, hipGraphExec_t> graphs;   // one captured train step per batch size, kept until destroy (or a settings change)
    int destroy_sync = 1;                   // slnlp_*_set_destroy_sync: wait for the device before the plan goes away (launch.hpp)
    int last_B = 0;                         // batch of the last forward
    float last_p = 0.f;                     // dropout used by the last forward (0 in eval)
    int planes_B = -1;                      // batch size the activation planes' zero padding is valid for
    // split-bf16 passes of the plane GEMM's gradient products: the process default AT CREATION (slnlp_set_backward_passes), fixed for the
    // plan's life -- a captured graph, a recorded lockstep program and every host thread that steps this plan issue the same products
    int wgrad_np = wgrad_passes(), dgrad_np = dgrad_passes();
    int wgrad_prec(int precision) const { return precision == 3 ? wgrad_np : precision; }
    int dgrad_prec(int precision) const { return precision == 3 ? dgrad_np : precision; }     // (dY's bf16 head only)
    // Lockstep (lockstep.hip): where this fit's per-step outputs go while it advances as one of K fits -- an epoch-long
    // log-prob buffer and a per-batch loss history, indexed through two device scalars the driver updates per step
    float* ls_logp = nullptr;               // [rows of the epoch, Vt]
    float* ls_loss = nullptr;               // [batches of the epoch]
    const int* ls_dyn = nullptr;            // {first row of the batch, index of the batch}
    // fixed at creation (the plan's create call): arena floats, the update's [1024] scratch, and the configuration fields the
    // shared code reads
    int64_t arena = 0;
    float* opt_partials = nullptr;
    // slnlp_*_set_averaging (average.hip): the running average of the arena a train step feeds behind its update; `forced` is up
    // only while a lockstep group with averaging records (every fit then issues the two launches, with a null avg if it is not
    // averaging yet: one kernel per call site)
    struct Averaging {
        float* avg = nullptr;
        float* count = nullptr;
        int kind = 0;
        float decay = 0.f;
        bool forced = false;
    } averaging;
    int max_B = 0, S = 0, Vt = 0;
    float dropout = 0.f;

    virtual ~PlanCore() = default;

    // ---- what a plan type brings
    virtual int forward(const int64_t* X, const int64_t* y, const int64_t* lengths, int B, int train, float* logp, hipStream_t st) = 0;
    virtual int backward(hipStream_t st) = 0;
    // zero padding of the activation planes is per batch size: re-zero when it changes (outside any capture)
    virtual int prepare_planes(int B, hipStream_t st) = 0;
    // everything that must stay outside a recorded lockstep program (memsets, re-splits)
    virtual int prepare(int B, hipStream_t st) { return prepare_planes(B, st); }
    // the update's weight-plane output, floats [wp_begin, wp_end) (-1: to the end), and the range [skip_begin, skip_end) the
    // decaying updates leave alone
    struct UpdateRanges {
        PlaneOut wp{};
        int64_t wp_begin = 0, wp_end = -1, skip_begin = 0, skip_end = 0;
    };
    virtual UpdateRanges update_ranges() const = 0;
    virtual void params_stepped() {}        // the optimizer just rewrote the arena
    virtual void before_capture() {}        // first thing inside a graph capture
    virtual int check_recordable() const { return 0; }
    virtual bool same_shape(const PlanCore& other) const = 0;   // may the two advance through one lockstep launch sequence?

    // ---- what every plan does the same way; `what` is the calling entry point's name, the prefix of its error texts
    int update_sgd(float momentum, float max_norm, hipStream_t st);
    int update_adam(float* exp_avg_sq, float beta1, float beta2, float eps, float weight_decay, float max_norm, hipStream_t st);
    void drop_graphs();     // a settings change: the captured graphs baked the old settings into their launches (the caller re-captures)
    int set_criterion(const float* class_weight, float label_smoothing, int reduction, hipStream_t st);
    int set_update(int kind, float dampening, float weight_decay, int nesterov);
    int set_param_groups(const char* what, int n_segments, const int64_t* seg_begin, const int32_t* seg_group, int n_groups,
                         const float* weight_decay, const float* lr_dev, hipStream_t st);
    int set_averaging(const char* what, float* avg, float* count, int kind, float decay);
    int average_after_update(hipStream_t st);
    int train_step(const int64_t* X, const int64_t* y, const int64_t* lengths, int B, float momentum, float max_norm, float* logp,
                   hipStream_t st);
    int graph_capture_train(const char* what, const int64_t* X, const int64_t* y, const int64_t* lengths, int B, float momentum,
                            float max_norm, float* logp, hipStream_t st);
    int graph_launch(const char* what, int B, hipStream_t st);
    void destroy();
    // lockstep: the ordinary step code, run under a Recorder; host bookkeeping after the step's launches were issued; the device
    // float(s) the update launches read the learning rate from
    int record(const int64_t* X, const int64_t* y, const int64_t* lengths, int B, int train, float momentum, float max_norm,
               const LsAdam* adam, float* exp_avg_sq, hipStream_t st);
    void replayed(int B, int train);
    float* lr_target() const { return opts.groups ? const_cast<float*>(opts.groups_lr) : buf.lr; }
};

// average.hip: the accumulator's two launches (the average, then its count) and the in-place exchange of two arenas
int average_step(float* avg, const float* params, int64_t n, float* count, int kind, float decay, int64_t skip_begin, int64_t skip_end,
                 hipStream_t st);
int swap_arenas(float* a, float* b, int64_t n, hipStream_t st);

// the RNN plan as its PlanCore (its struct is private to rnn_plan.hip)
PlanCore* rnn_core(slnlp_rnn_plan* plan);

}  // namespace slnlp
