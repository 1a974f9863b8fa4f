// plan_core.hip -- what every plan type does the same way (plan_core.hpp).
#include "plan_core.hpp"

namespace slnlp {

// A plan's criterion / update / param-group settings (TrainOpts, common.hpp)
TrainOpts::~TrainOpts() {
    if (class_weight) (void)hipFree(class_weight);
    param_groups_destroy(groups);
    param_groups_destroy(one);
}

int TrainOpts::one_segment(int64_t n, float wd, hipStream_t st, const slnlp_param_groups** out) {
    float have = 0.f;
    if (one) memcpy(&have, &one->host[2], sizeof(float));
    if (!one || one->n != n || have != wd) {
        // (a changed weight decay moved the settings generation: no recorded program reads the old table any more, and
        //  hipFree waits for the device)
        param_groups_destroy(one);
        one = nullptr;
        const int64_t begin = 0;
        const int group = 0;
        SLNLP_TRY(param_groups_create(n, 1, &begin, &group, 1, &wd, st, &one));
    }
    *out = one;
    return 0;
}

int TrainOpts::set_criterion(int V, const float* cw, float eps, int red, hipStream_t st, bool* changed) {
    SLNLP_CHECK_ARG(V > 0 && eps >= 0.f && eps <= 1.f && (red == 0 || red == 1),
                    "set_criterion: label_smoothing %g outside [0, 1] or reduction %d not 0 (mean) / 1 (sum)", eps, red);
    std::vector<float> host;
    if (cw) host.assign(cw, cw + V);   // host memory
    *changed = host != class_weight_host || eps != label_smoothing || red != reduction;
    if (!*changed) return 0;
    if (cw && !class_weight && hipMalloc(&class_weight, (size_t)V * sizeof(float)) != hipSuccess) {
        class_weight = nullptr;
        set_error("set_criterion: allocating the class weights failed");
        return SLNLP_ERR_LAUNCH;
    }
    class_weight_host.swap(host);
    // from the plan's own host copy (alive until the next change), ordered on the fit's stream before its next step
    if (cw && hipMemcpyAsync(class_weight, class_weight_host.data(), (size_t)V * sizeof(float), hipMemcpyHostToDevice, st) !=
                  hipSuccess) {
        set_error("set_criterion: copying the class weights failed");
        return SLNLP_ERR_LAUNCH;
    }
    if (!cw && class_weight) {
        (void)hipFree(class_weight);
        class_weight = nullptr;
    }
    label_smoothing = eps;
    reduction = red;
    ++gen;
    return 0;
}

int TrainOpts::set_update(int k, float damp, float wd, int nest, bool* changed) {
    SLNLP_CHECK_ARG(k == SLNLP_UPDATE_SGD || k == SLNLP_UPDATE_ADAM || k == SLNLP_UPDATE_ADAMW, "set_update: unknown kind %d", k);
    SLNLP_CHECK_ARG(damp >= 0.f && wd >= 0.f, "set_update: dampening %g / weight_decay %g must be >= 0", damp, wd);
    SLNLP_CHECK_ARG(!nest || damp == 0.f, "set_update: Nesterov momentum requires zero dampening");
    SLNLP_CHECK_ARG(k == SLNLP_UPDATE_SGD || (damp == 0.f && !nest), "set_update: dampening / nesterov are SGD's");
    nest = nest ? 1 : 0;
    *changed = k != kind || damp != dampening || wd != weight_decay || nest != nesterov;
    if (!*changed) return 0;
    kind = k; dampening = damp; weight_decay = wd; nesterov = nest;
    ++gen;
    return 0;
}

int TrainOpts::set_param_groups(int64_t n, int n_segments, const int64_t* seg_begin, const int* seg_group, int n_groups,
                                const float* wd, const float* lr_dev, hipStream_t st) {
    slnlp_param_groups* pg = nullptr;
    if (n_segments != 0) {
        SLNLP_CHECK_ARG(lr_dev, "set_param_groups: null lr_dev");
        SLNLP_TRY(param_groups_create(n, n_segments, seg_begin, seg_group, n_groups, wd, st, &pg));
    }
    // the old table may still be read by queued work: the caller drops its graphs (a device-wide wait) before this returns;
    // freeing goes through hipFree, which waits for the device itself
    param_groups_destroy(groups);
    groups = pg;
    groups_lr = pg ? lr_dev : nullptr;
    ++gen;
    return 0;
}

// clip_grad_norm_ + torch.optim.SGD on the arena.  Beside a grouped fit of a lockstep group a plan without groups records the
// same kernel with a one-segment table: its own lr scalar, its own weight decay
int PlanCore::update_sgd(float momentum, float max_norm, hipStream_t st) {
    StepScope scope(st);
    SLNLP_TRY(scope.rc);
    const slnlp_param_groups* pg = opts.groups;
    const float* lr = pg ? opts.groups_lr : buf.lr;
    if (!pg && opts.force_groups) SLNLP_TRY(opts.one_segment(arena, opts.sgd(nullptr, 0, 0).weight_decay, st, &pg));
    const UpdateRanges r = update_ranges();
    SLNLP_TRY(clip_sgd_step(buf.params, buf.grads, buf.momentum, arena, pg, lr, momentum, max_norm, opt_partials, buf.scalars + 1,
                            buf.rng, st, r.wp, r.wp_begin, r.wp_end, opts.sgd(buf.scalars + 3, r.skip_begin, r.skip_end)));
    SLNLP_TRY(average_after_update(st));
    if (!recording()) params_stepped();      // (a lockstep replay does this per step itself)
    return 0;
}

// clip_grad_norm_ + torch.optim.Adam / AdamW on the arena: exp_avg = buf.momentum, exp_avg_sq = the caller's arena-shaped
// buffer, step count = scalars[2] (advanced on the device).  With groups the weight decay is per group: the call's one value
// is not read
int PlanCore::update_adam(float* exp_avg_sq, float beta1, float beta2, float eps, float weight_decay, float max_norm, hipStream_t st) {
    StepScope scope(st);
    SLNLP_TRY(scope.rc);
    const slnlp_param_groups* pg = opts.groups;
    const float* lr = pg ? opts.groups_lr : buf.lr;
    if (!pg && opts.force_groups) SLNLP_TRY(opts.one_segment(arena, weight_decay, st, &pg));
    const UpdateRanges r = update_ranges();
    SLNLP_TRY(clip_adam_step(buf.params, buf.grads, buf.momentum, exp_avg_sq, arena, pg, lr, beta1, beta2, eps, weight_decay, max_norm,
                             opt_partials, buf.scalars + 1, buf.rng, buf.scalars + 2, st, r.wp, r.wp_begin, r.wp_end,
                             opts.adam(r.skip_begin, r.skip_end)));
    SLNLP_TRY(average_after_update(st));
    if (!recording()) params_stepped();
    return 0;
}

void PlanCore::drop_graphs() {
    if (graphs.empty()) return;
    (void)hipDeviceSynchronize();   // an exec may still be running
    for (auto& kv : graphs) (void)hipGraphExecDestroy(kv.second);
    graphs.clear();
}

int PlanCore::set_criterion(const float* class_weight, float label_smoothing, int reduction, hipStream_t st) {
    bool changed = false;
    SLNLP_TRY(opts.set_criterion(Vt, class_weight, label_smoothing, reduction, st, &changed));
    if (changed) drop_graphs();
    return 0;
}

int PlanCore::set_update(int kind, float dampening, float weight_decay, int nesterov) {
    bool changed = false;
    SLNLP_TRY(opts.set_update(kind, dampening, weight_decay, nesterov, &changed));
    if (changed) drop_graphs();
    return 0;
}

int PlanCore::set_param_groups(const char* what, int n_segments, const int64_t* seg_begin, const int32_t* seg_group, int n_groups,
                               const float* weight_decay, const float* lr_dev, hipStream_t st) {
    SLNLP_CHECK_ARG(n_segments >= 0, "%s: %d segments", what, n_segments);
    if (n_segments == 0 && !opts.groups) return 0;
    drop_graphs();                  // before the old table goes away: a captured update holds its pointers
    return opts.set_param_groups(arena, n_segments, seg_begin, seg_group, n_groups, weight_decay, lr_dev, st);
}

int PlanCore::train_step(const int64_t* X, const int64_t* y, const int64_t* lengths, int B, float momentum, float max_norm,
                         float* logp, hipStream_t st) {
    StepScope scope(st);            // one scope for the whole step (the nested calls re-enter it)
    SLNLP_TRY(scope.rc);
    SLNLP_TRY(forward(X, y, lengths, B, 1, logp, st));
    SLNLP_TRY(backward(st));
    return update_sgd(momentum, max_norm, st);
}

// Capture one train step (fixed X / y / lengths / logp device buffers and batch size) into a hipGraph and keep the executable
// graph in the plan; replay with graph_launch.  lr, rng step and the data are read from device memory, so the same graph
// serves every step of a fit.
int PlanCore::graph_capture_train(const char* what, const int64_t* X, const int64_t* y, const int64_t* lengths, int B, float momentum,
                                  float max_norm, float* logp, hipStream_t st) {
    SLNLP_CHECK_ARG(st, "%s: needs a plan and a non-default stream", what);
    SLNLP_TRY(prepare_planes(B, st));       // must not be captured: it runs once per batch-size change
    auto old = graphs.find(B);
    if (old != graphs.end()) {              // re-capture for this batch size: the old exec may still be running
        (void)hipStreamSynchronize(st);
        (void)hipGraphExecDestroy(old->second);
        graphs.erase(old);
    }
    if (hipStreamBeginCapture(st, hipStreamCaptureModeThreadLocal) != hipSuccess) {
        set_error("%s: begin capture failed: %s", what, hipGetErrorString(hipGetLastError()));
        return SLNLP_ERR_LAUNCH;
    }
    before_capture();
    int rc = train_step(X, y, lengths, B, momentum, max_norm, logp, st);
    hipGraph_t g = nullptr;
    hipError_t e = hipStreamEndCapture(st, &g);
    if (rc != 0) {
        if (g) (void)hipGraphDestroy(g);
        return rc;
    }
    if (e != hipSuccess || !g) {
        set_error("%s: end capture failed: %s", what, hipGetErrorString(e));
        return SLNLP_ERR_LAUNCH;
    }
    hipGraphExec_t exec = nullptr;
    e = hipGraphInstantiate(&exec, g, nullptr, nullptr, 0);
    (void)hipGraphDestroy(g);
    if (e != hipSuccess) {
        set_error("%s: instantiate failed: %s", what, hipGetErrorString(e));
        return SLNLP_ERR_LAUNCH;
    }
    graphs[B] = exec;
    return 0;
}

int PlanCore::graph_launch(const char* what, int B, hipStream_t st) {
    auto it = graphs.find(B);
    SLNLP_CHECK_ARG(it != graphs.end(), "%s: no captured graph for batch %d", what, B);
    StepScope scope(st);
    SLNLP_TRY(scope.rc);
    SLNLP_TRY(prepare_planes(B, st));
    if (hipGraphLaunch(it->second, st) != hipSuccess) {
        set_error("%s: %s", what, hipGetErrorString(hipGetLastError()));
        return SLNLP_ERR_LAUNCH;
    }
    params_stepped();
    return 0;
}

void PlanCore::destroy() {
    if (!graphs.empty()) (void)hipDeviceSynchronize();   // graph execs are torn down below
    else slnlp::destroy_sync(destroy_sync);              // nothing of this plan may still be in flight when its buffers go
    for (auto& kv : graphs) (void)hipGraphExecDestroy(kv.second);
    delete this;
}

int PlanCore::record(const int64_t* X, const int64_t* y, const int64_t* lengths, int B, int train, float momentum, float max_norm,
                     const LsAdam* adam, float* exp_avg_sq, hipStream_t st) {
    SLNLP_TRY(check_recordable());
    SLNLP_TRY(forward(X, y, lengths, B, train, nullptr, st));
    if (!train) return 0;
    SLNLP_TRY(backward(st));
    if (adam)
        return update_adam(exp_avg_sq, adam->beta1, adam->beta2, adam->eps, opts.adam_weight_decay(adam->weight_decay), max_norm, st);
    return update_sgd(momentum, max_norm, st);
}

void PlanCore::replayed(int B, int train) {
    last_B = B;
    last_p = train ? dropout : 0.f;
    if (train) params_stepped();
}

}  // namespace slnlp
