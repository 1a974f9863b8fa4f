// update.hip -- the fused optimizer step over one flat arena: grad-norm clip + torch.optim.SGD / Adam / AdamW, with one
// learning rate and weight decay for the arena or per parameter group.  HBM-bound, fp32, 16-B vector accesses.
#include "common.hpp"
#include "launch.hpp"

namespace slnlp {

// ================================================================= optimizer
// clip_grad_norm_(max_norm) + torch.optim.SGD(momentum) over one flat arena.
constexpr int OPT_BLOCKS = 1024;

__device__ __forceinline__ void sumsq_body(const float* __restrict__ g, long n4, float* __restrict__ partials,
                                           float* __restrict__ sgd_steps) {
    // sgd_steps (optional): the SGD step count, advanced HERE -- before the update launch, which only reads it (every block
    // of sgd_kernel sees the same value: 1 on the first step)
    if (sgd_steps && blockIdx.x == 0 && threadIdx.x == 0) sgd_steps[0] += 1.f;
    __shared__ float red[4];
    float s = 0.f;
    for (long i = blockIdx.x * 256L + threadIdx.x; i < n4; i += (long)OPT_BLOCKS * 256) {
        const float4 v = reinterpret_cast<const float4*>(g)[i];
        s += v.x * v.x + v.y * v.y + v.z * v.z + v.w * v.w;
    }
    s = wave_sum(s);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
    __syncthreads();
    if (threadIdx.x == 0) partials[blockIdx.x] = red[0] + red[1] + red[2] + red[3];
}
SLNLP_ZKERNEL(sumsq_kernel, 256, sumsq_body)

// ------------------------------------------------ the pieces every update kernel shares ----
// Every block re-derives the gradient norm from sumsq's partials in the same fixed order (deterministic, no third launch) and
// from it the clip coefficient.  Its barrier also publishes what the caller staged in LDS before the call.
__device__ __forceinline__ float clip_coef(const float* __restrict__ partials, float max_norm, float& norm) {
    __shared__ float red[4];
    float s = 0.f;
    for (int i = threadIdx.x; i < OPT_BLOCKS; i += 256) s += partials[i];
    s = wave_sum(s);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
    __syncthreads();
    norm = sqrtf(red[0] + red[1] + red[2] + red[3]);
    // a NaN norm (one NaN gradient element) gives a NaN coefficient, as torch's clamp does: fminf alone would return its other
    // operand, 1, and every finite element would take an unclipped step.  An infinite norm gives 0
    const float coef = norm != norm ? norm : fminf(max_norm / (norm + 1e-6f), 1.f);
    return max_norm > 0.f ? coef : 1.f;
}

__device__ __forceinline__ void update_done(float norm, float* __restrict__ norm_out, unsigned long long* __restrict__ rng) {
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        if (norm_out) norm_out[0] = norm;
        if (rng) rng[1] += 1ull;
    }
}

// Where a float4's learning rate and weight decay come from.  TABLE false: one pair for the arena, gt.lr[0] and the launch's
// scalar.  TABLE true (optimizer__param_groups): the segment its index falls in.  The table is staged in LDS once per block
// with the group's settings resolved per segment, so the loop does one short binary search over LDS (no global reads) per
// float4; segment boundaries are float4 indices, so the four floats of a vector always share a group.  Both kinds run the
// same body: a one-segment table gives the one-pair kernel's bits.
struct GroupLds {
    int begin[GROUPS_MAX_SEGMENTS];
    float lr[GROUPS_MAX_SEGMENTS], wd[GROUPS_MAX_SEGMENTS];
};
__device__ __forceinline__ GroupLds& group_lds() {
    __shared__ GroupLds tab;
    return tab;
}

template <bool TABLE>
struct Rates {
    float lr = 0.f, wd = 0.f;
    int n_seg = 0;
    // before clip_coef(), whose barrier publishes the table
    __device__ __forceinline__ void stage(const GroupTab& gt) {
        if constexpr (TABLE) {
            GroupLds& t = group_lds();
            n_seg = gt.n_seg;
            for (int s = threadIdx.x; s < gt.n_seg; s += 256) {
                const int gi = gt.seg_group[s];
                t.begin[s] = gt.seg_begin4[s];
                t.lr[s] = gt.lr[gi];
                t.wd[s] = gt.wd[gi];
            }
        }
    }
    // behind it
    __device__ __forceinline__ void one_pair(const GroupTab& gt, float weight_decay) {
        if constexpr (!TABLE) {
            lr = gt.lr[0];
            wd = weight_decay;
        }
    }
    // of float4 index i: its segment is the last s with begin[s] <= i (begin[0] == 0)
    __device__ __forceinline__ void at(long i, float& lr_i, float& wd_i) const {
        if constexpr (TABLE) {
            const GroupLds& t = group_lds();
            int lo = 0, hi = n_seg;
            while (hi - lo > 1) {
                const int mid = (lo + hi) >> 1;
                if ((long)t.begin[mid] <= i) lo = mid;
                else hi = mid;
            }
            lr_i = t.lr[lo];
            wd_i = t.wd[lo];
        } else {
            lr_i = lr;
            wd_i = wd;
        }
    }
};

// general: dampening, nesterov or any weight decay.  The one-pair kernel decides it from its own scalars; with a table the
// host does (ANY group's weight decay) and weight_decay is not read.
template <bool TABLE>
__device__ __forceinline__ void sgd_body(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ buf, long n4,
                                         GroupTab gt, float momentum, float max_norm, const float* __restrict__ partials,
                                         float* __restrict__ norm_out, unsigned long long* __restrict__ rng, PlaneOut wp,
                                         long wp_begin4, long wp_end4, float dampening, float weight_decay, int general,
                                         int nesterov, const float* __restrict__ sgd_steps, long skip_begin4, long skip_end4) {
    // wp (optional): the updated weights also leave as bf16 hi / lo planes (same offsets as the arena) -- the operand
    // form the plane GEMMs of the NEXT step stage by LDS-DMA -- instead of a separate pass that re-reads the arena.
    // Only float4 indices in [wp_begin4, wp_end4) are written: the plan passes the range of the weights that FEED plane GEMMs
    // (the encoder layers: a third of a Transformer's parameters), the rest of the plane arena has no reader
    Rates<TABLE> rates;
    rates.stage(gt);
    float norm;
    const float coef = clip_coef(partials, max_norm, norm);
    rates.one_pair(gt, weight_decay);
    if constexpr (!TABLE) general = dampening != 0.f || weight_decay != 0.f || nesterov;
    if (general) {
        // torch/optim/sgd.py _single_tensor_sgd: d = g' + wd p; buf = d on the first step, else m buf + (1 - dampening) d;
        // d = d + m buf (nesterov) or buf; p -= lr d.  Float indices [skip_begin4, skip_end4) are a parameter torch never
        // steps (its grad is None): left untouched.  Kept apart from the plain loop below, whose arithmetic stays as it was.
        const bool first = sgd_steps[0] == 1.f;
        const float damp = first ? 0.f : 1.f - dampening, keep = first ? 0.f : momentum;
        for (long i = blockIdx.x * 256L + threadIdx.x; i < n4; i += (long)gridDim.x * 256) {
            float4 w = reinterpret_cast<float4*>(p)[i];
            if (i < skip_begin4 || i >= skip_end4) {
                float lr, wd;
                rates.at(i, lr, wd);
                const float4 gv = reinterpret_cast<const float4*>(g)[i];
                float4 b = reinterpret_cast<float4*>(buf)[i];
                float ge[4] = {gv.x * coef, gv.y * coef, gv.z * coef, gv.w * coef};
                float be[4] = {b.x, b.y, b.z, b.w}, we[4] = {w.x, w.y, w.z, w.w};
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    float d = ge[e] + wd * we[e];
                    be[e] = first ? d : keep * be[e] + damp * d;
                    d = nesterov ? d + momentum * be[e] : be[e];
                    we[e] -= lr * d;
                }
                b = make_float4(be[0], be[1], be[2], be[3]);
                w = make_float4(we[0], we[1], we[2], we[3]);
                reinterpret_cast<float4*>(buf)[i] = b;
                reinterpret_cast<float4*>(p)[i] = w;
            }
            if (i >= wp_begin4 && i < wp_end4) store_planes4(wp, i * 4, w);
        }
        update_done(norm, norm_out, rng);
        return;
    }
    for (long i = blockIdx.x * 256L + threadIdx.x; i < n4; i += (long)gridDim.x * 256) {
        float lr, wd;
        rates.at(i, lr, wd);
        const float4 gv = reinterpret_cast<const float4*>(g)[i];
        float4 b = reinterpret_cast<float4*>(buf)[i];
        float4 w = reinterpret_cast<float4*>(p)[i];
        b.x = momentum * b.x + gv.x * coef; b.y = momentum * b.y + gv.y * coef;
        b.z = momentum * b.z + gv.z * coef; b.w = momentum * b.w + gv.w * coef;
        w.x -= lr * b.x; w.y -= lr * b.y; w.z -= lr * b.z; w.w -= lr * b.w;
        reinterpret_cast<float4*>(buf)[i] = b;
        reinterpret_cast<float4*>(p)[i] = w;
        if (i >= wp_begin4 && i < wp_end4) store_planes4(wp, i * 4, w);
    }
    update_done(norm, norm_out, rng);
}
SLNLP_ZKERNEL(sgd_kernel, 256, sgd_body<false>)
SLNLP_ZKERNEL(sgd_groups_kernel, 256, sgd_body<true>)

// torch.optim.Adam (amsgrad False, maximize False) fused with clip_grad_norm_, same two-launch shape as clip + SGD:
//   g' = g * clip_coef (+ weight_decay * p);  m += (1 - b1)(g' - m);  v = b2 v + (1 - b2) g'^2;
//   p -= (lr / (1 - b1^t)) * m / (sqrt(v) / sqrt(1 - b2^t) + eps)            (torch/optim/adam.py _single_tensor_adam)
// The step count t lives in device memory (step_f[0], a float: exact to 2^24 steps) and is advanced on the device, so a
// captured or recorded step needs no host-side argument that changes per step.  With a table weight_decay is not read.
template <bool TABLE>
__device__ __forceinline__ void adam_body(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m,
                                          float* __restrict__ v, long n4, GroupTab gt, float beta1, float beta2, float eps,
                                          float weight_decay, float max_norm, const float* __restrict__ partials,
                                          float* __restrict__ norm_out, unsigned long long* __restrict__ rng,
                                          float* __restrict__ step_f, PlaneOut wp, long wp_begin4, long wp_end4, int decoupled,
                                          long skip_begin4, long skip_end4) {
    // decoupled (torch.optim.AdamW): p *= 1 - lr wd first, then the Adam update with no L2 term; float indices
    // [skip_begin4, skip_end4) (a parameter torch never steps) are left untouched.  Plain Adam ignores the skip range.
    Rates<TABLE> rates;
    rates.stage(gt);
    float norm;
    const float coef = clip_coef(partials, max_norm, norm);
    rates.one_pair(gt, weight_decay);
    const float t = step_f[0] + 1.f;                       // every block reads the OLD count (adam_count_kernel advances it afterwards)
    const float bc1 = 1.f - powf(beta1, t), bc2 = 1.f - powf(beta2, t);
    const float rsq_bc2 = 1.f / sqrtf(bc2);
    for (long i = blockIdx.x * 256L + threadIdx.x; i < n4; i += (long)gridDim.x * 256) {
        if (decoupled && i >= skip_begin4 && i < skip_end4) {
            if (i >= wp_begin4 && i < wp_end4) store_planes4(wp, i * 4, reinterpret_cast<const float4*>(p)[i]);
            continue;
        }
        float lr, wd;
        rates.at(i, lr, wd);
        const float step_size = lr / bc1;
        const float l2 = decoupled ? 0.f : wd, decay = 1.f - lr * wd;
        const float4 gv = reinterpret_cast<const float4*>(g)[i];
        float4 mm = reinterpret_cast<float4*>(m)[i], vv = reinterpret_cast<float4*>(v)[i], w = reinterpret_cast<float4*>(p)[i];
        float ge[4] = {gv.x * coef, gv.y * coef, gv.z * coef, gv.w * coef};
        float me[4] = {mm.x, mm.y, mm.z, mm.w}, ve[4] = {vv.x, vv.y, vv.z, vv.w}, we[4] = {w.x, w.y, w.z, w.w};
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            if (decoupled) we[e] *= decay;
            if (l2 != 0.f) ge[e] += l2 * we[e];
            me[e] += (1.f - beta1) * (ge[e] - me[e]);
            ve[e] = beta2 * ve[e] + (1.f - beta2) * ge[e] * ge[e];
            we[e] -= step_size * (me[e] / (sqrtf(ve[e]) * rsq_bc2 + eps));
        }
        reinterpret_cast<float4*>(m)[i] = make_float4(me[0], me[1], me[2], me[3]);
        reinterpret_cast<float4*>(v)[i] = make_float4(ve[0], ve[1], ve[2], ve[3]);
        const float4 wn = make_float4(we[0], we[1], we[2], we[3]);
        reinterpret_cast<float4*>(p)[i] = wn;
        if (i >= wp_begin4 && i < wp_end4) store_planes4(wp, i * 4, wn);
    }
    update_done(norm, norm_out, rng);
}
SLNLP_ZKERNEL(adam_kernel, 256, adam_body<false>)
SLNLP_ZKERNEL(adam_groups_kernel, 256, adam_body<true>)

// the count is advanced by its own one-thread launch AFTER the update (every block of the Adam kernels must read the same old value)
__device__ __forceinline__ void adam_count_body(float* __restrict__ step_f) { if (threadIdx.x == 0 && blockIdx.x == 0) step_f[0] += 1.f; }
SLNLP_ZKERNEL(adam_count_kernel, 64, adam_count_body)

// What both updates check and derive the same way.  n against the table, the arenas' alignment (arena_bits: their addresses
// or-ed), the skip range [skip_begin, skip_end) in floats (multiples of 4; empty when skip_end <= skip_begin); then the float4
// ranges of the skip and of the planes written, and the update's grid.  pg (optional): the launch's one-pair table otherwise
struct UpdateLaunch {
    long n4, sb4, se4, wb4, we4;
    int grid;
    GroupTab gt;
};
static int update_launch(const char* what, int64_t n, const slnlp_param_groups* pg, const float* lr_dev, uintptr_t arena_bits,
                         int64_t skip_begin, int64_t skip_end, int64_t wp_begin, int64_t wp_end, UpdateLaunch* u) {
    if (pg)
        SLNLP_CHECK_ARG(n > 0 && n % 4 == 0 && n == pg->n, "%s: n=%ld must be the table's (%ld), a positive multiple of 4", what, (long)n,
                        (long)pg->n);
    else
        SLNLP_CHECK_ARG(n > 0 && n % 4 == 0, "%s: n=%ld must be a positive multiple of 4", what, (long)n);
    SLNLP_CHECK_ARG((arena_bits & 15) == 0, "%s: arenas must be 16-byte aligned", what);
    const bool skip = skip_end > skip_begin;
    SLNLP_CHECK_ARG(!skip || (skip_begin >= 0 && skip_end <= n && skip_begin % 4 == 0 && skip_end % 4 == 0),
                    "%s: skip range [%ld, %ld) must lie in [0, %ld) on multiples of 4", what, (long)skip_begin, (long)skip_end, (long)n);
    u->n4 = (long)(n / 4);
    u->sb4 = skip ? (long)(skip_begin / 4) : 0;
    u->se4 = skip ? (long)(skip_end / 4) : 0;
    u->wb4 = (long)(wp_begin / 4);
    u->we4 = (long)(wp_end < 0 ? n / 4 : (wp_end + 3) / 4);
    u->grid = ceil_div(n / 4, 256);
    if (u->grid > 2048) u->grid = 2048;
    u->gt = pg ? pg->tab(lr_dev) : GroupTab{nullptr, nullptr, nullptr, lr_dev, 0};
    return 0;
}

// pg (optional): lr_dev holds the groups' rates and each group decays with its own weight decay (so.weight_decay is not read)
int clip_sgd_step(float* params, const float* grads, float* momentum_buf, int64_t n, const slnlp_param_groups* pg, const float* lr_dev,
                  float momentum, float max_norm, float* partials, float* norm_out, unsigned long long* rng,
                  hipStream_t st, PlaneOut wp, int64_t wp_begin, int64_t wp_end, SgdOpts so) {
    const char* what = pg ? "clip_sgd_step_groups" : "clip_sgd_step";
    SLNLP_CHECK_ARG(params && grads && momentum_buf && lr_dev && partials, "%s: null pointer", what);
    UpdateLaunch u;
    SLNLP_TRY(update_launch(what, n, pg, lr_dev, (uintptr_t)params | (uintptr_t)grads | (uintptr_t)momentum_buf, so.skip_begin,
                            so.skip_end, wp_begin, wp_end, &u));
    // torch's argument rules (torch.optim.SGD.__init__); without momentum torch keeps no buffer, so dampening is moot
    if (pg)
        SLNLP_CHECK_ARG(so.dampening >= 0.f && (!so.nesterov || (momentum > 0.f && so.dampening == 0.f)),
                        "clip_sgd_step_groups: bad dampening %g / nesterov (needs momentum > 0 and dampening 0)", so.dampening);
    else
        SLNLP_CHECK_ARG(so.dampening >= 0.f && so.weight_decay >= 0.f && (!so.nesterov || (momentum > 0.f && so.dampening == 0.f)),
                        "clip_sgd_step: bad dampening %g / weight_decay %g / nesterov (needs momentum > 0 and dampening 0)",
                        so.dampening, so.weight_decay);
    const float damp = momentum != 0.f ? so.dampening : 0.f;
    const bool general = damp != 0.f || (pg ? pg->any_wd : so.weight_decay != 0.f) || so.nesterov;
    SLNLP_CHECK_ARG(!general || so.steps, "%s: dampening / weight decay / nesterov need the step counter", what);
    SLNLP_TRY(zlaunch(sumsq_kernel, dim3(OPT_BLOCKS), 256, 0, st, "sumsq", grads, u.n4, partials, so.steps));
    return zlaunch(pg ? sgd_groups_kernel : sgd_kernel, dim3(u.grid), 256, 0, st, pg ? "sgd_groups" : "sgd",
                   params, grads, momentum_buf, u.n4, u.gt, momentum, max_norm, partials, norm_out, rng, wp, u.wb4, u.we4, damp,
                   so.weight_decay, general ? 1 : 0, so.nesterov ? 1 : 0, (const float*)so.steps, u.sb4, u.se4);
}

// pg (optional): lr_dev holds the groups' rates and each group decays with its own weight decay (weight_decay is not read)
int clip_adam_step(float* params, const float* grads, float* exp_avg, float* exp_avg_sq, int64_t n, const slnlp_param_groups* pg,
                   const float* lr_dev, float beta1, float beta2, float eps, float weight_decay, float max_norm, float* partials,
                   float* norm_out, unsigned long long* rng, float* step_f, hipStream_t st, PlaneOut wp, int64_t wp_begin, int64_t wp_end,
                   AdamOpts ao) {
    const char* what = pg ? "clip_adam_step_groups" : "clip_adam_step";
    SLNLP_CHECK_ARG(params && grads && exp_avg && exp_avg_sq && lr_dev && partials && step_f, "%s: null pointer", what);
    UpdateLaunch u;
    SLNLP_TRY(update_launch(what, n, pg, lr_dev, (uintptr_t)params | (uintptr_t)grads | (uintptr_t)exp_avg | (uintptr_t)exp_avg_sq,
                            ao.skip_begin, ao.skip_end, wp_begin, wp_end, &u));
    SLNLP_CHECK_ARG(pg || weight_decay >= 0.f, "clip_adam_step: weight_decay %g < 0", weight_decay);
    SLNLP_CHECK_ARG(beta1 >= 0.f && beta1 < 1.f && beta2 >= 0.f && beta2 < 1.f && eps >= 0.f, "%s: bad betas / eps", what);
    SLNLP_TRY(zlaunch(sumsq_kernel, dim3(OPT_BLOCKS), 256, 0, st, "sumsq", grads, u.n4, partials, (float*)nullptr));
    SLNLP_TRY(zlaunch(pg ? adam_groups_kernel : adam_kernel, dim3(u.grid), 256, 0, st, pg ? "adam_groups" : "adam",
                      params, grads, exp_avg, exp_avg_sq, u.n4, u.gt, beta1, beta2, eps, weight_decay, max_norm, partials, norm_out, rng,
                      step_f, wp, u.wb4, u.we4, ao.decoupled ? 1 : 0, u.sb4, u.se4));
    return zlaunch(adam_count_kernel, dim3(1), 64, 0, st, "adam_count", step_f);
}

int param_groups_create(int64_t n, int n_segments, const int64_t* seg_begin, const int* seg_group, int n_groups,
                        const float* weight_decay, hipStream_t st, slnlp_param_groups** out) {
    SLNLP_CHECK_ARG(out && seg_begin && seg_group && weight_decay, "param_groups_create: null pointer");
    *out = nullptr;
    SLNLP_CHECK_ARG(n > 0 && n % 4 == 0 && n / 4 < 0x7fffffffL, "param_groups_create: n=%ld must be a positive multiple of 4", (long)n);
    SLNLP_CHECK_ARG(n_segments >= 1 && n_segments <= GROUPS_MAX_SEGMENTS && n_groups >= 1 && n_groups <= n_segments,
                    "param_groups_create: %d segments (1..%d) in %d groups (1..segments)", n_segments, GROUPS_MAX_SEGMENTS, n_groups);
    SLNLP_CHECK_ARG(seg_begin[0] == 0, "param_groups_create: the first segment must begin at 0");
    for (int s = 0; s < n_segments; ++s) {
        SLNLP_CHECK_ARG(seg_begin[s] % 4 == 0 && seg_begin[s] < n && (s == 0 || seg_begin[s] > seg_begin[s - 1]),
                        "param_groups_create: segment %d begins at %ld: must be a multiple of 4 in [0, %ld), strictly increasing", s,
                        (long)seg_begin[s], (long)n);
        SLNLP_CHECK_ARG(seg_group[s] >= 0 && seg_group[s] < n_groups, "param_groups_create: segment %d in group %d of %d", s, seg_group[s],
                        n_groups);
    }
    bool any = false;
    for (int gi = 0; gi < n_groups; ++gi) {
        SLNLP_CHECK_ARG(weight_decay[gi] >= 0.f, "param_groups_create: weight_decay %g of group %d < 0", weight_decay[gi], gi);
        any = any || weight_decay[gi] != 0.f;
    }
    slnlp_param_groups* pg = new slnlp_param_groups;
    pg->n = n; pg->n_seg = n_segments; pg->n_groups = n_groups; pg->any_wd = any;
    pg->host.resize(2 * (size_t)n_segments + n_groups);
    for (int s = 0; s < n_segments; ++s) {
        pg->host[s] = (int)(seg_begin[s] / 4);
        pg->host[n_segments + s] = seg_group[s];
    }
    memcpy(pg->host.data() + 2 * (size_t)n_segments, weight_decay, (size_t)n_groups * sizeof(float));
    const size_t bytes = pg->host.size() * sizeof(int);
    if (hipMalloc(&pg->dev, bytes) != hipSuccess ||
        hipMemcpyAsync(pg->dev, pg->host.data(), bytes, hipMemcpyHostToDevice, st) != hipSuccess) {
        set_error("param_groups_create: allocating / uploading the table failed: %s", hipGetErrorString(hipGetLastError()));
        param_groups_destroy(pg);
        return SLNLP_ERR_LAUNCH;
    }
    *out = pg;
    return 0;
}

void param_groups_destroy(slnlp_param_groups* pg) {
    if (!pg) return;
    if (pg->dev) (void)hipFree(pg->dev);
    delete pg;
}

}  // namespace slnlp

extern "C" {
int slnlp_clip_sgd_step(float* params, const float* grads, float* momentum_buf, int64_t n, const float* lr_dev,
                        float momentum, float max_norm, float* partials, float* norm_out, unsigned long long* rng,
                        void* stream) {
    return slnlp::clip_sgd_step(params, grads, momentum_buf, n, nullptr, lr_dev, momentum, max_norm, partials, norm_out, rng,
                                (hipStream_t)stream);
}
int slnlp_clip_sgd_step_ex(float* params, const float* grads, float* momentum_buf, int64_t n, const float* lr_dev,
                           float momentum, float dampening, float weight_decay, int nesterov, float max_norm, float* partials,
                           float* norm_out, float* step_count, int64_t skip_begin, int64_t skip_end, void* stream) {
    return slnlp::clip_sgd_step(params, grads, momentum_buf, n, nullptr, lr_dev, momentum, max_norm, partials, norm_out, nullptr,
                                (hipStream_t)stream, slnlp::PlaneOut{}, 0, -1,
                                slnlp::SgdOpts{dampening, weight_decay, nesterov, step_count, skip_begin, skip_end});
}
int slnlp_clip_adamw_step(float* params, const float* grads, float* exp_avg, float* exp_avg_sq, int64_t n, const float* lr_dev,
                          float beta1, float beta2, float eps, float weight_decay, float max_norm, float* partials, float* norm_out,
                          float* step_count, int64_t skip_begin, int64_t skip_end, void* stream) {
    return slnlp::clip_adam_step(params, grads, exp_avg, exp_avg_sq, n, nullptr, lr_dev, beta1, beta2, eps, weight_decay, max_norm, partials,
                                 norm_out, nullptr, step_count, (hipStream_t)stream, slnlp::PlaneOut{}, 0, -1,
                                 slnlp::AdamOpts{1, skip_begin, skip_end});
}
int slnlp_clip_adam_step(float* params, const float* grads, float* exp_avg, float* exp_avg_sq, int64_t n, const float* lr_dev,
                         float beta1, float beta2, float eps, float weight_decay, float max_norm, float* partials, float* norm_out,
                         float* step_count, void* stream) {
    return slnlp::clip_adam_step(params, grads, exp_avg, exp_avg_sq, n, nullptr, lr_dev, beta1, beta2, eps, weight_decay, max_norm, partials,
                                 norm_out, nullptr, step_count, (hipStream_t)stream);
}
int slnlp_param_groups_create(int64_t n, int n_segments, const int64_t* seg_begin, const int32_t* seg_group, int n_groups,
                              const float* weight_decay, void* stream, slnlp_param_groups** out) {
    return slnlp::param_groups_create(n, n_segments, seg_begin, seg_group, n_groups, weight_decay, (hipStream_t)stream, out);
}
void slnlp_param_groups_destroy(slnlp_param_groups* groups) { slnlp::param_groups_destroy(groups); }
int slnlp_clip_sgd_step_groups(float* params, const float* grads, float* momentum_buf, int64_t n, const slnlp_param_groups* groups,
                               const float* lr_dev, float momentum, float dampening, int nesterov, float max_norm, float* partials,
                               float* norm_out, float* step_count, int64_t skip_begin, int64_t skip_end, void* stream) {
    SLNLP_CHECK_ARG(groups, "clip_sgd_step_groups: null pointer");
    return slnlp::clip_sgd_step(params, grads, momentum_buf, n, groups, lr_dev, momentum, max_norm, partials, norm_out, nullptr,
                                (hipStream_t)stream, slnlp::PlaneOut{}, 0, -1,
                                slnlp::SgdOpts{dampening, 0.f, nesterov, step_count, skip_begin, skip_end});
}
int slnlp_clip_adam_step_groups(float* params, const float* grads, float* exp_avg, float* exp_avg_sq, int64_t n,
                                const slnlp_param_groups* groups, const float* lr_dev, float beta1, float beta2, float eps,
                                int decoupled, float max_norm, float* partials, float* norm_out, float* step_count,
                                int64_t skip_begin, int64_t skip_end, void* stream) {
    SLNLP_CHECK_ARG(groups, "clip_adam_step_groups: null pointer");
    return slnlp::clip_adam_step(params, grads, exp_avg, exp_avg_sq, n, groups, lr_dev, beta1, beta2, eps, 0.f, max_norm, partials,
                                 norm_out, nullptr, step_count, (hipStream_t)stream, slnlp::PlaneOut{}, 0, -1,
                                 slnlp::AdamOpts{decoupled ? 1 : 0, skip_begin, skip_end});
}
}
