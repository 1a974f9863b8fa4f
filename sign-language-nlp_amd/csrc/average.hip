// average.hip -- a running average of the parameter arena, kept on the device (torch.optim.swa_utils.AveragedModel).
//
// The reference fights overfitting on a few thousand samples with dropout, EarlyStopping and ReduceLROnPlateau; averaging
// the iterates is the other standard remedy.  On the host it would cost an arena download and upload per update and could
// not ride a captured graph or a lockstep group, so the accumulator is one more arena-shaped buffer and two launches:
//
//   average_kernel        avg <- params                             while count[0] == 0 (bit copy)
//                         avg += (params - avg) / (count[0] + 1)    SLNLP_AVG_SWA  (AveragedModel's default avg_fn)
//                         avg += (params - avg) * (1 - decay)       SLNLP_AVG_EMA  (get_ema_multi_avg_fn: a lerp)
//   average_count_kernel  count[0] += 1, one thread, behind the update: every block of average_kernel reads the OLD count
//                         (the Adam step count's rule, update.hip).
//
// Floats [skip_begin, skip_end) -- a parameter torch never steps -- are copied, so the average equals the model there.  The
// update kernels are not touched: the accumulator reads the arena they leave behind (4 B / parameter more than a fused form
// would read).  Both kernels take the argument-pack form of launch.hpp, so a lockstep group runs them once for its K fits;
// a null `avg` in a pack means "this fit is not averaging yet" and the block returns.
//
// swap_kernel exchanges two arenas in place: evaluating with the averaged weights is swap, forward, swap -- the plans keep
// their parameter pointer, and two swaps restore every bit.
#include "plan_core.hpp"

namespace slnlp {

constexpr int AVG_MAX_BLOCKS = 2048;    // x 256 threads x one float4: arenas past 2 Mi floats wrap the stride loop

__device__ __forceinline__ void average_body(float* __restrict__ avg, const float* __restrict__ p, long n4, const float* __restrict__ count,
                                             int kind, float decay, long skip_begin4, long skip_end4) {
    if (!avg) return;
    const float c = count[0];
    const bool first = c == 0.f;
    const float den = c + 1.f, w = 1.f - decay;
    for (long i = blockIdx.x * 256L + threadIdx.x; i < n4; i += (long)gridDim.x * 256) {
        const float4 pv = reinterpret_cast<const float4*>(p)[i];
        if (first || (i >= skip_begin4 && i < skip_end4)) {
            reinterpret_cast<float4*>(avg)[i] = pv;
            continue;
        }
        const float4 av = reinterpret_cast<const float4*>(avg)[i];
        float a[4] = {av.x, av.y, av.z, av.w};
        const float q[4] = {pv.x, pv.y, pv.z, pv.w};
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const float d = q[e] - a[e];
            a[e] += kind == SLNLP_AVG_SWA ? d / den : d * w;
        }
        reinterpret_cast<float4*>(avg)[i] = make_float4(a[0], a[1], a[2], a[3]);
    }
}
SLNLP_ZKERNEL(average_kernel, 256, average_body)

__device__ __forceinline__ void average_count_body(float* __restrict__ avg, float* __restrict__ count) {
    if (avg && threadIdx.x == 0 && blockIdx.x == 0) count[0] += 1.f;
}
SLNLP_ZKERNEL(average_count_kernel, 64, average_count_body)

__global__ __launch_bounds__(256) void swap_kernel(float* __restrict__ a, float* __restrict__ b, long n4) {
    probe_kernel_begin();
    for (long i = blockIdx.x * 256L + threadIdx.x; i < n4; i += (long)gridDim.x * 256) {
        const float4 x = reinterpret_cast<const float4*>(a)[i], y = reinterpret_cast<const float4*>(b)[i];
        reinterpret_cast<float4*>(a)[i] = y;
        reinterpret_cast<float4*>(b)[i] = x;
    }
    probe_kernel_end();
}

static int arena_grid(int64_t n) {
    const int64_t g = (n / 4 + 255) / 256;
    return (int)(g > AVG_MAX_BLOCKS ? AVG_MAX_BLOCKS : g);
}

int average_step(float* avg, const float* params, int64_t n, float* count, int kind, float decay, int64_t skip_begin, int64_t skip_end,
                 hipStream_t st) {
    // (avg may be null while a lockstep group records: that fit's entry of the merged launch does nothing)
    SLNLP_CHECK_ARG(params && (count || !avg), "average_step: null pointer");
    SLNLP_CHECK_ARG(n > 0 && n % 4 == 0, "average_step: n=%ld must be a positive multiple of 4", (long)n);
    SLNLP_CHECK_ARG((((uintptr_t)avg | (uintptr_t)params) & 15) == 0 && ((uintptr_t)count & 3) == 0, "average_step: arenas must be 16-byte aligned");
    SLNLP_CHECK_ARG(kind == SLNLP_AVG_SWA || (kind == SLNLP_AVG_EMA && decay > 0.f && decay < 1.f),
                    "average_step: kind %d / decay %g (SLNLP_AVG_SWA, or SLNLP_AVG_EMA with 0 < decay < 1)", kind, decay);
    SLNLP_CHECK_ARG(skip_begin >= 0 && skip_end >= skip_begin && skip_end <= n && skip_begin % 4 == 0 && skip_end % 4 == 0,
                    "average_step: skip range [%ld, %ld) must lie in [0, %ld) on multiples of 4", (long)skip_begin, (long)skip_end, (long)n);
    SLNLP_CHECK_ARG(!avg || avg + n <= params || params + n <= avg, "average_step: avg and params overlap");
    SLNLP_TRY(zlaunch(average_kernel, dim3(arena_grid(n)), 256, 0, st, "average", avg, params, (long)(n / 4), (const float*)count, kind, decay,
                      (long)(skip_begin / 4), (long)(skip_end / 4)));
    return zlaunch(average_count_kernel, dim3(1), 64, 0, st, "average_count", avg, count);
}

int swap_arenas(float* a, float* b, int64_t n, hipStream_t st) {
    SLNLP_CHECK_ARG(a && b, "swap_arenas: null pointer");
    SLNLP_CHECK_ARG(n > 0 && n % 4 == 0, "swap_arenas: n=%ld must be a positive multiple of 4", (long)n);
    SLNLP_CHECK_ARG((((uintptr_t)a | (uintptr_t)b) & 15) == 0, "swap_arenas: arenas must be 16-byte aligned");
    SLNLP_CHECK_ARG(a + n <= b || b + n <= a, "swap_arenas: the two arenas overlap");
    hipLaunchKernelGGL(swap_kernel, dim3(arena_grid(n)), dim3(256), 0, st, a, b, (long)(n / 4));
    SLNLP_CHECK_LAUNCH("swap_arenas");
    return 0;
}

// ---- the plans' setting (plan_core.hpp)
int PlanCore::set_averaging(const char* what, float* avg, float* count, int kind, float decay) {
    if (!avg) {
        if (!averaging.avg) return 0;
        averaging = Averaging{};
    } else {
        SLNLP_CHECK_ARG(count, "%s: averaging needs its device count", what);
        SLNLP_CHECK_ARG(((uintptr_t)avg & 15) == 0 && (avg + arena <= buf.params || buf.params + arena <= avg),
                        "%s: avg must be a 16-byte aligned arena of its own", what);
        SLNLP_CHECK_ARG(kind == SLNLP_AVG_SWA || (kind == SLNLP_AVG_EMA && decay > 0.f && decay < 1.f),
                        "%s: kind %d / decay %g (SLNLP_AVG_SWA, or SLNLP_AVG_EMA with 0 < decay < 1)", what, kind, decay);
        if (kind == SLNLP_AVG_SWA) decay = 0.f;
        if (averaging.avg == avg && averaging.count == count && averaging.kind == kind && averaging.decay == decay) return 0;
        averaging = Averaging{avg, count, kind, decay};
    }
    ++opts.gen;             // a lockstep group re-records its programs: the launch sequence changed
    drop_graphs();
    return 0;
}

// behind the update of a train step: eager, captured and recorded alike
int PlanCore::average_after_update(hipStream_t st) {
    if (!averaging.avg && !averaging.forced) return 0;
    const UpdateRanges r = update_ranges();
    const bool skip = r.skip_end > r.skip_begin;
    return average_step(averaging.avg, buf.params, arena, averaging.count, averaging.kind, averaging.decay, skip ? r.skip_begin : 0,
                        skip ? r.skip_end : 0, st);
}

}  // namespace slnlp

extern "C" {

int slnlp_average_step(float* avg, const float* params, int64_t n, float* count, int kind, float decay, int64_t skip_begin,
                       int64_t skip_end, void* stream) {
    SLNLP_CHECK_ARG(avg && count, "average_step: null pointer");
    return slnlp::average_step(avg, params, n, count, kind, decay, skip_begin, skip_end, (hipStream_t)stream);
}

int slnlp_swap_arenas(float* a, float* b, int64_t n, void* stream) { return slnlp::swap_arenas(a, b, n, (hipStream_t)stream); }

}  // extern "C"
