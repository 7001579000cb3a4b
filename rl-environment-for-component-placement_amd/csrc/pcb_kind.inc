// pcb_kind.inc -- kernel instantiations and launch switch of ONE environment kind (PCB_KIND / PCB_KIND_NAME set by the
// including pcb_kind_<name>[_<part>].hip).  Build: hipcc --offload-arch=gfx950 -O3 -ffp-contract=off (one IEEE operation
// per written operator; the only fused multiply-add is the explicit __fma_rn in norm2).
// The pin kinds are split into PARTS, one translation unit each, so that the build is as long as its slowest part:
//   0 = reset + gather + launch switch + k_step without routes (in-place and rollout builds), 1 = k_step without routes, one
//   transition into a trajectory slot, 2 / 3 = k_step with beam / both routes on one / four wavefronts, 4 = the in-place
//   k_step without routes on one wavefront with the 64 x 64 grid compiled in (STEP_GEO_64);
// PCB_PART undefined = a kind without routes (square, rect), everything in one unit.
// (The slot build has a unit of its own for its code, not only for the build time: next to the rollout build every
// function only the trajectory layout uses has two callers instead of one and is no longer inlined -- 437 instead of
// 143 spilled scalars in the spatial kernel and 76 instead of 68 us per c4 step.)
#include "pcb_kernels.h"
#include "pcb_launch.h"

#define PCB_CAT3_(a, b, c) a##b##c
#define PCB_CAT3(a, b, c) PCB_CAT3_(a, b, c)
#define PCB_FN(stem) PCB_CAT3(stem, _, PCB_KIND_NAME)
static constexpr int KIND = PCB_KIND;
#ifdef PCB_PART
#define PCB_HAS(part) (PCB_PART == (part))
#define PCB_ROUTES 1
#else
#define PCB_HAS(part) ((part) <= 1)
#define PCB_ROUTES 0
#endif

int PCB_FN(pcb_step_plain)(const StepLaunch &a);
int PCB_FN(pcb_step_slot)(const StepLaunch &a);
int PCB_FN(pcb_step_routed1)(const StepLaunch &a);
int PCB_FN(pcb_step_routed4)(const StepLaunch &a);
int PCB_FN(pcb_step_fixed)(const StepLaunch &a);

// the build of the launch (pcb_kernels.h STEP_BUILD_*): in-place layout with the store policy compiled in, one transition
// into a trajectory slot, or the persistent rollout
#define LAUNCH_STEP_(WW_, NW_, RT_, BUILD_) hipLaunchKernelGGL((k_step<KIND, WW_, NW_, RT_, BUILD_>), dim3(d.B + d.term_wgs * d.term_hpe), dim3(64 * NW_), d.ldsBytes, a.stream, d, a.actions, a.fmt, a.sampled, a.seed, a.first_env, a.step_index, a.num_steps)
#define LAUNCH_STEP_INPLACE_OR_ROLLOUT(WW_, NW_, RT_) do { \
    if (a.traj) LAUNCH_STEP_(WW_, NW_, RT_, STEP_BUILD_ROLLOUT); \
    else if (d.stream_stores) LAUNCH_STEP_(WW_, NW_, RT_, STEP_BUILD_INPLACE_STREAM); \
    else LAUNCH_STEP_(WW_, NW_, RT_, STEP_BUILD_INPLACE); } while (0)
#define LAUNCH_STEP_ROUTED(WW_, NW_) do { \
    if (a.traj && a.num_steps == 1) LAUNCH_STEP_(WW_, NW_, true, STEP_BUILD_SLOT); else LAUNCH_STEP_INPLACE_OR_ROLLOUT(WW_, NW_, true); } while (0)

// The run-time shape of a launch as compile-time constants: f(ww) / f(ww, nw) get std::integral_constants for the
// 64-bit words per bit row (1 / 2) and the wavefronts per team (1 / 4), so a generic lambda names its kernel by them.
typedef std::integral_constant<int, 1> int1_t;
typedef std::integral_constant<int, 2> int2_t;
typedef std::integral_constant<int, 4> int4_t;
template <class F> static inline void with_row_words(int WW, F f) { if (WW == 1) f(int1_t{}); else f(int2_t{}); }
template <class F> static inline void with_team_shape(int WW, int threads, F f) {
    with_row_words(WW, [&](auto ww) { if (pcb_layout::wavefronts(threads) == 1) f(ww, int1_t{}); else f(ww, int4_t{}); });
}
#define WW_OF(ww) decltype(ww)::value
#define NW_OF(nw) decltype(nw)::value

#if PCB_HAS(0)
int PCB_FN(pcb_launch_reset)(const ResetLaunch &a) {
    const DevParams &d = a.d;
    with_team_shape(d.WW, a.threads, [&](auto ww, auto nw) {
        hipLaunchKernelGGL((k_reset<KIND, WW_OF(ww), NW_OF(nw)>), dim3(d.B), dim3(64 * NW_OF(nw)), d.ldsBytes, a.stream, d, a.mask);
    });
    return 0;
}
int PCB_FN(pcb_launch_gather)(const GatherLaunch &a) {
    const DevParams &d = a.d;
    with_team_shape(d.WW, a.threads, [&](auto ww, auto nw) {
        hipLaunchKernelGGL((k_gather<KIND, WW_OF(ww), NW_OF(nw)>), dim3(d.B), dim3(64 * NW_OF(nw)), d.ldsBytes, a.stream, d, a.g);
    });
    return 0;
}
int PCB_FN(pcb_step_plain)(const StepLaunch &a) {
    const DevParams &d = a.d;
    if (a.traj && a.num_steps == 1) return PCB_FN(pcb_step_slot)(a);
#if PCB_ROUTES
    if (pcb_layout::fixed_geometry_applies(step_shape(a))) return PCB_FN(pcb_step_fixed)(a);
#endif
    with_team_shape(d.WW, a.threads, [&](auto ww, auto nw) { LAUNCH_STEP_INPLACE_OR_ROLLOUT(WW_OF(ww), NW_OF(nw), false); });
    return 0;
}
#endif
#if PCB_HAS(1)
int PCB_FN(pcb_step_slot)(const StepLaunch &a) {
    const DevParams &d = a.d;
    with_team_shape(d.WW, a.threads, [&](auto ww, auto nw) { LAUNCH_STEP_(WW_OF(ww), NW_OF(nw), false, STEP_BUILD_SLOT); });
    return 0;
}
#endif
#if PCB_HAS(0)
int PCB_FN(pcb_launch_step)(const StepLaunch &a) {
#if PCB_ROUTES
    if (a.routes) return a.threads == 64 ? PCB_FN(pcb_step_routed1)(a) : PCB_FN(pcb_step_routed4)(a);
#endif
    return PCB_FN(pcb_step_plain)(a);
}
#endif

#if PCB_ROUTES
#if PCB_HAS(4)
// only for launches pcb_layout::fixed_geometry_applies admits (pcb_step_plain asks): one wavefront, one word per bit row, in place
int PCB_FN(pcb_step_fixed)(const StepLaunch &a) {
    const DevParams &d = a.d;
    if (d.stream_stores) hipLaunchKernelGGL((k_step<KIND, 1, 1, false, STEP_BUILD_INPLACE_STREAM, STEP_GEO_64>), dim3(d.B + d.term_wgs * d.term_hpe), dim3(64), d.ldsBytes, a.stream, d, a.actions, a.fmt, a.sampled, a.seed, a.first_env, a.step_index, a.num_steps);
    else hipLaunchKernelGGL((k_step<KIND, 1, 1, false, STEP_BUILD_INPLACE, STEP_GEO_64>), dim3(d.B + d.term_wgs * d.term_hpe), dim3(64), d.ldsBytes, a.stream, d, a.actions, a.fmt, a.sampled, a.seed, a.first_env, a.step_index, a.num_steps);
    return 0;
}
#endif
#if PCB_HAS(2)
int PCB_FN(pcb_step_routed1)(const StepLaunch &a) {
    const DevParams &d = a.d;
    with_row_words(d.WW, [&](auto ww) { LAUNCH_STEP_ROUTED(WW_OF(ww), 1); });
    return 0;
}
#endif
#if PCB_HAS(3)
int PCB_FN(pcb_step_routed4)(const StepLaunch &a) {
    const DevParams &d = a.d;
    with_row_words(d.WW, [&](auto ww) { LAUNCH_STEP_ROUTED(WW_OF(ww), 4); });
    return 0;
}
#endif
#endif
