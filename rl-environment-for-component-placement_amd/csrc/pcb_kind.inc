// pcb_kind.inc -- what is particular to k_step, k_reset and k_gather in the unit of ONE environment kind and part, compiled
// once per row of build.py's table (-DPCB_KIND= and, for the pin kinds, -DPCB_PART=n): how a candidate build of k_step is
// launched, and in part 0 the entries of k_reset and k_gather.  Build: hipcc --offload-arch=gfx950 -O3 -ffp-contract=off
// (one IEEE operation per written operator; the only fused multiply-add is the explicit __fma_rn in norm2).
// Which k_step a launch runs is pcb_layout::select_step_build, which unit compiles it pcb_layout::step_build_part
// (pcb_layout.h lists the parts): a unit holds the builds that function gives it and nothing else says so; the walk over
// the candidates and the entry that picks the part are pcb_dispatch.h's and pcb_launch.h's, for every family alike.  The
// pin kinds are split so that the build is as long as its slowest part.
// (The slot build has a unit of its own for its code, not only for the build time: next to the rollout build every
// function only the trajectory layout uses has two callers instead of one and is no longer inlined -- 437 instead of
// 143 spilled scalars in the spatial kernel and 76 instead of 68 us per c4 step.)
#include "pcb_kernels.h"
#include "pcb_dispatch.h"

template <int KIND, int I> void StepFamily::launch(const StepLaunch &a) {
    constexpr Build c = build_at(I);
    const DevParams &d = a.d;
    hipLaunchKernelGGL((k_step<KIND, c.ww, c.nw, c.routes, c.build, c.geo>), dim3(d.B + d.term_wgs * d.term_hpe), dim3(64 * c.nw), d.ldsBytes, a.stream,
                       d, a.actions, a.fmt, a.sampled, a.seed, a.first_env, a.step_index, a.num_steps);
}
PCB_UNIT(StepFamily, PCB_PART)

#if PCB_PART == 0
// The run-time shape of a k_reset / k_gather launch as compile-time constants: f(ww, nw) gets std::integral_constants for
// the 64-bit words per bit row (1 / 2) and the wavefronts per team (1 / 4), so a generic lambda names its kernel by them.
typedef std::integral_constant<int, 1> int1_t;
typedef std::integral_constant<int, 2> int2_t;
typedef std::integral_constant<int, 4> int4_t;
template <class F> static inline void with_team_shape(int WW, int threads, F f) {
    const auto with_row_words = [&](auto ww) { if (pcb_layout::wavefronts(threads) == 1) f(ww, int1_t{}); else f(ww, int4_t{}); };
    if (WW == 1) with_row_words(int1_t{}); else with_row_words(int2_t{});
}
#define WW_OF(ww) decltype(ww)::value
#define NW_OF(nw) decltype(nw)::value

template <int KIND> int pcb_launch_reset(const ResetLaunch &a) {
    const DevParams &d = a.d;
    with_team_shape(d.WW, a.threads, [&](auto ww, auto nw) {
        hipLaunchKernelGGL((k_reset<KIND, WW_OF(ww), NW_OF(nw)>), dim3(d.B), dim3(64 * NW_OF(nw)), d.ldsBytes, a.stream, d, a.mask);
    });
    return 0;
}
template <int KIND> int pcb_launch_gather(const GatherLaunch &a) {
    const DevParams &d = a.d;
    with_team_shape(d.WW, a.threads, [&](auto ww, auto nw) {
        hipLaunchKernelGGL((k_gather<KIND, WW_OF(ww), NW_OF(nw)>), dim3(d.B), dim3(64 * NW_OF(nw)), d.ldsBytes, a.stream, d, a.g);
    });
    return 0;
}
template int pcb_launch_reset<PCB_KIND>(const ResetLaunch &);
template int pcb_launch_gather<PCB_KIND>(const GatherLaunch &);
#endif
