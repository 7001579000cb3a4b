// pcb_kind.inc -- kernel instantiations and launch switch of ONE environment kind, compiled once per unit of build.py's
// table (-DPCB_KIND=, -DPCB_KIND_NAME= and, for the pin kinds, -DPCB_PART=n).  Build: hipcc --offload-arch=gfx950 -O3
// -ffp-contract=off (one IEEE operation per written operator; the only fused multiply-add is the explicit __fma_rn in norm2).
// Which k_step a launch runs is pcb_layout::select_step_build, which unit compiles it pcb_layout::step_build_part
// (pcb_layout.h lists the parts): a unit holds the builds that function gives it and nothing else says so.  The pin
// kinds are split so that the build is as long as its slowest part; part 0 also has k_reset, k_gather and the entry
// points.  PCB_PART undefined = a kind without routes (square, rect), everything in one unit, part 0.
// (The slot build has a unit of its own for its code, not only for the build time: next to the rollout build every
// function only the trajectory layout uses has two callers instead of one and is no longer inlined -- 437 instead of
// 143 spilled scalars in the spatial kernel and 76 instead of 68 us per c4 step.)
#include <utility>

#include "pcb_kernels.h"
#include "pcb_launch.h"

#define PCB_CAT3_(a, b, c) a##b##c
#define PCB_CAT3(a, b, c) PCB_CAT3_(a, b, c)
#define PCB_FN(stem) PCB_CAT3(stem, _, PCB_KIND_NAME)
#ifndef PCB_PART
#define PCB_PART 0
#endif
using pcb_layout::StepBuild;
static constexpr int KIND = PCB_KIND;

// pcb_step_part<n>_<kind>: launches build b, which step_build_part gives part n, from the unit that compiles it
#define PCB_STEP_PART(part) int PCB_FN(PCB_CAT3(pcb_step_part, part, ))(const StepLaunch &a, const StepBuild &b)
PCB_STEP_PART(0); PCB_STEP_PART(1); PCB_STEP_PART(2); PCB_STEP_PART(3); PCB_STEP_PART(4);

// Candidate I of the STEP_BUILDS builds: compiled here if this unit is its part, launched if it is b.
template <int I> static inline bool launch_step_if(const StepLaunch &a, const StepBuild &b) {
    constexpr StepBuild c = pcb_layout::step_build_at(I);
    if constexpr (pcb_layout::step_build_part(KIND, c) == PCB_PART) {
        if (pcb_layout::build_index(b) != I) return false;
        const DevParams &d = a.d;
        hipLaunchKernelGGL((k_step<KIND, c.ww, c.nw, c.routes, c.build, c.geo>), dim3(d.B + d.term_wgs * d.term_hpe), dim3(64 * c.nw), d.ldsBytes, a.stream,
                           d, a.actions, a.fmt, a.sampled, a.seed, a.first_env, a.step_index, a.num_steps);
        return true;
    }
    return false;
}
template <int... I> static inline bool launch_step_in_unit(const StepLaunch &a, const StepBuild &b, std::integer_sequence<int, I...>) {
    return (launch_step_if<I>(a, b) || ...);
}
PCB_STEP_PART(PCB_PART) { return launch_step_in_unit(a, b, std::make_integer_sequence<int, STEP_BUILDS>{}) ? 0 : -1; }

#if PCB_PART == 0
int PCB_FN(pcb_launch_step)(const StepLaunch &a) {
    const StepBuild b = pcb_layout::select_step_build(step_shape(a), a.d.stream_stores != 0);
    if constexpr (pcb_layout::is_pin_kind(KIND)) switch (pcb_layout::step_build_part(KIND, b)) {
        case 1: return PCB_FN(pcb_step_part1)(a, b);
        case 2: return PCB_FN(pcb_step_part2)(a, b);
        case 3: return PCB_FN(pcb_step_part3)(a, b);
        case 4: return PCB_FN(pcb_step_part4)(a, b);
    }
    return PCB_FN(pcb_step_part0)(a, b);
}

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
#endif
