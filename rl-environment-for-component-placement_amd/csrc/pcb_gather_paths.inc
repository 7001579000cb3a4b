// pcb_gather_paths.inc -- instantiations and launch switch of k_gather_paths (pcb_gather_paths.h) for ONE environment
// kind, compiled once per unit of build.py's table (-DPCB_KIND=, -DPCB_KIND_NAME=, [-DPCB_PART=n]).  Build: as pcb_kind.inc.
// Which k_gather_paths a launch runs is pcb_layout::select_gather_paths_build, which unit compiles it
// pcb_layout::gather_paths_build_part (the parts of k_playout: the pin kinds are split by routes and team size).
// PCB_PART undefined = a kind without routes (square, rect), one unit, part 0.
#include <utility>

#include "pcb_gather_paths.h"
#define PCB_CAT3_(a, b, c) a##b##c
#define PCB_CAT3(a, b, c) PCB_CAT3_(a, b, c)
#define PCB_FN(stem) PCB_CAT3(stem, _, PCB_KIND_NAME)
#ifndef PCB_PART
#define PCB_PART 0
#endif
using pcb_layout::GatherPathsBuild;
static constexpr int KIND = PCB_KIND;
// pcb_gather_paths_unit<n>_<kind>: launches build b, which gather_paths_build_part gives part n, from the unit that compiles it
#define PCB_GATHER_PATHS_UNIT(part) int PCB_FN(PCB_CAT3(pcb_gather_paths_unit, part, ))(const GatherPathsLaunch &a, const GatherPathsBuild &b)
PCB_GATHER_PATHS_UNIT(0); PCB_GATHER_PATHS_UNIT(1); PCB_GATHER_PATHS_UNIT(2);

// Candidate I of the GATHER_PATHS_BUILDS builds: compiled here if this unit is its part, launched if it is b.
template <int I> static inline bool launch_gather_paths_if(const GatherPathsLaunch &a, const GatherPathsBuild &b) {
    constexpr GatherPathsBuild c = pcb_layout::gather_paths_build_at(I);
    if constexpr (pcb_layout::gather_paths_build_part(KIND, c) == PCB_PART) {
        if (pcb_layout::build_index(b) != I) return false;
        hipLaunchKernelGGL((k_gather_paths<KIND, c.ww, c.nw, c.routes>), dim3(a.d.B), dim3(64 * c.nw), a.d.ldsBytes, a.stream, a.d, a.g, a.q);
        return true;
    }
    return false;
}
template <int... I> static inline bool launch_gather_paths_in_unit(const GatherPathsLaunch &a, const GatherPathsBuild &b, std::integer_sequence<int, I...>) {
    return (launch_gather_paths_if<I>(a, b) || ...);
}
PCB_GATHER_PATHS_UNIT(PCB_PART) { return launch_gather_paths_in_unit(a, b, std::make_integer_sequence<int, GATHER_PATHS_BUILDS>{}) ? 0 : -1; }

#if PCB_PART == 0
int PCB_FN(pcb_launch_gather_paths)(const GatherPathsLaunch &a) {
    const GatherPathsBuild b = pcb_layout::select_gather_paths_build(a.d.WW, a.threads, a.routes);
    if constexpr (pcb_layout::is_pin_kind(KIND)) {
        const int part = pcb_layout::gather_paths_build_part(KIND, b);
        if (part == 1) return PCB_FN(pcb_gather_paths_unit1)(a, b);
        if (part == 2) return PCB_FN(pcb_gather_paths_unit2)(a, b);
    }
    return PCB_FN(pcb_gather_paths_unit0)(a, b);
}
#endif
