// pcb_playout.inc -- instantiations and launch switch of k_playout (pcb_playout.h) for ONE environment kind, compiled once
// per unit of build.py's table (-DPCB_KIND=, -DPCB_KIND_NAME=, [-DPCB_PART=n], [-DPCB_PATHS=1]).  Build: as pcb_kind.inc.
// Which k_playout a launch runs is pcb_layout::select_playout_build, which unit compiles it pcb_layout::playout_build_part
// (pcb_layout.h lists the parts; the pin kinds are split like their step kernels, so that no unit is slower to build than
// the slowest of those).  PCB_PART undefined = a kind without routes (square, rect), one unit, part 0.  PCB_PATHS=1 = the
// PATHS = true instantiations (pcbenv_playout_paths) in units of their own: pcbenv_playout's compile exactly as without them.
#include <utility>

#include "pcb_playout.h"
#define PCB_CAT3_(a, b, c) a##b##c
#define PCB_CAT3(a, b, c) PCB_CAT3_(a, b, c)
#define PCB_FN(stem) PCB_CAT3(stem, _, PCB_KIND_NAME)
#ifndef PCB_PART
#define PCB_PART 0
#endif
#ifndef PCB_PATHS
#define PCB_PATHS 0
#endif
using pcb_layout::PlayoutBuild;
static constexpr int KIND = PCB_KIND;
// pcb_playout_unit<paths><n>_<kind>: launches build b, which playout_build_part gives part n, from the unit that compiles it
#define PCB_PLAYOUT_UNIT(paths, part) int PCB_FN(PCB_CAT3(pcb_playout_unit, paths, part))(const PlayoutLaunch &a, const PlayoutBuild &b)
PCB_PLAYOUT_UNIT(0, 0); PCB_PLAYOUT_UNIT(0, 1); PCB_PLAYOUT_UNIT(0, 2); PCB_PLAYOUT_UNIT(1, 0); PCB_PLAYOUT_UNIT(1, 1); PCB_PLAYOUT_UNIT(1, 2);

// Candidate I of the PLAYOUT_BUILDS builds: compiled here if this unit is its part, launched if it is b.
template <int I> static inline bool launch_playout_if(const PlayoutLaunch &a, const PlayoutBuild &b) {
    constexpr PlayoutBuild c = pcb_layout::playout_build_at(I);
    if constexpr (pcb_layout::playout_build_part(KIND, c) == PCB_PART && c.paths == (PCB_PATHS != 0)) {
        if (pcb_layout::build_index(b) != I) return false;
        hipLaunchKernelGGL((k_playout<KIND, c.ww, c.nw, c.routes, c.paths>), dim3(a.g.n), dim3(64 * c.nw), a.d.ldsBytes, a.stream, a.d, a.g);
        return true;
    }
    return false;
}
template <int... I> static inline bool launch_playout_in_unit(const PlayoutLaunch &a, const PlayoutBuild &b, std::integer_sequence<int, I...>) { return (launch_playout_if<I>(a, b) || ...); }
PCB_PLAYOUT_UNIT(PCB_PATHS, PCB_PART) { return launch_playout_in_unit(a, b, std::make_integer_sequence<int, PLAYOUT_BUILDS>{}) ? 0 : -1; }

#if PCB_PART == 0 && !PCB_PATHS
int PCB_FN(pcb_launch_playout)(const PlayoutLaunch &a) {
    const PlayoutBuild b = pcb_layout::select_playout_build(a.d.WW, a.threads, a.routes, a.paths);
    const int part = pcb_layout::playout_build_part(KIND, b);
    if constexpr (pcb_layout::is_pin_kind(KIND)) {
        if (part == 1) return b.paths ? PCB_FN(pcb_playout_unit11)(a, b) : PCB_FN(pcb_playout_unit01)(a, b);
        if (part == 2) return b.paths ? PCB_FN(pcb_playout_unit12)(a, b) : PCB_FN(pcb_playout_unit02)(a, b);
    }
    return b.paths ? PCB_FN(pcb_playout_unit10)(a, b) : PCB_FN(pcb_playout_unit00)(a, b);
}
#endif
