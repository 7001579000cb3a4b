// pcb_gather_paths.inc -- how a candidate build of k_gather_paths (pcb_gather_paths.h) is launched, in the unit of ONE
// environment kind and part, compiled once per row of build.py's table (-DPCB_KIND=, [-DPCB_PART=n]).  Build: as pcb_kind.inc.
// Which k_gather_paths a launch runs is pcb_layout::select_gather_paths_build, which unit compiles it
// pcb_layout::gather_paths_build_part (the parts of k_playout: the pin kinds are split by routes and team size).
#include "pcb_gather_paths.h"
#include "pcb_dispatch.h"

template <int KIND, int I> void GatherPathsFamily::launch(const GatherPathsLaunch &a) {
    constexpr Build c = build_at(I);
    hipLaunchKernelGGL((k_gather_paths<KIND, c.ww, c.nw, c.routes>), dim3(a.d.B), dim3(64 * c.nw), a.d.ldsBytes, a.stream, a.d, a.g, a.q);
}
PCB_UNIT(GatherPathsFamily, PCB_PART)
