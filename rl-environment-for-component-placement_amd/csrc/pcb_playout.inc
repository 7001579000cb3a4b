// pcb_playout.inc -- how a candidate build of k_playout (pcb_playout.h) is launched, in the unit of ONE environment kind
// and part, compiled once per row of build.py's table (-DPCB_KIND=, [-DPCB_PART=n], [-DPCB_PATHS=1]).  Build: as pcb_kind.inc.
// Which k_playout a launch runs is pcb_layout::select_playout_build, which unit compiles it pcb_layout::playout_build_unit
// (pcb_layout.h lists the parts; the pin kinds are split like their step kernels, so that no unit is slower to build than
// the slowest of those).  PCB_PATHS=1 = the PATHS = true instantiations (pcbenv_playout_paths) in units of their own, the
// parts behind PLAYOUT_PARTS: pcbenv_playout's compile exactly as without them.
#include "pcb_playout.h"
#include "pcb_dispatch.h"

#ifndef PCB_PATHS
#define PCB_PATHS 0
#endif
template <int KIND, int I> void PlayoutFamily::launch(const PlayoutLaunch &a) {
    constexpr Build c = build_at(I);
    hipLaunchKernelGGL((k_playout<KIND, c.ww, c.nw, c.routes, c.paths>), dim3(a.g.n), dim3(64 * c.nw), a.d.ldsBytes, a.stream, a.d, a.g);
}
PCB_UNIT(PlayoutFamily, PCB_PART + PLAYOUT_PARTS * PCB_PATHS)
