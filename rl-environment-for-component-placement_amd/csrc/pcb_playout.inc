// pcb_playout.inc -- instantiations and launch switch of k_playout (pcb_playout.h) for ONE environment kind (PCB_KIND /
// PCB_KIND_NAME set by the including pcb_playout_<name>[_<part>].hip).  Build: as pcb_kind.inc.
// The pin kinds are split into PARTS, one translation unit each, like their step kernels, so that no unit is slower to
// build than the slowest of those: 0 = without routes + the launch switch, 1 / 2 = with beam / both routes on one / four
// wavefronts.  PCB_PART undefined = a kind without routes (square, rect), everything in one unit.
// PCB_PATHS defined (pcb_playout_paths_<name>[_<part>].hip) = the PATHS = true instantiations, the kernels of
// pcbenv_playout_paths, in units of their own: what pcbenv_playout launches compiles exactly as without them.
#include "pcb_playout.h"

#define PCB_CAT3_(a, b, c) a##b##c
#define PCB_CAT3(a, b, c) PCB_CAT3_(a, b, c)
#define PCB_FN(stem) PCB_CAT3(stem, _, PCB_KIND_NAME)
static constexpr int KIND = PCB_KIND;
#ifdef PCB_PATHS
static constexpr bool PATHS = true;
#define PCB_STEM(stem) PCB_FN(stem##_paths)
#else
static constexpr bool PATHS = false;
#define PCB_STEM(stem) PCB_FN(stem)
#endif
#ifdef PCB_PART
#define PCB_HAS(part) (PCB_PART == (part))
#else
#define PCB_HAS(part) ((part) == 0)
#endif

int PCB_STEM(pcb_playout_routed1)(const PlayoutLaunch &a);
int PCB_STEM(pcb_playout_routed4)(const PlayoutLaunch &a);

#define LAUNCH_PLAYOUT(NW_, RT_) do { \
    if (a.d.WW == 1) hipLaunchKernelGGL((k_playout<KIND, 1, NW_, RT_, PATHS>), dim3(a.g.n), dim3(64 * NW_), a.d.ldsBytes, a.stream, a.d, a.g); \
    else hipLaunchKernelGGL((k_playout<KIND, 2, NW_, RT_, PATHS>), dim3(a.g.n), dim3(64 * NW_), a.d.ldsBytes, a.stream, a.d, a.g); } while (0)

#if PCB_HAS(0)
int PCB_STEM(pcb_launch_playout)(const PlayoutLaunch &a) {
#ifdef PCB_PART
    if (a.routes) return a.threads == 64 ? PCB_STEM(pcb_playout_routed1)(a) : PCB_STEM(pcb_playout_routed4)(a);
#endif
    if (pcb_layout::wavefronts(a.threads) == 1) LAUNCH_PLAYOUT(1, false); else LAUNCH_PLAYOUT(4, false);
    return 0;
}
#endif
#if PCB_HAS(1)
int PCB_STEM(pcb_playout_routed1)(const PlayoutLaunch &a) { LAUNCH_PLAYOUT(1, true); return 0; }
#endif
#if PCB_HAS(2)
int PCB_STEM(pcb_playout_routed4)(const PlayoutLaunch &a) { LAUNCH_PLAYOUT(4, true); return 0; }
#endif
