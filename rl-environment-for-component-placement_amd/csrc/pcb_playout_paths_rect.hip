// pcb_playout_paths_rect.hip -- k_playout<PATHS = true> of the rect environment (pcb_playout.inc lists the parts; one translation unit each: they compile in parallel)
#include <hip/hip_runtime.h>
#include "pcbenv.h"
#define PCB_KIND PCBENV_RECT
#define PCB_KIND_NAME rect
#define PCB_PATHS 1
#include "pcb_playout.inc"
