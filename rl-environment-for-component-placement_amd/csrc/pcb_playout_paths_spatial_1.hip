// pcb_playout_paths_spatial_1.hip -- k_playout<PATHS = true> of the spatial environment, part 1 (pcb_playout.inc lists the parts; one translation unit each: they compile in parallel)
#include <hip/hip_runtime.h>
#include "pcbenv.h"
#define PCB_KIND PCBENV_SPATIAL
#define PCB_KIND_NAME spatial
#define PCB_PART 1
#define PCB_PATHS 1
#include "pcb_playout.inc"
