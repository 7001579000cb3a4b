// pcb_playout_paths_square.hip -- k_playout<PATHS = true> of the square environment (pcb_playout.inc lists the parts; one translation unit each: they compile in parallel)
#include <hip/hip_runtime.h>
#include "pcbenv.h"
#define PCB_KIND PCBENV_SQUARE
#define PCB_KIND_NAME square
#define PCB_PATHS 1
#include "pcb_playout.inc"
