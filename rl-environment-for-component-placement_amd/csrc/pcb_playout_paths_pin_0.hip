// pcb_playout_paths_pin_0.hip -- k_playout<PATHS = true> of the pin environment, part 0 (pcb_playout.inc lists the parts; one translation unit each: they compile in parallel)
#include <hip/hip_runtime.h>
#include "pcbenv.h"
#define PCB_KIND PCBENV_PIN
#define PCB_KIND_NAME pin
#define PCB_PART 0
#define PCB_PATHS 1
#include "pcb_playout.inc"
