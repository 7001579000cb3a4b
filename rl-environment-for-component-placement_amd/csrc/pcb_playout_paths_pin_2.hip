// pcb_playout_paths_pin_2.hip -- k_playout<PATHS = true> of the pin environment, part 2 (pcb_playout.inc lists the parts; one translation unit each: they compile in parallel)
#include <hip/hip_runtime.h>
#include "pcbenv.h"
#define PCB_KIND PCBENV_PIN
#define PCB_KIND_NAME pin
#define PCB_PART 2
#define PCB_PATHS 1
#include "pcb_playout.inc"
