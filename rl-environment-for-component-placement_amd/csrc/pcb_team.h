// pcb_team.h -- everything a TEAM of TN threads does for one environment, as static members of Team<TN>.
// Part of libpcbenv.so (CDNA4 / gfx950 only).
//
// A team is the set of threads that work on one environment: one wavefront (TN = 64) for grids up to 64 x 64, four
// (TN = 256) for the 128 x 128 spatial configuration.  A team is one workgroup.  For an environment that is certain to
// end its episode in a step launch, k_step starts helper workgroups next to the environment's own -- REWARD_PARTS
// teams of the same size that share the routing reward and, with PCBENV_FLAG_AUTO_RESET, one that writes the feature
// half of the reset -- each with its own LDS copy of the state block (see Team<>::run_env).
// The team size decides the lane stride of every loop, whether a phase boundary needs an s_barrier (a one-wavefront
// team's LDS traffic executes in program order) and how work is dealt to wavefronts, so it is a compile-time
// property: the sections below are textually included inside the class template, where NT is TN.  The class holds only what
// depends on NT -- a lane stride of NT, lds_sync / store_drain_sync / block_any; everything else is free functions in the headers
// included first, each of which compiles on its own.  The __global__ kernels that pick teams are in pcb_kernels.h.
#pragma once
#include "pcb_device.h"
#include "pcb_env_lds.h"   // Lds, carve, out_row, pin tables, InstRegs
#include "pcb_routing.h"   // norm2, candidate test, beam search of one net (with pcb_geometry.h, pcb_setmodel.h)
#include "pcb_sampler.h"   // uniform legal-action draw
#include "pcb_transition.h"  // action code, validity, extent and row fill, pin rotation, cursor and done: the scalar core

#define NT TN  // inside Team<TN> only (undefined again below)
template <int TN> struct Team {
    static_assert(TN == 64 || TN == 256, "one or four wavefronts per environment");
#include "pcb_team_io.h"   // LDS barrier, any(), plane emission, window fold
#include "pcb_reward.h"    // centroid routes, pair sweep, wirelength
#include "pcb_beam.h"      // beam-search routes of all nets
#include "pcb_observe.h"   // state staging, mask + observation emission, pin_grid, features, terminal reward
#include "pcb_reset.h"     // reset from the instance queue
#include "pcb_step.h"      // transition, run_env
};
#undef NT
