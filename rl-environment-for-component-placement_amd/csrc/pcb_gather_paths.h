// pcb_gather_paths.h -- k_gather_paths, the kernel of pcbenv_gather_paths: k_gather followed, in the same launch, by a
// per-row path of forced actions -- the tree node a path names, materialised with its observations.
// Part of libpcbenv.so (CDNA4 / gfx950 only).  Instantiated in translation units of its own (pcb_gather_paths.inc), never
// next to k_step or k_playout: their inlining depends on every function having one caller in their units (pcb_kind.inc).
//
// One team per destination environment e, the team size of the DESTINATION (as k_gather: the state layout is the same
// for both team sizes, so gathers between handles with different threads_per_env work).  The composition of three pieces
// that exist, each stated once in pcb_walk.h and expanded here as in its first home: k_gather's head -- the source's block
// of the CURRENT state set -> LDS, the header patched (PCB_GATHER_PATCH_HEADER says what must not be taken over) -- then
// the forced-action loop of k_playout<PATHS = true> (pcb_playout.h) -- at most path_len[e] <= path_steps transitions, each
// the one a handle without PCBENV_FLAG_AUTO_RESET would make (PCB_READ_FORCED_ACTION, PCB_TRANSITION_NO_OBS): window_mask
// through mask_and_emit(emit = false), no draw, no store, break on done -- then k_gather's tail (PCB_GATHER_EMIT_SLOT):
// ONE whole emission of every bound tensor of the destination's selected slot from LDS, reward / done / info of the last
// transition applied (the source row's if none was), and the block into the destination's OTHER state set.  The
// observations are written once however long the path is.
//
// Rows that keep their episode -- src_index -1, out of range (error bit 0), or path_len outside [0, path_steps] (error
// bit 1, checked before it bounds anything) -- copy their own block and touch no tensor; their path is not read.
#pragma once
#include "pcb_walk.h"
#include "pcb_launch.h"

template <int KIND, int WW, int NW, bool ROUTES>
__global__ __launch_bounds__(64 * NW) void k_gather_paths(DevParams p, GatherArgs g, GatherPathArgs q) {
    typedef Team<64 * NW> T;
    constexpr int NT = 64 * NW;
    constexpr bool PINS = KIND == PCBENV_PIN || KIND == PCBENV_SPATIAL;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int e = xcd_contiguous_env((int)blockIdx.x, 0, p.B), lane0 = threadIdx.x;
    const int H = p.H, W = p.W, HW = H * W, plane = H * WW;
    const int j = __builtin_amdgcn_readfirstlane(g.src_index[e]);
    const bool in_range = (unsigned)j < (unsigned)g.src_B;  // checked before it addresses anything
    // the length of row e's path (wave-uniform; every wavefront of the team reads the same word), read for taken rows only
    const int plen = !in_range ? 0 : q.path_len ? __builtin_amdgcn_readfirstlane(q.path_len[e]) : q.path_steps;
    const bool bad_path = (unsigned)plen > (unsigned)q.path_steps;  // checked before it bounds anything
    const bool take = in_range && !bad_path;
    if (!take && lane0 == 0) {
        if (j != -1 && g.errors) atomicOr(g.errors, in_range ? 2u : 1u);
        if (q.length) q.length[e] = 0;
    }
    const unsigned char *own = p.state + (size_t)e * p.stateStride;
    T::load_state_from(smem, take ? g.src_state + (size_t)j * p.stateStride : own, p, lane0);
    Lds l = carve(smem, p);
    if (take) {  // (team-uniform: j and plen are)
        PCB_GATHER_PATCH_HEADER(own, lane0)
        T::lds_sync();
        const size_t per_step = (size_t)p.B * (q.fmt == PCBENV_ACTION_TUPLE ? 3 : 1);
        bool done = false, valid = false;
        int length = 0;
        // (a `for` bounded by the host's path_steps: no data on the device can keep a team here)
        for (int t = 0; t < q.path_steps; t++) {
            if (t >= plen) break;
            // every iteration sees the lane index as a fresh value (run_env: keeps per-lane addressing out of the loop's live set)
            int lane = lane0;
            asm volatile("" : "+v"(lane));
            int o = 0, x = 0, y = 0, given = 0;  // (`given` is k_playout's: nothing here records the code as written)
            const int *fa = q.path_actions + per_step * (size_t)t;
            PCB_READ_FORCED_ACTION(fa, q.fmt, e, given, o, x, y)
            PCB_TRANSITION_NO_OBS(e, lane, o, x, y, valid, done)
            length = t + 1;
            if (done) break;  // team-uniform
            T::lds_sync();
        }
        T::lds_sync();  // team-uniform, as the loop's exit is: the state the last transition left is visible to every wavefront
        // the one emission, as k_gather has it
        const int lane = lane0;
        const int row = out_row(p, p.slot, e);
        PCB_GATHER_EMIT_SLOT(e, row, lane)
        // reward / done / info: the source row's if no transition was applied, else the last transition's (Team<>::transition's rules)
        if (lane == 0) {
            if (q.length) q.length[e] = length;
            p.buf.done[row] = length == 0 ? g.done[j] : done ? 1 : 0;
        }
        if (length == 0) {
            if (lane == 0) {
                p.buf.reward[row] = g.reward[j];
                if (p.buf.info) {
                    p.buf.info[2 * (size_t)row] = g.info ? g.info[2 * (size_t)j] : nan("");
                    p.buf.info[2 * (size_t)row + 1] = g.info ? g.info[2 * (size_t)j + 1] : nan("");
                }
            }
        } else if (PINS && done) {  // routed if everything is placed, else the worst case (S:853-863)
            T::lds_sync();  // the route segments share their zone with the class map emit_pin_grid has just read
            T::template terminal_reward<KIND, ROUTES>(p, l, row, lane, 0, 1, 0u);
        } else if (lane == 0) {
            p.buf.reward[row] = PINS ? 0.0 : (valid ? 1.0 : 0.0);  // R:424-432
            if (p.buf.info) { p.buf.info[2 * (size_t)row] = nan(""); p.buf.info[2 * (size_t)row + 1] = nan(""); }
        }
    }
    T::store_state(smem, p, e, lane0);
}
