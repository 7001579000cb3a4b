// pcb_playout.h -- k_playout, the kernel of pcbenv_playout: forked episodes played to their end without observations.
// Part of libpcbenv.so (CDNA4 / gfx950 only).  Instantiated in translation units of its own (pcb_playout.inc), never next
// to k_step: the step kernels' inlining depends on every function having one caller in their units (pcb_kind.inc).
//
// One team per playout, the team size of the handle (the state layout and the fold staging depend on it).  The root's
// state block of the CURRENT state set -> LDS, then a loop of at most max_steps transitions, each exactly the transition
// a handle without PCBENV_FLAG_AUTO_RESET would make after pcbenv_gather had put the root's episode into its environment
// i (Team<>::transition in MODE_ALL, pcb_step.h): draw (sample_action on l.vm, keyed by (seed, first_env + i,
// step_index0 + t)) or, at t = 0, the caller's forced action -> validate -> placement update -> legal mask without
// emission -> done -> reward.  The state never leaves LDS: no store_state, no observation byte, nothing the library owns
// is written.  What a playout writes is its row of the caller's outputs, each element by one lane, once:
// reward / done / length / info after the last transition and the action of every recorded step.
//
// Team<>::transition is not called: that function stores done and reward rows at every transition (the playout's done row
// is optional and its reward is the LAST transition's only) and carries the reset and every emission under run-time flags,
// which this kernel would compile in and hold registers for.  The loop below has the same steps: the draw is
// Team<>::draw_action, which run_env calls too; the read of a forced action and the transition itself -- validate, update,
// barriers, window_mask through mask_and_emit(emit = false), done -- are pcb_walk.h's PCB_READ_FORCED_ACTION and
// PCB_TRANSITION_NO_OBS, the one statement k_gather_paths expands too; sample_action and terminal_reward are the step kernel's
// -- the latter through the parameter block, whose buf.reward / buf.info the host points at the
// playout's rows (every other tensor null, flags and the terminal list zeroed: pcbenv_playout).
//
// PATHS = true is the kernel of pcbenv_playout_paths (instantiated in pcb_playout_paths_*.hip): transition t < path_len[i]
// applies path_actions[t, i] instead of a draw -- every lane reads the same element, as at the forced t = 0 of PATHS =
// false, so no wavefront needs another's value -- and the legal-mask bit rows of the node the path ends in (l.vm before
// transition path_len[i], or after the last transition where the episode ended on the path) go to leaf_mask row i, stored
// by the whole team, once.  Nothing else differs: with PATHS = false every line added for it is compiled out.
#pragma once
#include "pcb_walk.h"
#include "pcb_launch.h"

template <int KIND, int WW, int NW, bool ROUTES, bool PATHS>
// (PATHS on the kinds without pins: the path's few scalars must not cost the eighth wave their PATHS = false twins have)
__global__ __attribute__((amdgpu_waves_per_eu(PATHS && KIND != PCBENV_PIN && KIND != PCBENV_SPATIAL ? 8 : 4, 8))) __launch_bounds__(64 * NW) void k_playout(DevParams p, PlayoutArgs g) {
    typedef Team<64 * NW> T;
    constexpr int NT = 64 * NW;
    constexpr bool PINS = KIND == PCBENV_PIN || KIND == PCBENV_SPATIAL;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    // the children of one root are neighbours in i: with an XCD's playouts contiguous the root block is fetched once per L2
    const int i = xcd_contiguous_env((int)blockIdx.x, 0, g.n), lane0 = threadIdx.x;
    const int H = p.H, W = p.W, HW = H * W, plane = H * WW;
    const int r = __builtin_amdgcn_readfirstlane(g.root_index ? g.root_index[i] : i / g.per_root);
    // the length of playout i's path (wave-uniform; every wavefront of the team reads the same word)
    const int plen = !PATHS ? 0 : g.path_len ? __builtin_amdgcn_readfirstlane(g.path_len[i]) : g.path_steps;
    const bool bad_path = PATHS && (unsigned)plen > (unsigned)g.path_steps;
    u64 *leaf = PATHS && g.leaf_mask ? g.leaf_mask + (size_t)i * 2 * plane : 0;
    if ((unsigned)r >= (unsigned)p.B || bad_path) {  // checked before either addresses anything (team-uniform: nobody meets a barrier below)
        if (PATHS && leaf) for (int k = lane0; k < 2 * plane; k += NT) leaf[k] = 0ull;
        if (lane0 == 0) {
            if (g.errors) atomicOr(g.errors, ((unsigned)r >= (unsigned)p.B ? 1u : 0u) | (bad_path ? 2u : 0u));
            g.reward[i] = 0.0;
            if (g.done) g.done[i] = 0;
            if (g.length) g.length[i] = 0;
            if (PINS && g.info) { g.info[2 * (size_t)i] = nan(""); g.info[2 * (size_t)i + 1] = nan(""); }
        }
        return;
    }
    T::load_state_from(smem, p.state + (size_t)r * p.stateStride, p, lane0);
    Lds l = carve(smem, p);
    const int genv = (int)g.first_env + i;
    const size_t per_step = (size_t)g.n * (g.fmt == PCBENV_ACTION_TUPLE ? 3 : 1);
    bool done = false, valid = false;
    int length = 0;
    // (a `for` bounded by the host's max_steps: no data on the device can keep a team here)
    for (int t = 0; t < g.max_steps; t++) {
        // every iteration sees the lane index as a fresh value (run_env: keeps per-lane addressing out of the loop's live set)
        int lane = lane0;
        asm volatile("" : "+v"(lane));
        int o = 0, x = 0, y = 0, given = 0;
        // the node the path names: l.vm as the last transition left it, behind the barrier that ended it (or load_state_from's)
        if (PATHS && leaf && t == plen) for (int k = lane0; k < 2 * plane; k += NT) leaf[k] = l.vm[k];
        const bool forced = PATHS ? t < plen : (t == 0 && g.first_actions);
        const int *fa = PATHS ? g.path_actions + per_step * (size_t)t : g.first_actions;
        if (forced) {
            PCB_READ_FORCED_ACTION(fa, g.fmt, i, given, o, x, y)
        } else T::draw_action(p, l, genv, lane, g.seed, g.step_index0 + (u64)t, &o, &x, &y);
        if (lane == 0 && t < g.actions_steps) {
            int *act = g.actions_out + per_step * (size_t)t;
            if (g.fmt == PCBENV_ACTION_FLAT) act[i] = forced ? given : PCB_FLATTEN_ACTION(o, x, y, HW, W);
            else { act[3 * (size_t)i] = o; act[3 * (size_t)i + 1] = x; act[3 * (size_t)i + 2] = y; }
        }
        PCB_TRANSITION_NO_OBS(i, lane, o, x, y, valid, done)
        length = t + 1;
        if (done) break;  // team-uniform
        T::lds_sync();
    }
    if (PATHS && leaf && length <= plen) {  // the episode ended on the path, or was cut at its end: the state it is left in
        T::lds_sync();  // team-uniform, as the loop's exit is; mask_and_emit's last words of l.vm are visible behind it
        for (int k = lane0; k < 2 * plane; k += NT) leaf[k] = l.vm[k];
    }
    // the outputs of the last transition played (Team<>::transition's reward rules)
    if (lane0 == 0) {
        if (g.done) g.done[i] = done ? 1 : 0;
        if (g.length) g.length[i] = length;
    }
    if (PINS && done) {  // routed if everything is placed, else the worst case (S:853-863): reward and info of row i
        T::template terminal_reward<KIND, ROUTES>(p, l, i, lane0, 0, 1, 0u);
    } else if (lane0 == 0) {
        g.reward[i] = PINS ? 0.0 : (valid ? 1.0 : 0.0);  // R:424-432
        if (PINS && g.info) { g.info[2 * (size_t)i] = nan(""); g.info[2 * (size_t)i + 1] = nan(""); }
    }
}
