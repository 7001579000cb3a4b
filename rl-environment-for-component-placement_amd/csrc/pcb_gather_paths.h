// pcb_gather_paths.h -- k_gather_paths, the kernel of pcbenv_gather_paths: k_gather followed, in the same launch, by a
// per-row path of forced actions -- the tree node a path names, materialised with its observations.
// Part of libpcbenv.so (CDNA4 / gfx950 only).  Instantiated in translation units of its own (pcb_gather_paths.inc), never
// next to k_step or k_playout: their inlining depends on every function having one caller in their units (pcb_kind.inc).
//
// One team per destination environment e, the team size of the DESTINATION (as k_gather: the state layout is the same
// for both team sizes, so gathers between handles with different threads_per_env work).  The composition of three pieces
// that exist: k_gather's head -- the source's block of the CURRENT state set -> LDS, the header patched (pcb_kernels.h
// says what must not be taken over) -- then the forced-action loop of k_playout<PATHS = true> (pcb_playout.h) -- at most
// path_len[e] <= path_steps transitions, each the one a handle without PCBENV_FLAG_AUTO_RESET would make: the text of
// pcb_transition.h, expanded here as there, window_mask through mask_and_emit(emit = false), no draw, no store, break on
// done -- then k_gather's tail: ONE whole emission of every bound tensor of the destination's selected slot from LDS,
// reward / done / info of the last transition applied (the source row's if none was), and the block into the
// destination's OTHER state set.  The observations are written once however long the path is.
//
// Rows that keep their episode -- src_index -1, out of range (error bit 0), or path_len outside [0, path_steps] (error
// bit 1, checked before it bounds anything) -- copy their own block and touch no tensor; their path is not read.
#pragma once
#include "pcb_team.h"
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
        if (lane0 == 0) {
            const EnvHdr *oh = (const EnvHdr *)own;
            l.hdr->qcursor = oh->qcursor; l.hdr->episode = oh->episode;
            l.hdr->term_seq = 0u; l.hdr->term_pos = 0u;
            l.hdr->pre_action = 0u;
            if (PINS) l.hdr->feat_gen = p.bind_gen;
        }
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
            int o = 0, x = 0, y = 0;
            // as run_env reads a caller's action: out of range is data (an invalid action), checked before use below
            const int *fa = q.path_actions + per_step * (size_t)t;
            if (q.fmt == PCBENV_ACTION_FLAT) {
                unflatten_action(fa[e], p.O, HW, W, &o, &x, &y);
            } else {
                o = fa[3 * (size_t)e]; x = fa[3 * (size_t)e + 1]; y = fa[3 * (size_t)e + 2];
                if (KIND == PCBENV_SQUARE) o = 0;
            }
            // validate_action and the update, as Team<>::transition has them: the text of pcb_transition.h, expanded in place
            const int cur = l.hdr->cur, ncomp = l.hdr->ncomp, npins = l.hdr->npins;
            valid = PCB_ACTION_IN_RANGE(o, x, y, p.O, H, W) && (KIND == PCBENV_SQUARE || cur >= 0);
            if (valid) valid = PCB_LEGAL_BIT(l.vm, (o & 1) * plane, WW, x, y);
            if (NT > WAVE) T::lds_sync();  // every wavefront has read the cursor and the mask bit before anything below changes them
            done = true;  // an invalid action is a terminal transition with the state unchanged (quirk Q8 iii)
            if (valid) {
                int ph, pw;
                CompRec cr = CompRec();
                if (KIND == PCBENV_SQUARE) ph = pw = p.component_n;
                else {
                    cr = l.comps[cur];
                    ph = PCB_PLACED_H(o, cr.h, cr.w);
                    pw = PCB_PLACED_W(o, cr.h, cr.w);
                }
                for (int rr = x + lane; rr < x + ph && rr < H; rr += NT) {
                    PCB_OCCUPY_ROW(l.occ, rr * WW, WW, y, pw)
                }
                if (KIND != PCBENV_SQUARE) {
                    if (lane == 0) { l.comps[cur].px = (signed char)x; l.comps[cur].py = (signed char)y; l.comps[cur].o = (unsigned char)o; }
                    if (PINS) {
                        const int ch = cr.h, cw = cr.w;
                        for (int k = lane; k < npins; k += NT) {  // S:149-190 place_component
                            PinRec pr = l.pins[k];
                            if (pr.comp != cur) continue;
                            PCB_PLACE_PIN(pr, o, ch, cw, x, y)
                            l.pins[k] = pr;
                        }
                    }
                    if (lane == 0) l.hdr->cur = (short)next_component(cur, ncomp);
                }
                T::lds_sync();
                const bool any = T::template mask_and_emit<KIND, WW>(p, l, e, lane, false, 0, 0);  // team-uniform (block_any)
                done = episode_done<KIND>(l.hdr->cur, any);
            }
            length = t + 1;
            // `done` is team-uniform: valid, cur and `any` are functions of LDS words every wavefront read behind a barrier
            if (done) break;
            T::lds_sync();
        }
        T::lds_sync();  // team-uniform, as the loop's exit is: the state the last transition left is visible to every wavefront
        // the one emission, as k_gather has it
        const int lane = lane0;
        const int row = out_row(p, p.slot, e);
        if (KIND == PCBENV_SPATIAL) T::build_pin_tables(p, l, lane);
        T::template emit_features_full<KIND>(p, l, row, lane);
        if (KIND == PCBENV_SPATIAL) {
            T::emit_component_grid(p, l, row, lane);  // from the pin tables (unrotated coordinates)
            T::feat_cache_fill(p, l, e, lane);        // trajectory layout: what this episode's steps copy, tagged with `episode`
            T::lds_sync();                            // the tables share their zone with the class map of emit_pin_grid
        }
        T::template mask_and_emit<KIND, WW>(p, l, row, lane, true, 0, p.H);
        if (KIND == PCBENV_SPATIAL) T::template emit_pin_grid<WW>(p, l, row, lane, 0, p.H);
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
