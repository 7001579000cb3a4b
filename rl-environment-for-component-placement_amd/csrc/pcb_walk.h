// pcb_walk.h -- kernel text that more than one of k_gather, k_playout and k_gather_paths runs, stated once: the read of a
// caller's forced action, the transition without observations, and k_gather's head (the header patch) and tail (the one
// whole emission of a slot).  Part of libpcbenv.so (CDNA4 / gfx950 only); pcb_kernels.h, pcb_playout.h and
// pcb_gather_paths.h include it.
//
// Every piece is a text macro, expanded where the copies used to stand, for the reason pcb_transition.h gives: the same
// steps as a __forceinline__ member of Team<> reach the optimiser in another shape and move a few bytes and scalar spills
// in every kernel that uses them, while the expanded text leaves every kernel's instructions as they were
// (profiles/path_walk_refactor.txt).  As the class sections of Team<> do, the macros take the names that every kernel has
// from the enclosing kernel -- KIND, WW, NT, T, p, l, H, W, HW, plane -- and as parameters what differs between them.
#pragma once
#include "pcb_team.h"

// ---- a caller's action of environment / playout `idx` from fa = one step of [steps, n] or [steps, n, 3] storage -----------
// As run_env reads a caller's action: out of range is data (an invalid action), checked before use by the transition.
// `given` receives the flat code as the caller wrote it (flat format only).
#define PCB_READ_FORCED_ACTION(fa, fmt, idx, given, o, x, y) \
    if ((fmt) == PCBENV_ACTION_FLAT) { \
        (given) = (fa)[idx]; \
        unflatten_action((given), p.O, HW, W, &(o), &(x), &(y)); \
    } else { \
        (o) = (fa)[3 * (size_t)(idx)]; (x) = (fa)[3 * (size_t)(idx) + 1]; (y) = (fa)[3 * (size_t)(idx) + 2]; \
        if (KIND == PCBENV_SQUARE) (o) = 0; \
    }

// ---- one transition of the state in LDS with action (o, x, y), without observations -----------------------------------
// The transition a handle without PCBENV_FLAG_AUTO_RESET makes (Team<>::transition in MODE_ALL, pcb_step.h, which
// interleaves the observation stores with the same steps): validate_action -> update_grid -> place_component -> cursor ->
// legal mask without emission -> done.  The arithmetic is pcb_transition.h's.  `env` is the index mask_and_emit is given
// (nothing is emitted, so no row is addressed by it); `lane` the caller's lane index; `valid` and `done` the caller's
// bools, assigned here.  Team-uniform: every wavefront takes the same branches, so the barriers are met by all.
#define PCB_TRANSITION_NO_OBS(env, lane, o, x, y, valid, done) { \
        const int cur = l.hdr->cur, ncomp = l.hdr->ncomp, npins = l.hdr->npins; \
        (valid) = PCB_ACTION_IN_RANGE(o, x, y, p.O, H, W) && (KIND == PCBENV_SQUARE || cur >= 0); \
        if (valid) (valid) = PCB_LEGAL_BIT(l.vm, ((o) & 1) * plane, WW, x, y); \
        if (NT > WAVE) T::lds_sync();  /* every wavefront has read the cursor and the mask bit before anything below changes them */ \
        (done) = true;  /* an invalid action is a terminal transition with the state unchanged (quirk Q8 iii) */ \
        if (valid) { \
            int ph, pw; \
            CompRec cr = CompRec(); \
            if (KIND == PCBENV_SQUARE) ph = pw = p.component_n; \
            else { \
                cr = l.comps[cur]; \
                ph = PCB_PLACED_H(o, cr.h, cr.w); \
                pw = PCB_PLACED_W(o, cr.h, cr.w); \
            } \
            for (int rr = (x) + (lane); rr < (x) + ph && rr < H; rr += NT) { \
                PCB_OCCUPY_ROW(l.occ, rr * WW, WW, y, pw) \
            } \
            if (KIND != PCBENV_SQUARE) { \
                if ((lane) == 0) { l.comps[cur].px = (signed char)(x); l.comps[cur].py = (signed char)(y); l.comps[cur].o = (unsigned char)(o); } \
                if (KIND == PCBENV_PIN || KIND == PCBENV_SPATIAL) { \
                    const int ch = cr.h, cw = cr.w; \
                    for (int pin = (lane); pin < npins; pin += NT) {  /* S:149-190 place_component */ \
                        PinRec pr = l.pins[pin]; \
                        if (pr.comp != cur) continue; \
                        PCB_PLACE_PIN(pr, o, ch, cw, x, y) \
                        l.pins[pin] = pr; \
                    } \
                } \
                if ((lane) == 0) l.hdr->cur = (short)next_component(cur, ncomp); \
            } \
            T::lds_sync();  /* the placement is visible to every wavefront before the mask is derived from it */ \
            const bool any = T::template mask_and_emit<KIND, WW>(p, l, env, lane, false, 0, 0);  /* team-uniform (block_any) */ \
            (done) = episode_done<KIND>(l.hdr->cur, any); \
        } \
        /* `done` is team-uniform: valid, cur and `any` are functions of LDS words every wavefront read behind a barrier */ \
    }

// ---- k_gather's head: the header of a block taken over from another environment, patched ------------------------------
// l holds the source's block; own = the destination environment's block in HBM.  What the header must not take over:
//   qcursor, episode  the destination's instance stream: its next reset takes its own next record.  feat_cache_valid
//                     compares the cache tag with `episode`, so the spatial cache is refilled by the emission below
//                     under that tag;
//   term_seq / pos    a copied terminal-list mark would claim the source's list entry in the next step launch
//                     (MODE_DELEGATED waiting for helpers that work on another environment): not listed;
//   pre_action        drawn from the source's mask for the source's global index: cleared;
//   feat_gen          the destination's bind generation: its pin-feature rows are written whole by the emission below.
#define PCB_GATHER_PATCH_HEADER(own, lane) \
    if ((lane) == 0) { \
        const EnvHdr *oh = (const EnvHdr *)(own); \
        l.hdr->qcursor = oh->qcursor; l.hdr->episode = oh->episode; \
        l.hdr->term_seq = 0u; l.hdr->term_pos = 0u; \
        l.hdr->pre_action = 0u; \
        if (KIND == PCBENV_PIN || KIND == PCBENV_SPATIAL) l.hdr->feat_gen = p.bind_gen; \
    }

// ---- k_gather's tail: every bound tensor of row `row` (environment e's, in the selected slot) written whole from LDS ---
// The emission of a trajectory slot, where nothing may be assumed about what the destination holds.
#define PCB_GATHER_EMIT_SLOT(e, row, lane) { \
        if (KIND == PCBENV_SPATIAL) T::build_pin_tables(p, l, lane); \
        T::template emit_features_full<KIND>(p, l, row, lane); \
        if (KIND == PCBENV_SPATIAL) { \
            T::emit_component_grid(p, l, row, lane);  /* from the pin tables (unrotated coordinates) */ \
            T::feat_cache_fill(p, l, e, lane);        /* trajectory layout: what this episode's steps copy, tagged with `episode` */ \
            T::lds_sync();                            /* the tables share their zone with the class map of emit_pin_grid */ \
        } \
        T::template mask_and_emit<KIND, WW>(p, l, row, lane, true, 0, p.H); \
        if (KIND == PCBENV_SPATIAL) T::template emit_pin_grid<WW>(p, l, row, lane, 0, p.H); \
    }
