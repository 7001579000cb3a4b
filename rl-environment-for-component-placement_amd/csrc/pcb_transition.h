// pcb_transition.h -- the scalar core of one transition, stated once: the flat action code, validate_action's range and
// bit test, update_grid's extent and row fill (in LDS words, and for one 64-column row held as a value, with the legal-mask
// window folded from such rows), place_component's pin rotation with its inverse, the cursor and `done`.
// This is the arithmetic that must match the reference bit for bit.  Plain C++17 behind PCB_HD (it includes only
// pcb_records.h): the step, playout and policy kernels and tools/transition_check.cpp, which replays the recorded reference
// transitions of tests/golden on the CPU, compile the same text.  Nothing here knows a team size: the loops over rows and
// pins that stride by it, and the barriers, stay with the two callers: Team<>::transition (pcb_step.h) and, without
// observations, PCB_TRANSITION_NO_OBS (pcb_walk.h), which k_playout and k_gather_paths expand.
//
// Each piece is a macro with a function of the same name in lower case around it.  The step and playout kernels expand
// the macros where the text used to stand: an inlined function body reaches the optimiser in another shape than the same expression
// written in place (other operand order, the component record read whole), which moved instructions and registers in
// dozens of k_step builds (profiles/transition_refactor.txt).  The CPU check and pcb_policy.hip call the functions.
#pragma once
#include "pcb_records.h"

// ---- the flat action code a = o*H*W + x*W + y (utils/environment/env_wrappers.py:80-98, :184-199); HW = H * W ----------
#define PCB_FLATTEN_ACTION(o, x, y, HW, W) ((o) * (HW) + (x) * (W) + (y))
PCB_HD inline int flatten_action(int o, int x, int y, int HW, int W) { return PCB_FLATTEN_ACTION(o, x, y, HW, W); }
// (a in [0, O*H*W): what a kernel has computed itself)
PCB_HD inline void split_action(int a, int HW, int W, int *o, int *x, int *y) {
    *o = a / HW;
    const int r = a - *o * HW;
    *x = r / W; *y = r - *x * W;
}
// a caller's code: out of range is data (an invalid action), o = -1
PCB_HD inline void unflatten_action(int a, int O, int HW, int W, int *o, int *x, int *y) {
    if (a < 0 || a >= O * HW) { *o = -1; *x = *y = 0; }
    else split_action(a, HW, W, o, x, y);
}

// ---- validate_action (S:1699-1723): action_mask[o, x, y] == 1; anything out of range is invalid ---------------------
#define PCB_ACTION_IN_RANGE(o, x, y, O, H, W) ((o) >= 0 && (o) < (O) && (x) >= 0 && (x) < (H) && (y) >= 0 && (y) < (W))
PCB_HD inline bool action_in_range(int o, int x, int y, int O, int H, int W) { return PCB_ACTION_IN_RANGE(o, x, y, O, H, W); }
// vm: the legal-action bit rows [2, H, WW]; orientations 2 / 3 share the planes of 0 / 1, so the plane of orientation o
// starts at word plane_off = (o & 1) * H * WW (the caller's product: it has one at hand).  (o, x, y) in range.
#define PCB_LEGAL_BIT(vm, plane_off, WW, x, y) (((vm)[(plane_off) + (x) * (WW) + ((y) >> 6)] >> ((y) & 63)) & 1ull)
PCB_HD inline bool legal_bit(const u64 *vm, int H, int WW, int o, int x, int y) { return PCB_LEGAL_BIT(vm, (o & 1) * (H * WW), WW, x, y); }

// ---- update_grid (S:1742-1747): rows x..x+ph-1, columns y..y+pw-1 of a ch x cw component ------------------------------
#define PCB_PLACED_H(o, ch, cw) (((o) & 1) ? (cw) : (ch))
#define PCB_PLACED_W(o, ch, cw) (((o) & 1) ? (ch) : (cw))
PCB_HD inline void placed_extent(int ch, int cw, int o, int *ph, int *pw) { *ph = PCB_PLACED_H(o, ch, cw); *pw = PCB_PLACED_W(o, ch, cw); }
// columns y..y+pw-1 of the occupancy bit row whose WW words start at words[first]
#define PCB_IMAX(a, b) ((a) > (b) ? (a) : (b))
#define PCB_IMIN(a, b) ((a) < (b) ? (a) : (b))
#define PCB_OCCUPY_ROW(words, first, WW, y, pw) \
    for (int w_ = 0; w_ < (WW); w_++) { \
        const int lo_ = PCB_IMAX(y, 64 * w_) - 64 * w_, hi_ = PCB_IMIN((y) + (pw), 64 * w_ + 64) - 64 * w_;  /* bit range in word w_ */ \
        if (hi_ > lo_) (words)[(first) + w_] |= ((hi_ - lo_) >= 64 ? ~0ull : ((1ull << (hi_ - lo_)) - 1ull)) << lo_; \
    }
PCB_HD inline void occupy_row(u64 *row_words, int WW, int y, int pw) { PCB_OCCUPY_ROW(row_words, 0, WW, y, pw) }
// The same for WW == 1 with the row held as a value: `row` after columns y..y+pw-1 are filled, 0 <= y, 1 <= pw, y + pw <= 64
// (what a valid action gives).  pw == 64 forces y == 0, and y + pw == 64 shifts by y < 64: no shift by 64 either way.
#define PCB_OCCUPIED_ROW1(row, y, pw) ((row) | (((pw) >= 64 ? ~0ull : ((1ull << (pw)) - 1ull)) << (y)))
PCB_HD inline u64 occupied_row1(u64 row, int y, int pw) { return PCB_OCCUPIED_ROW1(row, y, pw); }
// row r of the grid, `row` before, after update_grid has placed ph x pw cells at (x, y)
#define PCB_ROW_AFTER_UPDATE1(row, r, x, ph, y, pw) (((r) >= (x) && (r) < (x) + (ph)) ? PCB_OCCUPIED_ROW1(row, y, pw) : (row))
PCB_HD inline u64 row_after_update1(u64 row, int r, int x, int ph, int y, int pw) { return PCB_ROW_AFTER_UPDATE1(row, r, x, ph, y, pw); }

// ---- the legal-mask window on rows held as values, one 64-column row per lane (WW == 1; R:526-567, S:1792-1835) -------
// Team<>::window_mask's one-row-per-lane arm in three pieces that know no lane: the horizontal OR over pw columns, the
// vertical OR over ph rows by log-step doubling -- `down(a, s)` is the value `a` of the lane s further on, 0 beyond the
// last; V is one lane's u64 on the device and all 64 of them in tools/step_dataflow_check.cpp -- and the cut to the
// columns where the window fits.  Team<>::window_mask_row (pcb_team_io.h) puts them together.
PCB_HD inline u64 row1_hfold(u64 f, int pw) {
    int s = 1;
    while (2 * s <= pw) { f |= f >> s; s *= 2; }
    if (s < pw) f |= f >> (pw - s);
    return f;
}
template <class V, class Down> PCB_HD inline V rows_vfold(V a, int ph, Down down) {
    int s = 1;
    while (2 * s <= ph) { a = a | down(a, s); s *= 2; }
    if (s < ph) a = a | down(a, ph - s);
    return a;
}
PCB_HD inline u64 row1_free_below(u64 a, int n) { return n <= 0 ? 0ull : (~a & (n >= 64 ? ~0ull : ((1ull << n) - 1ull))); }

// ---- place_component (S:149-190): pin pr of the ch x cw component placed at (x, y) with orientation o.  The rotation
// is kept in rel_x / rel_y (in place, as the reference does); PCB_UNROTATE_REL, just below, undoes it. ------------------
#define PCB_PLACE_PIN(pr, o, ch, cw, x, y) { \
        const int rx_ = (pr).rel_x, ry_ = (pr).rel_y; \
        if ((o) == 1) { (pr).rel_x = ry_; (pr).rel_y = (ch) - rx_ - 1; } \
        else if ((o) == 2) { (pr).rel_x = (ch) - rx_ - 1; (pr).rel_y = (cw) - ry_ - 1; } \
        else if ((o) == 3) { (pr).rel_x = (cw) - ry_ - 1; (pr).rel_y = rx_; } \
        (pr).abs_x = (signed char)((x) + (pr).rel_x); (pr).abs_y = (signed char)((y) + (pr).rel_y); \
    }
PCB_HD inline PinRec place_pin(PinRec pr, int o, int ch, int cw, int x, int y) { PCB_PLACE_PIN(pr, o, ch, cw, x, y) return pr; }
// (rx, ry): the relative cell of a placed component's pin, in; as the instance gave it, out.  draw_components
// (S:1677-1697) runs at reset only, so component_grid never shows the rotation (quirk Q4): build_pin_tables undoes it.
#define PCB_UNROTATE_REL(o, ch, cw, rx, ry) { \
        const int ax_ = (rx), ay_ = (ry); \
        if ((o) == 1) { (rx) = (ch) - 1 - ay_; (ry) = ax_; } \
        else if ((o) == 2) { (rx) = (ch) - 1 - ax_; (ry) = (cw) - 1 - ay_; } \
        else if ((o) == 3) { (rx) = ay_; (ry) = (cw) - 1 - ax_; } \
    }
PCB_HD inline void unrotate_rel(int o, int ch, int cw, int *rx, int *ry) { PCB_UNROTATE_REL(o, ch, cw, *rx, *ry) }

// ---- cursor and done (S:1856-1869) -------------------------------------------------------------------------------
PCB_HD inline int next_component(int cur, int ncomp) { return cur + 1 < ncomp ? cur + 1 : -1; }  // -1: all placed
// cur_after: the cursor after the placement; any: a legal cell is left for the next component
template <int KIND> PCB_HD inline bool episode_done(int cur_after, bool any) { return KIND == PCBENV_SQUARE ? !any : (cur_after < 0 || !any); }
