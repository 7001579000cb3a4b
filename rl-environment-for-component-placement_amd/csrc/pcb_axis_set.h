// pcb_axis_set.h -- the per-axis legal set of the factorised policies, stated once: which values of one action
// coordinate are still open when some of the other coordinates are fixed.  Plain C++17 (it includes pcb_layout.h for
// PCB_HD only): the axis kernels (pcb_policy_axis.hip) and tools/axis_set_check.cpp -- a CPU program that sweeps it
// against a brute-force dense mask -- compile the same text.
//
// Axes are 0 = orientation (n = O), 1 = x (n = H), 2 = y (n = W); `given` is a bit set (1u << axis) of the other axes
// whose values vals[axis] are fixed.  For target axis t
//   L = { v in [0, n) : some legal (o, x, y) has coordinate t equal to v and every given coordinate equal to its value }
// where (o, x, y) is legal when o < O and bit y % 64 of word [o & 1, x, y / 64] of the bit rows ([2][H][WW], the layout
// pcbenv_mask_bits documents) is set.  Bits of columns >= W never count, and O == 1 (the square kind) never reads plane 1.
// This is every mask of utils/agent/factorized_action_distributions.py: reduce_max over (H, W) (:358), gather o then
// reduce_max over W (:398-401), gather o, x (:445-448), reduce_max over (o, W) (:717), gather x then max over o
// (:757-758), gather x, y (:803-808) -- and of the four orders the reference does not ship.
//
// The pieces below are what one lane does; legal_set() composes them serially, the kernels compose the same pieces with
// the rows spread over a wavefront.
#pragma once
#include <stdint.h>

#include "pcb_layout.h"

namespace pcb_axis {

typedef unsigned long long word_t;
enum { AXIS_O = 0, AXIS_X = 1, AXIS_Y = 2, MAX_N = 128 };

struct Geom { int O, H, W, WW; };
struct Set128 {
    word_t lo, hi;  // bit v of lo: value v, bit v of hi: value 64 + v
    PCB_HD bool any() const { return (lo | hi) != 0; }
    PCB_HD bool has(int v) const { return v >= 0 && v < MAX_N && (((v < 64 ? lo : hi) >> (v & 63)) & 1ull); }
};
PCB_HD inline Set128 operator|(Set128 a, Set128 b) { return Set128{a.lo | b.lo, a.hi | b.hi}; }
PCB_HD inline Set128 operator&(Set128 a, Set128 b) { return Set128{a.lo & b.lo, a.hi & b.hi}; }

PCB_HD inline int axis_size(const Geom &g, int axis) { return axis == AXIS_O ? g.O : axis == AXIS_X ? g.H : g.W; }
PCB_HD inline word_t low_bits64(int n) { return n <= 0 ? 0ull : n >= 64 ? ~0ull : (1ull << n) - 1ull; }
// the values [0, n)
PCB_HD inline Set128 first_n(int n) { return Set128{low_bits64(n), low_bits64(n - 64)}; }
PCB_HD inline Set128 only(int v) { return v < 64 ? Set128{1ull << v, 0ull} : Set128{0ull, 1ull << (v - 64)}; }

// every given value inside its axis (a value outside makes L empty: error bit 3 of the entry points)
PCB_HD inline bool given_in_range(const Geom &g, unsigned given, const int vals[3]) {
    for (int a = 0; a < 3; a++)
        if (((given >> a) & 1u) && (vals[a] < 0 || vals[a] >= axis_size(g, a))) return false;
    return true;
}
// the legal columns of row x of a plane; columns >= W are cut off here, so nothing downstream can count them
PCB_HD inline Set128 row_cols(const word_t *bits, const Geom &g, int plane, int x) {
    const word_t *r = bits + ((long long)plane * g.H + x) * g.WW;
    return Set128{r[0], g.WW > 1 ? r[1] : 0ull} & first_n(g.W);
}
// the planes a stage reads, as a bit set: the given orientation's, otherwise those some o < O uses
PCB_HD inline unsigned planes_read(const Geom &g, unsigned given, const int vals[3]) {
    if ((given >> AXIS_O) & 1u) return 1u << (vals[AXIS_O] & 1);
    return g.O > 1 ? 3u : 1u;
}
// the columns a stage looks at: the given y alone, otherwise all W
PCB_HD inline Set128 cols_read(const Geom &g, unsigned given, const int vals[3]) {
    return ((given >> AXIS_Y) & 1u) ? only(vals[AXIS_Y]) : first_n(g.W);
}
// the rows a stage looks at, [*x0, *x1): the given x alone, otherwise all H
PCB_HD inline void rows_read(const Geom &g, unsigned given, const int vals[3], int *x0, int *x1) {
    if ((given >> AXIS_X) & 1u) { *x0 = vals[AXIS_X]; *x1 = vals[AXIS_X] + 1; }
    else { *x0 = 0; *x1 = g.H; }
}
// OR of the rows x0, x0 + step, ... below x1 of the planes in `planes` (a lane's share, or with step 1 the whole)
PCB_HD inline Set128 rows_or(const word_t *bits, const Geom &g, unsigned planes, int x0, int x1, int step) {
    Set128 s{0ull, 0ull};
    for (int p = 0; p < 2; p++)
        if ((planes >> p) & 1u)
            for (int x = x0; x < x1; x += step) s = s | row_cols(bits, g, p, x);
    return s;
}
// target x: is row v open in one of the planes, within the columns
PCB_HD inline bool row_open(const word_t *bits, const Geom &g, unsigned planes, Set128 cols, int v) {
    return v < g.H && (rows_or(bits, g, planes, v, v + 1, 1) & cols).any();
}
// target orientation: the values o < O whose plane o & 1 is open (open0 / open1: plane 0 / 1 has a legal cell in range)
PCB_HD inline Set128 orientations_open(const Geom &g, bool open0, bool open1) {
    return Set128{(open0 ? 0x5ull : 0ull) | (open1 ? 0xAull : 0ull), 0ull} & first_n(g.O);
}

// The whole derivation, serially.  vals[a] is read only where `given` names a; `given` must not name `axis`.
PCB_HD inline Set128 legal_set(const word_t *bits, const Geom &g, int axis, unsigned given, const int vals[3]) {
    if (!given_in_range(g, given, vals)) return Set128{0ull, 0ull};
    const unsigned planes = planes_read(g, given, vals);
    const Set128 cols = cols_read(g, given, vals);
    int x0, x1;
    rows_read(g, given, vals, &x0, &x1);
    if (axis == AXIS_Y) return rows_or(bits, g, planes, x0, x1, 1);
    if (axis == AXIS_X) {
        Set128 s{0ull, 0ull};
        for (int v = 0; v < g.H; v++)
            if (row_open(bits, g, planes, cols, v)) s = s | only(v);
        return s;
    }
    const bool open0 = (rows_or(bits, g, 1u, x0, x1, 1) & cols).any();
    const bool open1 = g.O > 1 && (rows_or(bits, g, 2u, x0, x1, 1) & cols).any();
    return orientations_open(g, open0, open1);
}

}  // namespace pcb_axis
