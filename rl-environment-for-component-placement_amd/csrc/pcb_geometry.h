// pcb_geometry.h -- the segment-pair geometry of the routing reward as pure scalar code: the reference's intersection test, the
// form of it the kernels run (per-segment terms hoisted, branch-free) and the exact integer extent pre-filter.  Plain C++17
// behind PCB_HD (it includes only <math.h> and pcb_layout.h): the kernels (pcb_reward.h) and tools/kernel_models_check.cpp, which
// sweeps the forms against each other on the CPU, compile the same text, one IEEE operation per written operator (-ffp-contract=off).
#pragma once
#include <math.h>

#include "pcb_layout.h"

// S:653-702 is_intersect, in the reference's own form.  Its only caller is the CPU check: the kernels run slots_intersect.
PCB_HD inline bool is_intersect(double x1, double y1, double x2, double y2, double x3, double y3, double x4, double y4) {
    if ((x1 == x3 && y1 == y3) || (x1 == x4 && y1 == y4) || (x2 == x3 && y2 == y3) || (x2 == x4 && y2 == y4)) return true;
    double det = (x1 - x2) * (y3 - y4) - (y1 - y2) * (x3 - x4);
    if (det == 0) return false;
    double a = x1 * y2 - y1 * x2, b = x3 * y4 - y3 * x4;
    double x = (a * (x3 - x4) - (x1 - x2) * b) / det;
    double y = (a * (y3 - y4) - (y1 - y2) * b) / det;
    return fmin(x1, x2) <= x && x <= fmax(x1, x2) && fmin(x3, x4) <= x && x <= fmax(x3, x4) &&
           fmin(y1, y2) <= y && y <= fmax(y1, y2) && fmin(y3, y4) <= y && y <= fmax(y3, y4);
}

// ---- routes -------------------------------------------------------------------------------------
// A route is kept as one segment slot per pin q (slots of net n are nstart[n]..nstart[n+1]-1, so slots are
// net-major like the reference's route lists); act[q] = 1 if the slot carries a segment.
struct SegView { double *X1, *Y1, *X2, *Y2, *D, *A, *DX, *DY, *cen; int *act, *nstart, *nsum; unsigned *bbox; unsigned short *pairs; unsigned char *beam; int N; };  // N = max_num_nets: the per-net tables' size
// PAIR_ENTRIES_PER_WAVE and the zone sizes SEG_*: pcb_layout.h (the host sizes the zone by the same formulas)
PCB_HD inline SegView seg_view(double *seg, int P, int N) {
    SegView v;
    v.N = N;
    v.X1 = seg; v.Y1 = seg + P; v.X2 = seg + 2 * P; v.Y2 = seg + 3 * P; v.D = seg + 4 * P;
    v.cen = seg + 5 * P;                              // cx[N], cy[N]
    v.act = (int *)(v.cen + 2 * N);                   // [P]
    v.nstart = v.act + P;                             // [N + 1], then 3 spare words (nstart[N + 1] = pair counter)
    v.nsum = v.nstart + N + 1 + 3;                    // [2 * N] integer coordinate sums per net
    v.beam = (unsigned char *)seg + ((SEG_FIXED_BYTES(P, N) + 7) & ~7);
    v.A = (double *)v.beam; v.DX = v.A + P; v.DY = v.A + 2 * P;  // per segment: x1*y2 - y1*x2, x1 - x2, y1 - y2
    v.bbox = (unsigned *)(v.A + 3 * P);               // [P] integer extents (x_lo, x_hi, y_lo, y_hi), one byte each
    v.pairs = (unsigned short *)(v.bbox + P);         // [PAIR_ENTRIES_PER_WAVE] per wavefront
    return v;
}

// is_intersect (S:653-702) on two slots, with the per-segment terms hoisted: the operations and their order are
// exactly the reference's -- (x1*y2 - y1*x2), (x1 - x2), (y1 - y2) are sub-expressions of its formulas.
// Written without branches so that several candidates per lane can be in flight at once (the count is bound by
// the LDS and float64 division latency of one wavefront, not by issue slots): det == 0 gives inf / NaN
// coordinates, which is harmless and masked by the explicit test.
PCB_HD inline bool slots_intersect(const SegView &v, int i, int j) {
    const double x1 = v.X1[i], y1 = v.Y1[i], x2 = v.X2[i], y2 = v.Y2[i];
    const double x3 = v.X1[j], y3 = v.Y1[j], x4 = v.X2[j], y4 = v.Y2[j];
    const double dxi = v.DX[i], dyi = v.DY[i], dxj = v.DX[j], dyj = v.DY[j];
    const double a = v.A[i], b = v.A[j];
    const bool shared = ((x1 == x3) & (y1 == y3)) | ((x1 == x4) & (y1 == y4)) | ((x2 == x3) & (y2 == y3)) | ((x2 == x4) & (y2 == y4));
    const double det = dxi * dyj - dyi * dxj;
    const double x = (a * dxj - dxi * b) / det;
    const double y = (a * dyj - dyi * b) / det;
    const bool inside = (fmin(x1, x2) <= x) & (x <= fmax(x1, x2)) & (fmin(x3, x4) <= x) & (x <= fmax(x3, x4)) &
                        (fmin(y1, y2) <= y) & (y <= fmax(y1, y2)) & (fmin(y3, y4) <= y) & (y <= fmax(y3, y4));
    return shared | ((det != 0) & inside);
}
// Exact pre-filter: if the closed x- (or y-) extents of the two segments are disjoint, no x (y) can lie in both,
// so the reference's final range test fails whatever the computed intersection point is (a shared end point,
// its only early "True", puts a common point in both extents).  The extents are kept as conservatively rounded
// integers (floor of the minimum, ceil of the maximum; coordinates are in [0, 127]), four bytes per segment, so
// the filter is one LDS word per segment and a few integer compares; a pair it lets through is decided by the
// full float64 test, a pair it rejects has disjoint real extents.  Saves the two float64 divisions.
PCB_HD inline unsigned pack_extents(double x1, double y1, double x2, double y2) {
    const unsigned xl = (unsigned)floor(fmin(x1, x2)), xh = (unsigned)ceil(fmax(x1, x2));
    const unsigned yl = (unsigned)floor(fmin(y1, y2)), yh = (unsigned)ceil(fmax(y1, y2));
    return xl | (xh << 8) | (yl << 16) | (yh << 24) | 0x80000000u;  // bit 31 = slot carries a segment
}
PCB_HD inline unsigned umin(unsigned a, unsigned b) { return a < b ? a : b; }
PCB_HD inline unsigned umax(unsigned a, unsigned b) { return a > b ? a : b; }
PCB_HD inline bool extents_overlap(unsigned a, unsigned b) {  // branch-free
    const unsigned xl = umax(a & 0xFFu, b & 0xFFu), xh = umin((a >> 8) & 0xFFu, (b >> 8) & 0xFFu);
    const unsigned yl = umax((a >> 16) & 0xFFu, (b >> 16) & 0xFFu), yh = umin((a >> 24) & 0x7Fu, (b >> 24) & 0x7Fu);
    return ((a & b & 0x80000000u) != 0) & (xl <= xh) & (yl <= yh);
}
// What the pair count keeps per slot q next to its end points: the hoisted terms of slots_intersect and the extents.
PCB_HD inline void prepare_slot(const SegView &v, int q) {
    const double x1 = v.X1[q], y1 = v.Y1[q], x2 = v.X2[q], y2 = v.Y2[q];
    v.A[q] = x1 * y2 - y1 * x2; v.DX[q] = x1 - x2; v.DY[q] = y1 - y2;
    v.bbox[q] = v.act[q] ? pack_extents(x1, y1, x2, y2) : 0u;
}
