// pcb_routing.h -- what the routing reward does that does not depend on the team size: the float64 norm, the full intersection
// test on a wavefront's candidate buffer, and the beam search of one net on its four lanes.  Free device functions; the sweeps
// that call them depend on the team size and are class sections of Team<> (pcb_reward.h, pcb_beam.h).  CDNA4 / gfx950 only.
#pragma once
#include "pcb_device.h"
#include "pcb_geometry.h"
#include "pcb_setmodel.h"

// S:1288-1301 euclidean_distance == np.linalg.norm == sqrt(ddot): sqrt(fma(dy, dy, dx*dx))
__device__ inline double norm2(double dx, double dy) { return __dsqrt_rn(__fma_rn(dy, dy, __dmul_rn(dx, dx))); }
// Full test on candidates [0, n) of a wavefront's buffer, two per lane and step so that their LDS reads and
// divisions overlap.
typedef __attribute__((address_space(3))) unsigned short lds_u16;  // keeps the buffer accesses ds_* instead of flat_*
__device__ inline int count_candidates(const SegView &v, const volatile lds_u16 *buf, int n, int wl_lane) {
    int cnt = 0;
    for (int base = 0; base < n; base += 2 * WAVE) {
        const int i0 = base + wl_lane, i1 = i0 + WAVE;
        const unsigned short p0 = i0 < n ? buf[i0] : (unsigned short)0, p1 = i1 < n ? buf[i1] : (unsigned short)0;
        const bool r0 = slots_intersect(v, p0 & 0xFF, p0 >> 8), r1 = slots_intersect(v, p1 & 0xFF, p1 >> 8);
        cnt += ((i0 < n) & r0) + ((i1 < n) & r1);
    }
    return cnt;
}

// ---- beam-search routing (S:1273-1286 pin_outlier, S:1303-1369 beam_search, S:1371-1406) -----------------
// beam_search keeps, per popped path, the beam_width nearest unvisited points of
// `sorted(points_to_visit - visited, key=distance)`.  Python's sort is stable, so neighbours at equal distance
// keep the iteration order of that temporary CPython set -- a pure function of the tuple hashes and of
// Objects/setobject.c's open-addressing table (SURVEY.md trap T2).  That order can only change WHICH points are
// kept when the beam_width-th and the next distance tie (the order among kept neighbours is irrelevant: heapq
// pops by (priority, path), not by insertion).  So the set model below runs only on such boundary ties.
// Four lanes per net (one per heappop of a level, see "laid out for latency" below); all per-net scratch lives in LDS
// (no private-memory arrays -> no scratch segment).
// one partial path of the beam: four 64-bit words so that queue traffic is wide LDS accesses and the popped
// entry lives in registers.  meta = visited (bits 0-15) | length (bits 16-23); p0/p1 = the path, one byte per
// point index (0xFF = the start point).
struct BsEntry {
    double prio; u64 meta, p0, p1;
    __device__ unsigned visited() const { return (unsigned)(meta & 0xFFFFull); }
    __device__ int len() const { return (int)((meta >> 16) & 0xFFull); }
    __device__ int at(int j) const { return (int)(((j < 8 ? p0 : p1) >> ((j & 7) * 8)) & 0xFFull); }
    __device__ void push(int idx) {
        const int l = len();
        const u64 b = (u64)(unsigned)idx << ((l & 7) * 8);
        if (l < 8) p0 |= b; else p1 |= b;
        meta = (meta & ~(0xFFull << 16)) | ((u64)(l + 1) << 16) | (1ull << idx);
    }
};
static_assert(sizeof(BsEntry) == 32, "beam LDS records");
// BEAM_LDS_PER_NET / BEAM_LDS_BYTES: pcb_layout.h (the host sizes the zone by the same formulas)
static_assert(PCBENV_MAX_PINS_PER_NET <= 16, "BsEntry::meta / p0 / p1: 16 visited bits, 16 path bytes; dist, order and hs of beam_route_lanes: 16 entries");

// ---- beam search laid out for latency -----------------------------------------------------------------------
// A terminal wavefront is alone with a short dependent chain (one level per pin of the net): what counts is the
// number of dependent instructions and LDS round trips per level, not lanes.  So:
//  * a net gets PCBENV_MAX_BEAM_WIDTH lanes, one per heappop of a level: all entries of a level have the same length,
//    hence the same number of unvisited points and the same number of children -- lane t selects the t-th smallest
//    queue entry by itself, expands it and writes its children to next[t * take ...): the only thing lanes of a net
//    share is the queue in LDS (wave-level ordering, a net's lanes never span two wavefronts);
//  * "the k nearest unvisited points, index order among equals" is taken on integer keys (dx*dx + dy*dy) << 4 | index
//    held in registers: coordinates are small integers, the squared distance is exact and np.linalg.norm is strictly
//    monotone on it, so the order (and the boundary tie) is the reference's; only the priorities need float64 norms;
//  * the farthest-from-centroid start pin and the route segments are computed one pin per lane before / after;
//  * the rare boundary tie still runs the serial CPython-set model, the lanes of a net taking turns (shared scratch).
// Same results as round 1's one-lane-per-net search (git history): same pop order (first index among fully equal
// entries), same children in the same queue order.
#define BEAM_LANES_PER_NET PCBENV_MAX_BEAM_WIDTH
static_assert(BEAM_LANES_PER_NET == PCBENV_MAX_BEAM_WIDTH && (BEAM_LANES_PER_NET & (BEAM_LANES_PER_NET - 1)) == 0 && WAVE % BEAM_LANES_PER_NET == 0,
              "route_beam: lane = group * BEAM_LANES_PER_NET + turn (lane & (BEAM_LANES_PER_NET - 1)), a lane per heappop of a level");
#if defined(PCBENV_STAMPS) && defined(PCBENV_STAMPS_BEAM)  // phase cycles of the search, accumulated by lane 0 into stamp slots 26..29
#define BEAM_T0() unsigned long long bt0_; asm volatile("s_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(bt0_) :: "memory")
#define BEAM_ACC(k) do { unsigned long long t_; asm volatile("s_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(t_) :: "memory"); if (threadIdx.x == 0 && beam_dbg) beam_dbg[(size_t)blockIdx.x * 32 + (k)] += t_ - bt0_; bt0_ = t_; } while (0)
#else
#define BEAM_T0() do { } while (0)
#define BEAM_ACC(k) do { } while (0)
#endif
__device__ inline void wave_lds_order() {  // LDS traffic of one wavefront executes in order: only the compiler must not reorder
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront", "local");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront", "local");
}
// all pins of a net, original order (index = offset from the net's first slot), one byte per coordinate
template <int MAXC> struct NetAll {
    u64 xs0, xs1, ys0, ys1;
    __device__ int x(int i) const { return (int)(((MAXC <= 8 || i < 8 ? xs0 : xs1) >> ((i & 7) * 8)) & 0xFFull); }
    __device__ int y(int i) const { return (int)(((MAXC <= 8 || i < 8 ? ys0 : ys1) >> ((i & 7) * 8)) & 0xFFull); }
    __device__ static NetAll load(const PinRec *p, int cnt) {
        NetAll n{0ull, 0ull, 0ull, 0ull};
        #pragma unroll
        for (int i = 0; i < MAXC; i++) {  // all loads go out together; slots past the net repeat pin 0 and are masked
            const PinRec pr = p[i < cnt ? i : 0];
            const u64 x = i < cnt ? (u64)(unsigned char)pr.abs_x << ((i & 7) * 8) : 0ull, y = i < cnt ? (u64)(unsigned char)pr.abs_y << ((i & 7) * 8) : 0ull;
            if (i < 8) { n.xs0 |= x; n.ys0 |= y; } else { n.xs1 |= x; n.ys1 |= y; }
        }
        return n;
    }
};
// python's list comparison of two queued paths of equal priority (entries hold pin indices; all paths of a queue have one length)
template <int MAXC> __device__ inline bool path_less(const BsEntry &a, const BsEntry &e, const NetAll<MAXC> &pt) {
    bool less = a.len() < e.len();
    const int n = a.len() < e.len() ? a.len() : e.len();
    for (int j = 0; j < n; j++) {
        const int pa = a.at(j), pb = e.at(j);
        const int ax = pt.x(pa), ay = pt.y(pa), bx = pt.x(pb), by = pt.y(pb);
        if (ax != bx) { less = ax < bx; break; }
        if (ay != by) { less = ay < by; break; }
    }
    return less;
}
// SMALL: nets of <= 8 pins and beam widths <= 2 (queue <= 4 entries): everything unrolled in registers
template <bool SMALL>
__device__ __forceinline__ void beam_route_lanes(const SegView &v, const PinRec *pins, int s, int cnt, int st, int k, unsigned char *scratch, int t, unsigned long long *beam_dbg) {
    constexpr int MAXC = SMALL ? 8 : PCBENV_MAX_PINS_PER_NET, MAXQ = SMALL ? 4 : PCBENV_MAX_BEAM_WIDTH * PCBENV_MAX_BEAM_WIDTH;
    constexpr unsigned KINF = 0x7FFFFFFFu;
    BEAM_T0();
    BsEntry *queue = (BsEntry *)scratch, *next = queue + k * k;
    double *dist = (double *)(scratch + 64 * k * k);
    unsigned char *order = (unsigned char *)(dist + 16);
    CSet *A = (CSet *)(order + 16), *R = A + 1;
    unsigned *hs = (unsigned *)(R + 1);  // tuple hashes (low words) of the points to visit, valid once A is built
    const NetAll<MAXC> pt = NetAll<MAXC>::load(pins + s, cnt);
    const unsigned all = (1u << cnt) - 1u;
    int qn = 1;
    if (t == 0) {
        BsEntry e0; e0.prio = 0.0; e0.meta = (1ull << 16) | (1ull << st); e0.p0 = (u64)(unsigned)st; e0.p1 = 0ull; queue[0] = e0;
        A->mask = 0;  // "the points' set is not built yet" (a built table has mask >= 7)
    }
    wave_lds_order();
    BEAM_ACC(26);
    for (;;) {
        const int pops = k < qn ? k : qn;
        const bool worker = t < pops;
        // heappop number t: the (t+1)-th smallest (priority, path) of the queue, first index among fully equal entries
        int sel = 0;
        if (SMALL) {
            double pr[MAXQ];
            #pragma unroll
            for (int i = 0; i < MAXQ; i++) { const double q = queue[i].prio; pr[i] = i < qn ? q : __builtin_inf(); }  // stale slots: read, ranked last
            // rank of every entry by priority alone (six compares); two live entries of equal priority are rare and
            // take the general selection below, where python's path comparison breaks the tie
            int rk[MAXQ]; bool eq = false;
            #pragma unroll
            for (int i = 0; i < MAXQ; i++) rk[i] = 0;
            #pragma unroll
            for (int i = 0; i < MAXQ; i++) {
                #pragma unroll
                for (int j = i + 1; j < MAXQ; j++) {
                    const bool lt = pr[j] < pr[i];
                    rk[i] += lt ? 1 : 0; rk[j] += lt ? 0 : 1;
                    eq |= j < qn && pr[j] == pr[i];
                }
            }
            if (!eq) {
                const int want = t < pops ? t : pops - 1;
                #pragma unroll
                for (int i = 0; i < MAXQ; i++) if (rk[i] == want) sel = i;
            } else {
                unsigned taken = 0;
                for (int it = 0; it <= t && it < pops; it++) {
                    int best = -1; double bp = 0.0;
                    #pragma unroll
                    for (int i = 0; i < MAXQ; i++) {
                        if (i >= qn || (taken >> i & 1u)) continue;
                        bool less = best < 0 || pr[i] < bp;
                        if (best >= 0 && pr[i] == bp) less = path_less<MAXC>(queue[i], queue[best], pt);
                        if (less) { best = i; bp = pr[i]; }
                    }
                    taken |= 1u << best; sel = best;
                }
            }
        } else {
            unsigned taken = 0;
            for (int it = 0; it <= t && it < pops; it++) {
                int best = -1; double bp = 0.0;
                for (int i = 0; i < qn; i++) {
                    if (taken >> i & 1u) continue;
                    const double pi = queue[i].prio;
                    bool less = best < 0 || pi < bp;
                    if (best >= 0 && pi == bp) less = path_less<MAXC>(queue[i], queue[best], pt);
                    if (less) { best = i; bp = pi; }
                }
                taken |= 1u << best; sel = best;
            }
        }
        BEAM_ACC(27);
        const BsEntry e = queue[sel];
        const unsigned vis = e.visited();
        if (vis == all) {  // every entry of this level is a complete path: the first pop is the answer
            wave_lds_order();
            if (t == 0) *(BsEntry *)scratch = e;
            break;
        }
        const int cur = e.at(e.len() - 1);
        const int ux = pt.x(cur), uy = pt.y(cur);
        const int cntn = __popc(all & ~vis), take = cntn < k ? cntn : k;
        unsigned chosen[PCBENV_MAX_BEAM_WIDTH + 1];  // the k + 1 smallest keys, ascending
        if (SMALL) {
            unsigned key[MAXC];
            #pragma unroll
            for (int j = 0; j < MAXC; j++) {
                const int dx = ux - pt.x(j), dy = uy - pt.y(j);
                key[j] = (j < cnt && !(vis >> j & 1u)) ? (((unsigned)(dx * dx + dy * dy) << 4) | (unsigned)j) : KINF;
            }
            #pragma unroll
            for (int r = 0; r <= PCBENV_MAX_BEAM_WIDTH; r++) {
                if (r > 2) { chosen[r] = KINF; continue; }
                unsigned mn = KINF;
                #pragma unroll
                for (int j = 0; j < MAXC; j++) mn = min(mn, key[j]);
                chosen[r] = mn;
                #pragma unroll
                for (int j = 0; j < MAXC; j++) key[j] = key[j] == mn ? KINF : key[j];
            }
        } else {  // wide nets / beams: the keys are recomputed per round instead of held (register pressure, not speed)
            unsigned prev = 0u;
            #pragma unroll
            for (int r = 0; r <= PCBENV_MAX_BEAM_WIDTH; r++) {
                unsigned mn = KINF;
                if (r <= k) {
                    for (int j = 0; j < cnt; j++) {
                        const int dx = ux - pt.x(j), dy = uy - pt.y(j);
                        const unsigned kj = (((unsigned)(dx * dx + dy * dy) << 4) | (unsigned)j) + 1u;  // + 1: above `prev` = 0 in round 0
                        if (!(vis >> j & 1u) && kj > prev) mn = min(mn, kj);
                    }
                }
                prev = mn;
                chosen[r] = mn == KINF ? KINF : mn - 1u;
            }
        }
        bool tie = false;
        #pragma unroll
        for (int q = 1; q <= PCBENV_MAX_BEAM_WIDTH; q++) if (q == k && cntn > k) tie = (chosen[q - 1] >> 4) == (chosen[q] >> 4);
        BsEntry *dst = next + t * take;
        if (worker && !tie) {
            #pragma unroll
            for (int r = 0; r < PCBENV_MAX_BEAM_WIDTH; r++) {
                if (r >= take || (SMALL && r >= 2)) continue;
                const int j = (int)(chosen[r] & 15u);
                BsEntry w = e; w.push(j); w.prio = e.prio + norm2((double)(ux - pt.x(j)), (double)(uy - pt.y(j)));
                dst[r] = w;
            }
        }
        BEAM_ACC(28);
        // boundary tie: the CPython set order decides who is kept.  The model works on the points to visit (the
        // pins without the start pin, list order); the lanes of a net share its scratch and take turns.
        const bool my_tie = worker && tie;
        if (__ballot(my_tie) != 0ull)  // (of the lanes still searching)
        for (int turn = 0; turn < BEAM_LANES_PER_NET; turn++) {
            if (!(my_tie && t == turn)) continue;
            const int m = cnt - 1;
            const NetPts pv = NetPts::load(pins + s, cnt, st);
            const unsigned vpt = (vis & ((1u << st) - 1u)) | ((vis >> (st + 1)) << st);  // visited without the start pin's bit
            if (A->mask == 0) cs_build_points(A, R, hs, m, pv);  // first tie of this net
            int nset; unsigned packed = 0;
            const int nleft = m - (int)__popc(vpt);
            const bool small = !((m >> 2) > (int)__popc(vpt)) && nleft <= 4;
            if (small) nset = cs_small_difference_order(A, hs, vpt, pv, &packed);
            else {  // the general model works on a copy of the points' table (it recycles its first argument)
                CSet *A2 = (CSet *)dist;
                nset = cs_difference_order(A2, R, m, vpt, pv, order);
            }
            // sorted(key=distance) is stable: ties keep the iteration order; exact integer keys as above
            unsigned skey[4];
            if (small) {
                #pragma unroll
                for (int i = 0; i < 4; i++) {
                    const int o = (int)((packed >> (8 * i)) & 0xFFu);
                    const int dx = ux - pv.x(o), dy = uy - pv.y(o);
                    skey[i] = i < nset ? (((unsigned)(dx * dx + dy * dy) << 8) | ((unsigned)i << 4) | (unsigned)o) : KINF;
                }
                #pragma unroll
                for (int r = 0; r < 4; r++) {  // `take` smallest (distance, position in the iteration order)
                    unsigned mn = KINF;
                    #pragma unroll
                    for (int i = 0; i < 4; i++) mn = min(mn, skey[i]);
                    #pragma unroll
                    for (int i = 0; i < 4; i++) skey[i] = skey[i] == mn ? KINF : skey[i];
                    if (r < take) {
                        const int o = (int)(mn & 15u);
                        BsEntry q = e; q.push(o + (o >= st ? 1 : 0));
                        q.prio = e.prio + norm2((double)(ux - pv.x(o)), (double)(uy - pv.y(o)));
                        dst[r] = q;
                    }
                }
            } else {
                for (int i = 0; i < nset; i++) dist[i] = norm2((double)(ux - pv.x(order[i])), (double)(uy - pv.y(order[i])));
                for (int i = 1; i < nset; i++) {
                    const unsigned char o = order[i]; const double dd = dist[i];
                    int j = i - 1;
                    while (j >= 0 && dist[j] > dd) { order[j + 1] = order[j]; dist[j + 1] = dist[j]; j--; }
                    order[j + 1] = o; dist[j + 1] = dd;
                }
                for (int i = 0; i < take; i++) { BsEntry q = e; q.push(order[i] + (order[i] >= st ? 1 : 0)); q.prio = e.prio + dist[i]; dst[i] = q; }
            }
        }
        wave_lds_order();
        BEAM_ACC(29);
        { BsEntry *tmp = queue; queue = next; next = tmp; }
        qn = pops * take;
        if (qn == 0) {  // cannot happen (an incomplete path always has an unvisited point); leave an empty route
            wave_lds_order();
            if (t == 0) { BsEntry z; z.prio = 0.0; z.meta = 0ull; z.p0 = 0ull; z.p1 = 0ull; *(BsEntry *)scratch = z; }
            break;
        }
    }
    wave_lds_order();
}
