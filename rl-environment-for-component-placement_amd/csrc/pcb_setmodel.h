// pcb_setmodel.h -- the model of CPython's set iteration order (SURVEY.md trap T2) as pure scalar code: tuple hashes,
// Objects/setobject.c's open-addressing table, `set(points) - visited`, and the register fast path for small results.
// Plain C++17 behind PCB_HD (it includes only pcb_records.h): beam_route_lanes (pcb_routing.h) runs it on boundary ties,
// and tools/kernel_models_check.cpp checks the same text on the CPU against recorded and live CPython orders.
#pragma once
#include "pcb_records.h"

#define CS_EMPTY 0xFF
#define CS_DUMMY 0xFE
struct CSet { int mask, fill, used; unsigned char t[32]; int pad; };  // 48 bytes
static_assert(sizeof(CSet) == 48, "beam LDS records");
// points to visit of one net: the net's pins without the start pin `st`
struct NetPts {  // coordinates packed one byte each into registers (<= 15 points): no LDS round trip per access
    u64 xs0, xs1, ys0, ys1;
    PCB_HD int x(int i) const { return (int)(((i < 8 ? xs0 : xs1) >> ((i & 7) * 8)) & 0xFFull); }
    PCB_HD int y(int i) const { return (int)(((i < 8 ? ys0 : ys1) >> ((i & 7) * 8)) & 0xFFull); }
    PCB_HD static NetPts load(const PinRec *p, int cnt, int st) {
        NetPts n{0ull, 0ull, 0ull, 0ull};
        int m = 0;
        for (int i = 0; i < cnt; i++) {
            if (i == st) continue;
            const u64 x = (u64)(unsigned char)p[i].abs_x << ((m & 7) * 8), y = (u64)(unsigned char)p[i].abs_y << ((m & 7) * 8);
            if (m < 8) { n.xs0 |= x; n.ys0 |= y; } else { n.xs1 |= x; n.ys1 |= y; }
            m++;
        }
        return n;
    }
};

PCB_HD inline u64 tuple_hash2(int x, int y) {  // Objects/tupleobject.c (xxHash-style), hash(int) == int
    const u64 P1 = 11400714785074694791ull, P2 = 14029467366897019727ull, P5 = 2870177450012600261ull;
    u64 acc = P5;
    acc += (u64)(long long)x * P2; acc = (acc << 31) | (acc >> 33); acc *= P1;
    acc += (u64)(long long)y * P2; acc = (acc << 31) | (acc >> 33); acc *= P1;
    acc += 2ull ^ (P5 ^ 3527539ull);
    return acc == ~0ull ? 1546275796ull : acc;
}
PCB_HD inline void cs_init(CSet *s, int size) {
    s->mask = size - 1; s->fill = 0; s->used = 0;
    for (int i = 0; i < 32; i++) s->t[i] = CS_EMPTY;
}
// first unused slot on the probe sequence of `hash` (set_insert_clean / the miss path of set_add_entry)
PCB_HD inline int cs_probe_unused(const CSet *s, u64 hash, int *freeslot) {
    const unsigned mask = (unsigned)s->mask;
    u64 perturb = hash;
    unsigned i = (unsigned)hash & mask;
    for (;;) {
        const unsigned probes = (i + 9u <= mask) ? 9u : 0u;
        for (unsigned k = 0; k <= probes; k++) {
            const unsigned char c = s->t[i + k];
            if (c == CS_EMPTY) return (int)(i + k);
            if (c == CS_DUMMY && freeslot) *freeslot = (int)(i + k);
        }
        perturb >>= 5;
        i = (unsigned)(((u64)i * 5u + 1u + perturb) & mask);
    }
}
// set_table_resize: re-insert the active keys in old slot order (the old table is copied to `tmp` first)
PCB_HD inline void cs_resize(CSet *s, CSet *tmp, int minused, const NetPts &pt) {
    int newsize = 8;
    while (newsize <= minused) newsize <<= 1;
    *tmp = *s;
    cs_init(s, newsize);
    for (int i = 0; i <= tmp->mask; i++)
        if (tmp->t[i] < CS_DUMMY) s->t[cs_probe_unused(s, tuple_hash2(pt.x(tmp->t[i]), pt.y(tmp->t[i])), 0)] = tmp->t[i];
    s->fill = s->used = tmp->used;
}
PCB_HD inline void cs_add(CSet *s, CSet *tmp, int key, const NetPts &pt) {
    int freeslot = -1;
    const int slot = cs_probe_unused(s, tuple_hash2(pt.x(key), pt.y(key)), &freeslot);
    if (freeslot >= 0) { s->t[freeslot] = (unsigned char)key; s->used++; return; }
    s->t[slot] = (unsigned char)key; s->fill++; s->used++;
    if (s->fill * 5 >= s->mask * 3) cs_resize(s, tmp, s->used * 4, pt);
}
PCB_HD inline void cs_discard(CSet *s, int key, const NetPts &pt) {
    const unsigned mask = (unsigned)s->mask;
    const u64 hash = tuple_hash2(pt.x(key), pt.y(key));
    u64 perturb = hash;
    unsigned i = (unsigned)hash & mask;
    for (;;) {
        const unsigned probes = (i + 9u <= mask) ? 9u : 0u;
        for (unsigned k = 0; k <= probes; k++) {
            const unsigned char c = s->t[i + k];
            if (c == CS_EMPTY) return;
            if (c == (unsigned char)key) { s->t[i + k] = CS_DUMMY; s->used--; return; }
        }
        perturb >>= 5;
        i = (unsigned)(((u64)i * 5u + 1u + perturb) & mask);
    }
}
// Iteration order of `set(points) - visited` (set_difference: copy-and-discard when len(A) >> 2 > len(visited),
// else a fresh set filled in A's slot order).  A and R are LDS tables; `order` receives point indices.
PCB_HD inline int cs_difference_order(CSet *A, CSet *R, int m, unsigned visited, const NetPts &pt, unsigned char *order) {
    // points_to_visit = set(points): inserted in list order.  R doubles as the resize temporary while A is built.
    cs_init(A, 8);
    for (int i = 0; i < m; i++) cs_add(A, R, i, pt);
    if ((m >> 2) > __builtin_popcount(visited)) {
        cs_init(R, 8);
        if (m * 5 >= R->mask * 3) { int ns = 8; while (ns <= 2 * m) ns <<= 1; cs_init(R, ns); }
        if (R->mask == A->mask) { *R = *A; }  // set_merge: same size, no dummies -> the table is copied as is
        else {
            for (int i = 0; i <= A->mask; i++)
                if (A->t[i] < CS_DUMMY) R->t[cs_probe_unused(R, tuple_hash2(pt.x(A->t[i]), pt.y(A->t[i])), 0)] = A->t[i];
            R->fill = R->used = A->used;
        }
        for (int k = 0; k < m; k++) if (visited >> k & 1u) cs_discard(R, k, pt);
        // "if more than 1/4th are dummies, resize them away" cannot trigger for m <= 15 (<= 2 dummies, mask >= 15)
    } else {
        // fresh result set filled in A's slot order: collect the survivors first, after which A is free to
        // serve as the temporary of R's set_table_resize (5th insert: 8 -> 32 slots)
        int ns = 0;
        for (int i = 0; i <= A->mask; i++)
            if (A->t[i] < CS_DUMMY && !(visited >> A->t[i] & 1u)) order[ns++] = A->t[i];
        cs_init(R, 8);
        for (int i = 0; i < ns; i++) cs_add(R, A, order[i], pt);
    }
    int n = 0;
    for (int i = 0; i <= R->mask; i++) if (R->t[i] < CS_DUMMY) order[n++] = R->t[i];
    return n;
}

// ---- boundary ties, fast path ------------------------------------------------------------------------------
// `A = set(points)` and the tuple hashes depend on the net only: built once per net (first tie) and kept in LDS.
// (Low 32 bits of each hash: they carry the first five perturb steps of an 8-slot walk; a longer walk -- occupied slots
// can be revisited -- recomputes the full hash.)
PCB_HD inline void cs_build_points(CSet *A, CSet *tmp, unsigned *hs, int m, const NetPts &pt) {
    cs_init(A, 8);
    for (int i = 0; i < m; i++) { hs[i] = (unsigned)tuple_hash2(pt.x(i), pt.y(i)); cs_add(A, tmp, i, pt); }
}
// Iteration order of `A - visited` when the result has at most 4 elements and comes from the "fresh set filled in
// A's slot order" branch of set_difference: the result table keeps its 8 slots (no resize before the 5th insert), so
// it lives in one 64-bit register, one byte per slot (mask 7: LINEAR_PROBES never applies, only the perturb walk).
// Returns the number of elements, their point indices in iteration order packed one per byte.
PCB_HD inline int cs_small_difference_order(const CSet *A, const unsigned *hs, unsigned visited, const NetPts &pt, unsigned *packed) {
    const unsigned *tw = (const unsigned *)A->t;  // 4-byte aligned (offset 12 of a 16-byte aligned record)
    const int nw = (A->mask + 1) >> 2;            // 2 or 8 words
    unsigned w[8];
    PCB_UNROLL
    for (int i = 0; i < 8; i++) w[i] = i < nw ? tw[i < nw ? i : 0] : 0xFFFFFFFFu;
    u64 rt = ~0ull;
    int ns = 0;
    PCB_UNROLL
    for (int i = 0; i < 8; i++) {
        if (w[i] == 0xFFFFFFFFu) continue;  // four empty slots
        PCB_UNROLL
        for (int b = 0; b < 4; b++) {
            const unsigned c = (w[i] >> (8 * b)) & 0xFFu;
            if (c >= CS_DUMMY || (visited >> c & 1u)) continue;
            u64 perturb = hs[c];
            unsigned slot = (unsigned)perturb & 7u;
            for (int step = 1; ((rt >> (8 * slot)) & 0xFFull) != 0xFFull; step++) {
                if (step == 6) perturb = tuple_hash2(pt.x(c), pt.y(c)) >> 25;  // the cached low word has run out: the full hash, five steps in
                perturb >>= 5;
                slot = (unsigned)(((u64)slot * 5u + 1u + perturb) & 7u);
            }
            rt = (rt & ~(0xFFull << (8 * slot))) | ((u64)c << (8 * slot));
            ns++;
        }
    }
    unsigned out = 0; int n = 0;
    PCB_UNROLL
    for (int sl = 0; sl < 8; sl++) {
        const unsigned c = (unsigned)(rt >> (8 * sl)) & 0xFFu;
        if (c != 0xFFu) { out |= c << (8 * n); n++; }
    }
    *packed = out;
    return ns;
}
