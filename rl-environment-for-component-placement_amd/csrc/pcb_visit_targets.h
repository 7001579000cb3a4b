// pcb_visit_targets.h -- the target side of pcbenv_evaluate_visits, stated once: which entries of a row's (visits,
// actions) pair are valid, their total T, the weight pi of an entry and the weight of a logit when several entries name
// it.  Plain C++17 that compiles alone, on the host and on the device: k_evaluate_visits and its backward
// (pcb_policy_visits.hip) compose the pieces below around their loads and wavefront reductions, and
// tools/visit_targets_check.cpp -- a CPU program under AddressSanitizer and UBSan -- composes them serially over the rows
// of tests/visits_contract.py.
//
// The rule (include/pcbenv_train.h): entry c is valid if visits[c] > 0, its action is in range and its bit is set; an
// entry with visits[c] == 0 is skipped silently; every other entry is skipped and raises bit 2.  T is the int64 sum of
// the valid visits; entries with the same action add up, as integers, and the weight of a logit is
// float32((double)(its visits) / (double)T).  map_place / slot_of say how the backward kernel finds the visits of a logit
// without searching the entries.
// Range and legality are the caller's: `legal_action(c)` gives the flat index of entry c's action when it is in range
// and legal, and -1 otherwise; it is asked only about entries with visits[c] > 0.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define PCB_VISITS_HD __host__ __device__
#else
#define PCB_VISITS_HD
#endif

namespace pcb_visits {

constexpr int MAX_TARGETS = 64;      // PCBENV_MAX_TREE_CHILDREN: one wavefront holds a row's entries, one each
constexpr unsigned ERR_TARGET = 4u;  // bit 2: an entry with negative visits, or visited with an action out of range or not legal

// What entry c contributes: its flat index (-1: nothing) and its visits (0 then); *bad: the entry raises bit 2.
struct Entry { int index, visits; };
template <class LegalAction>
PCB_VISITS_HD inline Entry entry_of(int visits, int c, LegalAction legal_action, bool *bad) {
    *bad = visits < 0;
    if (visits <= 0) return Entry{-1, 0};
    const int a = legal_action(c);
    *bad = a < 0;
    return a < 0 ? Entry{-1, 0} : Entry{a, visits};
}

// what the cross entropy sums per valid entry, before the division by T: visits (l - M) in float64
PCB_VISITS_HD inline double weighted_logit(int visits, float l, float M) { return (double)visits * ((double)l - (double)M); }

// Where the <= 64 targets of a row meet its up to 65 536 gradient elements: a target bit map laid out like the legal bit
// rows' segments -- word (o*H + x)*WW + y/64, bit y%64 of flat index a = (o*H + x)*W + y -- and, per word, how many target
// bits the words before it hold.  The distinct targets of a row then have slots 0, 1, .. in flat-index order: the slot of
// a set bit is the targets before its word plus the set bits below it in the word, and the visits of every entry that
// names the logit are added into that slot -- integers, so the order does not matter and nothing is rounded.
PCB_VISITS_HD inline void map_place(int a, int W, int WW, int *word, int *bit) {
    const int ox = a / W, y = a - ox * W;
    *word = ox * WW + (y >> 6); *bit = y & 63;
}
PCB_VISITS_HD inline int slot_of(int before, uint64_t word, int bit) { return before + __builtin_popcountll(word & ((1ull << bit) - 1ull)); }
// the weight of a logit with `visits` valid visits, T > 0: one float64 division rounded once to float32
PCB_VISITS_HD inline float pi_of(int64_t visits, int64_t T) { return (float)((double)visits / (double)T); }

// A whole row, serially: index[C] and kept[C] (the visits of the valid entries, 0 elsewhere) as the backward kernel lists
// them, *T and the error bits.  (The kernels do this with one entry per lane and a wavefront sum for T.)
template <class LegalAction>
inline unsigned reduce_row(const int32_t *visits, int C, LegalAction legal_action, int *index, int *kept, int64_t *T) {
    unsigned bits = 0u;
    *T = 0;
    for (int c = 0; c < C; c++) {
        bool bad;
        const Entry e = entry_of(visits[c], c, legal_action, &bad);
        if (bad) bits |= ERR_TARGET;
        index[c] = e.index; kept[c] = e.visits;
        *T += (int64_t)e.visits;
    }
    return bits;
}

// The map [S], the targets before each word [S] and the visits per slot [MAX_TARGETS] of a row whose entries reduce_row
// listed, serially.  (The backward kernel builds them with LDS atomics and a wavefront scan.)
inline void build_slots(const int *index, const int *kept, int C, int W, int WW, int S, uint64_t *map, unsigned char *before, int64_t *sums) {
    for (int j = 0; j < S; j++) map[j] = 0;
    for (int c = 0; c < MAX_TARGETS; c++) sums[c] = 0;
    int word, bit;
    for (int c = 0; c < C; c++)
        if (index[c] >= 0) { map_place(index[c], W, WW, &word, &bit); map[word] |= 1ull << bit; }
    int count = 0;
    for (int j = 0; j < S; j++) { before[j] = (unsigned char)count; count += __builtin_popcountll(map[j]); }
    for (int c = 0; c < C; c++)
        if (index[c] >= 0) { map_place(index[c], W, WW, &word, &bit); sums[slot_of(before[word], map[word], bit)] += (int64_t)kept[c]; }
}

}  // namespace pcb_visits
