// pcb_group.h -- the lane-group tree step, stated once: what a search kernel with "a group of G lanes per root" consists
// of besides its own loads and stores.  Part of libpcbenv.so (CDNA4 / gfx950 only); k_tree_advance (pcb_tree.hip),
// k_puct_advance (pcb_puct.hip) and k_puct_leaves (pcb_puct_leaves.hip) are built from it, and k_puct_move
// (pcb_puct_move.hip, one wavefront per root) takes the fence and the argmax.
//
// The mapping.  The step of ONE root is plain C++ (pcb_tree.h, pcb_puct.h, pcb_puct_leaves.h: the text the CPU model
// programs replay); a kernel composes the same pieces with a group of G lanes per root, G = group_lanes(C) the power of
// two >= max(C, 4), lane c of the group at child c of the current node, so a wavefront carries 64 / G roots and a
// 256-thread workgroup 256 / G.  Groups share nothing: no LDS, no barrier, and a group whose root does not exist exits
// whole.  A launch runs the phases its request names in the order INIT, ABSORB, SELECT and ORs the error bits of a root
// into the caller's word.  A later phase reads what an earlier one stored through other lanes of the same wavefront; a
// wavefront-scope fence between the phases keeps the compiler from moving those loads up (the memory operations of one
// wavefront reach the cache in order).
//
// The form.  A kernel stays a `template <int G> __global__` of its own unit, under its own name.  What is a function here
// is one because the kernels' instructions are the same with it; the phase driver and the argmax are text macros,
// expanded where the copies stood, because the same text as a function template reaches the optimiser in another shape
// and moves bytes in every kernel (profiles/tree_group_refactor.txt; pcb_walk.h is the precedent).
#pragma once
#include <hip/hip_runtime.h>

#include "pcb_tree.h"

namespace pcb_group {

constexpr int BLOCK = 256;  // threads of a workgroup: BLOCK / G roots

// the lanes per root for max_children = C (host side; tests/tree_cases.py:group_lanes mirrors it)
inline int group_lanes(int C) { int g = 4; while (g < C) g <<= 1; return g; }

__device__ inline void fence() { __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront"); }

// the ballot of this lane's group, bit c = lane c of the group
template <int G> __device__ inline unsigned long long group_ballot(bool v, int base) {
    const unsigned long long b = __ballot(v);
    if constexpr (G == 64) return b;
    else return (b >> base) & ((1ull << G) - 1ull);
}

}  // namespace pcb_group

// ---- the head of a kernel<G>(const Args a): the root p of this lane's group, its lane in it, the group's first lane ------
#define PCB_GROUP_ENTER(G, a) \
    static_assert(G >= 4 && G <= 64 && (G & (G - 1)) == 0, "a group is a power-of-two part of a wavefront"); \
    const unsigned p = blockIdx.x * (pcb_group::BLOCK / G) + threadIdx.x / G; \
    if (p >= (unsigned)a.P) return; \
    const int lane = threadIdx.x % G, base = (threadIdx.x & 63) - lane

// ---- the rest of it: the phases a.phases names, in order; ABSORB and SELECT are expressions that give their error bits ----
#define PCB_GROUP_PHASES(a, INIT, ABSORB, SELECT) \
    unsigned err = 0u; \
    if (a.phases & pcb_tree::PHASE_INIT) { \
        INIT; \
        pcb_group::fence(); \
    } \
    if (a.phases & pcb_tree::PHASE_ABSORB) { \
        err |= ABSORB; \
        pcb_group::fence(); \
    } \
    if (a.phases & pcb_tree::PHASE_SELECT) err |= SELECT; \
    if (err != 0u && lane == 0 && a.errors) atomicOr(a.errors, err)

// ---- the argmax of (s, c) over the G lanes of a group (every lane ends with the same pair): a shuffle butterfly ----------
// Declares c, the child this lane stands for; BETTER(sb, cb, sa, ca) is the order (pcb_tree::beats, pcb_move::more_visits).
#define PCB_GROUP_ARGMAX(G, mine, lane, s, c, BETTER) \
    int c = (mine) ? (lane) : pcb_tree::MAX_CHILDREN + (lane);  /* a lane without a child loses against any child, whatever its score */ \
    _Pragma("unroll") \
    for (int o = (G) / 2; o > 0; o >>= 1) { \
        const auto so = __shfl_xor(s, o); \
        const int co = __shfl_xor(c, o); \
        const bool other = co < pcb_tree::MAX_CHILDREN && (c >= pcb_tree::MAX_CHILDREN || BETTER(so, co, s, c)); \
        s = other ? so : s; \
        c = other ? co : c; \
    }

// ---- host: one launch of K<G>, G from a.C, BLOCK / G roots per workgroup ---------------------------------------------------
#define PCB_GROUP_LAUNCH(K, a, stream) \
    do { \
        const int G = pcb_group::group_lanes(a.C); \
        const dim3 grid((unsigned)(((long long)a.P + pcb_group::BLOCK / G - 1) / (pcb_group::BLOCK / G))), block(pcb_group::BLOCK); \
        switch (G) { \
        case 4: hipLaunchKernelGGL(K<4>, grid, block, 0, stream, a); break; \
        case 8: hipLaunchKernelGGL(K<8>, grid, block, 0, stream, a); break; \
        case 16: hipLaunchKernelGGL(K<16>, grid, block, 0, stream, a); break; \
        case 32: hipLaunchKernelGGL(K<32>, grid, block, 0, stream, a); break; \
        default: hipLaunchKernelGGL(K<64>, grid, block, 0, stream, a); break; \
        } \
    } while (0)
