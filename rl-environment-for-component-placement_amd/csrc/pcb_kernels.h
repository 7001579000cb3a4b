// pcb_kernels.h -- the __global__ kernel templates of the environment kinds: k_reset, k_gather, k_step
// Part of libpcbenv.so (CDNA4 / gfx950 only).
#pragma once
#include "pcb_walk.h"
#include "pcb_launch.h"

template <int KIND, int WW, int NW>
__global__ __launch_bounds__(64 * NW) void k_reset(DevParams p, const unsigned char *__restrict__ mask) {
    typedef Team<64 * NW> T;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int e = xcd_contiguous_env((int)blockIdx.x, 0, p.B), lane = threadIdx.x;
    if (mask && !mask[e]) return;
    T::load_state(smem, p, e, lane);  // cursor / episode survive; the old pins tell which feature rows to clear
    Lds l = carve(smem, p);
    const int row = out_row(p, p.slot, e);
    T::template reset_env<KIND, WW, true>(p, l, e, row, lane);
    if (lane == 0) {
        l.hdr->pre_action = 0u;  // the mask changed under any presampled action
        l.hdr->term_seq = 0u;    // and the environment leaves the terminal list of the next step launch (its helpers find a stale entry)
        p.buf.reward[row] = 0.0;
        p.buf.done[row] = 0;
        if (p.buf.info) { p.buf.info[2 * (size_t)row] = nan(""); p.buf.info[2 * (size_t)row + 1] = nan(""); }
    }
    T::store_state(smem, p, e, lane);
}

// pcbenv_gather: environment e of the destination continues the episode in progress of environment j = src_index[e] of the
// source (same handle or another one with the same definition).  One team per destination environment, like k_reset:
// the source's block of the CURRENT state set -> LDS, the header patched, the block written to the destination's OTHER
// set (the host swaps the sets afterwards, as after a step launch: a permutation inside one handle reads nothing this
// launch writes), and every bound tensor of the destination's selected slot written whole from LDS -- the emission of a
// trajectory slot, where nothing may be assumed about what the destination holds.  Rows with j == -1 or j out of
// range keep their episode: their block is copied as it is, and none of their tensors is touched.
// The header patch and the emission are pcb_walk.h's text, which k_gather_paths expands too; it says what the header must
// not take over from the source, and why.
template <int KIND, int WW, int NW>
__global__ __launch_bounds__(64 * NW) void k_gather(DevParams p, GatherArgs g) {
    typedef Team<64 * NW> T;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int e = xcd_contiguous_env((int)blockIdx.x, 0, p.B), lane = threadIdx.x;
    const int j = __builtin_amdgcn_readfirstlane(g.src_index[e]);
    const bool take = (unsigned)j < (unsigned)g.src_B;  // checked before it addresses anything
    if (!take && j != -1 && g.errors && lane == 0) atomicOr(g.errors, 1u);
    const unsigned char *own = p.state + (size_t)e * p.stateStride;
    T::load_state_from(smem, take ? g.src_state + (size_t)j * p.stateStride : own, p, lane);
    Lds l = carve(smem, p);
    if (take) {
        PCB_GATHER_PATCH_HEADER(own, lane)
        T::lds_sync();
        const int row = out_row(p, p.slot, e);
        PCB_GATHER_EMIT_SLOT(e, row, lane)
        if (lane == 0) {
            p.buf.reward[row] = g.reward[j];
            p.buf.done[row] = g.done[j];
            if (p.buf.info) {
                p.buf.info[2 * (size_t)row] = g.info ? g.info[2 * (size_t)j] : nan("");
                p.buf.info[2 * (size_t)row + 1] = g.info ? g.info[2 * (size_t)j + 1] : nan("");
            }
        }
    }
    T::store_state(smem, p, e, lane);
}

// The step kernel, one team of NW wavefronts per workgroup (Team<>::run_env has the story).  A launch with helpers
// (p.term_wgs > 0: one transition per launch, pin kinds) starts with term_wgs * term_hpe
// helpers -- workgroup k * term_hpe + part serves entry k of the terminal list, entries being numbered idx *
// TERM_SHARDS + shard so that the occupied ones (the low idx of every shard) come first; unused ones look at their
// shard's counter and leave -- followed by the B environments' own teams.  The helpers come FIRST so that they hold a
// slot from the first cycle of the launch (behind 4 096 environments' workgroups the last of them found none until the
// first environments had finished, 14 us into a 20 us launch), and there are only as many as the lists have lately been
// long: the first environment workgroup reports this launch's longest shard to host memory, pcbenv_step* sizes the next
// helper grids from it (an environment is only delegated if its entry's helpers were started).
// Four wavefronts per SIMD (16 one-wavefront workgroups per CU) is all a launch of up to ~4 workgroups per SIMD needs and
// what LDS allows anyway; holding the lean build to 72 VGPRs for 7 wavefronts (spills inside the routing reward and one
// at entry) measured 2-5 % slower at every batch size, so both builds may use up to 128.
// BUILD (pcb_layout.h STEP_BUILD_*, chosen by pcb_layout::select_step_build): what is a compile-time fact of the launch.  STEP_BUILD_INPLACE / _INPLACE_STREAM: the in-place layout, one
// transition, write-through / streaming stores (the lean build: no step loop, no whole-tensor feature emission);
// STEP_BUILD_SLOT: the trajectory layout, one transition per launch (what a PPO collect runs: whole-tensor emission, no
// loop -- 80 VGPRs and 140 spilled scalars against the rollout build's 125 and 800, c4 68 instead of 80 us per step);
// STEP_BUILD_ROLLOUT: the trajectory layout and num_steps transitions per launch (the persistent rollout).
// GEO: the grid shape as a compile-time fact of the launch.  STEP_GEO_RUNTIME: H, W, O come with the parameter block;
// STEP_GEO_64: the 64 x 64 grid of a pin kind (pcb_layout::fixed_geometry), for launches pcb_layout::fixed_geometry_applies
// admits -- the in-place builds on one wavefront without routes only (part 4 of pcb_layout::step_build_part).  The routed, slot and rollout
// builds, k_reset and k_gather keep the run-time geometry: none of them is on the path of a step of the lock-step loop.
template <int KIND, int WW, int NW, bool ROUTES, int BUILD, int GEO = STEP_GEO_RUNTIME>
__global__ __attribute__((amdgpu_waves_per_eu(4, 8))) __launch_bounds__(64 * NW) void k_step(DevParams p, int *__restrict__ actions, int fmt, int sampled,
                                               u64 seed, u64 first_env, u64 step_index, int num_steps_) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    constexpr bool TRAJ = BUILD == STEP_BUILD_SLOT || BUILD == STEP_BUILD_ROLLOUT;
#if PCB_GEO64_UNIT
    // (the segment: the block, a multiple of 8 bytes, then actions .. num_steps_ without padding between them)
    kernarg_warm<sizeof(DevParams) + sizeof(int *) + 2 * sizeof(int) + 3 * sizeof(u64) + sizeof(int)>();
#endif
    if (!TRAJ) p.stream_stores = BUILD == STEP_BUILD_INPLACE_STREAM;  // the launch's choice as a compile-time constant: only one store policy is compiled in
    if (GEO == STEP_GEO_64) {  // likewise the geometry, before anything reads it: what the host put there are these very values
        static_assert(GEO == STEP_GEO_RUNTIME || (pcb_layout::is_pin_kind(KIND) && WW == 1 && NW == 1 && !ROUTES && !TRAJ), "pcb_layout::fixed_geometry_applies");
        constexpr pcb_layout::FixedGeometry g = pcb_layout::fixed_geometry(KIND);
        p.H = g.H; p.W = g.W; p.O = g.O; p.WW = g.WW;
        p.offOcc = g.offOcc; p.offVm = g.offVm; p.offComps = g.offComps;
        // The bound cell tensors start at 16-byte boundaries (checked when they were bound): with the low bits masked
        // the compiler knows it too, and the byte paths of emit_plane_* / emit_pin_grid are not compiled in.
        p.buf.grid = (uint8_t *)((uintptr_t)p.buf.grid & ~(uintptr_t)15);
        p.buf.action_mask = (uint8_t *)((uintptr_t)p.buf.action_mask & ~(uintptr_t)15);
        p.buf.pin_grid = (uint8_t *)((uintptr_t)p.buf.pin_grid & ~(uintptr_t)15);
    }
    const int num_steps = BUILD == STEP_BUILD_ROLLOUT ? num_steps_ : 1;
    // above the generator's wavefronts (priority 0) when both share a SIMD: the step kernel is the latency-critical one
    __builtin_amdgcn_s_setprio(3);
    constexpr bool HELPERS = KIND == PCBENV_PIN || KIND == PCBENV_SPATIAL;
    const int nh = HELPERS ? p.term_wgs * p.term_hpe : 0;  // helper workgroups at the head of the grid
    int e = (int)blockIdx.x - nh, role = ROLE_ENV, part = 0;
    if (e >= 0) e = xcd_contiguous_env((int)blockIdx.x, nh, p.B);
    unsigned pos = 0u;
    if (HELPERS && e < 0) {  // a reward helper
        const unsigned hb = blockIdx.x, hpe = (unsigned)p.term_hpe, k = hb / hpe;  // hpe = REWARD_PARTS (+ 1: the feature helper)
        part = (int)(hb - k * hpe);
        const unsigned ring = p.seq & 3u, cps = (unsigned)p.term_cap / TERM_SHARDS, shard = k & (TERM_SHARDS - 1u), idx = k >> TERM_SHARD_BITS;
        const unsigned cnt = (unsigned)__builtin_amdgcn_readfirstlane((int)load_agent(p.term_cnt + (ring * TERM_SHARDS + shard) * TERM_CNT_STRIDE));
        if (idx >= cps || idx >= cnt) return;
        pos = k;
        // (wave-uniform values the compiler cannot see as such: kept in scalar registers, like blockIdx.x)
        e = __builtin_amdgcn_readfirstlane(p.term_list[ring * (unsigned)p.term_cap + pos]);
        if ((unsigned)e >= (unsigned)p.B) return;  // (never in a list this library wrote; an index is checked before it addresses memory all the same)
        role = part < REWARD_PARTS ? ROLE_REWARD : ROLE_FEATURES;
    } else if (p.term_cap > 0 && e == 0 && threadIdx.x < TERM_SHARDS) {
        // List bookkeeping, by the first environment workgroup: the ring after next starts empty, and the host learns how
        // long the lists are (any later launch may read it, whenever: it only sizes helper grids).  Loads first, stores
        // last: on gfx9 a wavefront's loads and stores retire through one in-order counter, so a load issued behind a
        // store waits for that store's acknowledgement -- microseconds while the chip is saturated with stores, and this
        // wavefront has a whole transition to do afterwards (0.3 us per launch on the lock-step loop).
        unsigned *hist = p.term_cnt + TERM_HIST_OFFSET;  // behind the counters, TERM_HIST_WORDS words: four launches' figures, then the one the host was last told
        unsigned longest = load_agent(p.term_cnt + (((p.seq & 3u) * TERM_SHARDS + threadIdx.x) * TERM_CNT_STRIDE));
        const unsigned h1 = hist[(p.seq + 1u) & 3u], h2 = hist[(p.seq + 2u) & 3u], h3 = hist[(p.seq + 3u) & 3u], told = hist[4];
        for (int o = TERM_SHARDS / 2; o > 0; o >>= 1) longest = max(longest, (unsigned)__shfl_xor((int)longest, o, TERM_SHARDS));
        // ... the SHORTEST of the last four launches' longest shards: with episodes in lock-step the list is full once per
        // episode and empty otherwise -- sized on that one launch, the launches that follow would each start ~2 000 idle
        // helper workgroups (+ 4 % on the lock-step loop) -- while staggered phases give steady lengths, which the minimum
        // tracks as well.  (Kept per launch on the device: the host reads whenever it enqueues, many times per launch or
        // once in many.)
        const unsigned least = min(min(longest, h1), min(h2, h3));
        store_agent(p.term_cnt + ((((p.seq + 2u) & 3u) * TERM_SHARDS + threadIdx.x) * TERM_CNT_STRIDE), 0u);
        if (threadIdx.x == 0) {
            hist[p.seq & 3u] = longest;
            // (a store to host memory: only when the figure has grown, or shrunk by more than an eighth + 2)
            if (least > told || least + (told >> 3) + 2u < told) {
                hist[4] = least;
                __hip_atomic_store(p.term_seen, least, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
            }
        }
    }
    Team<64 * NW>::template run_env<KIND, WW, ROUTES, TRAJ>(p, smem, e, threadIdx.x, actions, fmt, sampled, seed, first_env, step_index,
                                                           num_steps, role, part, pos);
}
