// pcb_layout.h -- the layout contract between the host side and the kernels of libpcbenv.so, stated once: every size,
// offset and predicate that pcb_config.hip / pcbenv_api.hip allocate by and the kernels index by.  Plain C++17 (it
// includes only pcbenv.h and <stdint.h>): the host units, the kernel units and tools/layout_check.cpp -- a CPU program
// that sweeps the geometry and asserts that no zone is smaller than what its user indexes -- compile the same text.
#pragma once
#include <stdint.h>

#include "pcbenv.h"

#if defined(__HIPCC__) || defined(__CUDACC__)
#define PCB_HD __host__ __device__
#define PCB_UNROLL _Pragma("unroll")  // (`#pragma unroll` is unknown to a host compiler)
#else
#define PCB_HD
#define PCB_UNROLL
#endif

#define WAVE 64
#define MAX_NT 256
#define HDR_BYTES 64  // sizeof(EnvHdr), pcb_records.h

// ---- terminal list (DevParams::term_*, Team<>::run_env): four rings of TERM_SHARDS shards ------------------------
#define TERM_CNT_STRIDE 32u  // unsigned words between the shard counters of the terminal list: one 128-byte line each
#define TERM_SHARD_BITS 4
#define TERM_SHARDS (1u << TERM_SHARD_BITS)
// The allocations are sized for the largest capacity an option can ask for.
#define PCBENV_TERM_CAP_MAX 4096  // entries per ring of the terminal list = the most terminal workgroups of a launch
#define TERM_LIST_BYTES ((size_t)4 * PCBENV_TERM_CAP_MAX * sizeof(int))  // DevParams::term_list
// DevParams::term_cnt: a line per shard counter, then k_step's history of list lengths -- hist[0..3] = the longest shard
// of the last four launches, hist[4] = the figure the host was last told
#define TERM_HIST_OFFSET (4u * TERM_SHARDS * TERM_CNT_STRIDE)  // in unsigned words: behind the counters of the four rings
#define TERM_HIST_WORDS 5
#define TERM_CNT_BYTES ((size_t)TERM_HIST_OFFSET * sizeof(unsigned) + 32)
#define TERM_ARRIVE_BYTES ((size_t)PCBENV_TERM_CAP_MAX * sizeof(uint64_t))  // DevParams::term_arrive
static_assert(TERM_HIST_WORDS * sizeof(unsigned) <= 32, "TERM_CNT_BYTES: the history words behind the counters");
static_assert(PCBENV_TERM_CAP_MAX % TERM_SHARDS == 0 && TERM_SHARDS <= WAVE, "a ring is TERM_SHARDS equal shards, one lane of k_step each");

// ---- terminal reward: LDS zones (pcb_geometry.h seg_view, pcb_routing.h beam_route_lanes) ------------------------------------------------
#define REWARD_PARTS 2  // reward helpers per listed environment (+ one feature helper with PCBENV_FLAG_AUTO_RESET)
// compaction buffer of candidate (i, j) pairs, per wavefront: a dense batch is two candidates per lane (128), a
// sweep step appends at most 4 * 64 to a partial batch (< 128), and what does not fill a batch is moved to the front
#define PAIR_ENTRIES_PER_WAVE 384
// [segments X1 Y1 X2 Y2 D | centroids | act nstart total nsum] then a zone used only by the pair count
// (A DX DY bbox pairs), which the beam search -- finished before the count starts -- overlays with its per-net scratch.
// (the per-net tables are sized by the configuration's max_num_nets N, not by PCBENV_MAX_NETS: at c3 / c4 that and a fold
// scratch sized by need bring a workgroup's LDS from 7.8 to 6.6 KB -- 24 instead of 20 one-wavefront workgroups per CU,
// the headroom the reward helpers start in)
#define SEG_INTS(P, N) ((P) + ((N) + 1) + 3 + 2 * (N))
#define SEG_FIXED_BYTES(P, N) ((5 * (P) + 2 * (N)) * 8 + SEG_INTS(P, N) * 4)
#define SEG_COUNT_BYTES(P, NW) (3 * (P) * 8 + (P) * 4 + PAIR_ENTRIES_PER_WAVE * 2 * (NW))
#define SEG_LDS_BYTES(P, N, NW, beam) (((SEG_FIXED_BYTES(P, N) + 7) & ~7) + ((beam) > SEG_COUNT_BYTES(P, NW) ? (beam) : SEG_COUNT_BYTES(P, NW)))
// per net of a beam search of width k (beam_route_lanes): two queues of k * k BsEntry (32 bytes), 16 distances, 16
// order bytes, two CSet (48 bytes), 16 tuple hashes
#define BEAM_LDS_PER_NET(k) (64 * (k) * (k) + 16 * 8 + 16 + 2 * 48 + 16 * 4)
#define BEAM_LDS_BYTES(nets, k) ((nets) * BEAM_LDS_PER_NET(k))

namespace pcb_layout {

PCB_HD constexpr int align16(long long v) { return (int)((v + 15) & ~15ll); }
PCB_HD constexpr int imax(int a, int b) { return a > b ? a : b; }
PCB_HD constexpr bool is_pin_kind(int k) { return k == PCBENV_PIN || k == PCBENV_SPATIAL; }
// threads per environment (64 / 256) -> wavefronts of a team: Team<64 * NW>
PCB_HD constexpr int wavefronts(int threads) { return threads / WAVE; }
// Whether the kernels of a handle have the beam / both routes of the terminal reward compiled in (ROUTES of k_step and
// k_playout) and its LDS holds the beam search's scratch.
PCB_HD constexpr bool routes_compiled_in(int kind, int reward_type) { return is_pin_kind(kind) && reward_type != PCBENV_REWARD_CENTROID; }

// Whether window_mask (pcb_team_io.h) folds its rows across the lanes of a one-wavefront team, one row per lane, and
// never touches hf -- `threads` is the team size, NT in the kernels -- or stages the folded rows in LDS at hf.
// -DPCBENV_FOLD_LDS (A/B builds) stages them always.
PCB_HD constexpr bool fold_across_lanes(int WW, int threads, int H) {
#ifdef PCBENV_FOLD_LDS
    return false;
#else
    return WW == 1 && threads == WAVE && H <= WAVE;
#endif
}
PCB_HD constexpr bool fold_in_lds(int WW, int threads, int H) { return !fold_across_lanes(WW, threads, H); }
PCB_HD constexpr int fold_words(int WW, int threads, int H) { return fold_in_lds(WW, threads, H) ? H * WW : 0; }
// 64-bit words of the pin kind's row-membership bit map at hf: one bit per row [component, pin_id] of the pin feature
// tensors (pinRows == C * mp for that kind), so emit_features_* and reset_env index it by any row without a test.
PCB_HD constexpr int member_words(int kind, int C, int mp) { return kind == PCBENV_PIN ? (C * mp + 63) / 64 : 0; }

// Pin tables of the spatial kind in the class-map zone (pcb_env_lds.h pin_tables): pid, 2 bytes per component cell, at
// 0; netmask, 4 bytes per component cell, at the next multiple of 4.
PCB_HD constexpr int pin_table_netmask_offset(int comp_cells) { return (comp_cells * 2 + 3) & ~3; }
PCB_HD constexpr int pin_table_bytes(int comp_cells) { return comp_cells * 6 + 4; }
// The class-map zone: a byte per grid cell for emit_pin_grid; at a reset the same zone holds the pin tables.
PCB_HD constexpr int class_map_bytes(int kind, int H, int W, int C, int mp) {
    return kind == PCBENV_SPATIAL ? imax(H * W, pin_table_bytes(C * mp)) : 0;
}

// Per-episode feature cache of the spatial kind (pcb_observe.h feat_cache_*), per environment: the compact
// all_components_feature, C x F int16, then component_grid at a 16-byte boundary; feat_cache_emit reads the latter in
// whole 16-byte chunks, so the stride pads it to whole chunks.
PCB_HD constexpr int feat_cache_grid_bytes(int C, int mp, int K) { return C * mp * K; }
PCB_HD constexpr int feat_cache_grid_offset(int C, int F) { return align16(2ll * C * F); }
PCB_HD constexpr int feat_cache_stride(int C, int F, int mp, int K) {
    return align16((long long)feat_cache_grid_offset(C, F) + (long long)feat_cache_grid_bytes(C, mp, K));
}

// What the layout follows from.  C, P, N are the configuration's maxima (0 for a kind without them), threads the team size.
struct Geometry { int kind, H, W, C, P, N, mh, mw, threads, reward_type, beam_width; };
// A state block in HBM -- header | occ | vm (both orientations) | comps | pins | rank, padded to 16 bytes -- which a
// team mirrors at the start of its LDS, and the LDS scratch zones behind the mirror.  All byte offsets; DevParams
// carries them under the same names.
struct Layout {
    int WW;
    int offOcc, offVm, offComps, offPins, offRank;
    long long stateStride;
    int ldsHf, ldsHfWords;  // fold scratch of window_mask, doubling as the pin kind's row-membership bit map
    int ldsCls, ldsSeg;     // the class map (pin_grid emission) and the route segments (terminal reward) are never live together
    int ldsBytes;
};
PCB_HD constexpr int beam_bytes(const Geometry &g) {
    return routes_compiled_in(g.kind, g.reward_type) ? BEAM_LDS_BYTES(g.N, g.beam_width) : 0;
}
PCB_HD constexpr int seg_bytes(const Geometry &g) {
    return is_pin_kind(g.kind) ? SEG_LDS_BYTES(g.P, g.N, wavefronts(g.threads), beam_bytes(g)) : 0;
}
PCB_HD constexpr Layout state_layout(const Geometry &g) {
    Layout l{};
    l.WW = (g.W + 63) / 64;
    const int mp = g.mh * g.mw;
    l.offOcc = HDR_BYTES;
    l.offVm = l.offOcc + g.H * l.WW * 8;
    l.offComps = l.offVm + 2 * g.H * l.WW * 8;
    l.offPins = l.offComps + 8 * g.C;
    l.offRank = l.offPins + 8 * g.P;  // rank of each pin inside its component (spatial env)
    l.stateStride = align16((long long)l.offRank + (g.kind == PCBENV_SPATIAL ? g.P : 0));
    l.ldsHf = (int)l.stateStride;
    l.ldsHfWords = imax(fold_words(l.WW, g.threads, g.H), member_words(g.kind, g.C, mp));
    l.ldsCls = align16(l.ldsHf + l.ldsHfWords * 8);
    l.ldsSeg = l.ldsCls;
    l.ldsBytes = align16(l.ldsCls + imax(class_map_bytes(g.kind, g.H, g.W, g.C, mp), seg_bytes(g)));
    return l;
}

// ---- the geometry-fixed build of k_step (pcb_kernels.h STEP_GEO_64) ------------------------------------------------
// The grid shape of a handle never changes, and every shipped 64 x 64 configuration (c3, c4) has this one: a build of
// the in-place step kernel that overwrites the geometry fields of its parameter block with these constants -- H, W, O
// and what is a pure function of them: WW and the offsets of occ, vm and comps inside a state block -- so that every
// division by W, every "is W a power of two", the LDS-staged fold, the flat-action decode's divisions and the byte paths
// of the plane emission fold away.
#define FIXED_GEO_SIDE 64
#define FIXED_GEO_ORIENTATIONS 4  // DevParams::O of the pin kinds
struct FixedGeometry { int H, W, O, WW, offOcc, offVm, offComps; };
PCB_HD constexpr FixedGeometry fixed_geometry(int kind) {
    const Layout l = state_layout(Geometry{kind, FIXED_GEO_SIDE, FIXED_GEO_SIDE, 0, 0, 0, 0, 0, WAVE, PCBENV_REWARD_CENTROID, 0});
    return FixedGeometry{FIXED_GEO_SIDE, FIXED_GEO_SIDE, FIXED_GEO_ORIENTATIONS, l.WW, l.offOcc, l.offVm, l.offComps};
}
// What a step launch is, as far as the choice of its build goes.  cells_aligned16: every bound cell tensor (grid,
// action_mask, pin_grid) starts at a 16-byte boundary -- checked once, when the buffers are bound -- so that the fixed
// build needs no byte path in emit_plane_* / emit_pin_grid; enabled: PCBENV_OPT_FIXED_GEOMETRY.
struct StepShape {
    int kind, H, W, O, WW, threads, num_slots, num_steps;
    bool routes, cells_aligned16, enabled;
};
// The one predicate that says when the fixed build applies (select_step_build below uses nothing else): a
// pin kind without routes on the 64 x 64 grid, one wavefront per environment, in-place layout, one transition per launch.
PCB_HD constexpr bool fixed_geometry_applies(const StepShape &s) {
    return s.enabled && is_pin_kind(s.kind) && !s.routes && s.H == FIXED_GEO_SIDE && s.W == FIXED_GEO_SIDE &&
           s.O == FIXED_GEO_ORIENTATIONS && s.WW == 1 && wavefronts(s.threads) == 1 && s.num_slots == 1 && s.num_steps == 1 &&
           s.cells_aligned16;
}
PCB_HD inline bool aligned16(const void *p) { return ((uintptr_t)p & 15) == 0; }  // (a null pointer -- tensor not bound -- is)

// ---- which instantiation of k_step / k_playout a launch runs, and which translation unit compiles it -----------------
// BUILD of k_step (pcb_kernels.h has what each compiles in): the in-place layout with write-through / streaming stores,
// one transition into a trajectory slot, the persistent rollout; GEO: the grid shape at run time / the 64 x 64 constants.
#define STEP_BUILD_INPLACE 0
#define STEP_BUILD_INPLACE_STREAM 1
#define STEP_BUILD_SLOT 2
#define STEP_BUILD_ROLLOUT 3
#define STEP_GEO_RUNTIME 0
#define STEP_GEO_64 1
#define BUILD_PART_NONE (-1)  // no unit compiles that combination: it does not exist
// The template arguments every family has -- words per bit row (1 / 2), wavefronts per team (1 / 4), routes -- are the low
// TEAM_BUILD_BITS bits of its numbering; those of k_step<KIND, ww, nw, routes, build, geo> and of k_playout<KIND, ww, nw,
// routes, paths> follow them; k_gather_paths<KIND, ww, nw, routes> (pcb_gather_paths.h) has no others.
struct TeamBuild { int ww, nw; bool routes; };
struct StepBuild { int ww, nw; bool routes; int build, geo; };
struct PlayoutBuild { int ww, nw; bool routes, paths; };
typedef TeamBuild GatherPathsBuild;
// The candidates of a family, numbered: pcb_dispatch.h walks them and a unit compiles those that are its part.
#define TEAM_BUILD_BITS 3
#define STEP_BUILDS (8 << TEAM_BUILD_BITS)
#define PLAYOUT_BUILDS (2 << TEAM_BUILD_BITS)
#define GATHER_PATHS_BUILDS (1 << TEAM_BUILD_BITS)
PCB_HD constexpr TeamBuild team_build_at(int i) { return TeamBuild{1 + (i & 1), (i >> 1 & 1) ? 4 : 1, (i >> 2 & 1) != 0}; }
PCB_HD constexpr int build_index(const TeamBuild &b) { return (b.ww - 1) | (b.nw == 4) << 1 | (int)b.routes << 2; }
PCB_HD constexpr StepBuild step_build_at(int i) {
    const TeamBuild t = team_build_at(i);
    return StepBuild{t.ww, t.nw, t.routes, i >> TEAM_BUILD_BITS & 3, i >> (TEAM_BUILD_BITS + 2) & 1};
}
PCB_HD constexpr PlayoutBuild playout_build_at(int i) {
    const TeamBuild t = team_build_at(i);
    return PlayoutBuild{t.ww, t.nw, t.routes, (i >> TEAM_BUILD_BITS & 1) != 0};
}
PCB_HD constexpr GatherPathsBuild gather_paths_build_at(int i) { return team_build_at(i); }
PCB_HD constexpr int build_index(const StepBuild &b) {
    return build_index(TeamBuild{b.ww, b.nw, b.routes}) | b.build << TEAM_BUILD_BITS | b.geo << (TEAM_BUILD_BITS + 2);
}
PCB_HD constexpr int build_index(const PlayoutBuild &b) { return build_index(TeamBuild{b.ww, b.nw, b.routes}) | (int)b.paths << TEAM_BUILD_BITS; }

// The build of a step launch; stream_stores is the launch's store policy (DevParams::stream_stores).  A launch is of the
// trajectory layout if it writes one of several slots or makes several transitions.
PCB_HD constexpr StepBuild select_step_build(const StepShape &s, bool stream_stores) {
    const bool traj = s.num_slots > 1 || s.num_steps > 1;
    return StepBuild{s.WW, wavefronts(s.threads), s.routes,
                     traj ? (s.num_steps == 1 ? STEP_BUILD_SLOT : STEP_BUILD_ROLLOUT) : stream_stores ? STEP_BUILD_INPLACE_STREAM : STEP_BUILD_INPLACE,
                     fixed_geometry_applies(s) ? STEP_GEO_64 : STEP_GEO_RUNTIME};
}
PCB_HD constexpr PlayoutBuild select_playout_build(int WW, int threads, bool routes, bool paths) {
    return PlayoutBuild{WW, wavefronts(threads), routes, paths};
}
// (threads: the DESTINATION's team size, as for k_gather)
PCB_HD constexpr GatherPathsBuild select_gather_paths_build(int WW, int threads, bool routes) {
    return GatherPathsBuild{WW, wavefronts(threads), routes};
}
// The unit of build.py's table that compiles a build.  k_step of a pin kind: 4 = the 64 x 64 grid compiled in, 2 / 3 =
// with routes on one / four wavefronts, 1 = without routes into a trajectory slot, 0 = everything else, next to k_reset,
// k_gather and the entry points (pcb_kind.inc says why the slot build is on its own); k_playout of a pin kind, PATHS or
// not, and k_gather_paths in units of its own: 0 = without routes, 1 / 2 = with routes on one / four wavefronts.  Square
// and rect have no routes and one unit.  STEP_PARTS / PLAYOUT_PARTS: one more than the highest part.
#define STEP_PARTS 5
#define PLAYOUT_PARTS 3
PCB_HD constexpr int step_build_part(int kind, const StepBuild &b) {
    if (b.geo == STEP_GEO_64)
        return is_pin_kind(kind) && !b.routes && b.ww == 1 && b.nw == 1 && b.build <= STEP_BUILD_INPLACE_STREAM ? 4 : BUILD_PART_NONE;
    if (b.routes) return is_pin_kind(kind) ? (b.nw == 1 ? 2 : 3) : BUILD_PART_NONE;
    return is_pin_kind(kind) && b.build == STEP_BUILD_SLOT ? 1 : 0;
}
PCB_HD constexpr int playout_build_part(int kind, const PlayoutBuild &b) {
    if (b.routes) return is_pin_kind(kind) ? (b.nw == 1 ? 1 : 2) : BUILD_PART_NONE;
    return 0;
}
PCB_HD constexpr int gather_paths_build_part(int kind, const GatherPathsBuild &b) {
    return playout_build_part(kind, PlayoutBuild{b.ww, b.nw, b.routes, true});
}
// k_playout's unit, numbered as one family's parts: the PATHS = true builds behind the PLAYOUT_PARTS of the others.
PCB_HD constexpr int playout_build_unit(int kind, const PlayoutBuild &b) {
    const int part = playout_build_part(kind, b);
    return part == BUILD_PART_NONE ? BUILD_PART_NONE : part + (b.paths ? PLAYOUT_PARTS : 0);
}
// Every launch of a handle that pcbenv_create admits has a unit, and c3 / c4 in place on one wavefront run the fixed build.
PCB_HD constexpr bool every_launch_has_a_unit() {
    for (int i = 0; i < 4 * 2 * 2 * 2 * 2 * 2 * 2 * 2 * 2; i++) {
        const int kind = i & 3, WW = 1 + (i >> 2 & 1), side = (i >> 3 & 1) ? FIXED_GEO_SIDE : 40, threads = (i >> 4 & 1) ? MAX_NT : WAVE;
        const bool routes = routes_compiled_in(kind, (i >> 5 & 1) ? PCBENV_REWARD_BOTH : PCBENV_REWARD_CENTROID);
        const StepShape s{kind, side, side * WW, is_pin_kind(kind) ? FIXED_GEO_ORIENTATIONS : 2, WW, threads, 1 + (i >> 6 & 1), 1 + 2 * (i >> 7 & 1), routes, (i >> 8 & 1) != 0, true};
        for (int policy = 0; policy < 2; policy++) {
            const StepBuild b = select_step_build(s, policy != 0);
            if (step_build_part(kind, b) == BUILD_PART_NONE || build_index(step_build_at(build_index(b))) != build_index(b)) return false;
        }
        for (int paths = 0; paths < 2; paths++)
            if (playout_build_part(kind, select_playout_build(WW, threads, routes, paths != 0)) == BUILD_PART_NONE) return false;
        const GatherPathsBuild gb = select_gather_paths_build(WW, threads, routes);
        if (gather_paths_build_part(kind, gb) == BUILD_PART_NONE || build_index(gather_paths_build_at(build_index(gb))) != build_index(gb)) return false;
    }
    return true;
}
static_assert(every_launch_has_a_unit(), "select_step_build / select_playout_build / select_gather_paths_build give a build no unit compiles");
static_assert(select_step_build(StepShape{PCBENV_PIN, 64, 64, 4, 1, WAVE, 1, 1, false, true, true}, false).geo == STEP_GEO_64 &&
              select_step_build(StepShape{PCBENV_SPATIAL, 64, 64, 4, 1, WAVE, 1, 1, false, true, true}, true).geo == STEP_GEO_64 &&
              step_build_part(PCBENV_SPATIAL, select_step_build(StepShape{PCBENV_SPATIAL, 64, 64, 4, 1, WAVE, 1, 1, false, true, true}, true)) == 4,
              "c3 / c4 on one wavefront in place run the geometry-fixed build");

}  // namespace pcb_layout
