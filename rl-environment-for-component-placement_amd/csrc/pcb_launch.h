// pcb_launch.h -- what the host side (pcbenv_api.hip) and the kernel translation units (pcb_kind.inc, pcb_playout.inc and
// pcb_gather_paths.inc, once per unit of build.py's table; pcb_sample.hip, pcb_policy*.hip) share: the launch structs and
// one launch entry per kernel family, so that the host side compiles no device code and the kernel instantiations of the
// four kinds compile in parallel.  The families compiled per kind and part are described at the end; which instantiation
// their entries launch is pcb_layout::select_step_build / select_playout_build / select_gather_paths_build.
#pragma once
#include <hip/hip_runtime.h>

#include "pcb_records.h"

struct StepLaunch {
    DevParams d;
    int *actions;
    int fmt, sampled;
    u64 seed, first_env, step_index;
    int num_steps;
    int threads;        // threads per environment of the plain kernels (64 / 256)
    bool routes;        // pcb_layout::routes_compiled_in
    bool cells_aligned16, fixed_geometry;  // of the binding / PCBENV_OPT_FIXED_GEOMETRY: pcb_layout::StepShape, step_shape() below
    hipStream_t stream;
};
// what pcb_layout::select_step_build is asked about a launch (besides d.stream_stores)
static inline pcb_layout::StepShape step_shape(const StepLaunch &a) {
    const DevParams &d = a.d;
    return pcb_layout::StepShape{d.kind, d.H, d.W, d.O, d.WW, a.threads, d.num_slots, a.num_steps, a.routes, a.cells_aligned16, a.fixed_geometry};
}
struct ResetLaunch { DevParams d; const unsigned char *mask; int threads; hipStream_t stream; };
// pcbenv_gather: d is the destination's parameter block (d.state = its current state set, d.state_out = the other one);
// the source's current state set and the rows of its selected slot (or, source == destination, the snapshot of them
// taken before the launch) travel in GatherArgs.
struct GatherArgs {
    const unsigned char *src_state;
    const int *src_index;
    unsigned *errors;
    const double *reward, *info;  // row j of the source = element j (info: 2 j, 2 j + 1); info may be null
    const unsigned char *done;
    int src_B;
};
struct GatherLaunch { DevParams d; GatherArgs g; int threads; hipStream_t stream; };
// pcbenv_gather_paths (pcb_gather_paths.inc): d and g as for pcbenv_gather; the paths travel in GatherPathArgs.
struct GatherPathArgs {
    const int *path_actions;  // [path_steps, B, 3] / [path_steps, B] of the destination's B, null if path_steps == 0
    const int *path_len;      // [B] or null: path_steps for every row
    int *length;              // [B], may be null
    int fmt, path_steps;
};
struct GatherPathsLaunch { DevParams d; GatherArgs g; GatherPathArgs q; int threads; bool routes; hipStream_t stream; };

// pcbenv_playout and pcbenv_playout_paths (pcb_playout.inc; paths says which): d is the root handle's parameter block with d.state = the current state set,
// buf.reward / buf.info repointed at the playout's rows and everything else a playout must not touch taken out (every
// other tensor null, flags 0, no terminal list); the rest travels in PlayoutArgs.
struct PlayoutArgs {
    const int *root_index;     // [n] or null: playout i plays root i / per_root
    const int *first_actions;  // [n, 3] / [n] or null: the action of transition 0
    double *reward;            // [n]
    unsigned char *done;       // [n], may be null
    int *length;               // [n], may be null
    double *info;              // [n, 2], may be null (pin kinds only)
    int *actions_out;          // [actions_steps, n, 3] / [actions_steps, n], null if actions_steps == 0
    unsigned *errors;          // may be null
    int n, per_root, fmt, max_steps, actions_steps;
    u64 seed, first_env, step_index0;
    // pcbenv_playout_paths only (k_playout<..., PATHS = true>; pcbenv_playout leaves them null / 0)
    const int *path_actions;   // [path_steps, n, 3] / [path_steps, n], null if path_steps == 0
    const int *path_len;       // [n] or null: path_steps for every playout
    u64 *leaf_mask;            // [n, 2, H, WW], may be null
    int path_steps;
};
struct PlayoutLaunch { DevParams d; PlayoutArgs g; int threads; bool routes, paths; hipStream_t stream; };

// pcbenv_sample_actions and pcbenv_queue_cursors (pcb_sample.hip): d.state = the current state set; out = two words, min and max
struct SampleLaunch { DevParams d; int *actions; int fmt; u64 seed, first_env, step_index; hipStream_t stream; };
int pcb_launch_sample(const SampleLaunch &a);
int pcb_launch_cursor_range(const DevParams &d, unsigned *out, hipStream_t stream);

// pcbenv_sample_logits (pcb_policy.hip): d is the handle's parameter block with d.state = the current state set
struct SampleLogitsArgs {
    const void *logits;  // [B, O*H*W], float32 or bf16
    int *actions;
    float *log_prob, *entropy;  // may be null
    unsigned *errors;           // may be null
    u64 seed, first_env, step_index;
    int fmt, greedy;
};
struct SampleLogitsLaunch { DevParams d; SampleLogitsArgs g; int dtype; hipStream_t stream; };
int pcb_launch_sample_logits(const SampleLogitsLaunch &a);

// pcbenv_evaluate_logits / pcbenv_evaluate_logits_backward (pcb_policy_eval.hip): the handle gives the geometry only;
// the rows are the caller's (a minibatch of stored steps), with their own bit rows [rows, 2, H, WW]
struct EvalGeom { int O, H, W, WW, rows; };
struct EvalLogitsArgs {
    const void *logits;  // [rows, O*H*W], float32 or bf16
    const u64 *mask_bits;
    const int *actions;
    float *log_prob, *entropy, *stats;  // may be null; stats: [rows, 4] = (M, log Z, entropy, row status)
    unsigned *errors;                   // may be null
    int fmt;
};
struct EvalLogitsLaunch { EvalGeom q; EvalLogitsArgs g; int dtype; hipStream_t stream; };
struct EvalLogitsBackwardArgs {
    const void *logits;
    const u64 *mask_bits;
    const int *actions;
    const float *stats, *grad_log_prob, *grad_entropy;  // the two gradients may be null (zero)
    void *grad_logits;  // [rows, O*H*W] in the logits' dtype, written whole
    int fmt;
};
struct EvalLogitsBackwardLaunch { EvalGeom q; EvalLogitsBackwardArgs g; int dtype; hipStream_t stream; };
int pcb_launch_evaluate_logits(const EvalLogitsLaunch &a);
int pcb_launch_evaluate_logits_backward(const EvalLogitsBackwardLaunch &a);

// pcbenv_sample_axis / pcbenv_evaluate_axis / pcbenv_evaluate_axis_backward (pcb_policy_axis.hip): one stage of a
// factorised policy.  The sampler reads the bit rows of d.state (the current state set), the evaluate calls the caller's.
struct AxisStage { int axis; unsigned given; };
struct SampleAxisArgs {
    const void *logits;  // [B, n], n = O, H or W by the axis; float32 or bf16
    int *actions;        // [B, 3]: the given columns are read, column `axis` is written
    float *log_prob, *entropy;  // may be null
    unsigned *errors;           // may be null
    u64 seed, first_env, step_index;
    int greedy;
};
struct SampleAxisLaunch { DevParams d; AxisStage s; SampleAxisArgs g; int dtype; hipStream_t stream; };
struct EvalAxisArgs {
    const void *logits;  // [rows, n]
    const u64 *mask_bits;
    const int *actions;  // [rows, 3]: the given columns and the stored value in column `axis`
    float *log_prob, *entropy;  // may be null
    unsigned *errors;           // may be null
};
struct EvalAxisLaunch { EvalGeom q; AxisStage s; EvalAxisArgs g; int dtype; hipStream_t stream; };
struct EvalAxisBackwardArgs {
    const void *logits;
    const u64 *mask_bits;
    const int *actions;
    const float *grad_log_prob, *grad_entropy;  // may be null (zero)
    void *grad_logits;  // [rows, n] in the logits' dtype, written whole
};
struct EvalAxisBackwardLaunch { EvalGeom q; AxisStage s; EvalAxisBackwardArgs g; int dtype; hipStream_t stream; };
int pcb_launch_sample_axis(const SampleAxisLaunch &a);
int pcb_launch_evaluate_axis(const EvalAxisLaunch &a);
int pcb_launch_evaluate_axis_backward(const EvalAxisBackwardLaunch &a);

// ---- the kernel families compiled per environment kind and part (build.py's unit table) -----------------------------------
// A family names its launch and build structs, numbers its candidate builds and forwards to pcb_layout.h, which alone
// says which build a launch runs (select) and which part compiles it (part).  launch<KIND, I> enqueues candidate I: the
// unit that sees the kernel template defines it (pcb_kind.inc, pcb_playout.inc, pcb_gather_paths.inc).
struct StepFamily {
    typedef StepLaunch Launch;
    typedef pcb_layout::StepBuild Build;
    static constexpr int builds = STEP_BUILDS, parts = STEP_PARTS;
    static constexpr Build build_at(int i) { return pcb_layout::step_build_at(i); }
    static constexpr int part(int kind, const Build &b) { return pcb_layout::step_build_part(kind, b); }
    static Build select(const Launch &a) { return pcb_layout::select_step_build(step_shape(a), a.d.stream_stores != 0); }
    template <int KIND, int I> static void launch(const Launch &a);
};
struct PlayoutFamily {  // (k_playout's PATHS = true builds have units of their own: playout_build_unit counts them as further parts)
    typedef PlayoutLaunch Launch;
    typedef pcb_layout::PlayoutBuild Build;
    static constexpr int builds = PLAYOUT_BUILDS, parts = 2 * PLAYOUT_PARTS;
    static constexpr Build build_at(int i) { return pcb_layout::playout_build_at(i); }
    static constexpr int part(int kind, const Build &b) { return pcb_layout::playout_build_unit(kind, b); }
    static Build select(const Launch &a) { return pcb_layout::select_playout_build(a.d.WW, a.threads, a.routes, a.paths); }
    template <int KIND, int I> static void launch(const Launch &a);
};
struct GatherPathsFamily {
    typedef GatherPathsLaunch Launch;
    typedef pcb_layout::GatherPathsBuild Build;
    static constexpr int builds = GATHER_PATHS_BUILDS, parts = PLAYOUT_PARTS;
    static constexpr Build build_at(int i) { return pcb_layout::gather_paths_build_at(i); }
    static constexpr int part(int kind, const Build &b) { return pcb_layout::gather_paths_build_part(kind, b); }
    static Build select(const Launch &a) { return pcb_layout::select_gather_paths_build(a.d.WW, a.threads, a.routes); }
    template <int KIND, int I> static void launch(const Launch &a);
};
// Whether build.py's table has a unit for part `part` of family F and kind `kind`: some candidate is that part's.
template <class F> constexpr bool part_exists(int kind, int part) {
    for (int i = 0; i < F::builds; i++)
        if (F::part(kind, F::build_at(i)) == part) return true;
    return false;
}
// Build b of family F, which F::part gives part PART, launched from the unit that compiles it: pcb_dispatch.h defines
// this, and each unit instantiates it for its own F, KIND and PART.  0, or -1 if b is not among the unit's candidates.
template <class F, int KIND, int PART> int launch_in_unit(const typename F::Launch &a, const typename F::Build &b);
// The entry of family F for kind KIND: selects the build and makes one call into the part that compiles it, among the
// parts build.py's table has.  -1: no unit compiles b (pcb_layout::every_launch_has_a_unit asserts there is no such launch).
template <class F, int KIND, int PART = 0> int launch_part(const typename F::Launch &a, const typename F::Build &b, int part) {
    if constexpr (PART < F::parts) {
        if constexpr (part_exists<F>(KIND, PART))
            if (part == PART) return launch_in_unit<F, KIND, PART>(a, b);
        return launch_part<F, KIND, PART + 1>(a, b, part);
    }
    return -1;
}
template <class F, int KIND> int launch_family(const typename F::Launch &a) {
    const typename F::Build b = F::select(a);
    return launch_part<F, KIND>(a, b, F::part(KIND, b));
}
// k_reset and k_gather have one build per team shape and live in part 0 of pcb_kind.inc.
template <int KIND> int pcb_launch_reset(const ResetLaunch &a);
template <int KIND> int pcb_launch_gather(const GatherLaunch &a);
