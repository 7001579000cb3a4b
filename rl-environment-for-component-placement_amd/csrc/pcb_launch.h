// pcb_launch.h -- what the host side (pcbenv_api.hip) and the kernel translation units (pcb_kind.inc, pcb_playout.inc and
// pcb_gather_paths.inc, once per unit of build.py's table; pcb_sample.hip, pcb_policy*.hip) share: one launch entry per kernel family and
// environment kind, so that the host side compiles no device code and the kernel instantiations of the four kinds compile
// in parallel.  Which instantiation an entry launches is pcb_layout::select_step_build / select_playout_build.
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

#define PCB_DECLARE_KIND(name) int pcb_launch_step_##name(const StepLaunch &a); int pcb_launch_reset_##name(const ResetLaunch &a); \
    int pcb_launch_gather_##name(const GatherLaunch &a); int pcb_launch_playout_##name(const PlayoutLaunch &a); \
    int pcb_launch_gather_paths_##name(const GatherPathsLaunch &a);
PCB_DECLARE_KIND(square) PCB_DECLARE_KIND(rect) PCB_DECLARE_KIND(pin) PCB_DECLARE_KIND(spatial)
