/*
 * pcbenv.h -- C ABI of libpcbenv.so: batched PCB component-placement
 * environments on MI355X (gfx950).  Plain C, plain pointers and sizes, no torch
 * or C++ types.  The compute calls are asynchronous on the caller's HIP stream.
 *
 * Streams.  Every entry point with a `stream` parameter works on that stream and on no other (tests/stream_cases.py is
 * this paragraph as a table).  These only enqueue -- kernels, device-to-device copies and, with the on-device generator,
 * event waits -- and return without waiting for the stream, with no allocation, host copy or synchronisation:
 * pcbenv_reset, pcbenv_step, pcbenv_sample_actions, pcbenv_step_sampled, pcbenv_rollout_sampled, pcbenv_gather,
 * pcbenv_playout, pcbenv_sample_logits, pcbenv_evaluate_logits[_backward], pcbenv_sample_axis and
 * pcbenv_evaluate_axis[_backward].  These move data between the host and the device and return only when `stream` (and,
 * where the on-device generator is on, its own stream) has done everything enqueued before and by the call:
 * pcbenv_load_instances, pcbenv_get_instances, pcbenv_get_state, pcbenv_set_state, pcbenv_queue_cursors,
 * pcbenv_instgen_device_enable and pcbenv_instgen_device_status.  pcbenv_set_option(PCBENV_OPT_TERMINAL_TEAMS) and
 * pcbenv_bind_buffers[_slots] take no stream and synchronise the whole device, before and after what they change on it;
 * the other options, pcbenv_bind_compact_features and pcbenv_select_slot change host-side fields only, which the next
 * call reads.  pcbenv_playout_paths takes its stream as a field of its request and only enqueues on it, exactly as
 * pcbenv_playout does.  pcbenv_tree_advance likewise: it only enqueues one kernel on its request's stream.
 * pcbenv_gather_paths takes its stream as a field of its request too and only enqueues on it, exactly as pcbenv_gather
 * does.  A handle may
 * be used from different streams as long as the caller orders the calls (an event recorded behind one call and waited
 * for by the stream of the next) and never makes two calls on one handle at the same time.
 * Two handles share nothing on the device: they may run concurrently on two streams (pcbenv_gather between two handles
 * reads the source, whose last launch the caller orders before it).  pcbenv_last_error(env) is per handle;
 * pcbenv_last_error(NULL) is the message of the latest failure in the process.
 *
 * What each entry point replaces in the reference (PBozmarov/RL-Environment-for-
 * Component-Placement, paths relative to its root):
 *
 *   pcbenv_create          DummyPlacementEnv.__init__ + parameter validation
 *                            environment/dummy_env_square.py:37-72
 *                            environment/dummy_env_rectangular.py:152-251
 *                            environment/dummy_env_rectangular_pin.py:396-641
 *                            environment/dummy_env_rectangular_pin_spatial.py:396-607
 *                          and the factory utils/agent/utils.py:317-418 (init_env/create_env)
 *   pcbenv_instgen_*       generate_instances() itself (NumPy legacy RandomState + CPython random restated)
 *   pcbenv_load_instances  the tables generate_instances() draws at reset
 *                            ..._spatial.py:960-989 (and :931-1212, :1408-1443)
 *   pcbenv_reset           DummyPlacementEnv.reset   ..._spatial.py:1487-1549,
 *                            ..._pin.py:1544-1597, ..._rectangular.py:310-351, ..._square.py:74-113
 *   pcbenv_step            DummyPlacementEnv.step    ..._spatial.py:1551-1661,
 *                            ..._pin.py:1599-1710, ..._rectangular.py:353-432, ..._square.py:115-153
 *                          incl. validate_action, update_grid, place_component,
 *                          compute_action_mask, compute_if_done, find_reward
 *   action formats         utils/environment/env_wrappers.py:80-98, :184-199 (flat Discrete action)
 *   pcbenv_sample_actions, pcbenv_step_sampled
 *                          the uniform-random valid-action policy and its simulate() loop body
 *                            agent/random/random_policy_square.py:11-23 (and siblings)
 *   pcbenv_sample_logits   the masked Categorical of every reference model: the logits masked with
 *                          `logits += max(log(action_mask), float32.min)`
 *                            agent/models/square_model.py:137-139, rectangle_pin_spatial_model.py:268-270 (and siblings)
 *                          and RLlib's Categorical sample / deterministic_sample / logp / entropy
 *                            utils/agent/factorized_action_distributions.py:21-91
 *   pcbenv_evaluate_logits, pcbenv_evaluate_logits_backward
 *                          RLlib's Categorical logp / entropy of the same masked logits for stored actions, and their
 *                          gradient with respect to the logits (what a PPO update back-propagates)
 *                            utils/agent/factorized_action_distributions.py:21-91
 *   pcbenv_sample_axis, pcbenv_evaluate_axis, pcbenv_evaluate_axis_backward
 *                          one stage of the factorised distributions p(o) p(x|o) p(y|o,x) and p(x) p(y|x) p(o|x,y): the
 *                          stage's mask (reduce_max / gather of action_mask), its masked Categorical and the gradient
 *                            utils/agent/factorized_action_distributions.py:107-818
 *   pcbenv_gather          no counterpart: the closest is copy.deepcopy(env) of a reference env object, which a
 *                          caller uses to fork an episode (lookahead, beam search, population resampling)
 *   pcbenv_playout         copy.deepcopy(env) of a reference env object followed by the random policy's simulate() loop
 *                          on the copy, played per fork
 *                            agent/random/random_policy_square.py:25-58 (and siblings)
 *   pcbenv_playout_paths   copy.deepcopy(env), env.step(a) for every action of the path, then the random policy's
 *                          simulate() loop on the copy: the evaluation of a tree node named by its path from the root
 *                            agent/random/random_policy_square.py:25-58 (and siblings)
 *   pcbenv_tree_advance    no counterpart: the reference has no search.  The bookkeeping of a batched UCT around
 *                          pcbenv_playout_paths (selection, expansion, backup), one launch for all roots
 *   pcbenv_gather_paths    copy.deepcopy(env) followed by env.step(a) for every action of a path: a tree node named by
 *                          its path from a root, with its observations (what a network needs to score the node)
 *
 * Observations are written into caller-owned device buffers (pcbenv_buffers)
 * and updated in place by the next call; the library owns only the handle, the
 * compact per-environment state and the instance queue.  Invalid actions are
 * data (a terminal transition), never an error.
 */
#ifndef PCBENV_H
#define PCBENV_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PCBENV_ABI_VERSION 3

/* status codes (every function returning int) */
#define PCBENV_OK 0
#define PCBENV_EINVAL (-1)  /* bad parameter: the reference raises ValueError here */
#define PCBENV_ELIMIT (-2)  /* valid for the reference but beyond the HIP path's limits below */
#define PCBENV_EHIP (-3)    /* a HIP runtime call failed (no device, out of memory, launch error) */
#define PCBENV_ESTATE (-4)  /* call order: buffers not bound, no instance loaded, ... */

/* limits of the HIP path */
#define PCBENV_MAX_SIDE 128
#define PCBENV_MAX_COMPONENTS 64
#define PCBENV_MAX_PINS 256
#define PCBENV_MAX_NETS 32
#define PCBENV_MAX_PINS_PER_NET 16
#define PCBENV_MAX_PINS_PER_COMPONENT 64
#define PCBENV_MAX_BEAM_WIDTH 4

enum pcbenv_kind {
    PCBENV_SQUARE = 0,  /* environment/dummy_env_square.py */
    PCBENV_RECT = 1,    /* environment/dummy_env_rectangular.py */
    PCBENV_PIN = 2,     /* environment/dummy_env_rectangular_pin.py */
    PCBENV_SPATIAL = 3  /* environment/dummy_env_rectangular_pin_spatial.py */
};
enum pcbenv_reward_type { PCBENV_REWARD_BEAM = 0, PCBENV_REWARD_CENTROID = 1, PCBENV_REWARD_BOTH = 2 };

/* action encodings accepted by pcbenv_step / produced by pcbenv_sample_actions */
enum pcbenv_action_format {
    PCBENV_ACTION_TUPLE = 0, /* int32 [num_envs, 3] = (orientation, x, y); square reads (x, y) from columns 1, 2 */
    PCBENV_ACTION_FLAT = 1   /* int32 [num_envs]: a = o*H*W + x*W + y (square: x*W + y) */
};

/* flags */
#define PCBENV_FLAG_INCREMENTAL_OBS 1u /* grid / pin_grid: a step writes only the rows it changed (the caller must
                                          not modify those buffers between calls); action_mask is always whole */
#define PCBENV_FLAG_AUTO_RESET 2u      /* a terminal transition is followed, inside the same pcbenv_step, by the
                                          reset of that environment: reward / done / info describe the terminal
                                          transition, the observation tensors already show the next episode
                                          (vector-env convention).  Without it pcbenv_step never resets. */

/* Constructor parameters: the reference constructors' arguments, same names. */
typedef struct pcbenv_config {
    int32_t kind;
    int32_t height, width;
    int32_t min_component_w, max_component_w, min_component_h, max_component_h;
    int32_t max_num_components, min_num_components;
    int32_t net_distribution, pin_spread;
    int32_t min_num_nets, max_num_nets, max_num_pins_per_net, min_num_pins_per_net;
    int32_t reward_type;       /* enum pcbenv_reward_type */
    int32_t reward_beam_width;
    int32_t component_n;       /* square env only */
    double weight_wirelength, weight_num_intersections;
    /* batch */
    int32_t num_envs;          /* environments on this device (one handle per process / GPU) */
    int32_t queue_depth;       /* instances queued per environment (>= 1) */
    uint32_t flags;
    int32_t threads_per_env;   /* 0 = choose; 64 / 256 = threads (1 / 4 wavefronts) per environment */
} pcbenv_config;

/* Observation tensors (device pointers, C-contiguous, leading dim num_envs).
 * A null pointer means "do not produce this tensor".  Cell tensors are uint8
 * (values 0/1, identical to the reference's float64 0.0/1.0); the small feature
 * tensors are float64 with exactly the reference's values.
 *   O  = 1 (square), 2 (rect), 4 (pin, spatial)      C = max_num_components
 *   mp = max_component_h*max_component_w             N = max_num_nets
 *   F  = 5 (rect, pin) or 5+mp (spatial)
 *   R  = C*mp (pin) or C*mp+1 (spatial)              Wc = 1 (pin) or 2 (spatial)            */
typedef struct pcbenv_buffers {
    uint8_t *grid;                  /* [B, H, W]                                all kinds  */
    uint8_t *action_mask;           /* [B, O, H, W] (square: [B, H, W])         all kinds  */
    uint8_t *pin_grid;              /* [B, H, W, N+1]                           spatial    */
    uint8_t *component_grid;        /* [B, C, mh, mw, N+1]; rows >= #components are 0   spatial */
    double *all_components_feature; /* [B, C, F]                                rect/pin/spatial */
    double *placement_mask;         /* [B, C]                                   rect/pin/spatial */
    double *component_mask;         /* [B, C]                                   rect       */
    double *all_pins_num_feature;   /* [B, R, 4] (pin: viewed as [B, C, mp, 4]) pin/spatial */
    double *all_pins_cat_feature;   /* [B, R, Wc] (pin: [B, C, mp, 1])          pin/spatial */
    double *reward;                 /* [B]   required                                       */
    uint8_t *done;                  /* [B]   required                                       */
    double *info;                   /* [B, 2] = (wirelength, num_intersections); NaN where the reference's
                                       info dict is empty                       pin/spatial */
    /* marginals of action_mask for the factorised policies p(o) p(x|o) p(y|o,x), straight from the bit rows
     * (utils/agent/factorized_action_distributions.py:358 reduce_max over (H, W); :401 reduce_max over W) */
    uint8_t *mask_orientation;      /* [B, O]    = max over (x, y) of action_mask     optional, all kinds */
    uint8_t *mask_rows;             /* [B, O, H] = max over y of action_mask          optional, all kinds */
} pcbenv_buffers;

/* Compact feature tensors for the trajectory layout (optional, pcbenv_bind_compact_features): the same values as the
 * float64 feature tensors above in the narrowest integer type that holds them -- every element is a small integer
 * except all_components_feature[..., 4] = area / (H * W), which is carried as its numerator h * w (divide by H * W in
 * float64 to get the reference's value bit for bit).  A rollout that keeps every step's observation writes 8x fewer
 * feature bytes this way (c3: 23.8 KB -> 3.0 KB per env-step).  Layout [num_slots, B, ...] like the other tensors;
 * a null pointer means "not wanted".  */
typedef struct pcbenv_compact_features {
    int16_t *all_components_feature; /* [B, C, F]: h, w, x, y (-1 unplaced), h * w, (spatial) pin ids padded with -1    */
    uint8_t *placement_mask;         /* [B, C]  the reference's codes 0..3 (rect: 0 / 1)                                 */
    uint8_t *component_mask;         /* [B, C]  rect                                                                     */
    int8_t *all_pins_num_feature;    /* [B, R, 4]  rel_x, rel_y, abs_x, abs_y (-1 unplaced; coordinates < 128)            */
    int8_t *all_pins_cat_feature;    /* [B, R, Wc] net (, component); spatial: last row -1                                */
} pcbenv_compact_features;

/* Instance wire format (host memory), one record of pcbenv_instance_stride() bytes:
 *   int32 num_components, num_nets, num_pins, reserved                      (16 bytes)
 *   max_num_components x { uint8 h, w; uint8 pad[6] }                       (8 bytes each)
 *   max_total_pins     x { uint8 rel_x, rel_y, net, component; uint16 pin_id; uint16 pad }
 * Pins are in the order of the reference's `self.pins` list (net-major);
 * max_total_pins = min(max_num_pins_per_net*max_num_nets,
 *                      max_num_components*max_component_h*max_component_w). */
typedef struct pcbenv pcbenv;

int pcbenv_abi_version(void);

/* Validates like the reference constructors (PCBENV_EINVAL) and against the
 * limits above (PCBENV_ELIMIT), selects `device`, allocates state + queue.
 * On failure *out is NULL and pcbenv_last_error(NULL) holds the message. */
int pcbenv_create(const pcbenv_config *cfg, int device, pcbenv **out);
void pcbenv_destroy(pcbenv *env);
const char *pcbenv_last_error(const pcbenv *env);

/* Sizes a host needs to allocate tensors and instance tables. */
int64_t pcbenv_instance_stride(const pcbenv_config *cfg);
int32_t pcbenv_max_total_pins(const pcbenv_config *cfg);

int pcbenv_bind_buffers(pcbenv *env, const pcbenv_buffers *buffers);

/* Tuning options of a handle (none changes a result; defaults are the measured choices of DESIGN.md).  They replace
 * the environment variables earlier builds read: nothing in the library calls getenv. */
enum pcbenv_option {
    PCBENV_OPT_STREAM_THRESHOLD_BYTES = 1, /* cell-tensor bytes per launch above which observation stores bypass the
                                              caches (`nt`); default 256 MiB = the Infinity Cache; 0 = always */
    PCBENV_OPT_TERMINAL_TEAMS = 2,         /* capacity of the terminal list: environments whose next transition is certain to
                                              end their episode get helper wavefronts in that launch (two that share the routing
                                              reward, one that writes the feature half of the reset), so that a batch whose
                                              episodes end at different times steps as fast as one in lock-step; default
                                              num_envs / 8 for the pin kinds, 0 = off */
    PCBENV_OPT_GEN_GRID = 3,               /* workgroups of a refill launch of the on-device generator (default 2 048) */
    PCBENV_OPT_GEN_LANES = 4,              /* lanes per environment of the generator kernel: 0 = narrowest the
                                              configuration allows, 32 / 64 force a wider group; before enabling it */
    PCBENV_OPT_FIXED_GEOMETRY = 5          /* 1 (default): a step launch of a pin kind on the 64 x 64 grid -- one wavefront
                                              per environment, no routes, in-place layout, one transition, cell tensors
                                              bound at 16-byte boundaries -- runs the build of the step kernel with that
                                              grid compiled in; 0: always the build that reads the grid at run time */
};
int pcbenv_set_option(pcbenv *env, int32_t option, int64_t value);

/* Trajectory layout: every tensor of `buffers` is [num_slots, num_envs, ...] (C-contiguous) instead of
 * [num_envs, ...].  pcbenv_reset / pcbenv_step* write their outputs (observations, reward, done, info, marginals)
 * into the slot chosen with pcbenv_select_slot (0 after binding); step t of pcbenv_rollout_sampled writes slot
 * (selected + t) % num_slots.  This is how a rollout loop (RLlib's sampler, the simulate() loops under agent/random) keeps
 * the observation of every step -- obs[t] -- without copying tensors after each call.  With num_slots > 1 a step
 * cannot rely on what an earlier step left in its destination, so every bound tensor is written whole (the float64
 * feature tensors and component_grid included); PCBENV_FLAG_INCREMENTAL_OBS requires num_slots == 1.  A masked
 * pcbenv_reset writes only the masked environments' rows of the selected slot (the explicit loop "step, then
 * reset the finished ones" therefore keeps one slot per step).
 * pcbenv_bind_buffers(env, b) == pcbenv_bind_buffers_slots(env, b, 1). */
int pcbenv_bind_buffers_slots(pcbenv *env, const pcbenv_buffers *buffers, int32_t num_slots);
int pcbenv_select_slot(pcbenv *env, int32_t slot);

/* Binds (or, with NULL, unbinds) compact feature tensors next to the buffers of pcbenv_bind_buffers_slots; needs the
 * trajectory layout (num_slots > 1, where every step writes every bound tensor whole).  Float64 feature pointers left
 * NULL in pcbenv_buffers are then simply not produced. */
int pcbenv_bind_compact_features(pcbenv *env, const pcbenv_compact_features *features);

/* Copies n packed instance records (host memory) into queue slot `slot`
 * (0 <= slot < queue_depth) of environments env_ids[0..n) (env_ids == NULL:
 * environments 0..n-1).  Synchronous with respect to `stream`. */
int pcbenv_load_instances(pcbenv *env, const int32_t *env_ids, int32_t n, int32_t slot,
                          const void *host_tables, void *stream);

/* reset(): every environment whose mask byte is non-zero (mask_dev == NULL: all)
 * takes the next instance of its queue (round robin over the slots) and
 * rewrites its observations.  Never called implicitly by pcbenv_step. */
int pcbenv_reset(pcbenv *env, const uint8_t *mask_dev, void *stream);

/* step(): one transition of every environment with the given actions.
 * (A launch issued while `stream` is being captured into a hipGraph will be replayed with the very same arguments: it
 * then runs without the helper wavefronts of the terminal list and updates the state blocks in place -- same results.
 * The graph may be replayed at any later time, in any order with eager calls on the same handle (pcbenv_step*,
 * pcbenv_rollout_sampled, pcbenv_reset, pcbenv_gather, pcbenv_set_state, pcbenv_set_option): a replay steps the state
 * the latest call left.  To keep that true, from the first captured launch on EVERY step launch of the handle works
 * in place on the set the graph was captured on -- no swap of the double-buffered state blocks, no helpers -- and
 * pcbenv_gather copies its result back into that set.  This holds for the rest of the handle's life:
 * PCBENV_OPT_TERMINAL_TEAMS is still accepted but starts no helpers on such a handle, because the library cannot know
 * whether a graph is still alive and a replay after a re-armed swap would silently step a stale set.  Create a new
 * handle to get helper launches back.  What stays frozen in a captured launch are its arguments: the actions pointer,
 * the selected trajectory slot, the store policy.) */
int pcbenv_step(pcbenv *env, const int32_t *actions_dev, int32_t action_format, void *stream);

/* Uniform draw over the currently legal actions of every environment
 * (counter-based generator keyed by (seed, first_env_index + env, step_index));
 * environments without a legal action get action 0. */
int pcbenv_sample_actions(pcbenv *env, int32_t *actions_dev, int32_t action_format, uint64_t seed,
                          uint64_t first_env_index, uint64_t step_index, void *stream);

/* pcbenv_sample_actions + pcbenv_step in one launch: draws the action exactly as pcbenv_sample_actions would,
 * stores it in actions_out_dev (the trajectory record) and applies it.  (The launch also draws, for the same seed and
 * step_index + 1, the action of the next call and keeps it in the state block; it is used only if the next call asks
 * for exactly that (seed, step, environment) and the mask has not changed since -- the result is the same function
 * of (mask, seed, environment, step) either way.) */
int pcbenv_step_sampled(pcbenv *env, int32_t *actions_out_dev, int32_t action_format, uint64_t seed,
                        uint64_t first_env_index, uint64_t step_index, void *stream);

/* num_steps consecutive pcbenv_step_sampled transitions in ONE persistent kernel launch: the per-environment
 * state stays in LDS between the steps (no reload, no launch latency per step), step t draws with step_index0 + t
 * -- the same action pcbenv_step_sampled would draw -- records it in actions_out_dev[t] (int32
 * [num_steps, num_envs, 3], or [num_steps, num_envs] for the flat format) and writes its outputs into slot
 * (selected + t) % num_slots.  The counterpart of the reference's simulate() loop
 * (agent/random/random_policy_square.py:25-58).  Intended with PCBENV_FLAG_AUTO_RESET; every environment may consume
 * up to one queued instance per terminal transition, so queue_depth bounds the resets per environment between
 * refills.  (With PCBENV_FLAG_INCREMENTAL_OBS the steps are separate launches.) */
int pcbenv_rollout_sampled(pcbenv *env, int32_t *actions_out_dev, int32_t action_format, int32_t num_steps,
                           uint64_t seed, uint64_t first_env_index, uint64_t step_index0, void *stream);

/* Native host-side instance generator: stream `seed` (< 2^32) yields, record by record (wire format above), the
 * instances the reference's generate_instances() draws after `np.random.seed(seed); random.seed(seed)`
 * (dummy_env_rectangular_pin_spatial.py:931-1212, :1408-1443; rect/pin siblings).  Not for PCBENV_SQUARE.
 * pcbenv_instgen_next_batch advances n independent streams with `threads` host threads. */
typedef struct pcbenv_instgen pcbenv_instgen;
int pcbenv_instgen_create(const pcbenv_config *cfg, uint64_t seed, pcbenv_instgen **out);
void pcbenv_instgen_destroy(pcbenv_instgen *gen);
int pcbenv_instgen_next(pcbenv_instgen *gen, void *record_out);
int pcbenv_instgen_next_batch(pcbenv_instgen *const *streams, int32_t n, void *records_out, int32_t threads);

/* On-device instance generator: the same streams as pcbenv_instgen_* (stream seeds_host[i] < 2^32 for environment i:
 * what the reference draws after `np.random.seed(s); random.seed(s)`), generated by a kernel on a stream of the
 * library's own, one lane per environment, straight into the instance queue -- so that EVERY reset takes a fresh
 * instance, as the reference's reset() does (..._spatial.py:1487-1549), at the rate the step kernels consume them.
 * Enable once, before or after the first reset; from then on the library owns the queue (pcbenv_load_instances is
 * refused): every pcbenv_reset / pcbenv_step* / pcbenv_rollout_sampled first makes the caller's stream wait (an
 * event wait on the device, never a host synchronisation) for a fill whose records cover whatever that launch can
 * consume -- one record per environment for a reset or an auto-reset step, num_steps for a rollout, which must not
 * exceed queue_depth -- and starts the next fill early enough to overlap the following launches.  A queue of
 * 2-4x the records one launch can consume keeps the generator off the critical path (queue_depth <= 256).
 * pcbenv_instgen_device_status brings the queue fully up to date (queue_depth records ahead of every cursor),
 * synchronises, and reports 0 unless a reset ever found its record missing (bit 0; it never should) or a stream hit
 * a draw the reference itself fails on / this library does not support (bit 1).  Such a stream has stopped: the records
 * before the failing one are queued and valid, none follows, and once they are consumed its environment must not be
 * reset again (the other environments' streams carry on unaffected).  pcbenv_get_instances copies one queue slot
 * (num_envs packed records) to the host, e.g. to replay an episode on the CPU.  All three synchronise with `stream`:
 * pcbenv_instgen_device_enable returns with the whole queue filled, pcbenv_get_instances with the records on the host. */
int pcbenv_instgen_device_enable(pcbenv *env, const uint32_t *seeds_host, void *stream);
int pcbenv_instgen_device_status(pcbenv *env, uint32_t *errors_out, void *stream);
int pcbenv_get_instances(pcbenv *env, int32_t slot, void *host_dst, void *stream);

/* Smallest and largest number of resets any environment has performed so far (= queue cursors; the next reset of
 * an environment with cursor c reads slot c % queue_depth).  A slot whose episode index is below *min_out has been
 * consumed by every environment and may be refilled.  Synchronises with `stream`. */
int pcbenv_queue_cursors(pcbenv *env, uint32_t *min_out, uint32_t *max_out, void *stream);

/* Checkpoint / resume of the library-owned environment state: pcbenv_state_bytes() bytes of host memory holding all state
 * blocks and -- once pcbenv_instgen_device_enable has been called, when the size grows accordingly -- the on-device
 * generator's streams, counters and queued records, so that a resumed run draws the very instances the original would
 * have (restore into a handle of the same configuration with the generator enabled as well).  A host-fed queue is an
 * input and is reloaded by the caller.  Synchronous w.r.t. `stream`. */
int64_t pcbenv_state_bytes(const pcbenv *env);
int pcbenv_get_state(pcbenv *env, void *host_dst, void *stream);
int pcbenv_set_state(pcbenv *env, const void *host_src, void *stream);

/* Fork / reorder episodes on the device.  Environment i of dst continues the episode in progress of environment
 * src_index[i] of src (src == NULL or src == dst: the same handle; any permutation or repetition is allowed).
 * src_index: int32 [dst num_envs] on the device; -1 = keep this environment's episode.  Any other out-of-range value
 * also keeps the episode, and if errors_dev is not NULL it ORs 1 into *errors_dev.  The two handles must have equal
 * environment definitions: every pcbenv_config field from kind through weight_num_intersections.  The batch fields
 * (num_envs, queue_depth, flags, threads_per_env) may differ.  Both handles must be on one device with buffers bound.
 * Asynchronous on `stream`, one kernel launch (and, within one handle, a 25-byte-per-environment device-to-device
 * snapshot of reward / done / info before it); the caller orders src's last launch before it.  Not capturable into a
 * hipGraph (PCBENV_ESTATE).
 * What moves is the episode: the state block (occupancy and legal-mask bit rows, component and pin records, the
 * current component) and, in the destination's selected slot, every bound tensor (pcbenv_buffers, the compact feature
 * tensors, the mask marginals) -- written whole -- and reward / done / info, copied from the source's selected slot.
 * Afterwards every tensor row of i is bit-identical to what src_index[i] showed, and every later step of i matches
 * what src_index[i] would have done.
 * What stays the destination's own -- the one deliberate difference from copy.deepcopy -- is its instance stream: the
 * queue cursor, the episode count, the queue and the on-device generator's state.  The next reset of i takes i's own
 * next instance, as it would have without the gather. */
int pcbenv_gather(pcbenv *dst, const pcbenv *src, const int32_t *src_index_dev, uint32_t *errors_dev, void *stream);

/* Play forked episodes to their end on the device, without observations: the rollout-policy primitive of a search.  One
 * kernel launch on `stream`, one team per playout; the root's state block is read once and the episode then lives in
 * LDS until it ends -- no observation tensor, no second handle, no launch per step.
 * The identity.  Playout i starts from the episode in progress of environment r = root_index_dev[i] of env (state read
 * from the current state set, as pcbenv_sample_actions reads it) and applies transitions t = 0, 1, ... until the first
 * `done` or until max_steps transitions, whichever comes first.  Transition t draws what
 * pcbenv_step_sampled(seed, first_env_index, step_index0 + t) would draw for environment i of a handle of num_playouts
 * environments without PCBENV_FLAG_AUTO_RESET after pcbenv_gather had put root r's episode there -- the uniform legal
 * draw keyed by (seed, first_env_index + i, step_index0 + t) -- and the transition is that handle's transition, bit for
 * bit.  That also covers a root whose episode is already over: one transition, as that handle would do it.
 * root_index_dev: int32 [num_playouts] on the device, or NULL: num_playouts must then be a multiple of num_envs and
 * playout i plays root i / (num_playouts / num_envs).
 * first_actions_dev: NULL, or int32 [num_playouts, 3] / [num_playouts] per action_format: transition 0 applies that
 * action instead of a draw; an illegal or out-of-range action is data -- a terminal transition with the worst-case
 * reward, as in pcbenv_step.  Later transitions draw.
 * Outputs (device pointers; only reward_dev is required, the others may be NULL):
 *   reward_dev[i]       float64: the value the reward tensor would show at the last transition played.  Not a sum
 *                       (square / rect: the return is length - 1 + reward).
 *   done_dev[i]         uint8: 0 when the playout was cut at max_steps
 *   length_dev[i]       int32: the number of transitions played
 *   info_dev[i, 2]      float64 (wirelength, num_intersections) of that last transition, NaN where the reference's info
 *                       dict is empty.  Pin kinds only (ignored otherwise).
 *   actions_out_dev     int32 [actions_steps, num_playouts, 3] or [actions_steps, num_playouts]: rows
 *                       t < min(length, actions_steps) are written (row 0 of a forced action: the action as given), the
 *                       others are untouched.  actions_steps is in 0 ... max_steps: a receding-horizon caller keeps
 *                       only the first action.
 * A root_index outside [0, num_envs) is checked before it addresses anything: bit 0 is ORed into *errors_dev (if not
 * NULL) and that playout reports length = 0, done = 0, reward = 0.0 and NaN info.
 * Writes nothing the library owns and nothing bound -- state blocks, the fused sampler's presampled action, the terminal
 * list and its marks, queue, cursors, observation tensors: a later call on the handle behaves exactly as without it.
 * PCBENV_FLAG_AUTO_RESET is ignored (a playout never resets and never consumes an instance), as are the trajectory
 * layout, the selected slot, helper marks in the root's header and its presampled action.
 * PCBENV_EINVAL (checked before any device call, in this order): null reward_dev; unknown format; max_steps < 1;
 * actions_steps outside [0, max_steps], or > 0 with null actions_out_dev; num_playouts < 0; null root_index_dev with
 * num_playouts not a multiple of num_envs; null handle.  num_playouts == 0 is a no-op success.  PCBENV_ESTATE: buffers
 * not bound, no episode in the handle yet (no reset, gather or restored state), or `stream` is being captured into a
 * hipGraph (the current-set pointer alternates; as pcbenv_sample_logits). */
int pcbenv_playout(const pcbenv *env, const int32_t *root_index_dev, int64_t num_playouts,
                   const int32_t *first_actions_dev, int32_t action_format, int32_t max_steps,
                   double *reward_dev, uint8_t *done_dev, int32_t *length_dev, double *info_dev,
                   int32_t *actions_out_dev, int32_t actions_steps, uint32_t *errors_dev,
                   uint64_t seed, uint64_t first_env_index, uint64_t step_index0, void *stream);

/* Playouts from tree nodes named by a path: pcbenv_playout with a sequence of forced actions per playout, and the legal
 * mask of the node the sequence leads to.  What a search deeper than one ply (MCTS / UCT, beam search over placements,
 * CEM over action sequences, re-scoring a stored episode prefix) needs to evaluate a node without materialising it: one
 * kernel launch on req->stream, no planner handle, no launch per ply, no observation.  The arguments travel in a struct.
 * The identity.  pcbenv_playout's, with one change: transition t < path_len[i] of playout i applies path_actions[t, i]
 * instead of a draw; transition t >= path_len[i] draws with the key (seed, first_env_index + i, step_index0 + t) -- what
 * pcbenv_step_sampled(seed, first_env_index, step_index0 + t) would draw for environment i of a handle of num_playouts
 * environments after pcbenv_gather and the path's steps had brought root r's episode there -- and every transition is
 * that handle's, bit for bit.  The draw key depends on t, not on the path.  Hence path_steps == 1 equals pcbenv_playout
 * with first_actions_dev, and a path equal to the first d actions of the path-less playout with the same keys gives that
 * playout's outputs bit for bit, for every d.
 * A bad path action is data: an illegal or out-of-range path action is a terminal transition with the worst-case
 * reward, as in pcbenv_step.  The playout ends there: the path rows after it are not read for effect and nothing after
 * it is drawn.
 * struct_size: sizeof(pcbenv_playout_request) as the caller compiled it.  root_index_dev, num_playouts, reward_dev,
 * done_dev, length_dev, info_dev, errors_dev, seed, first_env_index, step_index0: as pcbenv_playout.  max_steps counts
 * all transitions, the path's included.
 * path_actions_dev: int32 [path_steps, num_playouts, 3] or [path_steps, num_playouts] per action_format: step-major,
 * the layout of actions_out_dev; may be NULL iff path_steps == 0.  path_len_dev: int32 [num_playouts], or NULL =
 * path_steps for every playout.  Rows t >= path_len[i] of playout i are never read.
 * actions_out_dev: rows t < min(length, actions_steps) are written -- a path action is recorded as given (flat: the
 * value as given) -- and the others are untouched.
 * leaf_mask_bits_dev (optional): uint64 [num_playouts, 2, H, ceil(W/64)], 8-byte aligned.  Row i receives the legal-mask
 * bit rows, in the layout pcbenv_mask_bits documents, of the episode after transition min(path_len[i], length[i]) - 1:
 * the node the path names, or the state in which the episode ended if it ended on the path (an invalid action leaves the
 * state as it was).  With path_len[i] == 0 it is the root's own.  Every word of the row is written, once.  The bits of
 * columns >= W and plane 1 of the square kind are copied from the state block as they are and are left unspecified (no
 * entry point reads them).  Directly usable as mask_bits_dev of pcbenv_evaluate_logits / pcbenv_evaluate_axis.
 * A path_len[i] outside [0, path_steps] is checked before it addresses anything: bit 1 (value 2) is ORed into
 * *errors_dev (if not NULL) and the playout reports like a bad root -- length = 0, done = 0, reward = 0.0, NaN info.  A
 * root_index outside [0, num_envs) still sets bit 0.  A row refused for either reason gets an all-zero leaf mask and no
 * action row.
 * Writes nothing the library owns and nothing bound, exactly as pcbenv_playout: a later call on the handle behaves as
 * without it.  PCBENV_FLAG_AUTO_RESET is ignored, as are the trajectory layout, the selected slot, helper marks in the
 * root's header and its presampled action.  Not capturable into a hipGraph.
 * PCBENV_EINVAL (checked before any device call, in this order): null request; struct_size not
 * sizeof(pcbenv_playout_request); null reward_dev; unknown format; max_steps < 1; path_steps outside [0, max_steps];
 * path_steps > 0 with null path_actions_dev; actions_steps outside [0, max_steps], or > 0 with null actions_out_dev;
 * leaf_mask_bits_dev not 8-byte aligned; num_playouts < 0; null root_index_dev with num_playouts not a multiple of
 * num_envs; null handle.  num_playouts == 0 is a no-op success.  PCBENV_ESTATE: as pcbenv_playout (buffers not bound, no
 * episode in the handle yet, or req->stream is being captured). */
typedef struct pcbenv_playout_request {
    uint32_t struct_size;             /* sizeof(pcbenv_playout_request) as the caller compiled it; any other value: PCBENV_EINVAL */
    int32_t  action_format;           /* of path_actions_dev and actions_out_dev */
    const int32_t *root_index_dev;    /* as pcbenv_playout */
    int64_t  num_playouts;
    const int32_t *path_actions_dev;  /* int32 [path_steps, num_playouts, 3] or [path_steps, num_playouts]: step-major, the
                                         layout of actions_out_dev; may be NULL iff path_steps == 0 */
    const int32_t *path_len_dev;      /* int32 [num_playouts], or NULL = path_steps for every playout */
    int32_t  path_steps;              /* 0 ... max_steps */
    int32_t  max_steps;               /* all transitions, the path's included */
    double  *reward_dev; uint8_t *done_dev; int32_t *length_dev; double *info_dev;   /* as pcbenv_playout */
    int32_t *actions_out_dev; int32_t actions_steps;                                 /* as pcbenv_playout */
    uint64_t *leaf_mask_bits_dev;     /* optional: uint64 [num_playouts, 2, H, ceil(W/64)], 8-byte aligned */
    uint32_t *errors_dev;
    uint64_t seed, first_env_index, step_index0;
    void    *stream;
} pcbenv_playout_request;
int pcbenv_playout_paths(const pcbenv *env, const pcbenv_playout_request *req);

/* Materialise tree nodes named by a path: pcbenv_gather followed by a per-row path of forced actions, in ONE kernel
 * launch on req->stream (within one handle, preceded by the 25-byte-per-environment snapshot copy pcbenv_gather makes).
 * What a network needs to score a node -- priors at a tree's nodes, a learned rollout policy behind a path: the node's
 * grid, action_mask, pin_grid and feature tensors in a handle.  The observations are written once, however long the path.
 * The identity.  After the call, environment i of dst is what pcbenv_gather(dst, src, src_index) would have made it,
 * followed by transitions t = 0, 1, ..., path_len[i] - 1 of environment i ALONE, each the transition pcbenv_step would
 * make with action path_actions[t, i] on a handle without PCBENV_FLAG_AUTO_RESET, stopping behind the first one that
 * reports `done`.  Every bound tensor of row i in the destination's selected slot (pcbenv_buffers, the compact feature
 * tensors, the mask marginals) is written whole and shows the state after the last transition applied; reward / done /
 * info are those of the last transition applied, or -- with no transition applied -- the source row's, as pcbenv_gather
 * copies them; length_dev[i] is the number of transitions applied; and the state block is the one those calls would
 * have left, so every later call on dst behaves as after them.
 * path_steps == 0: the call is pcbenv_gather, bit for bit, state block included.
 * A bad path action is data: an illegal or out-of-range action is a terminal transition with the worst-case reward and
 * the state unchanged, as in pcbenv_step.  It is the last transition applied: path rows behind it, and rows
 * t >= path_len[i], are never read for effect.  A root whose episode is already over still gets its path applied (there
 * is no done latch, as in pcbenv_step): only a `done` among the row's own transitions stops it.
 * The call never resets and never consumes an instance: PCBENV_FLAG_AUTO_RESET of dst is ignored for these transitions
 * (a later pcbenv_step of dst resets as usual).  Everything pcbenv_gather says stays the destination's own stays so: the
 * queue cursor, the episode count, the generator state, the bind generation of its feature rows; no terminal-list mark
 * and no presampled action is left; the spatial feature cache is refilled under the destination's episode tag.
 * Rows with src_index[i] == -1 keep their episode: none of their tensors is touched, their path is not read and
 * length_dev[i] = 0.  Any other out-of-range src_index does the same and ORs bit 0 into *errors_dev (if not NULL).  A
 * path_len[i] outside [0, path_steps] is checked before it addresses or bounds anything: the row keeps its episode in
 * the same way and bit 1 (value 2) is ORed in.
 * Enqueue-only on req->stream: no allocation, no host synchronisation.  Not capturable into a hipGraph (PCBENV_ESTATE,
 * as pcbenv_gather); a handle that works in place after a capture gets the result copied back into its set, as
 * pcbenv_gather does.  Afterwards the handle has an episode.
 * PCBENV_EINVAL (checked before any device call, in this order): null request; struct_size not
 * sizeof(pcbenv_gather_paths_request); unknown format; path_steps < 0; path_steps > 0 with null path_actions_dev; null
 * src_index_dev; null handle; the definition / device mismatches pcbenv_gather refuses.  PCBENV_ESTATE: as pcbenv_gather. */
typedef struct pcbenv_gather_paths_request {
    uint32_t struct_size;             /* sizeof as the caller compiled it; any other value: PCBENV_EINVAL */
    int32_t  action_format;           /* of path_actions_dev */
    const pcbenv *src;                /* NULL or dst: the same handle; as pcbenv_gather */
    const int32_t *src_index_dev;     /* int32 [dst num_envs]; -1 keeps the row's episode; as pcbenv_gather */
    const int32_t *path_actions_dev;  /* int32 [path_steps, B, 3] or [path_steps, B], step-major; NULL iff path_steps == 0 */
    const int32_t *path_len_dev;      /* int32 [B], or NULL = path_steps for every row */
    int32_t  path_steps;              /* >= 0 */
    int32_t *length_dev;              /* optional int32 [B]: transitions applied to row i */
    uint32_t *errors_dev;             /* optional */
    void    *stream;
} pcbenv_gather_paths_request;
int pcbenv_gather_paths(pcbenv *dst, const pcbenv_gather_paths_request *req);

/* The tree around pcbenv_playout_paths: UCT selection, expansion and backup of P search trees, one per root, in one
 * kernel launch on req->stream.  An iteration of a batched search is then two launches with nothing between them:
 * pcbenv_tree_advance(ABSORB | SELECT) writes selected / path_len / paths, pcbenv_playout_paths plays the P nodes they
 * name, and the next pcbenv_tree_advance absorbs its reward / length / actions.  The caller owns every tensor; the
 * handle supplies the device and pcbenv_last_error only: nothing the library owns is read or written and no bound
 * buffers are needed.  Enqueue only, no allocation, no synchronisation.  Not meant to be captured into a hipGraph.
 * The tree of root p has N = capacity node slots, slot 0 the root, filled in the order the nodes are made; a node has
 * up to C = max_children children, children[p, n, 0 .. num_children[p, n]) in the order they were made, -1 behind them.
 * phases is a set of the three below; one launch runs them in the order INIT, ABSORB, SELECT.
 * PCBENV_TREE_INIT.  num_nodes = 1, reward_lo = +inf, reward_hi = -inf, best_reward = -inf, best_length = 0; every
 * slot (the root and the unused ones alike): parent = -1, depth = 0, visits = 0, num_children = 0, node_action = 0,
 * value_sum = 0, value_max = -inf, terminal = 0, children = -1.  best_actions is not written.
 * PCBENV_TREE_SELECT.  Start at node 0.  Stop at a node that is terminal or has fewer than C children; otherwise go to
 * the child with the highest q + c_uct * sqrt(ln[visits(node)] / visits(child)), with
 * q = (value_sum(child) / visits(child) - reward_lo) / (reward_hi - reward_lo) if reward_hi > reward_lo, else 0; all of
 * it float64, one IEEE operation per operator, visits taken as at least 1; ties go to the lowest child slot.  ln[n] is
 * ln_dev[min(n, N)]: the caller's table (the kernel never computes a logarithm, so a search is a function of the
 * table); a tree with N = iterations + 1 slots never reads past n = iterations.  Level d of the descent writes
 * paths[d, p, :] = node_action(child); then path_len[p] = depth(selected) = the levels taken and selected[p].  Rows
 * >= path_len[p] of paths are untouched.  At most max_steps levels.
 * PCBENV_TREE_ABSORB.  reward[p], length[p], actions[:, p, :] are what the playout from selected[p] returned (rewards
 * are finite).  With node = selected[p]: drew = length > depth(node) && !terminal(node), a = actions[min(depth,
 * T - 1), p].  If drew and a child of node has action a, the leaf is the first such child.  Else, if drew, node has fewer
 * than C children and num_nodes < N, the leaf is a new child in slot num_nodes (parent = node, depth + 1, node_action =
 * a, terminal = length <= depth + 1), appended to node's children.  Else the leaf is node; where only num_nodes == N
 * kept a child from being made, bit 0 (value 1) is ORed into *errors_dev.  Then reward_lo = min(reward_lo, r), reward_hi =
 * max(reward_hi, r); visits += 1, value_sum += r, value_max = max(value_max, r) on the leaf and every ancestor; and if
 * r > best_reward: best_reward = r, best_length = length, best_actions[t, p, :] = actions[t, p, :] for t < length.
 * Rows >= length of best_actions are untouched.
 * A slot number the kernel reads back -- selected[p], num_nodes[p], a child, a parent -- is compared with N before it
 * addresses anything; one out of range ends that root's phase where it stands and ORs bit 1 (value 2) into *errors_dev.
 * Layouts (int32 unless said): num_nodes [P]; parent, depth, visits, num_children [P, N]; node_action [P, N, 3];
 * children [P, N, C]; value_sum, value_max float64 [P, N]; terminal uint8 [P, N]; reward_lo, reward_hi, best_reward
 * float64 [P]; best_length [P]; best_actions [T, P, 3]; selected, path_len [P]; paths [T, P, 3]; reward float64 [P];
 * length [P]; actions [T, P, 3] -- the step-major tuple format of pcbenv_playout_paths' path_actions_dev and
 * actions_out_dev, T = max_steps.  errors_dev may be NULL.
 * PCBENV_EINVAL (checked before any device call, in this order): null request; struct_size not
 * sizeof(pcbenv_tree_request); phases 0 or with unknown bits, then INIT together with ABSORB; num_roots < 0; capacity < 1;
 * max_children outside [1, PCBENV_MAX_TREE_CHILDREN]; max_steps < 1; a null tensor among num_nodes ... reward_hi (every
 * phase), best_reward, best_length (INIT, ABSORB), best_actions (ABSORB); null selected (ABSORB, SELECT); null path_len or
 * paths (SELECT); null ln_dev (SELECT); null reward, length or actions (ABSORB); ln_dev or a float64 tensor not 8-byte
 * aligned; null handle.  num_roots == 0 is a no-op success. */
#define PCBENV_TREE_INIT 1
#define PCBENV_TREE_ABSORB 2
#define PCBENV_TREE_SELECT 4
#define PCBENV_MAX_TREE_CHILDREN 64
typedef struct pcbenv_tree_request {
    uint32_t struct_size; int32_t phases;            /* INIT, ABSORB, SELECT in that order; INIT|ABSORB is EINVAL */
    int32_t num_roots /*P*/, capacity /*N node slots per root*/, max_children /*C*/, max_steps /*T*/;
    double c_uct;
    const double *ln_dev;                            /* float64 [N + 1]: ln_dev[n] = the caller's ln n, n >= 1 */
    /* the tree, caller-owned device memory, root-major */
    int32_t *num_nodes;                              /* [P] */
    int32_t *parent, *depth, *visits, *num_children; /* [P, N] */
    int32_t *node_action;                            /* [P, N, 3] */
    int32_t *children;                               /* [P, N, C] */
    double *value_sum, *value_max;                   /* [P, N] */
    uint8_t *terminal;                               /* [P, N] */
    double *reward_lo, *reward_hi, *best_reward;     /* [P] */
    int32_t *best_length;                            /* [P] */
    int32_t *best_actions;                           /* [T, P, 3] */
    /* exchange with pcbenv_playout_paths (tuple format, step-major) */
    int32_t *selected, *path_len;                    /* [P]   written by SELECT */
    int32_t *paths;                                  /* [T, P, 3]: rows t < path_len[p] written, the others untouched */
    const double *reward; const int32_t *length; const int32_t *actions;  /* [P], [P], [T, P, 3]: read by ABSORB */
    uint32_t *errors_dev;                            /* optional */
    void *stream;
} pcbenv_tree_request;
int pcbenv_tree_advance(const pcbenv *env, const pcbenv_tree_request *req);

/* Masked categorical draw from a policy's logits, on the device, one kernel launch on `stream`.
 * logits_dev: C-contiguous [num_envs, A], A = O*H*W (square: H*W), in the flat action order of PCBENV_ACTION_FLAT
 * (a = o*H*W + x*W + y: what a Dense(action_space.n) head emits), float32 or bf16, aligned to its element size.
 * L_e, the legal set of environment e, is what action_mask shows, read from the bit rows of the current state set (as
 * pcbenv_sample_actions reads them; pin kinds: orientations 2 and 3 use mask planes 0 and 1).  An illegal logit is never
 * read: it may hold anything (NaN, or the already-masked logit + float32.min), so masked and unmasked logits give
 * identical results.  With M = max over L_e of l_i, w_i = exp(l_i - M), Z = sum over L_e of w_i, p_i = w_i / Z on L_e:
 *   PCBENV_DRAW_SAMPLE  u = hi32(rnd) / 2^32, rnd = mix64(mix64(seed ^ GOLDEN*(genv+1)) + step_index) -- the value
 *                       pcbenv_sample_actions uses, genv = first_env_index + e -- and the action is the first legal i in
 *                       flat order whose prefix sum C_i = sum over legal j <= i of w_j exceeds u*Z (up to float32
 *                       rounding of the partial sums, never an illegal action; the threshold and the sums across
 *                       segments of 64 columns are float64).  Constant logits draw bit for bit what pcbenv_sample_actions
 *                       draws.
 *   PCBENV_DRAW_GREEDY  argmax of l_i over L_e, the lowest flat index on ties (deterministic_sample; torch.argmax of the
 *                       masked logits).
 * In both modes log_prob[e] = l_a - M - log Z and entropy[e] = log Z - sum over L_e of p_i (l_i - M) (float32; the
 * reference's formula, factorized_action_distributions.py:49-59).  log_prob_dev, entropy_dev, errors_dev may be NULL.
 * No legal action: action 0, log_prob = entropy = 0 (data, not an error).  A legal logit that is NaN or +inf (bit 0 of
 * *errors_dev), or every legal logit -inf (bit 1): the draw is the uniform one of pcbenv_sample_actions,
 * log_prob = -log n, entropy = log n (n legal flat actions), and the bit is ORed into *errors_dev.
 * Writes nothing the library owns (state blocks, the fused sampler's presampled action, terminal list, queue): a later
 * pcbenv_step* behaves exactly as without the call.  PCBENV_EINVAL (checked before any device call): null handle, logits
 * or actions, unknown dtype, mode or format, misaligned logits.  PCBENV_ESTATE: buffers not bound, or `stream` is being
 * captured into a hipGraph (as pcbenv_gather). */
enum pcbenv_logits_dtype { PCBENV_LOGITS_F32 = 0, PCBENV_LOGITS_BF16 = 1 };
enum pcbenv_draw_mode { PCBENV_DRAW_SAMPLE = 0, PCBENV_DRAW_GREEDY = 1 };
int pcbenv_sample_logits(pcbenv *env, const void *logits_dev, int32_t logits_dtype, int32_t mode,
                         int32_t *actions_dev, int32_t action_format, float *log_prob_dev, float *entropy_dev,
                         uint32_t *errors_dev, uint64_t seed, uint64_t first_env_index, uint64_t step_index,
                         void *stream);

/* The update half of the same masked categorical: log-probability and entropy of stored actions, and their gradient
 * with respect to the logits.  One kernel launch each on `stream`.
 * Rows are independent and num_rows is arbitrary (a minibatch of stored steps, not the handle's num_envs).  The handle
 * supplies the geometry (kind, O, H, W) and the device only: neither call reads or writes anything the library owns, so
 * neither needs bound buffers.
 * logits_dev: C-contiguous [num_rows, A] float32 or bf16 in flat action order, aligned to its element size, as for
 * pcbenv_sample_logits.  mask_bits_dev: dense uint64 [num_rows, 2, H, ceil(W/64)], the layout pcbenv_mask_bits
 * documents (orientation o reads plane o & 1, square reads plane 0 only; bits of columns >= W are ignored).  An illegal
 * logit is never read: it may hold NaN or an already-masked value, so masked and unmasked logits give identical results.
 * actions_dev: int32 [num_rows] (PCBENV_ACTION_FLAT) or [num_rows, 3] (PCBENV_ACTION_TUPLE).
 * stats_dev: float32 [num_rows, 4] = (M, log Z, entropy, row status), 16-byte aligned; the forward call writes it and
 * the backward call consumes it, so that backward is one pass.  It may be NULL in forward when no gradient is wanted.
 * Forward, with L, M, w_i, Z, p_i as above: log_prob = l_a - M - log Z, entropy = log Z - sum over L of p_i (l_i - M)
 * (a legal logit whose weight is 0 contributes 0: -inf, or finite and so far below M that the weight underflows or
 * l_i - M is itself no float32).  log_prob_dev, entropy_dev, errors_dev may be NULL.
 * Backward writes EVERY element of grad_logits_dev [num_rows, A] in the logits' dtype (bf16: round to nearest even); the
 * caller passes uninitialised memory.  With log p_i = l_i - M - log Z and Hrow the row's entropy:
 *   g_i = g_lp (1[i = a] - p_i) - g_H p_i (log p_i + Hrow)   for i in L   (p_i = 0: the second term is 0, never NaN)
 *   g_i = 0                                                   for i not in L
 * grad_log_prob_dev (g_lp) and grad_entropy_dev (g_H) are float32 [num_rows]; either may be NULL, which means zero.
 * Edge cases are data:
 *   no legal action in a row         log_prob = entropy = 0, gradient row zero (what pcbenv_sample_logits reports)
 *   a legal NaN or +inf              bit 0 of *errors_dev; log_prob = -log n, entropy = log n, gradient row zero
 *   every legal logit -inf           bit 1; the same outputs
 *   the stored action out of range or not legal, in a row with legal actions and neither of the two cases above
 *                                    bit 2; log_prob = 0, the entropy as usual, the one-hot term dropped in backward
 * The bits are ORed into *errors_dev by the forward call.
 * PCBENV_EINVAL (checked before any device call): null handle, logits, mask bits, actions or (backward) stats or grad
 * logits; unknown dtype or format; misaligned logits, mask bits, stats or grad logits; num_rows < 0.  num_rows == 0 is a
 * no-op success.  Neither call is meant to be captured into a hipGraph. */
int pcbenv_evaluate_logits(const pcbenv *env, const void *logits_dev, int32_t logits_dtype,
                           const uint64_t *mask_bits_dev, const int32_t *actions_dev, int32_t action_format,
                           int64_t num_rows, float *log_prob_dev, float *entropy_dev, float *stats_dev,
                           uint32_t *errors_dev, void *stream);
int pcbenv_evaluate_logits_backward(const pcbenv *env, const void *logits_dev, int32_t logits_dtype,
                           const uint64_t *mask_bits_dev, const int32_t *actions_dev, int32_t action_format,
                           int64_t num_rows, const float *stats_dev, const float *grad_log_prob_dev,
                           const float *grad_entropy_dev, void *grad_logits_dev, void *stream);

/* One stage of a factorised policy: a masked categorical over ONE action coordinate, given some of the others.  One
 * kernel launch each on `stream`; a policy p(o) p(x|o) p(y|o,x) draws with three pcbenv_sample_axis calls and is
 * updated with three pcbenv_evaluate_axis + three pcbenv_evaluate_axis_backward calls.  Nothing reads action_mask.
 * Axes: 0 = orientation (n = O), 1 = x (n = H), 2 = y (n = W).  `given` is a bit set (1u << axis) of the OTHER axes whose
 * values are already fixed.  The legal set of a row for target axis t is
 *   L = { v in [0, n) : some legal (o, x, y) has coordinate t equal to v and every given coordinate equal to its value }
 * with (o, x, y) legal when o < O and bit y of word [o & 1, x, y / 64] of the row's bit rows is set (bits of columns >= W
 * never count; the square kind never reads plane 1).  pcbenv_sample_axis reads the bit rows of the current state set (as
 * pcbenv_sample_logits does: row e = environment e, num_envs rows); the evaluate calls read the caller's dense uint64
 * [num_rows, 2, H, ceil(W/64)] (the layout pcbenv_mask_bits documents), for any num_rows.
 * logits_dev: C-contiguous [rows, n], float32 or bf16, aligned to its element size.  A logit outside L is never read: it
 * may hold NaN or an already-masked value, so raw and masked logits give identical results.
 * actions_dev: int32 [rows, 3] = (o, x, y).  The columns named in `given` are read; the sampler writes column `axis` and
 * the evaluate calls read the stored value there; the remaining column is neither read nor written.
 * With M = max over L of l_v, w_v = exp(l_v - M), Z = sum over L of w_v, p_v = w_v / Z, as for pcbenv_sample_logits:
 *   log_prob = l_a - M - log Z        entropy = log Z - sum over L of p_v (l_v - M)     (a zero weight contributes 0)
 *   PCBENV_DRAW_SAMPLE  rnd = the value pcbenv_sample_actions uses for (seed, first_env_index + e, step_index),
 *                       rnd_axis = mix64(rnd + GOLDEN * (axis + 1)) -- the salt keeps the three stages of one step
 *                       independent -- u = hi32(rnd_axis) / 2^32, and the draw is the first v in L, in increasing v, whose
 *                       prefix sum exceeds u * Z (the threshold is float64, the partial sums carry float32 rounding); never
 *                       a value outside L, never one of weight 0.  Constant logits draw exactly member number
 *                       (hi32(rnd_axis) * |L|) >> 32 of L.
 *   PCBENV_DRAW_GREEDY  the lowest argmax over L.
 * Backward writes EVERY element of grad_logits_dev [num_rows, n] in the logits' dtype (bf16: round to nearest even); it
 * recomputes M and Z from the logits, so there is no statistics buffer.  With log p_v = l_v - M - log Z, Hrow the entropy:
 *   g_v = g_lp (1[v = a] - p_v) - g_H p_v (log p_v + Hrow)   for v in L   (p_v = 0: the second term is 0, never NaN)
 *   g_v = 0                                                   elsewhere
 * grad_log_prob_dev (g_lp) and grad_entropy_dev (g_H) are float32 [num_rows]; either may be NULL, which means zero.
 * Edge cases are data:
 *   L empty (no legal action at all, or a given combination with no legal completion)
 *                                    the value 0, log_prob = entropy = 0, gradient row zero; no error bit
 *   a NaN or +inf in L               bit 0 of *errors_dev; the sampler takes the uniform pick above (in both modes),
 *                                    log_prob = -log |L|, entropy = log |L|, gradient row zero
 *   every logit of L -inf            bit 1; the same outputs
 *   (evaluate) the stored value out of range or not in L, L not empty and neither of the two cases above
 *                                    bit 2; log_prob = 0, the entropy as usual, the one-hot term dropped in backward
 *   a given value out of range for its axis
 *                                    bit 3; otherwise treated as L empty
 * The bits are ORed into *errors_dev by the sampler and by the evaluate forward; errors_dev, log_prob_dev and entropy_dev
 * may be NULL.
 * PCBENV_EINVAL (checked before any device call, in this order): null logits or actions; unknown dtype, mode or axis;
 * `given` with a bit above 4 or containing 1u << axis; misaligned logits; null or misaligned mask bits; num_rows < 0; null
 * or misaligned grad logits; null handle.  PCBENV_ESTATE (sampler): buffers not bound, or `stream` is being captured into
 * a hipGraph (as pcbenv_sample_logits).  num_rows == 0 is a no-op success.
 * The sampler writes nothing the library owns; the evaluate calls use the handle for geometry and device only and need
 * no bound buffers. */
enum pcbenv_axis { PCBENV_AXIS_ORIENTATION = 0, PCBENV_AXIS_X = 1, PCBENV_AXIS_Y = 2 };
int pcbenv_sample_axis(pcbenv *env, int32_t axis, uint32_t given, const void *logits_dev, int32_t logits_dtype,
                       int32_t mode, int32_t *actions_dev, float *log_prob_dev, float *entropy_dev,
                       uint32_t *errors_dev, uint64_t seed, uint64_t first_env_index, uint64_t step_index, void *stream);
int pcbenv_evaluate_axis(const pcbenv *env, int32_t axis, uint32_t given, const void *logits_dev, int32_t logits_dtype,
                         const uint64_t *mask_bits_dev, const int32_t *actions_dev, int64_t num_rows,
                         float *log_prob_dev, float *entropy_dev, uint32_t *errors_dev, void *stream);
int pcbenv_evaluate_axis_backward(const pcbenv *env, int32_t axis, uint32_t given, const void *logits_dev,
                         int32_t logits_dtype, const uint64_t *mask_bits_dev, const int32_t *actions_dev,
                         int64_t num_rows, const float *grad_log_prob_dev, const float *grad_entropy_dev,
                         void *grad_logits_dev, void *stream);

/* Bit-packed legal-action mask of the current component, library-owned device
 * memory: uint64 [B, 2, H, ceil(W/64)] (orientation 0/1; pin kinds: 2 = 0, 3 = 1;
 * square: plane 0 only), bit y of word [b, o, x, y/64] = action_mask[b, o, x, y].
 * Also the row stride between environments in bytes.  The state blocks are double-buffered (a step launch reads one
 * set and writes the other): ask again after every pcbenv_step* / pcbenv_rollout_sampled, the pointer alternates. */
const uint64_t *pcbenv_mask_bits(const pcbenv *env, int64_t *env_stride_bytes);

#ifdef __cplusplus
}
#endif
#endif /* PCBENV_H */
