// pcbenv_api.hip -- host side of libpcbenv.so's C ABI (include/pcbenv.h): create / destroy / options / bind / load,
// reset / step / rollout / sample, checkpoint, gather, playout and the six policy entry points (the logits and the axis
// calls: their shared checks and prologue are stated once, in front of them).  No kernel is defined here: the
// environment kernels are instantiated per kind and part in pcb_kind.inc / pcb_playout.inc / pcb_gather_paths.inc, k_sample and k_cursor_range in pcb_sample.hip and the
// policy kernels in pcb_policy*.hip (all reached through pcb_launch.h); pcb_config.hip derives the layout from a
// configuration and pcb_gen.hip owns the on-device instance generator (pcb_host.h declares what the three share).
#include <stdlib.h>

#include <vector>

#include "pcb_host.h"
#include "pcb_launch.h"

static char g_err[256] = "";
int fail(pcbenv *env, int code, const char *fmt, const char *detail) {
    char *dst = env ? env->err : g_err;
    snprintf(dst, 256, fmt, detail);
    if (env) snprintf(g_err, 256, "%s", dst);
    return code;
}

extern "C" int pcbenv_abi_version(void) { return PCBENV_ABI_VERSION; }

extern "C" const char *pcbenv_last_error(const pcbenv *env) { return env ? env->err : g_err; }

// The launch functions of an environment kind (pcb_launch.h: the entries of the three families, k_reset and k_gather), indexed by pcbenv_config::kind.
struct KindLaunch {
    int (*step)(const StepLaunch &);
    int (*reset)(const ResetLaunch &);
    int (*gather)(const GatherLaunch &);
    int (*playout)(const PlayoutLaunch &);
    int (*gather_paths)(const GatherPathsLaunch &);
};
template <int KIND> static constexpr KindLaunch kind_entries() {
    return KindLaunch{launch_family<StepFamily, KIND>, pcb_launch_reset<KIND>, pcb_launch_gather<KIND>, launch_family<PlayoutFamily, KIND>, launch_family<GatherPathsFamily, KIND>};
}
static const KindLaunch kind_launch[] = {kind_entries<PCBENV_SQUARE>(), kind_entries<PCBENV_RECT>(), kind_entries<PCBENV_PIN>(), kind_entries<PCBENV_SPATIAL>()};
static_assert(PCBENV_SQUARE == 0 && PCBENV_RECT == 1 && PCBENV_PIN == 2 && PCBENV_SPATIAL == 3, "kind_launch is indexed by kind");
// A launch function's -1: the build pcb_layout selected is in no unit (pcb_layout::every_launch_has_a_unit asserts that
// there is no such launch): nothing was enqueued.
static int launched(pcbenv *env, int rc) { return rc == 0 ? PCBENV_OK : fail(env, PCBENV_EHIP, "no translation unit of the library compiles the kernel build of this launch"); }

// validate, derive, allocate, zero
extern "C" int pcbenv_create(const pcbenv_config *cfg, int device, pcbenv **out) {
    if (out) *out = 0;
    if (!cfg || !out) return fail(0, PCBENV_EINVAL, "null argument");
    int rc = validate(cfg);
    if (rc != PCBENV_OK) return rc;
    pcbenv *env = new pcbenv();
    memset(env, 0, sizeof(*env));
    env->cfg = *cfg;
    env->device = device;
    if (is_pin_kind(cfg->kind)) {  // P:467-468 / S:450-451: clipped after validation
        env->cfg.net_distribution = cfg->net_distribution < 0 ? 0 : cfg->net_distribution > 9 ? 9 : cfg->net_distribution;
        env->cfg.pin_spread = cfg->pin_spread < 0 ? 0 : cfg->pin_spread > 9 ? 9 : cfg->pin_spread;
    }
    derive_layout(env->cfg, env);
    DevParams &d = env->dp;
    DeviceGuard guard_(device);
    if (!guard_.ok) { int r = fail(0, PCBENV_EHIP, "hipSetDevice failed (no such device?)"); delete env; return r; }
    const size_t sbytes = (size_t)d.stateStride * d.B, qbytes = (size_t)d.instStride * d.B * d.Q;
    const struct { void **ptr; size_t bytes; } zeroed[] = {
        {(void **)&env->state_buf[0], sbytes}, {(void **)&env->state_buf[1], sbytes}, {(void **)&d.queue, qbytes ? qbytes : 16},
        {(void **)&d.cursor_pub, 4 * (size_t)d.B}, {(void **)&d.term_list, TERM_LIST_BYTES}, {(void **)&d.term_cnt, TERM_CNT_BYTES},
        {(void **)&d.term_arrive, TERM_ARRIVE_BYTES}};
    const char *what = 0;
    for (const auto &z : zeroed) {
        if (!what && hipMalloc(z.ptr, z.bytes) != hipSuccess) what = "hipMalloc failed";
        if (!what && hipMemset(*z.ptr, 0, z.bytes) != hipSuccess) what = "hipMemset failed";
    }
    if (!what && (hipHostMalloc((void **)&env->term_seen_host, 64, hipHostMallocMapped) != hipSuccess ||
                  hipHostGetDevicePointer((void **)&d.term_seen, env->term_seen_host, 0) != hipSuccess)) what = "hipMalloc failed";
    if (!what && hipDeviceSynchronize() != hipSuccess) what = "hipMemset failed";
    if (what) {
        int r = fail(0, PCBENV_EHIP, what);
        pcbenv_destroy(env);
        return r;
    }
#ifdef PCBENV_STAMPS
    { const char *ev = getenv("PCBENV_STAMPS"); if (ev && ev[0] == '1') { hipMalloc((void **)&d.dbg, (size_t)(d.B + PCBENV_TERM_CAP_MAX * (REWARD_PARTS + 1)) * 32 * 8); hipMemset(d.dbg, 0, (size_t)(d.B + PCBENV_TERM_CAP_MAX * (REWARD_PARTS + 1)) * 32 * 8); } }
#endif
    env->state_cur = 0;
    env->fixed_geometry = true;  // PCBENV_OPT_FIXED_GEOMETRY
    d.state = d.state_out = env->state_buf[0];
    *env->term_seen_host = 0u;
    *out = env;
    return PCBENV_OK;
}

// Releases whatever the handle holds: create zero-fills it, so a pointer, stream or event is either null or owned.
extern "C" void pcbenv_destroy(pcbenv *env) {
    if (!env) return;
    DeviceGuard guard_(env->device);
    gen_release(env);
    if (env->state_buf[0]) hipFree(env->state_buf[0]);
    if (env->state_buf[1]) hipFree(env->state_buf[1]);
    if (env->dp.queue) hipFree(env->dp.queue);
    if (env->dp.cursor_pub) hipFree(env->dp.cursor_pub);
    if (env->dp.term_list) hipFree(env->dp.term_list);
    if (env->dp.term_cnt) hipFree(env->dp.term_cnt);
    if (env->dp.term_arrive) hipFree(env->dp.term_arrive);
    if (env->dp.feat_cache) hipFree(env->dp.feat_cache);
    if (env->dp.feat_cache_tag) hipFree(env->dp.feat_cache_tag);
    if (env->term_seen_host) hipHostFree(env->term_seen_host);
    if (env->scratch) hipFree(env->scratch);
    if (env->gather_snap) hipFree(env->gather_snap);
    delete env;
}

extern "C" int pcbenv_set_option(pcbenv *env, int32_t option, int64_t value) {
    if (!env) return fail(0, PCBENV_EINVAL, "null handle");
    switch (option) {
    case PCBENV_OPT_STREAM_THRESHOLD_BYTES:
        if (value < 0) return fail(env, PCBENV_EINVAL, "threshold must not be negative");
        env->stream_threshold = value;
        env->dp.stream_stores = stream_stores(env, 1);
        return PCBENV_OK;
    case PCBENV_OPT_TERMINAL_TEAMS:
        if (value < 0 || value > PCBENV_TERM_CAP_MAX) return fail(env, PCBENV_EINVAL, "terminal-list entries must be in [0, 4096]");
        if (value > 0 && !is_pin_kind(env->cfg.kind))
            return fail(env, PCBENV_EINVAL, "reward helpers need an environment kind with a routing reward");
        value = (value + TERM_SHARDS - 1) & ~(long long)(TERM_SHARDS - 1);
        {   // The lists built so far were laid out for the old capacity: drop them (counters to zero once everything enqueued
            // has run; no mark matches the next launch's number).  A rare call: it synchronises the device, before the
            // fill and after it -- the fill goes to the null stream, which a non-blocking caller stream is not ordered with,
            // and the next launch on any stream must find the counters clear.
            DEVICE_GUARD(env);
            HIP_TRY(env, hipDeviceSynchronize());
            HIP_TRY(env, hipMemset(env->dp.term_cnt, 0, TERM_CNT_BYTES));
            HIP_TRY(env, hipDeviceSynchronize());
            *env->term_seen_host = 0u;
        }
        env->term_wgs = (int)value;
        env->dp.term_cap = (int)value;
        env->seq += 2;
        return PCBENV_OK;
    case PCBENV_OPT_GEN_GRID:
        if (value < 1) return fail(env, PCBENV_EINVAL, "generator grid must be at least 1");
        env->gen_grid = (int)value;
        return PCBENV_OK;
    case PCBENV_OPT_GEN_LANES:
        if (env->gen_on) return fail(env, PCBENV_ESTATE, "set the generator's group width before enabling it");
        if (value != 0 && value != 16 && value != 32 && value != 64) return fail(env, PCBENV_EINVAL, "generator lanes per environment: 0, 16, 32 or 64");
        env->gen_lanes = (int)value;
        return PCBENV_OK;
    case PCBENV_OPT_FIXED_GEOMETRY:
        if (value != 0 && value != 1) return fail(env, PCBENV_EINVAL, "fixed geometry: 0 or 1");
        env->fixed_geometry = value != 0;
        return PCBENV_OK;
    }
    return fail(env, PCBENV_EINVAL, "unknown option");
}

extern "C" int pcbenv_bind_buffers_slots(pcbenv *env, const pcbenv_buffers *b, int32_t num_slots);
extern "C" int pcbenv_bind_buffers(pcbenv *env, const pcbenv_buffers *b) { return pcbenv_bind_buffers_slots(env, b, 1); }

extern "C" int pcbenv_select_slot(pcbenv *env, int32_t slot) {
    if (!env) return fail(0, PCBENV_EINVAL, "null handle");
    if (slot < 0 || slot >= env->dp.num_slots) return fail(env, PCBENV_EINVAL, "slot out of range");
    env->dp.slot = slot;
    return PCBENV_OK;
}

extern "C" int pcbenv_bind_buffers_slots(pcbenv *env, const pcbenv_buffers *b, int32_t num_slots) {
    if (!env || !b) return fail(env, PCBENV_EINVAL, "null argument");
    if (num_slots < 1 || num_slots > 4096) return fail(env, PCBENV_EINVAL, "num_slots must be in [1, 4096]");
    if (num_slots > 1 && (env->cfg.flags & PCBENV_FLAG_INCREMENTAL_OBS))
        return fail(env, PCBENV_EINVAL, "PCBENV_FLAG_INCREMENTAL_OBS needs the in-place layout (num_slots = 1)");
    if ((long long)num_slots * env->dp.B > 0x7fffffffll / 8) return fail(env, PCBENV_ELIMIT, "num_slots * num_envs too large");
    if (!b->reward || !b->done) return fail(env, PCBENV_EINVAL, "reward and done buffers are required");
    // Everything that can fail comes first: a refused bind leaves the previous binding as it was.
    DEVICE_GUARD(env);
    DevParams &d = env->dp;
    const int k = env->cfg.kind;
    if (k == PCBENV_SPATIAL && num_slots > 1 && !d.feat_cache) {  // the episode-constant bytes a trajectory step copies
        const int cg = pcb_layout::feat_cache_grid_offset(d.C, d.F), stride = pcb_layout::feat_cache_stride(d.C, d.F, d.mp, d.K);
        if (hipMalloc((void **)&d.feat_cache, (size_t)stride * d.B) != hipSuccess || hipMalloc((void **)&d.feat_cache_tag, 4 * (size_t)d.B) != hipSuccess) {
            if (d.feat_cache) hipFree(d.feat_cache);  // both or neither: the next bind tries again
            d.feat_cache = 0; d.feat_cache_tag = 0;
            return fail(env, PCBENV_EHIP, "hipMalloc failed");
        }
        d.featCacheCg = cg; d.featCacheStride = stride;
    }
    // pcbenv_gather's snapshot (25 bytes per environment), allocated here and not per call
    if (!env->gather_snap && hipMalloc((void **)&env->gather_snap, 25 * (size_t)d.B) != hipSuccess) {
        env->gather_snap = 0;
        return fail(env, PCBENV_EHIP, "hipMalloc failed");
    }
    // Binding takes no stream: it synchronises the device, so that every launch enqueued so far (on any stream) has written
    // the old tensors and read the old tags before anything changes, and once more behind the tag fill (which goes to the
    // null stream), so that the next launch on any stream finds it done.  A rare call.
    HIP_TRY(env, hipDeviceSynchronize());
    if (d.feat_cache_tag) {  // no episode has that number: nothing cached yet
        HIP_TRY(env, hipMemset(d.feat_cache_tag, 0xFF, 4 * (size_t)d.B));
        HIP_TRY(env, hipDeviceSynchronize());
    }
    d.num_slots = num_slots; d.slot = 0;
    d.buf = *b;
    if (k != PCBENV_SPATIAL) { d.buf.pin_grid = 0; d.buf.component_grid = 0; }
    if (!is_pin_kind(k)) { d.buf.all_pins_num_feature = 0; d.buf.all_pins_cat_feature = 0; d.buf.info = 0; }
    if (k != PCBENV_RECT) d.buf.component_mask = 0;
    if (k == PCBENV_SQUARE) { d.buf.all_components_feature = 0; d.buf.placement_mask = 0; }
    env->cells_aligned16 = pcb_layout::aligned16(d.buf.grid) && pcb_layout::aligned16(d.buf.action_mask) && pcb_layout::aligned16(d.buf.pin_grid);
    d.bind_gen += 1;  // feature tensors of these buffers are uninitialised: the next reset of each env fills them
    memset(&d.cbuf, 0, sizeof(d.cbuf));  // compact tensors belong to a binding: bind them again
    env->bound = true;
    return PCBENV_OK;
}

extern "C" int pcbenv_bind_compact_features(pcbenv *env, const pcbenv_compact_features *f) {
    if (!env) return fail(0, PCBENV_EINVAL, "null handle");
    if (!env->bound) return fail(env, PCBENV_ESTATE, "pcbenv_bind_buffers has not been called");
    memset(&env->dp.cbuf, 0, sizeof(env->dp.cbuf));
    if (!f) return PCBENV_OK;
    if (env->dp.num_slots < 2) return fail(env, PCBENV_EINVAL, "compact feature tensors need the trajectory layout (pcbenv_bind_buffers_slots with num_slots > 1)");
    if (env->dp.H > 128 || env->dp.W > 128) return fail(env, PCBENV_ELIMIT, "coordinates do not fit the compact pin tensors");
    env->dp.cbuf = *f;
    const int k = env->cfg.kind;
    if (!is_pin_kind(k)) { env->dp.cbuf.all_pins_num_feature = 0; env->dp.cbuf.all_pins_cat_feature = 0; }
    if (k != PCBENV_RECT) env->dp.cbuf.component_mask = 0;
    if (k == PCBENV_SQUARE) memset(&env->dp.cbuf, 0, sizeof(env->dp.cbuf));
    return PCBENV_OK;
}

extern "C" int pcbenv_load_instances(pcbenv *env, const int32_t *env_ids, int32_t n, int32_t slot,
                                     const void *host_tables, void *stream) {
    if (!env || !host_tables) return fail(env, PCBENV_EINVAL, "null argument");
    const DevParams &d = env->dp;
    if (env->cfg.kind == PCBENV_SQUARE) return PCBENV_OK;  // the square env has no instance
    // refused before anything is copied: the generator owns the records, and k_gen_fill may be writing this very slot
    if (env->gen_on) return fail(env, PCBENV_ESTATE, "the on-device generator owns the queue (pcbenv_instgen_device_enable)");
    if (slot < 0 || slot >= d.Q || n < 0 || n > d.B) return fail(env, PCBENV_EINVAL, "slot or count out of range");
    DEVICE_GUARD(env);
    int rc = check_records(env, host_tables, n);
    if (rc != PCBENV_OK) return rc;
    const long long src_stride = pcbenv_instance_stride(&env->cfg);
    hipStream_t s = (hipStream_t)stream;
    const unsigned char *src = (const unsigned char *)host_tables;
    unsigned char *base = d.queue + (size_t)slot * d.B * d.instStride;
    if (!env_ids && src_stride == d.instStride) {
        HIP_TRY(env, hipMemcpyAsync(base, src, (size_t)n * src_stride, hipMemcpyHostToDevice, s));
    } else {
        for (int i = 0; i < n; i++) {
            int id = env_ids ? env_ids[i] : i;
            if (id < 0 || id >= d.B) return fail(env, PCBENV_EINVAL, "environment id out of range");
            HIP_TRY(env, hipMemcpyAsync(base + (size_t)id * d.instStride, src + (size_t)i * src_stride, (size_t)src_stride, hipMemcpyHostToDevice, s));
        }
    }
    HIP_TRY(env, hipStreamSynchronize(s));
    if (!env_ids && n == d.B) env->loaded_slots[slot >> 6] |= 1ull << (slot & 63);  // partial loads: caller's responsibility
    return PCBENV_OK;
}

static int launch_reset(pcbenv *env, const uint8_t *mask, hipStream_t s) {
    ResetLaunch a{env->dp, mask, env->threads, s};
    a.d.seq = env->seq;  // the next step launch is seq + 1: a reset takes its environments off that launch's terminal list
    return kind_launch[env->cfg.kind].reset(a);
}
// Every step launch has a number (DevParams::seq); see run_env (pcb_step.h) for what the terminal list is.
static int dispatch_step(pcbenv *env, int *actions, int fmt, int sampled, u64 seed, u64 first_env, u64 step_index, int num_steps, hipStream_t s) {
    StepLaunch a;
    a.d = env->dp;
    DevParams &d = a.d;
    a.actions = actions; a.fmt = fmt; a.sampled = sampled; a.seed = seed; a.first_env = first_env; a.step_index = step_index;
    a.num_steps = num_steps; a.threads = env->threads; a.stream = s;
    // The trajectory layout cycles through num_slots slots: the store policy is chosen on the bytes of all of them (a slot is
    // next written num_slots steps later; one launch per step into a [17, B, ...] trajectory measured + 14 % at c3, + 3 % at
    // c4 with streaming stores).  In place, the steps overwrite the same lines and the per-transition choice of
    // pcbenv_create stands.
    if (d.num_slots > 1) d.stream_stores = stream_stores(env, d.num_slots);
    a.routes = pcb_layout::routes_compiled_in(env->cfg.kind, env->cfg.reward_type);
    a.cells_aligned16 = env->cells_aligned16; a.fixed_geometry = env->fixed_geometry;
    if (++env->seq == 0u) env->seq = 1u;  // 0 is "not listed" in the marks
    d.seq = env->seq;
    // A launch that is being captured into a hipGraph will be replayed with these very arguments: no launch number,
    // no buffer swap -- it runs without helpers, keeps no list and works on the state blocks in place.  The graph may be
    // replayed at any later time, between eager calls, and must then find the current state where it was captured: from
    // the first capture on, every launch of the handle works in place on that same set (pcbenv_gather copies back).
    // The library cannot tell whether a graph is still alive, so nothing re-arms the swap: a replay after that would
    // silently step a stale set.
    if (stream_capturing(s)) env->in_place = true;
    const bool in_place = env->in_place;
    d.term_wgs = 0;
    if (num_steps == 1 && !in_place && env->term_wgs > 0) {  // reward helpers: one transition per launch only
        // as many entries' helpers as the lists have lately been long (k_step reports it: + 25 %, + 2 per shard; never none:
        // a shard's first entry)
        const unsigned seen = *(volatile unsigned *)env->term_seen_host;
        const long long want = (long long)TERM_SHARDS * ((long long)seen + seen / 4 + 2);
        d.term_wgs = (int)(want < env->term_wgs ? want : env->term_wgs);
    }
    if (in_place) d.term_cap = 0;
    // double-buffered state blocks: read the current ones, write the others
    d.state = env->state_buf[env->state_cur];
    d.state_out = env->state_buf[env->state_cur ^ (in_place ? 0 : 1)];
    const int rc = kind_launch[env->cfg.kind].step(a);
    if (!in_place) env->state_cur ^= 1;
    env->dp.state = env->dp.state_out = env->state_buf[env->state_cur];  // what k_reset / k_sample / get_state work on, in place
    return rc;
}

static int check_queue(pcbenv *env) {
    if (env->cfg.kind == PCBENV_SQUARE || env->gen_on) return PCBENV_OK;
    for (int s = 0; s < env->dp.Q; s++)
        if (!(env->loaded_slots[s >> 6] >> (s & 63) & 1ull))
            return fail(env, PCBENV_ESTATE, "every queue slot must be loaded (pcbenv_load_instances for all environments) first");
    return PCBENV_OK;
}

// The one path of every launch that may consume instance records (pcb_gen.hip has the protocol).  `checks` holds the entry
// point's own argument checks and says what it is going to launch; it runs on the handle's device, before anything of
// the generator is touched.
struct LaunchPlan {
    int consumes = 0;  // records per environment one launch may consume
    int launches = 1;
};
template <class Checks, class Launch>
static int consuming_launch(pcbenv *env, void *stream, Checks checks, Launch launch) {
    if (!env) return fail(0, PCBENV_EINVAL, "null handle");
    if (!env->bound) return fail(env, PCBENV_ESTATE, "pcbenv_bind_buffers has not been called");
    DEVICE_GUARD(env);
    LaunchPlan plan;
    int rc = checks(plan);
    if (rc) return rc;
    hipStream_t s = (hipStream_t)stream;
    for (int t = 0; t < plan.launches; t++) {
        rc = gen_before_launch(env, plan.consumes, s);
        if (rc) return rc;
        const int launch_rc = launch(t, s);
        if (t == plan.launches - 1) HIP_TRY(env, hipGetLastError());
        gen_after_launch(env, plan.consumes, s);
        if (launched(env, launch_rc)) return PCBENV_EHIP;
    }
    return PCBENV_OK;
}
// one transition per launch: a record per environment at most, and only where episodes restart in the launch
static int step_consumes(const pcbenv *env) { return (env->cfg.flags & PCBENV_FLAG_AUTO_RESET) ? 1 : 0; }
static int step_checks(pcbenv *env, const void *actions_dev, int fmt, LaunchPlan &plan) {
    if (!actions_dev) return fail(env, PCBENV_EINVAL, "null actions");
    CHECK_ACTION_FORMAT(env, fmt);
    plan.consumes = step_consumes(env);
    return PCBENV_OK;
}

extern "C" int pcbenv_reset(pcbenv *env, const uint8_t *mask_dev, void *stream) {
    const int rc = consuming_launch(
        env, stream, [&](LaunchPlan &plan) { plan.consumes = 1; return check_queue(env); },
        [&](int, hipStream_t s) { return launch_reset(env, mask_dev, s); });
    if (rc == PCBENV_OK) env->has_episode = true;
    return rc;
}

extern "C" int pcbenv_get_instances(pcbenv *env, int32_t slot, void *host_dst, void *stream) {
    if (!env || !host_dst) return fail(env, PCBENV_EINVAL, "null argument");
    if (slot < 0 || slot >= env->dp.Q) return fail(env, PCBENV_EINVAL, "slot out of range");
    DEVICE_GUARD(env);
    const DevParams &d = env->dp;
    const long long dst_stride = pcbenv_instance_stride(&env->cfg);
    // the copy runs on the stream that last wrote the queue (the generator's, if it is on): in order behind its kernels
    hipStream_t s = env->gen_on ? env->gen_stream : (hipStream_t)stream;
    HIP_TRY(env, hipStreamSynchronize((hipStream_t)stream));
    HIP_TRY(env, hipMemcpy2DAsync(host_dst, (size_t)dst_stride, d.queue + (size_t)slot * d.B * d.instStride, (size_t)d.instStride,
                                  (size_t)dst_stride, (size_t)d.B, hipMemcpyDeviceToHost, s));
    HIP_TRY(env, hipStreamSynchronize(s));
    return PCBENV_OK;
}

extern "C" int pcbenv_step(pcbenv *env, const int32_t *actions_dev, int32_t fmt, void *stream) {
    return consuming_launch(
        env, stream, [&](LaunchPlan &plan) { return step_checks(env, actions_dev, fmt, plan); },
        [&](int, hipStream_t s) { return dispatch_step(env, (int *)actions_dev, fmt, 0, 0, 0, 0, 1, s); });
}

extern "C" int pcbenv_step_sampled(pcbenv *env, int32_t *actions_out_dev, int32_t fmt, uint64_t seed,
                                   uint64_t first_env_index, uint64_t step_index, void *stream) {
    return consuming_launch(
        env, stream, [&](LaunchPlan &plan) { return step_checks(env, actions_out_dev, fmt, plan); },
        [&](int, hipStream_t s) { return dispatch_step(env, actions_out_dev, fmt, 1, seed, first_env_index, step_index, 1, s); });
}

// num_steps transitions: one launch of the persistent rollout kernel, every step of which may end an episode, or, with the
// row-incremental tensors, one launch per step as before
extern "C" int pcbenv_rollout_sampled(pcbenv *env, int32_t *actions_out_dev, int32_t fmt, int32_t num_steps,
                                      uint64_t seed, uint64_t first_env_index, uint64_t step_index0, void *stream) {
    bool per_step = false;
    return consuming_launch(
        env, stream,
        [&](LaunchPlan &plan) -> int {
            if (!actions_out_dev || num_steps < 0) return fail(env, PCBENV_EINVAL, "bad rollout arguments");
            CHECK_ACTION_FORMAT(env, fmt);
            per_step = (env->cfg.flags & PCBENV_FLAG_INCREMENTAL_OBS) != 0;
            plan.launches = per_step ? num_steps : num_steps > 0;
            plan.consumes = step_consumes(env) * (per_step ? 1 : num_steps);
            return PCBENV_OK;
        },
        [&](int t, hipStream_t s) {
            if (!per_step) return dispatch_step(env, actions_out_dev, fmt, 1, seed, first_env_index, step_index0, num_steps, s);
            const size_t actions_per_step = (size_t)env->dp.B * (fmt == PCBENV_ACTION_TUPLE ? 3 : 1);
            return dispatch_step(env, actions_out_dev + actions_per_step * (size_t)t, fmt, 1, seed, first_env_index, step_index0 + (uint64_t)t, 1, s);
        });
}

extern "C" int pcbenv_sample_actions(pcbenv *env, int32_t *actions_dev, int32_t fmt, uint64_t seed,
                                     uint64_t first_env_index, uint64_t step_index, void *stream) {
    if (!env || !actions_dev) return fail(env, PCBENV_EINVAL, "null argument");
    CHECK_ACTION_FORMAT(env, fmt);
    DEVICE_GUARD(env);
    pcb_launch_sample(SampleLaunch{env->dp, actions_dev, fmt, (u64)seed, (u64)first_env_index, (u64)step_index, (hipStream_t)stream});
    HIP_TRY(env, hipGetLastError());
    return PCBENV_OK;
}

extern "C" const uint64_t *pcbenv_mask_bits(const pcbenv *env, int64_t *env_stride_bytes) {
    if (!env) return 0;
    if (env_stride_bytes) *env_stride_bytes = env->dp.stateStride;
    return (const uint64_t *)(env->dp.state + env->dp.offVm);
}

// Checkpoint layout: [state blocks, B x stateStride] and, once the on-device generator is enabled, its section behind
// them (gen_section_bytes).
static size_t state_section_bytes(const pcbenv *env) { return (size_t)env->dp.stateStride * env->dp.B; }
extern "C" int64_t pcbenv_state_bytes(const pcbenv *env) {
    return env ? (int64_t)(state_section_bytes(env) + gen_section_bytes(env)) : 0;
}
extern "C" int pcbenv_get_state(pcbenv *env, void *host_dst, void *stream) {
    if (!env || !host_dst) return fail(env, PCBENV_EINVAL, "null argument");
    DEVICE_GUARD(env);
    hipStream_t s = (hipStream_t)stream;
    const size_t sb = state_section_bytes(env);
    unsigned char *dst = (unsigned char *)host_dst;
    HIP_TRY(env, hipMemcpyAsync(dst, env->dp.state, sb, hipMemcpyDeviceToHost, s));
    HIP_TRY(env, hipStreamSynchronize(s));
    return gen_save(env, dst + sb, s);
}
extern "C" int pcbenv_set_state(pcbenv *env, const void *host_src, void *stream) {
    if (!env || !host_src) return fail(env, PCBENV_EINVAL, "null argument");
    DEVICE_GUARD(env);
    hipStream_t s = (hipStream_t)stream;
    const size_t sb = state_section_bytes(env), B = (size_t)env->dp.B;
    // The terminal-list marks in a checkpoint refer to lists of the run that wrote it: restored environments are not listed.
    std::vector<unsigned char> blob((const unsigned char *)host_src, (const unsigned char *)host_src + sb);
    std::vector<unsigned> cur(B);  // the published copy of the queue cursors follows the restored headers
    for (size_t i = 0; i < B; i++) {
        EnvHdr *hd = (EnvHdr *)(blob.data() + i * env->dp.stateStride);
        hd->term_seq = 0u;
        cur[i] = hd->qcursor;
    }
    if (env->gen_on) {  // nothing of the generator may be in flight while its state is replaced
        HIP_TRY(env, hipStreamSynchronize(s));
        HIP_TRY(env, hipStreamSynchronize(env->gen_stream));
    }
    HIP_TRY(env, hipMemcpyAsync(env->dp.state, blob.data(), sb, hipMemcpyHostToDevice, s));
    HIP_TRY(env, hipMemcpyAsync(env->dp.cursor_pub, cur.data(), 4 * B, hipMemcpyHostToDevice, s));
    if (env->dp.feat_cache_tag) HIP_TRY(env, hipMemsetAsync(env->dp.feat_cache_tag, 0xFF, 4 * B, s));  // the cached bytes are another episode's
    const int rc = gen_restore(env, (const unsigned char *)host_src + sb, s);
    if (rc != PCBENV_OK) return rc;
    HIP_TRY(env, hipStreamSynchronize(s));
    env->has_episode = true;
    return PCBENV_OK;
}

// ---- pcbenv_gather ------------------------------------------------------------------------------------------
// The environment definition is every pcbenv_config field from kind through weight_num_intersections.
static_assert(offsetof(pcbenv_config, weight_num_intersections) + sizeof(double) == offsetof(pcbenv_config, num_envs),
              "the definition fields end where the batch fields begin");
// What pcbenv_gather and pcbenv_gather_paths do once their own arguments have passed (dst and src_index_dev are not
// null): the checks of the two handles, the parameter block, the same-handle snapshot, the launch -- k_gather, or with
// `paths` k_gather_paths -- then the set swap or, for a handle that works in place, the copy back.
static int gather_enqueue(pcbenv *dst, const pcbenv *src, const int32_t *src_index_dev, uint32_t *errors_dev, void *stream,
                          const GatherPathArgs *paths, const char *captured) {
    if (!src) src = dst;
    if (src != dst) {
        if (src->device != dst->device) return fail(dst, PCBENV_EINVAL, "the two handles are on different devices");
        if (memcmp(&src->cfg, &dst->cfg, offsetof(pcbenv_config, num_envs)) != 0)
            return fail(dst, PCBENV_EINVAL, "the two handles have different environment definitions");
    }
    if (!dst->bound || !src->bound) return fail(dst, PCBENV_ESTATE, "pcbenv_bind_buffers has not been called");
    DEVICE_GUARD(dst);
    hipStream_t s = (hipStream_t)stream;
    // A captured launch would be replayed with the state sets of the capture: the second replay would read a stale set.
    if (stream_capturing(s)) return fail(dst, PCBENV_ESTATE, captured);
    GatherPathsLaunch a;
    a.d = dst->dp;
    DevParams &d = a.d;
    a.threads = dst->threads; a.stream = s;
    a.routes = pcb_layout::routes_compiled_in(dst->cfg.kind, dst->cfg.reward_type);
    // the store policy a trajectory-layout step launch would use (dispatch_step)
    if (d.num_slots > 1) d.stream_stores = stream_stores(dst, d.num_slots);
    d.state = dst->state_buf[dst->state_cur];
    d.state_out = dst->state_buf[dst->state_cur ^ 1];
    const DevParams &sp = src->dp;
    const size_t r0 = (size_t)sp.slot * sp.B;  // first row of the source's selected slot
    GatherArgs &g = a.g;
    g.src_state = sp.state; g.src_index = src_index_dev; g.errors = (unsigned *)errors_dev; g.src_B = sp.B;
    if (src == dst) {
        // another team may overwrite row j of reward / done / info before the team that reads it runs: read a snapshot
        const size_t B = (size_t)d.B;
        unsigned char *snap = dst->gather_snap;
        HIP_TRY(dst, hipMemcpyAsync(snap, sp.buf.reward + r0, 8 * B, hipMemcpyDeviceToDevice, s));
        if (sp.buf.info) HIP_TRY(dst, hipMemcpyAsync(snap + 8 * B, sp.buf.info + 2 * r0, 16 * B, hipMemcpyDeviceToDevice, s));
        HIP_TRY(dst, hipMemcpyAsync(snap + 24 * B, sp.buf.done + r0, B, hipMemcpyDeviceToDevice, s));
        g.reward = (const double *)snap; g.info = sp.buf.info ? (const double *)(snap + 8 * B) : 0; g.done = snap + 24 * B;
    } else {
        g.reward = sp.buf.reward + r0; g.info = sp.buf.info ? sp.buf.info + 2 * r0 : 0; g.done = sp.buf.done + r0;
    }
    if (paths) a.q = *paths;
    if (launched(dst, paths ? kind_launch[dst->cfg.kind].gather_paths(a) : kind_launch[dst->cfg.kind].gather(GatherLaunch{a.d, a.g, a.threads, a.stream})))
        return PCBENV_EHIP;
    HIP_TRY(dst, hipGetLastError());
    dst->has_episode = true;
    if (dst->in_place) {  // a captured graph works on the current set (dispatch_step): the gathered blocks go back into it
        HIP_TRY(dst, hipMemcpyAsync(d.state, d.state_out, state_section_bytes(dst), hipMemcpyDeviceToDevice, s));
        return PCBENV_OK;
    }
    dst->state_cur ^= 1;
    dst->dp.state = dst->dp.state_out = dst->state_buf[dst->state_cur];
    return PCBENV_OK;
}

extern "C" int pcbenv_gather(pcbenv *dst, const pcbenv *src, const int32_t *src_index_dev, uint32_t *errors_dev, void *stream) {
    if (!dst) return fail(0, PCBENV_EINVAL, "null handle");
    if (!src_index_dev) return fail(dst, PCBENV_EINVAL, "null src_index");
    return gather_enqueue(dst, src, src_index_dev, errors_dev, stream, 0, "pcbenv_gather cannot be captured into a graph");
}

// ---- pcbenv_gather_paths -------------------------------------------------------------------------------------
// pcbenv_gather with a path of forced actions per row, applied in the same launch (k_gather_paths); the arguments in a
// struct (the stream among them).  Every argument check comes before a device is touched, the null handle behind them.
extern "C" int pcbenv_gather_paths(pcbenv *dst, const pcbenv_gather_paths_request *q) {
    if (!q) return fail(dst, PCBENV_EINVAL, "null request");
    if (q->struct_size != (uint32_t)sizeof(pcbenv_gather_paths_request)) return fail(dst, PCBENV_EINVAL, "struct_size is not sizeof(pcbenv_gather_paths_request)");
    CHECK_ACTION_FORMAT(dst, q->action_format);
    if (q->path_steps < 0) return fail(dst, PCBENV_EINVAL, "path_steps must not be negative");
    if (q->path_steps > 0 && !q->path_actions_dev) return fail(dst, PCBENV_EINVAL, "null path_actions with path_steps > 0");
    if (!q->src_index_dev) return fail(dst, PCBENV_EINVAL, "null src_index");
    if (!dst) return fail(0, PCBENV_EINVAL, "null handle");
    GatherPathArgs g;
    g.path_actions = q->path_actions_dev; g.path_len = q->path_len_dev; g.length = q->length_dev;
    g.fmt = q->action_format; g.path_steps = q->path_steps;
    return gather_enqueue(dst, q->src, q->src_index_dev, q->errors_dev, q->stream, &g, "pcbenv_gather_paths cannot be captured into a graph");
}

// ---- pcbenv_playout ------------------------------------------------------------------------------------------
// What pcbenv_playout and pcbenv_playout_paths do once their arguments have passed: the state checks, the parameter block
// and the launch.  `g` arrives with the caller's pointers and counts; n, per_root and info are filled in here.
static int playout_enqueue(pcbenv *env, int64_t num_playouts, PlayoutArgs g, void *stream, bool paths, const char *captured) {
    if (num_playouts > 0x7fffffffll / 8) return fail(env, PCBENV_ELIMIT, "num_playouts too large");
    if (num_playouts == 0) return PCBENV_OK;
    if (!env->bound) return fail(env, PCBENV_ESTATE, "pcbenv_bind_buffers has not been called");
    if (!env->has_episode) return fail(env, PCBENV_ESTATE, "no episode to play: reset the environments first");
    DEVICE_GUARD(env);
    hipStream_t s = (hipStream_t)stream;
    // A captured launch would keep reading the state set that was current at capture time (as pcbenv_sample_logits).
    if (stream_capturing(s)) return fail(env, PCBENV_ESTATE, captured);
    PlayoutLaunch a;
    a.d = env->dp;  // d.state: the current state set, as k_sample reads it
    DevParams &d = a.d;
    const bool pins = is_pin_kind(env->cfg.kind);
    // nothing bound and nothing of the library's can be reached through the block: terminal_reward writes row i of these two
    memset(&d.buf, 0, sizeof(d.buf));
    memset(&d.cbuf, 0, sizeof(d.cbuf));
    d.buf.reward = g.reward; d.buf.info = pins ? g.info : 0;
    d.flags = 0u; d.num_slots = 1; d.slot = 0; d.stream_stores = 0;
    d.queue = 0; d.feat_cache = 0; d.feat_cache_tag = 0; d.gen_produced = 0; d.gen_errors = 0; d.cursor_pub = 0;
    d.seq = 0u; d.term_wgs = 0; d.term_cap = 0; d.term_hpe = 0; d.term_list = 0; d.term_cnt = 0; d.term_arrive = 0; d.term_seen = 0;
    d.state_out = 0; d.dbg = 0;
    a.threads = env->threads; a.stream = s;
    a.routes = pcb_layout::routes_compiled_in(env->cfg.kind, env->cfg.reward_type); a.paths = paths;
    g.n = (int)num_playouts; g.per_root = g.root_index ? 1 : (int)(num_playouts / d.B);
    if (!pins) g.info = 0;
    a.g = g;
    if (launched(env, kind_launch[env->cfg.kind].playout(a))) return PCBENV_EHIP;
    HIP_TRY(env, hipGetLastError());
    return PCBENV_OK;
}

// The argument checks of pcbenv_playout and, with `paths` (its request; null otherwise), of pcbenv_playout_paths, whose own
// stand where its contract has them.  As pcbenv_sample_logits: they come before anything touches a device, the null
// handle last.
static int playout_checks(pcbenv *env, const double *reward_dev, int32_t fmt, int32_t max_steps, int32_t actions_steps, const int32_t *actions_out_dev,
                          const int32_t *root_index_dev, int64_t num_playouts, const pcbenv_playout_request *paths) {
    if (!reward_dev) return fail(env, PCBENV_EINVAL, "null reward");
    CHECK_ACTION_FORMAT(env, fmt);
    if (max_steps < 1) return fail(env, PCBENV_EINVAL, "max_steps must be at least 1");
    if (paths && (paths->path_steps < 0 || paths->path_steps > max_steps)) return fail(env, PCBENV_EINVAL, "path_steps must be in [0, max_steps]");
    if (paths && paths->path_steps > 0 && !paths->path_actions_dev) return fail(env, PCBENV_EINVAL, "null path_actions with path_steps > 0");
    if (actions_steps < 0 || actions_steps > max_steps) return fail(env, PCBENV_EINVAL, "actions_steps must be in [0, max_steps]");
    if (actions_steps > 0 && !actions_out_dev) return fail(env, PCBENV_EINVAL, "null actions_out with actions_steps > 0");
    if (paths && ((uintptr_t)paths->leaf_mask_bits_dev & 7u) != 0) return fail(env, PCBENV_EINVAL, "leaf_mask_bits must be 8-byte aligned");
    if (num_playouts < 0) return fail(env, PCBENV_EINVAL, "num_playouts must not be negative");
    if (env && !root_index_dev && num_playouts % env->dp.B != 0)
        return fail(env, PCBENV_EINVAL, "without root_index, num_playouts must be a multiple of num_envs");
    if (!env) return fail(0, PCBENV_EINVAL, "null handle");
    return PCBENV_OK;
}

// Nothing the library owns is written -- the kernel gets a parameter block in which nothing but the playout's own reward /
// info rows can be stored to.
extern "C" int pcbenv_playout(const pcbenv *cenv, const int32_t *root_index_dev, int64_t num_playouts,
                              const int32_t *first_actions_dev, int32_t fmt, int32_t max_steps, double *reward_dev,
                              uint8_t *done_dev, int32_t *length_dev, double *info_dev, int32_t *actions_out_dev,
                              int32_t actions_steps, uint32_t *errors_dev, uint64_t seed, uint64_t first_env_index,
                              uint64_t step_index0, void *stream) {
    pcbenv *env = const_cast<pcbenv *>(cenv);  // the error text only
    const int rc = playout_checks(env, reward_dev, fmt, max_steps, actions_steps, actions_out_dev, root_index_dev, num_playouts, 0);
    if (rc) return rc;
    PlayoutArgs g = PlayoutArgs();  // the path fields null / 0
    g.root_index = root_index_dev; g.first_actions = first_actions_dev; g.reward = reward_dev; g.done = done_dev;
    g.length = length_dev; g.info = info_dev; g.actions_out = actions_out_dev; g.errors = (unsigned *)errors_dev;
    g.fmt = fmt; g.max_steps = max_steps; g.actions_steps = actions_steps;
    g.seed = (u64)seed; g.first_env = (u64)first_env_index; g.step_index0 = (u64)step_index0;
    return playout_enqueue(env, num_playouts, g, stream, false, "pcbenv_playout cannot be captured into a graph");
}

// ---- pcbenv_playout_paths ------------------------------------------------------------------------------------
// pcbenv_playout with a path of forced actions per playout and the legal mask of the node it ends in; the arguments in a
// struct (the stream among them).  The same rules: every argument check before a device is touched, the null handle last.
extern "C" int pcbenv_playout_paths(const pcbenv *cenv, const pcbenv_playout_request *q) {
    pcbenv *env = const_cast<pcbenv *>(cenv);  // the error text only
    if (!q) return fail(env, PCBENV_EINVAL, "null request");
    if (q->struct_size != (uint32_t)sizeof(pcbenv_playout_request)) return fail(env, PCBENV_EINVAL, "struct_size is not sizeof(pcbenv_playout_request)");
    const int rc = playout_checks(env, q->reward_dev, q->action_format, q->max_steps, q->actions_steps, q->actions_out_dev, q->root_index_dev, q->num_playouts, q);
    if (rc) return rc;
    PlayoutArgs g = PlayoutArgs();
    g.root_index = q->root_index_dev; g.reward = q->reward_dev; g.done = q->done_dev;
    g.length = q->length_dev; g.info = q->info_dev; g.actions_out = q->actions_out_dev; g.errors = (unsigned *)q->errors_dev;
    g.fmt = q->action_format; g.max_steps = q->max_steps; g.actions_steps = q->actions_steps;
    g.seed = (u64)q->seed; g.first_env = (u64)q->first_env_index; g.step_index0 = (u64)q->step_index0;
    g.path_actions = q->path_actions_dev; g.path_len = q->path_len_dev; g.leaf_mask = (u64 *)q->leaf_mask_bits_dev; g.path_steps = q->path_steps;
    return playout_enqueue(env, q->num_playouts, g, q->stream, true, "pcbenv_playout_paths cannot be captured into a graph");
}

// ---- the policy entry points -----------------------------------------------------------------------------------
// pcbenv_sample_logits, pcbenv_evaluate_logits[_backward], pcbenv_sample_axis and pcbenv_evaluate_axis[_backward].  Their
// argument checks come before anything touches a device (a null handle included, and last), so that every one of them can
// be exercised without a GPU; the first to fire decides the message, in the order include/pcbenv.h gives.  Each check that
// more than one of them makes is stated once, here.
static int logits_elem_bytes(int32_t logits_dtype) { return logits_dtype == PCBENV_LOGITS_F32 ? 4 : 2; }
static int head_checks(pcbenv *env, const void *logits_dev, const int32_t *actions_dev, int32_t logits_dtype) {
    if (!logits_dev) return fail(env, PCBENV_EINVAL, "null logits");
    if (!actions_dev) return fail(env, PCBENV_EINVAL, "null actions");
    if (logits_dtype != PCBENV_LOGITS_F32 && logits_dtype != PCBENV_LOGITS_BF16) return fail(env, PCBENV_EINVAL, "unknown logits dtype");
    return PCBENV_OK;
}
static int logits_aligned(pcbenv *env, const void *logits_dev, int32_t logits_dtype) {
    if ((uintptr_t)logits_dev % logits_elem_bytes(logits_dtype) != 0)
        return fail(env, PCBENV_EINVAL, "logits pointer not aligned to its element size");
    return PCBENV_OK;
}
static int rows_checks(pcbenv *env, const uint64_t *mask_bits_dev, int64_t num_rows) {
    if (!mask_bits_dev) return fail(env, PCBENV_EINVAL, "null mask bits");
    if ((uintptr_t)mask_bits_dev % 8 != 0) return fail(env, PCBENV_EINVAL, "mask bits pointer not aligned to 8 bytes");
    if (num_rows < 0 || num_rows > INT32_MAX) return fail(env, PCBENV_EINVAL, "num_rows out of range");
    return PCBENV_OK;
}
static int grad_logits_checks(pcbenv *env, const void *grad_logits_dev, int32_t logits_dtype) {
    if (!grad_logits_dev) return fail(env, PCBENV_EINVAL, "null grad logits");
    if ((uintptr_t)grad_logits_dev % logits_elem_bytes(logits_dtype) != 0)
        return fail(env, PCBENV_EINVAL, "grad logits pointer not aligned to its element size");
    return PCBENV_OK;
}
// the checks pcbenv_sample_logits and pcbenv_evaluate_logits[_backward] share, and those of the three axis calls (the
// evaluate ones pass PCBENV_DRAW_SAMPLE)
static int logits_checks(pcbenv *env, const void *logits_dev, int32_t logits_dtype, const int32_t *actions_dev, int32_t fmt) {
    if (const int rc = head_checks(env, logits_dev, actions_dev, logits_dtype)) return rc;
    CHECK_ACTION_FORMAT(env, fmt);
    return logits_aligned(env, logits_dev, logits_dtype);
}
static int axis_checks(pcbenv *env, int32_t axis, uint32_t given, const void *logits_dev, int32_t logits_dtype, int32_t mode,
                       const int32_t *actions_dev) {
    if (const int rc = head_checks(env, logits_dev, actions_dev, logits_dtype)) return rc;
    if (mode != PCBENV_DRAW_SAMPLE && mode != PCBENV_DRAW_GREEDY) return fail(env, PCBENV_EINVAL, "unknown draw mode");
    if (axis != PCBENV_AXIS_ORIENTATION && axis != PCBENV_AXIS_X && axis != PCBENV_AXIS_Y) return fail(env, PCBENV_EINVAL, "unknown axis");
    if (given & ~7u) return fail(env, PCBENV_EINVAL, "given has a bit above 4");
    if (given & (1u << axis)) return fail(env, PCBENV_EINVAL, "given contains the axis itself");
    return logits_aligned(env, logits_dev, logits_dtype);
}
static EvalGeom eval_geom(const pcbenv *env, int64_t num_rows) {
    const DevParams &d = env->dp;
    return EvalGeom{d.O, d.H, d.W, d.WW, (int)num_rows};
}

// What the six do once their own arguments have passed.  `sampler`: the name of a function that reads the handle's current
// state set (null for the evaluate calls, which take geometry and device from the handle and nothing else): it needs
// bound buffers, and it cannot be captured -- a captured launch would keep reading the set that was current at capture
// time (as pcbenv_gather).  `no_rows`: the evaluate calls' num_rows == 0, a no-op behind the null handle.  `launch(s)`
// fills the launch struct and returns its launch function's value.  Nothing the library owns is written: no state block,
// presampled action, terminal list or queue, and no generator interaction (nothing is consumed).
template <class Launch>
static int policy_launch(pcbenv *env, const char *sampler, bool no_rows, void *stream, Launch launch) {
    if (!env) return fail(0, PCBENV_EINVAL, "null handle");
    if (sampler && !env->bound) return fail(env, PCBENV_ESTATE, "pcbenv_bind_buffers has not been called");
    if (no_rows) return PCBENV_OK;
    DEVICE_GUARD(env);
    hipStream_t s = (hipStream_t)stream;
    if (sampler && stream_capturing(s)) return fail(env, PCBENV_ESTATE, "%s cannot be captured into a graph", sampler);
    if (launched(env, launch(s))) return PCBENV_EHIP;
    HIP_TRY(env, hipGetLastError());
    return PCBENV_OK;
}

extern "C" int pcbenv_sample_logits(pcbenv *env, const void *logits_dev, int32_t logits_dtype, int32_t mode,
                                    int32_t *actions_dev, int32_t fmt, float *log_prob_dev, float *entropy_dev,
                                    uint32_t *errors_dev, uint64_t seed, uint64_t first_env_index, uint64_t step_index,
                                    void *stream) {
    if (const int rc = logits_checks(env, logits_dev, logits_dtype, actions_dev, fmt)) return rc;
    if (mode != PCBENV_DRAW_SAMPLE && mode != PCBENV_DRAW_GREEDY) return fail(env, PCBENV_EINVAL, "unknown draw mode");
    return policy_launch(env, "pcbenv_sample_logits", false, stream, [&](hipStream_t s) {
        SampleLogitsLaunch a;
        a.d = env->dp;  // d.state: the current state set, as k_sample reads it
        a.dtype = logits_dtype; a.stream = s;
        SampleLogitsArgs &g = a.g;
        g.logits = logits_dev; g.actions = actions_dev; g.log_prob = log_prob_dev; g.entropy = entropy_dev;
        g.errors = (unsigned *)errors_dev; g.seed = (u64)seed; g.first_env = (u64)first_env_index; g.step_index = (u64)step_index;
        g.fmt = fmt; g.greedy = mode == PCBENV_DRAW_GREEDY;
        return pcb_launch_sample_logits(a);
    });
}

extern "C" int pcbenv_evaluate_logits(const pcbenv *cenv, const void *logits_dev, int32_t logits_dtype,
                                      const uint64_t *mask_bits_dev, const int32_t *actions_dev, int32_t fmt,
                                      int64_t num_rows, float *log_prob_dev, float *entropy_dev, float *stats_dev,
                                      uint32_t *errors_dev, void *stream) {
    pcbenv *env = const_cast<pcbenv *>(cenv);  // the error text only
    if (const int rc = logits_checks(env, logits_dev, logits_dtype, actions_dev, fmt)) return rc;
    if (const int rc = rows_checks(env, mask_bits_dev, num_rows)) return rc;
    if ((uintptr_t)stats_dev % 16 != 0) return fail(env, PCBENV_EINVAL, "stats pointer not aligned to 16 bytes");
    return policy_launch(env, 0, num_rows == 0, stream, [&](hipStream_t s) {
        EvalLogitsLaunch a;
        a.q = eval_geom(env, num_rows); a.dtype = logits_dtype; a.stream = s;
        EvalLogitsArgs &g = a.g;
        g.logits = logits_dev; g.mask_bits = (const u64 *)mask_bits_dev; g.actions = actions_dev; g.log_prob = log_prob_dev;
        g.entropy = entropy_dev; g.stats = stats_dev; g.errors = (unsigned *)errors_dev; g.fmt = fmt;
        return pcb_launch_evaluate_logits(a);
    });
}

extern "C" int pcbenv_evaluate_logits_backward(const pcbenv *cenv, const void *logits_dev, int32_t logits_dtype,
                                               const uint64_t *mask_bits_dev, const int32_t *actions_dev, int32_t fmt,
                                               int64_t num_rows, const float *stats_dev, const float *grad_log_prob_dev,
                                               const float *grad_entropy_dev, void *grad_logits_dev, void *stream) {
    pcbenv *env = const_cast<pcbenv *>(cenv);  // the error text only
    if (const int rc = logits_checks(env, logits_dev, logits_dtype, actions_dev, fmt)) return rc;
    if (const int rc = rows_checks(env, mask_bits_dev, num_rows)) return rc;
    if (!stats_dev) return fail(env, PCBENV_EINVAL, "null stats");
    if ((uintptr_t)stats_dev % 16 != 0) return fail(env, PCBENV_EINVAL, "stats pointer not aligned to 16 bytes");
    if (const int rc = grad_logits_checks(env, grad_logits_dev, logits_dtype)) return rc;
    return policy_launch(env, 0, num_rows == 0, stream, [&](hipStream_t s) {
        EvalLogitsBackwardLaunch a;
        a.q = eval_geom(env, num_rows); a.dtype = logits_dtype; a.stream = s;
        EvalLogitsBackwardArgs &g = a.g;
        g.logits = logits_dev; g.mask_bits = (const u64 *)mask_bits_dev; g.actions = actions_dev; g.stats = stats_dev;
        g.grad_log_prob = grad_log_prob_dev; g.grad_entropy = grad_entropy_dev; g.grad_logits = grad_logits_dev; g.fmt = fmt;
        return pcb_launch_evaluate_logits_backward(a);
    });
}

// One stage of a factorised policy.
extern "C" int pcbenv_sample_axis(pcbenv *env, int32_t axis, uint32_t given, const void *logits_dev, int32_t logits_dtype,
                                  int32_t mode, int32_t *actions_dev, float *log_prob_dev, float *entropy_dev,
                                  uint32_t *errors_dev, uint64_t seed, uint64_t first_env_index, uint64_t step_index,
                                  void *stream) {
    if (const int rc = axis_checks(env, axis, given, logits_dev, logits_dtype, mode, actions_dev)) return rc;
    return policy_launch(env, "pcbenv_sample_axis", false, stream, [&](hipStream_t s) {
        SampleAxisLaunch a;
        a.d = env->dp;  // d.state: the current state set, as k_sample_logits reads it
        a.s = AxisStage{axis, given}; a.dtype = logits_dtype; a.stream = s;
        SampleAxisArgs &g = a.g;
        g.logits = logits_dev; g.actions = actions_dev; g.log_prob = log_prob_dev; g.entropy = entropy_dev;
        g.errors = (unsigned *)errors_dev; g.seed = (u64)seed; g.first_env = (u64)first_env_index; g.step_index = (u64)step_index;
        g.greedy = mode == PCBENV_DRAW_GREEDY;
        return pcb_launch_sample_axis(a);
    });
}

extern "C" int pcbenv_evaluate_axis(const pcbenv *cenv, int32_t axis, uint32_t given, const void *logits_dev,
                                    int32_t logits_dtype, const uint64_t *mask_bits_dev, const int32_t *actions_dev,
                                    int64_t num_rows, float *log_prob_dev, float *entropy_dev, uint32_t *errors_dev,
                                    void *stream) {
    pcbenv *env = const_cast<pcbenv *>(cenv);  // the error text only
    if (const int rc = axis_checks(env, axis, given, logits_dev, logits_dtype, PCBENV_DRAW_SAMPLE, actions_dev)) return rc;
    if (const int rc = rows_checks(env, mask_bits_dev, num_rows)) return rc;
    return policy_launch(env, 0, num_rows == 0, stream, [&](hipStream_t s) {
        EvalAxisLaunch a;
        a.q = eval_geom(env, num_rows); a.s = AxisStage{axis, given}; a.dtype = logits_dtype; a.stream = s;
        EvalAxisArgs &g = a.g;
        g.logits = logits_dev; g.mask_bits = (const u64 *)mask_bits_dev; g.actions = actions_dev; g.log_prob = log_prob_dev;
        g.entropy = entropy_dev; g.errors = (unsigned *)errors_dev;
        return pcb_launch_evaluate_axis(a);
    });
}

extern "C" int pcbenv_evaluate_axis_backward(const pcbenv *cenv, int32_t axis, uint32_t given, const void *logits_dev,
                                             int32_t logits_dtype, const uint64_t *mask_bits_dev, const int32_t *actions_dev,
                                             int64_t num_rows, const float *grad_log_prob_dev, const float *grad_entropy_dev,
                                             void *grad_logits_dev, void *stream) {
    pcbenv *env = const_cast<pcbenv *>(cenv);  // the error text only
    if (const int rc = axis_checks(env, axis, given, logits_dev, logits_dtype, PCBENV_DRAW_SAMPLE, actions_dev)) return rc;
    if (const int rc = rows_checks(env, mask_bits_dev, num_rows)) return rc;
    if (const int rc = grad_logits_checks(env, grad_logits_dev, logits_dtype)) return rc;
    return policy_launch(env, 0, num_rows == 0, stream, [&](hipStream_t s) {
        EvalAxisBackwardLaunch a;
        a.q = eval_geom(env, num_rows); a.s = AxisStage{axis, given}; a.dtype = logits_dtype; a.stream = s;
        EvalAxisBackwardArgs &g = a.g;
        g.logits = logits_dev; g.mask_bits = (const u64 *)mask_bits_dev; g.actions = actions_dev;
        g.grad_log_prob = grad_log_prob_dev; g.grad_entropy = grad_entropy_dev; g.grad_logits = grad_logits_dev;
        return pcb_launch_evaluate_axis_backward(a);
    });
}

extern "C" int pcbenv_queue_cursors(pcbenv *env, uint32_t *min_out, uint32_t *max_out, void *stream) {
    if (!env || !min_out || !max_out) return fail(env, PCBENV_EINVAL, "null argument");
    DEVICE_GUARD(env);
    if (!env->scratch) HIP_TRY(env, hipMalloc((void **)&env->scratch, 16));
    pcb_launch_cursor_range(env->dp, env->scratch, (hipStream_t)stream);
    unsigned host[2] = {0, 0};
    HIP_TRY(env, hipMemcpyAsync(host, env->scratch, 8, hipMemcpyDeviceToHost, (hipStream_t)stream));
    HIP_TRY(env, hipStreamSynchronize((hipStream_t)stream));
    *min_out = host[0]; *max_out = host[1];
    return PCBENV_OK;
}

#ifdef PCBENV_STAMPS
extern "C" int pcbenv_debug_stamps(pcbenv *env, unsigned long long *host) {  // diagnostic build only
    if (!env || !env->dp.dbg) return -1;
    hipDeviceSynchronize();
    const size_t rows = (size_t)env->dp.B + (size_t)env->dp.term_cap * (REWARD_PARTS + 1);  // environments, then the helpers
    const int rc = hipMemcpy(host, env->dp.dbg, rows * 32 * 8, hipMemcpyDeviceToHost) == hipSuccess ? 0 : -3;
    hipMemset(env->dp.dbg, 0, rows * 32 * 8);
    return rc;
}
#endif
