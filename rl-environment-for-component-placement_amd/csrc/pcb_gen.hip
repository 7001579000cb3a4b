// pcb_gen.hip -- the on-device instance generator's host side: its kernels (pcb_geninst.h, compiled here and nowhere
// else in the library), the stream protocol that orders every fill before the launches that can consume it, and the
// generator's share of enable / destroy / checkpoint.  Everything the generator acquires lives in the handle's gen_*
// fields, cursor_snap, gen_stream and the two events; gen_release is the only place that gives them back.
#include <vector>

#include "pcb_host.h"
#include "pcb_geninst.h"

// k_gen_seed / k_gen_fill's argument, from the handle (the queue cursors the kernels see are the snapshot's)
static GenParams gen_params(const pcbenv *env) {
    const DevParams &d = env->dp;
    const pcbenv_config &c = env->cfg;
    GenParams g{};
    g.kind = c.kind; g.C = d.C; g.P = d.P; g.Q = d.Q; g.B = d.B;
    g.min_comp = c.min_num_components; g.max_comp = c.max_num_components;
    g.min_h = c.min_component_h; g.max_h = c.max_component_h; g.min_w = c.min_component_w; g.max_w = c.max_component_w;
    g.min_nets = c.min_num_nets; g.max_nets = c.max_num_nets; g.min_ppn = c.min_num_pins_per_net; g.max_ppn = c.max_num_pins_per_net;
    g.net_distribution = c.net_distribution; g.pin_spread = c.pin_spread;  // clipped at create like the reference does
    g.instStride = d.instStride; g.queue = d.queue;
    g.cursor_pub = env->cursor_snap; g.gen = env->gen_state; g.produced = env->gen_produced;
    return g;
}

// ---- host protocol ------------------------------------------------------------------------------------------
// k_gen_fill runs on env->gen_stream, ordered after everything enqueued on the caller's stream at its snapshot
// (ev_snap): when it has completed, every environment holds queue_depth records ahead of the cursor it had at the
// snapshot.  A launch may consume at most n records per environment (one per reset, one per step with
// PCBENV_FLAG_AUTO_RESET, num_steps per rollout), so a launch is safe as long as the launches since the snapshot of
// the last fill the caller's stream has waited for add up to at most queue_depth; `since_waited` keeps that sum.
// Fills are started early (half of the queue consumed at worst; fewer, larger refills cost the step kernels less than
// many small ones) and waited for late, so they overlap the step
// kernels; the wait is a stream-side event wait, never a host synchronisation.
// one refill launch: 64 / G environments per wavefront (gen_group_lanes), capped grid
static void gen_launch_fill(pcbenv *env, hipStream_t s, bool whole_batch) {
    const DevParams &d = env->dp;
    const int G = gen_group_lanes(d.C, env->cfg.max_num_nets, d.P, env->gen_lanes), epw = WAVE / G;
    int grid = (d.B + epw - 1) / epw;
    if (!whole_batch && grid > env->gen_grid) grid = env->gen_grid;
    const size_t lds = GEN_LDS_BYTES(d.instStride, G);
    const GenParams gp = gen_params(env);
    if (G == 16) hipLaunchKernelGGL(k_gen_fill<16>, dim3(grid), dim3(WAVE), lds, s, gp);
    else if (G == 32) hipLaunchKernelGGL(k_gen_fill<32>, dim3(grid), dim3(WAVE), lds, s, gp);
    else hipLaunchKernelGGL(k_gen_fill<64>, dim3(grid), dim3(WAVE), lds, s, gp);
}
static void gen_start_fill(pcbenv *env, hipStream_t main) {
    // The fill works from a copy of the published cursors taken in stream order: it learns of a reset only once the launch
    // that made it has COMPLETED, so a record is never overwritten while a team of a running launch may still be reading it
    // (an environment's own team publishes its cursor as soon as it has its copy; its feature helper reads the same record).
    hipMemcpyAsync(env->cursor_snap, env->dp.cursor_pub, 4 * (size_t)env->dp.B, hipMemcpyDeviceToDevice, main);
    hipEventRecord(env->ev_snap, main);
    hipStreamWaitEvent(env->gen_stream, env->ev_snap, 0);
    gen_launch_fill(env, env->gen_stream, false);
    hipEventRecord(env->ev_fill, env->gen_stream);
    env->gen_outstanding = true;
    env->since_outstanding = 0;
}
int gen_before_launch(pcbenv *env, int n, hipStream_t main) {
    if (!env->gen_on) return PCBENV_OK;
    const long long Q = env->dp.Q;
    if (n > Q) return fail(env, PCBENV_ELIMIT, "this launch may consume more instances per environment than queue_depth holds");
    if (env->since_waited + n > Q) {
        if (!env->gen_outstanding) gen_start_fill(env, main);
        hipStreamWaitEvent(main, env->ev_fill, 0);
        env->since_waited = env->since_outstanding;
        env->gen_outstanding = false;
        if (env->since_waited + n > Q) {  // that fill was snapshotted too long ago for this launch: one more, in stream order
            gen_start_fill(env, main);
            hipStreamWaitEvent(main, env->ev_fill, 0);
            env->since_waited = 0;
            env->gen_outstanding = false;
        }
    }
    return PCBENV_OK;
}
void gen_after_launch(pcbenv *env, int n, hipStream_t main) {
    if (!env->gen_on) return;
    env->since_waited += n;
    if (env->gen_outstanding) env->since_outstanding += n;
    else if (env->since_waited * 2 >= env->dp.Q) gen_start_fill(env, main);
}
// the quiescent point: nothing in flight, every launch since then counted from zero
static void gen_reset_counters(pcbenv *env) { env->gen_outstanding = false; env->since_waited = 0; env->since_outstanding = 0; }
// Brings the queue fully up to date (queue_depth records ahead of every cursor as of `main`) and waits for it.  A fill
// that is still outstanding reads cursor_snap: the new snapshot is ordered behind it, as in gen_before_launch.
static int gen_quiesce(pcbenv *env, hipStream_t main) {
    if (env->gen_outstanding) hipStreamWaitEvent(main, env->ev_fill, 0);
    gen_start_fill(env, main);
    HIP_TRY(env, hipStreamSynchronize(env->gen_stream));
    gen_reset_counters(env);
    return PCBENV_OK;
}

// ---- enable / release ---------------------------------------------------------------------------------------
void gen_release(pcbenv *env) {
    if (env->gen_stream) hipStreamSynchronize(env->gen_stream);
    if (env->ev_snap) hipEventDestroy(env->ev_snap);
    if (env->ev_fill) hipEventDestroy(env->ev_fill);
    if (env->gen_stream) hipStreamDestroy(env->gen_stream);
    if (env->gen_state) hipFree(env->gen_state);
    if (env->gen_produced) hipFree(env->gen_produced);
    if (env->cursor_snap) hipFree(env->cursor_snap);
    env->ev_snap = env->ev_fill = 0; env->gen_stream = 0;
    env->gen_state = 0; env->gen_produced = 0; env->cursor_snap = 0;
    env->dp.gen_produced = env->dp.gen_errors = 0;
    env->gen_on = false;
}
// Acquires into the handle's fields (and *seeds_dev) and fills the whole queue; the caller releases on failure.
static int gen_acquire(pcbenv *env, const uint32_t *seeds_host, hipStream_t s, unsigned **seeds_dev) {
    const size_t B = (size_t)env->dp.B;
    HIP_TRY(env, hipMalloc((void **)&env->cursor_snap, 4 * B));
    HIP_TRY(env, hipMemcpyAsync(env->cursor_snap, env->dp.cursor_pub, 4 * B, hipMemcpyDeviceToDevice, s));
    HIP_TRY(env, hipMalloc((void **)&env->gen_state, sizeof(GenState) * B));
    HIP_TRY(env, hipMalloc((void **)&env->gen_produced, 4 * B + 4));  // the error word sits one word behind the counters
    HIP_TRY(env, hipMalloc((void **)seeds_dev, 4 * B));
    HIP_TRY(env, hipMemcpyAsync(*seeds_dev, seeds_host, 4 * B, hipMemcpyHostToDevice, s));
    {   // lowest priority: when both queues have workgroups to place, the step kernel's go first
        int lo_prio = 0, hi_prio = 0;
        HIP_TRY(env, hipDeviceGetStreamPriorityRange(&lo_prio, &hi_prio));
        HIP_TRY(env, hipStreamCreateWithPriority(&env->gen_stream, hipStreamNonBlocking, lo_prio));
    }
    HIP_TRY(env, hipEventCreateWithFlags(&env->ev_snap, hipEventDisableTiming));
    HIP_TRY(env, hipEventCreateWithFlags(&env->ev_fill, hipEventDisableTiming));
    const dim3 grid((env->dp.B + WAVE - 1) / WAVE);
    hipLaunchKernelGGL(k_gen_seed, grid, dim3(WAVE), 0, s, gen_params(env), *seeds_dev);
    gen_launch_fill(env, s, true);  // the whole queue, before anything can consume it
    HIP_TRY(env, hipGetLastError());
    HIP_TRY(env, hipStreamSynchronize(s));
    HIP_TRY(env, hipMemsetAsync(env->gen_produced + B, 0, 4, s));
    HIP_TRY(env, hipStreamSynchronize(s));  // enable is synchronous w.r.t. `stream`: the next call may come on another one
    return PCBENV_OK;
}
extern "C" int pcbenv_instgen_device_enable(pcbenv *env, const uint32_t *seeds_host, void *stream) {
    if (!env || !seeds_host) return fail(env, PCBENV_EINVAL, "null argument");
    if (env->cfg.kind == PCBENV_SQUARE) return fail(env, PCBENV_EINVAL, "the square environment has no instances");
    if (env->gen_on) return fail(env, PCBENV_ESTATE, "the on-device generator is already enabled");
    DEVICE_GUARD(env);
    unsigned *seeds_dev = 0;
    const int rc = gen_acquire(env, seeds_host, (hipStream_t)stream, &seeds_dev);
    if (seeds_dev) hipFree(seeds_dev);
    if (rc != PCBENV_OK) { gen_release(env); return rc; }  // as before the call: enable may be tried again
    env->dp.gen_produced = env->gen_produced;
    env->dp.gen_errors = env->gen_produced + env->dp.B;
    if (env->gen_grid < 1) env->gen_grid = GEN_MAX_GRID;  // unless PCBENV_OPT_GEN_GRID set it
    gen_reset_counters(env);
    env->gen_on = true;
    return PCBENV_OK;
}

extern "C" int pcbenv_instgen_device_status(pcbenv *env, uint32_t *errors_out, void *stream) {
    if (!env || !errors_out) return fail(env, PCBENV_EINVAL, "null argument");
    if (!env->gen_on) return fail(env, PCBENV_ESTATE, "the on-device generator is not enabled");
    DEVICE_GUARD(env);
    const int rc = gen_quiesce(env, (hipStream_t)stream);
    if (rc != PCBENV_OK) return rc;
    unsigned err = 0;
    HIP_TRY(env, hipMemcpyAsync(&err, env->dp.gen_errors, 4, hipMemcpyDeviceToHost, (hipStream_t)stream));
    HIP_TRY(env, hipStreamSynchronize((hipStream_t)stream));
    std::vector<int> status((size_t)env->dp.B);  // first failing record of any stream (the reference raises there)
    HIP_TRY(env, hipMemcpy2D(status.data(), 4, &env->gen_state->status, sizeof(GenState), 4, (size_t)env->dp.B, hipMemcpyDeviceToHost));
    for (int i = 0; i < env->dp.B; i++) if (status[(size_t)i] != 0) { err |= 2u; break; }
    *errors_out = err;
    return PCBENV_OK;
}

// ---- checkpoint ---------------------------------------------------------------------------------------------
// The generator's streams, counters and records are part of what a resumed run continues from.
struct GenSection { void *dev; size_t bytes; };
static int gen_sections(const pcbenv *env, GenSection out[3]) {
    if (!env->gen_on) return 0;
    const size_t B = (size_t)env->dp.B;
    out[0] = {env->gen_state, sizeof(GenState) * B};
    out[1] = {env->gen_produced, 4 * B};
    out[2] = {env->dp.queue, (size_t)env->dp.instStride * B * (size_t)env->dp.Q};
    return 3;
}
size_t gen_section_bytes(const pcbenv *env) {
    GenSection sec[3];
    size_t bytes = 0;
    for (int i = 0, n = gen_sections(env, sec); i < n; i++) bytes += sec[i].bytes;
    return bytes;
}
// Brings the queue to its quiescent point first (the state a restore re-creates), then copies on the generator's
// stream, in order behind its kernels.
int gen_save(pcbenv *env, unsigned char *host_dst, hipStream_t main) {
    GenSection sec[3];
    const int n = gen_sections(env, sec);
    if (n == 0) return PCBENV_OK;
    const int rc = gen_quiesce(env, main);
    if (rc != PCBENV_OK) return rc;
    for (int i = 0; i < n; host_dst += sec[i++].bytes)
        HIP_TRY(env, hipMemcpyAsync(host_dst, sec[i].dev, sec[i].bytes, hipMemcpyDeviceToHost, env->gen_stream));
    HIP_TRY(env, hipStreamSynchronize(env->gen_stream));
    return PCBENV_OK;
}
// The caller has made sure that nothing of the generator is in flight; the copies are enqueued on `main`.
int gen_restore(pcbenv *env, const unsigned char *host_src, hipStream_t main) {
    GenSection sec[3];
    const int n = gen_sections(env, sec);
    for (int i = 0; i < n; host_src += sec[i++].bytes)
        HIP_TRY(env, hipMemcpyAsync(sec[i].dev, host_src, sec[i].bytes, hipMemcpyHostToDevice, main));
    if (n) gen_reset_counters(env);
    return PCBENV_OK;
}
