// pcb_host.h -- what the host-side units of libpcbenv.so share: the handle, error reporting, the device guard and the
// functions one unit provides to another.  pcbenv_api.hip is the C ABI (include/pcbenv.h), pcb_config.hip turns a
// configuration into a layout, pcb_gen.hip owns the on-device instance generator.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include "pcbenv.h"
#include "pcb_records.h"

#pragma GCC visibility push(hidden)  // internal to the library: only include/pcbenv.h is exported from these units

struct GenState;  // pcb_geninst.h (pcb_gen.hip only)

struct pcbenv {
    pcbenv_config cfg;
    int device;
    DevParams dp;
    bool bound;
    int threads;  // workgroup size (threads per environment)
    long long cell_bytes_per_env, stream_threshold;  // store policy (see STORE16): cell-tensor bytes one transition writes per environment
    unsigned *scratch;  // 16 bytes of device memory for small read-backs
    unsigned long long loaded_slots[4];  // bit s = slot s loaded for all environments at least once
    // on-device instance generator (pcb_gen.hip): side stream + the bookkeeping that guarantees a record is complete
    // before any launch can consume it (see gen_before_launch).  gen_release is the one place that gives these back.
    bool gen_on, gen_outstanding;
    int gen_grid;  // workgroups of a refill launch (GEN_MAX_GRID; PCBENV_GEN_GRID overrides, for experiments)
    GenState *gen_state;     // [B] the two MT19937 streams of every environment
    unsigned *gen_produced;  // [B] records generated so far, + the error word (DevParams::gen_produced / gen_errors once enabled)
    unsigned *cursor_snap;   // the cursors as of a fill's snapshot: what k_gen_fill reads (see gen_start_fill)
    hipStream_t gen_stream;
    hipEvent_t ev_snap, ev_fill;
    long long since_waited, since_outstanding;
    int gen_lanes;      // PCBENV_OPT_GEN_LANES: 0 = the narrowest group the configuration allows
    // terminal list (run_env, pcb_step.h): launch counter, list entries that get helper teams per launch (0 = none)
    unsigned seq;
    int term_wgs;
    unsigned *term_seen_host;     // mapped host memory the step kernel reports its list length to (DevParams::term_seen)
    unsigned char *state_buf[2];  // double-buffered state blocks: dp.state is the current one, a step launch writes the other
    int state_cur;
    // Set by the first step launch captured into a hipGraph, for the rest of the handle's life: the graph works on
    // state_buf[state_cur] in place, so from then on every launch does (no buffer swap, no helpers) -- see dispatch_step.
    bool in_place;
    // The geometry-fixed build of k_step (pcb_layout::fixed_geometry_applies): PCBENV_OPT_FIXED_GEOMETRY, and whether every
    // cell tensor of the current binding starts at a 16-byte boundary (pcbenv_bind_buffers_slots looks once).
    bool fixed_geometry, cells_aligned16;
    unsigned char *gather_snap;   // pcbenv_gather within one handle: reward | info | done of the selected slot before the launch
    bool has_episode;  // a reset, a gather or a restored checkpoint has put episodes into the state blocks (pcbenv_playout asks)
    char err[256];
};

// Records the message in the handle (and for pcbenv_last_error(NULL)) and returns `code`.  Defined in pcbenv_api.hip.
int fail(pcbenv *env, int code, const char *fmt, const char *detail = "");
#define HIP_TRY(env, call)                                                          \
    do {                                                                            \
        hipError_t e_ = (call);                                                     \
        if (e_ != hipSuccess) return fail(env, PCBENV_EHIP, #call ": %s", hipGetErrorString(e_)); \
    } while (0)

// Every entry point works on the handle's device and leaves the caller's current device as it found it.
struct DeviceGuard {
    int prev = -1; bool ok = true, changed = false;
    explicit DeviceGuard(int dev) {
        if (hipGetDevice(&prev) != hipSuccess) prev = -1;
        if (prev != dev) { ok = hipSetDevice(dev) == hipSuccess; changed = ok && prev >= 0; }
    }
    ~DeviceGuard() { if (changed) (void)hipSetDevice(prev); }
};
#define DEVICE_GUARD(env) DeviceGuard guard_((env)->device); if (!guard_.ok) return fail(env, PCBENV_EHIP, "hipSetDevice failed")

using pcb_layout::align16;
using pcb_layout::is_pin_kind;
static inline bool action_format_ok(int fmt) { return fmt == PCBENV_ACTION_TUPLE || fmt == PCBENV_ACTION_FLAT; }
#define CHECK_ACTION_FORMAT(env, fmt) do { if (!action_format_ok(fmt)) return fail(env, PCBENV_EINVAL, "unknown action format"); } while (0)
static inline bool stream_capturing(hipStream_t s) {
    hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
    return hipStreamIsCapturing(s, &cap) == hipSuccess && cap != hipStreamCaptureStatusNone;
}

// Store policy of the cell tensors (see STORE16): streaming stores once the bytes a launch's destination spans -- one
// transition in place, all `slots` slots of the trajectory layout -- go beyond the threshold.
static inline int stream_stores(const pcbenv *env, int slots) {
    return env->cell_bytes_per_env * env->dp.B * slots > env->stream_threshold;
}

// ---- pcb_config.hip --------------------------------------------------------------------------------------------
int validate(const pcbenv_config *c);                      // the reference constructors' checks, then this library's limits
void derive_layout(const pcbenv_config &c, pcbenv *env);   // env->dp, threads, store policy, terminal-list capacity; no HIP call
int check_records(pcbenv *env, const void *host_tables, int n);  // pcbenv_load_instances: n records against the configuration

// ---- pcb_gen.hip -----------------------------------------------------------------------------------------------
// Around every launch that may consume up to n instance records per environment (both are no-ops while the generator is off).
int gen_before_launch(pcbenv *env, int n, hipStream_t main);
void gen_after_launch(pcbenv *env, int n, hipStream_t main);
void gen_release(pcbenv *env);  // everything pcbenv_instgen_device_enable acquired; safe on a handle that never enabled it
// The generator's section of a checkpoint (empty while it is off): GenState x B | produced, uint32 x B | the instance queue.
size_t gen_section_bytes(const pcbenv *env);
int gen_save(pcbenv *env, unsigned char *host_dst, hipStream_t main);          // quiesces first
int gen_restore(pcbenv *env, const unsigned char *host_src, hipStream_t main);  // a checkpoint is taken at the quiescent point

#pragma GCC visibility pop
