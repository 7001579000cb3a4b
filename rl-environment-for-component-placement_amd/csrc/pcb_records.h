// pcb_records.h -- the plain data the host side and the kernels of libpcbenv.so share: the device-side parameter block (kernel
// argument) and the records of a state block.  Plain C++17 (it includes only pcbenv.h and pcb_layout.h), like pcb_layout.h: the
// host units and pcb_launch.h take it from here, the kernels through pcb_device.h, and the CPU checks under tools/ compile the same text.
#pragma once
#include "pcbenv.h"
#include "pcb_layout.h"  // WAVE, HDR_BYTES, TERM_*: every size and offset the host side and the kernels share

typedef unsigned long long u64;

// device-side parameter block (kernel argument, by value)
// The layout fields (offOcc ... ldsHfWords) are pcb_layout::Layout's, copied by derive_layout (pcb_config.hip).
// The kernel-argument offsets of the fields must stay put: every wavefront starts by loading the fields it needs from
// the kernel-argument segment with scalar loads the compiler groups by offset, so adding, removing or moving a field
// regroups those loads and shifts the register allocation of every kernel -- a change to be measured like a kernel
// change, never a side effect of tidying the host side.
struct DevParams {
    int kind, H, W, WW, O, C, P, N, K, mp, mh, mw, F, pinRows, catW, B, Q;
    int reward_type, beam_width, component_n;
    unsigned flags, bind_gen;
    double w_wl, w_int, max_wl, max_int, wl_norm, int_norm, area;
    long long stateStride, instStride;
    int offOcc, offVm, offComps, offPins, offRank;   // byte offsets inside a state block
    int ldsHf, ldsCls, ldsSeg, ldsBytes;    // byte offsets of LDS scratch behind the state mirror
    int ldsHfWords;                         // 64-bit words of the fold scratch / row-membership bit map at ldsHf (sized by need)
    unsigned char *state, *queue;
    pcbenv_buffers buf;
    pcbenv_compact_features cbuf;           // compact feature tensors of the trajectory layout (all null unless bound)
    // episode-constant observation bytes per environment (spatial, trajectory layout; pcb_observe.h feat_cache_*)
    unsigned char *feat_cache; unsigned *feat_cache_tag; int featCacheStride, featCacheCg;
    unsigned long long *dbg;                // diagnostic build only (-DPCBENV_STAMPS): [B][32] s_memtime stamps
    int stream_stores;                      // observation stores bypass the caches (`nt`): see STORE16.  (Behind the
                                            // fields every wave loads first, so that their kernarg offsets stay put.)
    // Trajectory layout (pcbenv_bind_buffers_slots): every bound tensor is [num_slots, B, ...]; a launch writes its
    // outputs into `slot` (the persistent rollout kernel: one slot per step).  With num_slots > 1 nothing may rely on
    // what an earlier step left in the destination, so the float64 feature tensors are written whole every step.
    int num_slots, slot;
    // on-device instance generator (pcb_geninst.h), null when the host feeds the queue: records generated so far per
    // environment, and a sticky error word a reset raises if it ever finds its record missing (it never should:
    // the host-side bookkeeping of pcb_gen.hip orders every fill before the launches that can consume it)
    unsigned *gen_produced, *gen_errors;
    // Queue cursor of every environment, published with agent-scope (write-through) stores at each reset.  The copy
    // in the state block is written back lazily and only ever re-read on the environment's own XCD; a kernel on
    // another stream (k_gen_fill) may run on any XCD, whose L2 is not coherent with the writer's.
    unsigned *cursor_pub;
    // Terminal list (Team<>::run_env has the story): `seq` numbers the step launches of this handle; launch seq starts
    // REWARD_PARTS helper teams for each of the first term_wgs entries of ring seq & 3, appends to ring (seq + 1) & 3 and
    // clears the counters of ring (seq + 2) & 3.  A ring is TERM_SHARDS shards of term_cap / TERM_SHARDS entries, each with
    // a counter on a line of its own (term_cnt[(ring * TERM_SHARDS + shard) * TERM_CNT_STRIDE]); entry (shard, idx) has
    // the number idx * TERM_SHARDS + shard.  term_cap == 0: no lists are kept; term_wgs == 0: this launch has no helpers.
    unsigned seq;
    int term_wgs, term_cap, term_hpe;  // term_hpe = helper teams per entry: REWARD_PARTS, + 1 feature helper with PCBENV_FLAG_AUTO_RESET
    int *term_list;
    unsigned *term_cnt;
    u64 *term_arrive;  // [term_cap]: where the shares of a routing reward meet (terminal_reward)
    unsigned *term_seen;  // host memory: the longest shard of the latest launch's list (sizes later helper grids)
    unsigned char *state_out;  // the state blocks this launch writes (p.state: the ones it reads); equal for in-place kernels
};

// per-environment header at the start of a state block
struct __attribute__((aligned(16))) EnvHdr {
    short ncomp, nnets, npins, cur;  // cur = index of the current component, -1 = sentinel (all placed)
    unsigned episode;                // completed resets
    unsigned qcursor;                // next queue slot
    unsigned flag;                   // LDS scratch word: workgroup-wide any(), and y of the sampled action
    unsigned pad[2];                 // LDS scratch: (o, x) of the action drawn by wavefront 0 (fused sampler)
    unsigned feat_gen;               // bind generation for which the pin-feature tensors hold only this env's rows
    // Action of the NEXT fused-sampler step, drawn at the end of the launch that produced the mask (while its
    // stores drain) instead of at the head of the next launch, where the whole grid would wait for it.  Valid
    // (bit 31 of pre_action) only for exactly this (seed, step index, global env index) and only while vm is the
    // mask it was drawn from: every launch that rewrites vm redraws or clears it.
    u64 pre_seed, pre_step;
    unsigned pre_action;             // o | x << 8 | y << 16 | 1 << 31
    unsigned pre_genv;
    // Terminal list (run_env): the launch number for which this environment sits on the list of environments that are
    // certain to end their episode, and its entry there; anything else = not listed.
    unsigned term_seq, term_pos;
};
static_assert(sizeof(EnvHdr) == HDR_BYTES, "header size");
static_assert(PCBENV_MAX_SIDE <= 128, "EnvHdr::pre_action: x and y in 8 bits each; CompRec::px / py, PinRec::abs_x / abs_y: signed char");

// 8-byte records (state block and instance wire format share the pin layout up to abs_x/abs_y)
struct CompRec { unsigned char h, w; signed char px, py; unsigned char o, pad[3]; };  // o = orientation it was placed with
struct PinRec { unsigned char rel_x, rel_y; signed char abs_x, abs_y; unsigned char net, comp; unsigned short id; };
#define PIN_ID_MASK 0x7FFF
#define PIN_LOSER 0x8000  // pin env quirk Q1: a later pin of the same component shares this feature row
// PinRec::id is a row of the pin feature tensors (spatial: the global pin id; pin: the id inside the component) and
// PinTables::pid keeps one in 16 bits with 0xFFFF for "none": the largest pinRows (spatial: C * mp + 1) stays below both
static_assert(PCBENV_MAX_COMPONENTS * PCBENV_MAX_PINS_PER_COMPONENT + 1 <= PIN_ID_MASK && PIN_ID_MASK < 0xFFFF, "PinRec::id & PIN_ID_MASK, PinTables::pid");
static_assert(PCBENV_MAX_COMPONENTS <= 0xFF && PCBENV_MAX_NETS <= 0xFF, "PinRec::comp / net: unsigned char, 0xFF = no pin in this slot (reset_env)");
