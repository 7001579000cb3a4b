// pcb_config.hip -- from a configuration to a layout: the reference constructors' validation, the sizes of the wire
// format, everything pcbenv_create derives before it allocates (derive_layout), and the instance-record checker of
// pcbenv_load_instances.  Host arithmetic only: no HIP call, no kernel.
#include <math.h>
#include <stdlib.h>

#include "pcb_host.h"  // with pcb_layout.h: the state-block and LDS layout the kernels index by

extern "C" int32_t pcbenv_max_total_pins(const pcbenv_config *c) {
    if (!c || !is_pin_kind(c->kind)) return 0;
    long long a = (long long)c->max_num_pins_per_net * c->max_num_nets;
    long long b = (long long)c->max_num_components * c->max_component_h * c->max_component_w;
    return (int32_t)(a < b ? a : b);
}
extern "C" int64_t pcbenv_instance_stride(const pcbenv_config *c) {
    if (!c || c->kind == PCBENV_SQUARE) return 0;
    return 16 + 8ll * (c->max_num_components + pcbenv_max_total_pins(c));
}

// The reference constructors' checks (quirk Q6), then the HIP path's limits.
int validate(const pcbenv_config *c) {
    if (c->kind < PCBENV_SQUARE || c->kind > PCBENV_SPATIAL) return fail(0, PCBENV_EINVAL, "unknown environment kind");
    if (c->height < 0 || c->width < 0) return fail(0, PCBENV_EINVAL, "Grid size must not be negative.");
    if (c->num_envs < 1) return fail(0, PCBENV_EINVAL, "num_envs must be at least 1");
    if (c->kind == PCBENV_SQUARE) {
        if (c->component_n > c->height || c->component_n > c->width)
            return fail(0, PCBENV_EINVAL, "Component size must not exceed the grid size.");
        if (c->component_n < 1) return fail(0, PCBENV_ELIMIT, "component_n must be at least 1");
    } else {
        bool too_big = c->kind == PCBENV_PIN ? (c->max_component_w > c->width || c->max_component_h > c->height)
                                             : (c->max_component_w > c->height || c->max_component_h > c->width);
        if (too_big) return fail(0, PCBENV_EINVAL, "Component size must not exceed the grid size.");
        if (c->min_component_w < 1 || c->min_component_h < 1) return fail(0, PCBENV_EINVAL, "Component size must be at least 1.");
        if (c->max_num_components < 1 || c->max_num_components > c->height * c->width)
            return fail(0, PCBENV_EINVAL, "Number of components must be in [1, grid area].");
    }
    if (c->kind == PCBENV_PIN) {
        if (c->min_num_pins_per_net > c->max_num_pins_per_net) return fail(0, PCBENV_EINVAL, "min_num_pins_per_net must not exceed max_num_pins_per_net.");
        if (c->min_num_pins_per_net < 2) return fail(0, PCBENV_EINVAL, "min_num_pins_per_net must be at least 2.");
        if (c->min_num_pins_per_net * c->min_num_nets > c->min_component_w * c->min_component_h * c->min_num_components)
            return fail(0, PCBENV_EINVAL, "min_num_pins_per_net * min_num_nets exceeds the minimum total component area.");
        if (c->reward_beam_width < 1) return fail(0, PCBENV_EINVAL, "Beam width must be a positive integer.");
        if (c->reward_type < 0 || c->reward_type > 2) return fail(0, PCBENV_EINVAL, "Reward type must be 'beam', 'centroid' or 'both'.");
    }
    if (c->kind == PCBENV_SPATIAL) {
        if (c->reward_type < 0 || c->reward_type > 2) return fail(0, PCBENV_EINVAL, "Reward type must be 'beam', 'centroid' or 'both'.");
        if (c->reward_beam_width < 2 || c->reward_beam_width > c->max_num_pins_per_net)
            return fail(0, PCBENV_EINVAL, "Beam width must be an integer in [2, max_num_pins_per_net].");
        if (c->weight_wirelength < 0) return fail(0, PCBENV_EINVAL, "weight_wirelength must not be negative.");
    }
    // limits of this implementation
    if (c->height < 1 || c->width < 1 || c->height > PCBENV_MAX_SIDE || c->width > PCBENV_MAX_SIDE)
        return fail(0, PCBENV_ELIMIT, "grid side must be in [1, 128]");
    if (c->queue_depth < 1 || c->queue_depth > 256) return fail(0, PCBENV_ELIMIT, "queue_depth must be in [1, 256]");
    if (c->kind != PCBENV_SQUARE) {
        int side = c->max_component_h > c->max_component_w ? c->max_component_h : c->max_component_w;
        int shorter = c->height < c->width ? c->height : c->width;
        if (side > shorter) return fail(0, PCBENV_ELIMIT, "a component side exceeds the shorter grid side (the reference raises inside convolve2d)");
        if (c->max_num_components > PCBENV_MAX_COMPONENTS) return fail(0, PCBENV_ELIMIT, "too many components");
        if (c->min_num_components < 1 || c->min_num_components > c->max_num_components) return fail(0, PCBENV_ELIMIT, "min_num_components must be in [1, max_num_components]");
        if (c->min_component_h > c->max_component_h || c->min_component_w > c->max_component_w) return fail(0, PCBENV_ELIMIT, "min component size exceeds max");
    }
    if (is_pin_kind(c->kind)) {
        if (pcbenv_max_total_pins(c) > PCBENV_MAX_PINS || c->max_num_nets > PCBENV_MAX_NETS) return fail(0, PCBENV_ELIMIT, "too many pins or nets");
        if (c->max_num_pins_per_net > PCBENV_MAX_PINS_PER_NET) return fail(0, PCBENV_ELIMIT, "too many pins per net");
        if (c->max_component_h * c->max_component_w > PCBENV_MAX_PINS_PER_COMPONENT) return fail(0, PCBENV_ELIMIT, "too many pins per component");
        if (c->min_num_pins_per_net < 1 || c->min_num_nets < 1 || c->min_num_nets > c->max_num_nets) return fail(0, PCBENV_ELIMIT, "nets / pins per net must be at least 1");
        if (c->reward_type != PCBENV_REWARD_CENTROID && c->reward_beam_width > PCBENV_MAX_BEAM_WIDTH) return fail(0, PCBENV_ELIMIT, "beam width above 4");
    }
    return PCBENV_OK;
}

static double mean2(int a, int b) { return (double)(a + b) / 2.0; }

// Everything of the handle that follows from the configuration alone: DevParams geometry, reward normalisers, threads
// per environment, state-block offsets, LDS zones, store policy and terminal-list capacity.
void derive_layout(const pcbenv_config &c, pcbenv *env) {
    DevParams &d = env->dp;
    d.kind = c.kind; d.H = c.height; d.W = c.width; d.WW = (c.width + 63) / 64;  // (= pcb_layout::Layout::WW)
    d.O = c.kind == PCBENV_SQUARE ? 1 : c.kind == PCBENV_RECT ? 2 : 4;
    d.C = c.kind == PCBENV_SQUARE ? 0 : c.max_num_components;
    d.P = pcbenv_max_total_pins(&c);
    d.N = is_pin_kind(c.kind) ? c.max_num_nets : 0; d.K = d.N + 1;
    d.mh = c.max_component_h; d.mw = c.max_component_w; d.mp = d.mh * d.mw;
    d.F = c.kind == PCBENV_SPATIAL ? 5 + d.mp : 5;
    d.pinRows = c.kind == PCBENV_PIN ? d.C * d.mp : c.kind == PCBENV_SPATIAL ? d.C * d.mp + 1 : 0;
    d.catW = c.kind == PCBENV_SPATIAL ? 2 : 1;
    d.B = c.num_envs; d.Q = c.queue_depth;
    d.reward_type = c.reward_type; d.beam_width = c.reward_beam_width; d.component_n = c.component_n;
    d.flags = c.flags;
    {   // streaming stores when one launch writes well beyond the 256 MiB Infinity Cache (see STORE16)
        const long long cells = (long long)c.height * c.width;
        const long long per_env = (c.flags & PCBENV_FLAG_INCREMENTAL_OBS) ? cells * d.O : cells * (1 + d.O + (c.kind == PCBENV_SPATIAL ? d.K : 0));
        env->cell_bytes_per_env = per_env; env->stream_threshold = 256ll << 20;  // PCBENV_OPT_STREAM_THRESHOLD_BYTES
        d.stream_stores = stream_stores(env, 1);
    }
    d.w_wl = c.weight_wirelength; d.w_int = c.weight_num_intersections;
    d.area = (double)(c.height * c.width);
    if (is_pin_kind(c.kind)) {  // a15 (S:724-791, P:757-830) and the normalisers of find_reward (S:839-850)
        double dist = sqrt(fma((double)c.width, (double)c.width, (double)c.height * (double)c.height));
        double total = 0.5 * dist * (double)(c.max_num_nets * c.max_num_pins_per_net);
        d.max_wl = c.kind == PCBENV_SPATIAL ? total / (double)(c.height + c.width) : total;
        double mi = 0.5 * (double)(c.max_num_pins_per_net * c.max_num_pins_per_net) * (double)c.max_num_nets * (double)(c.max_num_nets - 1);
        d.max_int = c.kind == PCBENV_PIN ? (double)(long long)mi : mi;
        d.wl_norm = (double)(c.height + c.width);
        double a = mean2(c.min_component_h, c.max_component_h) * mean2(c.min_component_w, c.max_component_w) * mean2(c.min_num_components, c.max_num_components);
        double b = mean2(c.min_num_pins_per_net, c.max_num_pins_per_net) * mean2(c.min_num_nets, c.max_num_nets);
        d.int_norm = a < b ? a : b;
    }
    // threads per environment: one wave up to 64x64 cells of output per plane, four waves above
    env->threads = c.threads_per_env == 64 || c.threads_per_env == 256 ? c.threads_per_env
                   : ((long long)c.height * c.width * (c.kind == PCBENV_SPATIAL ? d.K + 5 : 5) > 64 * 1024 ? 256 : 64);
    // the state block and the LDS zones behind its mirror: pcb_layout.h, which the kernels compile too
    const pcb_layout::Geometry g{c.kind, d.H, d.W, d.C, d.P, d.N, d.mh, d.mw, env->threads, c.reward_type, c.reward_beam_width};
    const pcb_layout::Layout l = pcb_layout::state_layout(g);
    d.offOcc = l.offOcc; d.offVm = l.offVm; d.offComps = l.offComps; d.offPins = l.offPins; d.offRank = l.offRank;
    d.stateStride = l.stateStride;
    d.ldsHf = l.ldsHf; d.ldsHfWords = l.ldsHfWords; d.ldsCls = l.ldsCls; d.ldsSeg = l.ldsSeg; d.ldsBytes = l.ldsBytes;
    d.num_slots = 1; d.slot = 0;
    d.instStride = align16(pcbenv_instance_stride(&c));
#ifdef PCBENV_EXPERIMENTS
    { const char *ev = getenv("PCBENV_LDS_MIN"); if (ev && atoi(ev) > d.ldsBytes) d.ldsBytes = align16(atoi(ev)); }  // occupancy experiments
#endif
    // Terminal list: on for the kinds with a routing reward (run_env, pcb_step.h); B / 8 entries cover twice the
    // 1 / max_num_components of the batch that ends an episode per launch when the phases are spread evenly over a
    // 16-component episode (PCBENV_OPT_TERMINAL_TEAMS changes or disables it).
    env->seq = 0;
    env->term_wgs = 0;
    if (is_pin_kind(c.kind)) {
        int wgs = (c.num_envs / 8 + (int)TERM_SHARDS - 1) & ~((int)TERM_SHARDS - 1);
        env->term_wgs = wgs < (int)TERM_SHARDS ? (int)TERM_SHARDS : wgs > PCBENV_TERM_CAP_MAX ? PCBENV_TERM_CAP_MAX : wgs;
    }
    d.term_cap = env->term_wgs;  // one list entry per set of helper teams
    d.term_hpe = REWARD_PARTS + ((c.flags & PCBENV_FLAG_AUTO_RESET) ? 1 : 0);
}

// Sanity-checks n instance records: every index the kernels derive from a record (component, net, feature row, cell
// inside the component) must stay inside the tables and LDS zones sized from the configuration.
int check_records(pcbenv *env, const void *host_tables, int n) {
    const DevParams &d = env->dp;
    const long long src_stride = pcbenv_instance_stride(&env->cfg);
    const unsigned char *src = (const unsigned char *)host_tables;
    const bool pin_kind = is_pin_kind(env->cfg.kind), spatial = env->cfg.kind == PCBENV_SPATIAL;
    for (int i = 0; i < n; i++) {
        const int32_t *h = (const int32_t *)(src + (size_t)i * src_stride);
        if (h[0] < 1 || h[0] > d.C || h[2] < 0 || h[2] > d.P || h[1] < 0 || h[1] > d.N)
            return fail(env, PCBENV_EINVAL, "instance record out of range (components, nets or pins beyond the configuration)");
        if (!pin_kind && (h[1] != 0 || h[2] != 0)) return fail(env, PCBENV_EINVAL, "instance record carries pins for an environment kind without pins");
        const unsigned char *cr = (const unsigned char *)h + 16, *pr = cr + 8 * (size_t)d.C;
        for (int c = 0; c < h[0]; c++)
            if (cr[8 * c] < 1 || cr[8 * c] > d.mh || cr[8 * c + 1] < 1 || cr[8 * c + 1] > d.mw) return fail(env, PCBENV_EINVAL, "component size out of range");
        int prev = 0;
        unsigned char seen[(PCBENV_MAX_PINS + 7) / 8] = {0};
        int per_net[PCBENV_MAX_NETS] = {0};
        for (int q = 0; q < h[2]; q++) {
            const int net = pr[8 * q + 2], comp = pr[8 * q + 3], id = pr[8 * q + 4] | (pr[8 * q + 5] << 8);
            if (comp >= h[0] || net >= h[1] || (net != prev && net != prev + 1) || (q == 0 && net != 0))
                return fail(env, PCBENV_EINVAL, "pin record out of range, or the pins are not net-major with nets 0, 1, 2, ... in order");
            if (pr[8 * q] >= cr[8 * comp] || pr[8 * q + 1] >= cr[8 * comp + 1]) return fail(env, PCBENV_EINVAL, "pin outside its component");
            if (++per_net[net] > PCBENV_MAX_PINS_PER_NET) return fail(env, PCBENV_EINVAL, "too many pins in one net");
            if (spatial) {  // feature row = the global pin id: a permutation of 0..num_pins-1
                if (id >= h[2] || (seen[id >> 3] >> (id & 7) & 1)) return fail(env, PCBENV_EINVAL, "pin ids must be a permutation of 0..num_pins-1");
                seen[id >> 3] |= (unsigned char)(1u << (id & 7));
            } else if (id >= d.mp) {  // feature row = [component, pin_id]
                return fail(env, PCBENV_EINVAL, "pin id beyond max_num_pins_per_component");
            }
            prev = net;
        }
        if (h[2] > 0 && prev != h[1] - 1) return fail(env, PCBENV_EINVAL, "every net 0..num_nets-1 must have at least one pin");
        if (h[2] == 0 && h[1] != 0 && pin_kind) return fail(env, PCBENV_EINVAL, "nets without pins");
    }
    return PCBENV_OK;
}
