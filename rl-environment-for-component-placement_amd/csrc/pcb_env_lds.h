// pcb_env_lds.h -- a team's view of one environment in LDS and the small helpers on it that do not depend on the team size:
// the carved state mirror, output rows, the spatial kind's pin tables, a pin's feature row, the tail-safe 16-byte store, the
// feature-cache tag test and the registers a reset fetches an instance into.  Free device functions; CDNA4 / gfx950 only.
#pragma once
#include "pcb_device.h"

struct Lds {
    EnvHdr *hdr; u64 *occ, *vm; CompRec *comps; PinRec *pins; unsigned char *rank;
    u64 *hf; unsigned char *cls; double *seg;
};
// Row of environment e in the [num_slots, B, ...] output tensors for the slot a step writes (DevParams::slot).
__device__ inline int out_row(const DevParams &p, int slot, int e) { return slot * p.B + e; }
__device__ inline Lds carve(unsigned char *smem, const DevParams &p) {
    Lds l;
    l.hdr = (EnvHdr *)smem;
    l.occ = (u64 *)(smem + p.offOcc);
    l.vm = (u64 *)(smem + p.offVm);
    l.comps = (CompRec *)(smem + p.offComps);
    l.pins = (PinRec *)(smem + p.offPins);
    l.rank = smem + p.offRank;  // rank[q] = position of pin q among the pins of its component (self.pins order)
    l.hf = (u64 *)(smem + p.ldsHf);
    l.cls = smem + p.ldsCls;
    l.seg = (double *)(smem + p.ldsSeg);
    return l;
}

// Feature rows of one pin (P:72-103 / S:70-104 Pin.calculate_feature): [rel_x, rel_y, abs_x, abs_y]
template <int KIND> __device__ inline void write_pin_num(const DevParams &p, int row_, const PinRec &pr) {
    if (!p.buf.all_pins_num_feature) return;
    int row;
    if (KIND == PCBENV_SPATIAL) row = pr.id & PIN_ID_MASK;
    else { if (pr.id & PIN_LOSER) return; row = pr.comp * p.mp + (pr.id & PIN_ID_MASK); }
    double *f = p.buf.all_pins_num_feature + ((size_t)row_ * p.pinRows + row) * 4;
    f[0] = pr.rel_x; f[1] = pr.rel_y; f[2] = pr.abs_x; f[3] = pr.abs_y;
}

// Scratch tables in the class-map zone (free between two emit_pin_grid calls), spatial env only:
// pid[c][k] = global id of the k-th pin of component c in self.pins order (0xFFFF = none) -- the tail of
// all_components_feature (S:203-239); netmask[c][rel_x][rel_y] = nets with a pin on that cell of the component at
// its UNROTATED relative coordinates -- draw_components (S:1677-1697) runs at reset only, so component_grid never
// shows the in-place rotation of place_component (quirk Q4): for a placed component the rotation is undone here
// with the orientation kept in its record.
struct PinTables { unsigned short *pid; unsigned *netmask; };
__device__ inline PinTables pin_tables(const DevParams &p, Lds &l) {
    PinTables t;
    t.pid = (unsigned short *)l.cls;
    t.netmask = (unsigned *)(l.cls + pcb_layout::pin_table_netmask_offset(p.C * p.mp));
    return t;
}
static_assert(PCBENV_MAX_NETS <= 32, "PinTables::netmask: 1u << pr.net (build_pin_tables); emit_component_grid_to: a cell's field = netmask << 1 | exists, in 64 bits");
// chunk [bb, bb + 16) of a `total`-byte tensor row (total a multiple of 4): whole, or -- the last one -- the dwords inside the row
__device__ inline void store16_or_tail(const ObsDst &d, unsigned char *dst, int bb, int total, uint4 v, bool stream) {
    if (bb + 16 <= total) { STORE16_dyn(d, (unsigned)bb, v, stream); return; }
    const unsigned w[4] = {v.x, v.y, v.z, v.w};
    #pragma unroll
    for (int j = 0; j < 4; j++) if (bb + 4 * j < total) *(unsigned *)(dst + bb + 4 * j) = w[j];
}
// The episode-constant part of a spatial environment's trajectory slot, kept per environment in library memory so that a
// step of the trajectory layout copies it instead of rebuilding the pin tables: [compact all_components_feature, C x F
// int16 with x = y = -1 | component_grid].  Written by the reset that starts the episode (tagged with the episode number;
// a restored checkpoint invalidates the tags), used by steps whose slot takes no float64 all_components_feature.
__device__ inline bool feat_cache_valid(const DevParams &p, const Lds &l, int e) {
    return p.feat_cache && !p.buf.all_components_feature && p.feat_cache_tag[e] == l.hdr->episode;
}
// The next queued instance of environment e: header and 8-byte records, all loads issued together.
struct InstRegs { int nc, nn, np; u64 comp; u64 pin[4]; };
static_assert(PCBENV_MAX_PINS <= 4 * WAVE, "InstRegs::pin[4]: pin q = lane + r * NT of fetch_instance, NT >= WAVE");
static_assert(PCBENV_MAX_COMPONENTS <= WAVE, "InstRegs::comp: the record of component `lane` (lane < p.C), NT >= WAVE");
