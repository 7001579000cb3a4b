// pcb_reward.h -- the team's sweeps of the routing reward: net offsets and centroids, centroid routes, pair count, wirelength
// Class section, not a header: included INSIDE Team<TN> (pcb_team.h), because it strides by NT lanes or meets the team in lds_sync / store_drain_sync / block_any.
// net_pins offsets (self.pins is net-major) and S:1229-1241 get_centroid per net: np.mean of an integer array =
// (exact integer sum, as float64) / n -- the sums are gathered with LDS integer atomics (order-free because exact).
static __device__ inline void net_offsets_and_centroids(const SegView &v, const EnvHdr *hdr, const PinRec *pins, int lane) {
    const int np = hdr->npins, nn = hdr->nnets;
    lds_sync();  // the segment area aliases the class map of emit_pin_grid
    for (int n = lane; n < 2 * v.N; n += NT) v.nsum[n] = 0;
    lds_sync();
    for (int q = lane; q < np; q += NT) {
        const PinRec pr = pins[q];
        if (q == 0 || pr.net != pins[q - 1].net) v.nstart[pr.net] = q;
        atomicAdd(&v.nsum[pr.net], (int)pr.abs_x);
        atomicAdd(&v.nsum[v.N + pr.net], (int)pr.abs_y);
    }
    if (lane == 0) v.nstart[nn] = np;
    lds_sync();
    for (int n = lane; n < nn; n += NT) {
        const double cnt = (double)(v.nstart[n + 1] - v.nstart[n]);
        v.cen[n] = (double)v.nsum[n] / cnt;
        v.cen[v.N + n] = (double)v.nsum[v.N + n] / cnt;
    }
    lds_sync();
}

// S:1243-1271 route_pins_centroid: (pin, centroid) per pin; a 2-pin net is the single segment (p0, p1)
static __device__ inline void build_centroid_segments(const SegView &v, const EnvHdr *hdr, const PinRec *pins, int lane) {
    const int np = hdr->npins;
    for (int q = lane; q < np; q += NT) {
        const int n = pins[q].net, s = v.nstart[n], cnt = v.nstart[n + 1] - s;
        double x1 = pins[q].abs_x, y1 = pins[q].abs_y, x2, y2;
        int a = 1;
        if (cnt == 2) { a = (q == s); x2 = pins[s + 1].abs_x; y2 = pins[s + 1].abs_y; }
        else { x2 = v.cen[n]; y2 = v.cen[v.N + n]; }
        v.X1[q] = x1; v.Y1[q] = y1; v.X2[q] = x2; v.Y2[q] = y2; v.act[q] = a;
        v.D[q] = norm2(x1 - x2, y1 - y2);
    }
    lds_sync();
}


// S:629-651 find_num_intersection + S:704-722 find_wirelength over the slots.
// Slots are net-major, so the partners "segment of an earlier net" of the slots of net n are the slots
// 0..nstart[n]-1: net n contributes the block nstart[n] x (its own slots) of pairs.  The blocks are swept one
// after the other, 64 pairs at a time, the sweep steps dealt out to the wavefronts: every lane
// of every sweep step holds one pair, whatever the shape of the block (the triangle of the old per-slot sweep left
// half the lanes idle and cost one step per partner).  A pair is first tested on its packed integer extents; the
// survivors of a step are appended to the wavefront's compaction buffer with a ballot, and the buffer goes through
// the full float64 test in dense batches of 128.  The wirelength is summed sequentially in route order (bit-exact
// with the reference's python float loop).
// count_prepare reads the pins, count_finish only the segment zone.
static __device__ inline void count_prepare(const SegView &v, int np, int lane) {
    int *total_cnt = v.nstart + v.N + 1;  // spare slot behind nstart[0..MAX_NETS]
    for (int q = lane; q < np; q += NT) prepare_slot(v, q);
    if (lane == 0) *total_cnt = 0;
    lds_sync();
}
// (part, nparts): the sweep steps are dealt to `nparts` teams of a launch (the environment's own wavefront and its reward
// helpers, see run_env), this team being number `part`; *nintersections is then this team's share of the count.
static __device__ inline void count_finish(const DevParams &p, const SegView &v, int np_, int nn_, int lane, int part, int nparts, double *wirelength, int *nintersections) {
    int *total_cnt = v.nstart + v.N + 1;
    const int np = __builtin_amdgcn_readfirstlane(np_), nn = __builtin_amdgcn_readfirstlane(nn_);
    STAMP(12);
#ifndef PCBENV_STAMPS_BEAM
    STAMP_ZERO(26); STAMP_ZERO(27); STAMP_ZERO(28); STAMP_ZERO(29);
#endif
    const int wl_lane = lane & 63, wave = lane >> 6, nwaves = NT / WAVE;
    volatile lds_u16 *buf = (volatile lds_u16 *)(v.pairs + wave * PAIR_ENTRIES_PER_WAVE);  // wave-synchronous: written and read by different lanes
    int cnt = 0, nbuf = 0, step = 0;
    int pm = 0, pq = 0;  // step % nparts, step / nparts (kept incrementally: no division by a run-time value)
    for (int n = 1; n < nn; n++) {  // wave-uniform; net 0 has no earlier net
        const int s = __builtin_amdgcn_readfirstlane(v.nstart[n]), c = __builtin_amdgcn_readfirstlane(v.nstart[n + 1]) - s;
        const int R = s * c;                         // pairs (i, j): i in [0, s) earlier-net slot, j in [s, s + c)
        const unsigned magic = (65536u + (unsigned)c - 1u) / (unsigned)max(c, 1);  // r / c == (r * magic) >> 16 for r < 4160, c <= 16
        // four 64-pair groups per sweep step: their LDS reads go out together and the loop overhead is paid once
        for (int base = 0; base < R; base += 4 * WAVE, step++) {
            const bool mine = pm == part && (pq & (nwaves - 1)) == wave;  // nwaves is 1 or 4
            if (++pm == nparts) { pm = 0; pq++; }
            if (!mine) continue;
            unsigned bi[4], bj[4]; int pi[4], pj[4];
            #pragma unroll
            for (int u = 0; u < 4; u++) {
                const int r = base + u * WAVE + wl_lane;
                const bool in = r < R;
                pi[u] = in ? (int)(((unsigned)r * magic) >> 16) : 0;
                pj[u] = in ? s + (r - pi[u] * c) : 0;
                bi[u] = v.bbox[pi[u]]; bj[u] = v.bbox[pj[u]];
                if (!in) bi[u] = 0u;  // fails the "both slots carry a segment" bit
            }
            #pragma unroll
            for (int u = 0; u < 4; u++) {  // at most 4 * 64 new entries: the buffer holds them next to a partial batch
                const bool pass = extents_overlap(bi[u], bj[u]);
                const u64 ball = __ballot(pass);
                if (pass) buf[nbuf + __popcll(ball & ((1ull << wl_lane) - 1ull))] = (unsigned short)(pi[u] | (pj[u] << 8));
                nbuf += __popcll(ball);
            }
            while (nbuf >= 2 * WAVE) {  // dense batches; the rest (< 128 entries) moves to the front
                STAMP_T0();
                cnt += count_candidates(v, buf, 2 * WAVE, wl_lane);
#ifndef PCBENV_STAMPS_BEAM
                STAMP_ACC_SINCE(26, cnt); STAMP_ADD(27, 1); STAMP_ADD(28, 2 * WAVE);
#endif
                nbuf -= 2 * WAVE;
                for (int k = wl_lane; k < nbuf; k += WAVE) { const unsigned short rest = buf[2 * WAVE + k]; buf[k] = rest; }
            }
        }
    }
    STAMP(13);
#ifndef PCBENV_STAMPS_BEAM
    STAMP_ADD(28, nbuf); STAMP_ADD(29, step);
#endif
    cnt += count_candidates(v, buf, nbuf, wl_lane);
    STAMP(14);
    for (int o = 32; o > 0; o >>= 1) cnt += __shfl_xor(cnt, o);
    if (wl_lane == 0 && cnt) atomicAdd(total_cnt, cnt);
    lds_sync();
    STAMP(15);
    // find_wirelength: the adds happen in route order; empty slots add +0.0, which leaves a non-negative sum
    // unchanged bit for bit.  Every lane fetches the lengths of its own slots once (one LDS round trip), the sum
    // then runs over v_readlane broadcasts.
    double wl = 0.0;
    for (int base = 0; base < np; base += WAVE) {
        const int sidx = base + wl_lane;
        const double d = (sidx < np && v.act[sidx]) ? v.D[sidx] : 0.0;
        const int dlo = __double2loint(d), dhi = __double2hiint(d);
        #pragma unroll
        for (int blk = 0; blk < WAVE; blk += 16) {  // constant lane selects: the broadcasts run ahead of the add chain
            if (base + blk >= np) break;
            #pragma unroll
            for (int il = blk; il < blk + 16; il++)
                wl += __hiloint2double(__builtin_amdgcn_readlane(dhi, il), __builtin_amdgcn_readlane(dlo, il));
        }
    }
    *wirelength = wl;
    *nintersections = *total_cnt;
    lds_sync();
}
static __device__ inline void count_and_length(const DevParams &p, const SegView &v, const EnvHdr *hdr, const PinRec *pins, int lane, int part, int nparts,
                                        double *wirelength, int *nintersections) {
    const int np = hdr->npins, nn = hdr->nnets;
    count_prepare(v, np, lane);
    count_finish(p, v, np, nn, lane, part, nparts, wirelength, nintersections);
}

static __device__ inline void route_centroid(const DevParams &p, const EnvHdr *hdr, const PinRec *pins, double *seg,
                                      int lane, int part, int nparts, double *wirelength, int *nintersections) {
    const SegView v = seg_view(seg, p.P, p.N);
    net_offsets_and_centroids(v, hdr, pins, lane);
    STAMP(5);
    build_centroid_segments(v, hdr, pins, lane);
    STAMP(6);
    count_prepare(v, hdr->npins, lane);
    STAMP(22);
    count_finish(p, v, hdr->npins, hdr->nnets, lane, part, nparts, wirelength, nintersections);
    STAMP(8);
}
