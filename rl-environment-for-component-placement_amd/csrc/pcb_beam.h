// pcb_beam.h -- beam-search routes of all nets of an environment, dealt to the team's lanes (the search itself: pcb_routing.h)
// Class section, not a header: included INSIDE Team<TN> (pcb_team.h), because it strides by NT lanes or meets the team in lds_sync / store_drain_sync / block_any.
template <bool SMALL>
static __device__ __forceinline__ void beam_routes_lanes(const SegView &v, const PinRec *pins, int nn, int k, unsigned char *beam, int lane, unsigned long long *beam_dbg) {
    const int groups = NT / BEAM_LANES_PER_NET, gi = lane / BEAM_LANES_PER_NET, t = lane & (BEAM_LANES_PER_NET - 1);
    for (int n0 = 0; n0 < nn; n0 += groups) {
        const int n = n0 + gi;
        if (n >= nn) continue;
        const int s = v.nstart[n], cnt = v.nstart[n + 1] - s;
        // pin_outlier: first arg-max of the distance to the centroid (distances one pin per lane in v.D, below)
        int st = 0; double bd = v.D[s];
        if (SMALL) {
            double dd[8];
            #pragma unroll
            for (int i = 1; i < 8; i++) dd[i] = v.D[s + (i < cnt ? i : 0)];
            #pragma unroll
            for (int i = 1; i < 8; i++) if (i < cnt && dd[i] > bd) { bd = dd[i]; st = i; }
        } else {
            for (int i = 1; i < cnt; i++) { const double d = v.D[s + i]; if (d > bd) { bd = d; st = i; } }
        }
        beam_route_lanes<SMALL>(v, pins, s, cnt, st, k, beam + (size_t)n * BEAM_LDS_PER_NET(k), t, beam_dbg);
    }
}
// all nets of the environment: v.D / v.act / segment slots are filled with the beam routes
static __device__ __forceinline__ void beam_routes(const SegView &v, const EnvHdr *hdr, const PinRec *pins, int k, unsigned char *beam, int lane, unsigned long long *beam_dbg) {
    const int np = hdr->npins, nn = hdr->nnets;
    for (int q = lane; q < np; q += NT) {  // distance of every pin to its net's centroid (v.D is free until the segments are written)
        const PinRec pr = pins[q];
        v.D[q] = norm2((double)pr.abs_x - v.cen[pr.net], (double)pr.abs_y - v.cen[v.N + pr.net]);
    }
    lds_sync();
    // workgroup-uniform: the widest net of this instance decides which build runs (every wavefront looks at all nets)
    const int nl = lane & 63;
    const bool wide = __ballot(nl < nn && v.nstart[nl < nn ? nl + 1 : 0] - v.nstart[nl < nn ? nl : 0] > 8) != 0ull;
    if (!wide && k <= 2) beam_routes_lanes<true>(v, pins, nn, k, beam, lane, beam_dbg);
    else beam_routes_lanes<false>(v, pins, nn, k, beam, lane, beam_dbg);
    lds_sync();
    for (int q = lane; q < np; q += NT) {  // segment i of a net's route = (path[i], path[i + 1]), one slot per lane
        const int n = pins[q].net, s = v.nstart[n], i = q - s;
        const BsEntry res = *(const BsEntry *)(beam + (size_t)n * BEAM_LDS_PER_NET(k));
        const bool act = i + 1 < res.len();
        if (act) {
            const PinRec pa = pins[s + res.at(i)], pb = pins[s + res.at(i + 1)];
            const double x1 = pa.abs_x, y1 = pa.abs_y, x2 = pb.abs_x, y2 = pb.abs_y;
            v.X1[q] = x1; v.Y1[q] = y1; v.X2[q] = x2; v.Y2[q] = y2;
            v.D[q] = norm2(x1 - x2, y1 - y2);
        }
        v.act[q] = act ? 1 : 0;
    }
}

// beam (and, for "both", centroid) routes of the terminal state -> wirelength and this team's share of the #intersections
// of the beam route (wl[0], ni[0]) and, reward_type "both", of the centroid route (wl[1], ni[1]); the caller picks
// (S:609-627 lowest_num_intersections) once the shares of all teams are in.
static __device__ __forceinline__ void route_beam_or_both(const DevParams &p, const EnvHdr *hdr, const PinRec *pins, double *seg,
                                          int lane, int part, int nparts, double *wl, int *ni) {
    const SegView v = seg_view(seg, p.P, p.N);
    unsigned char *beam = v.beam;
    net_offsets_and_centroids(v, hdr, pins, lane);
    STAMP(5);
    STAMP_ZERO(26); STAMP_ZERO(27); STAMP_ZERO(28); STAMP_ZERO(29);
    beam_routes(v, hdr, pins, p.beam_width, beam, lane, p.dbg);
    lds_sync();
    STAMP(24);
    count_and_length(p, v, hdr, pins, lane, part, nparts, &wl[0], &ni[0]);
    STAMP(25);
    if (p.reward_type == PCBENV_REWARD_BOTH) {
        build_centroid_segments(v, hdr, pins, lane);
        count_and_length(p, v, hdr, pins, lane, part, nparts, &wl[1], &ni[1]);
    }
    STAMP(8);
}
