// kernel_models_check.cpp -- CPU check of the two pure scalar models the step kernel carries for the reference's traps,
// compiled from the very headers the kernels compile (csrc/pcb_setmodel.h, csrc/pcb_geometry.h):
//   (a) the model of CPython's set iteration order: every case read from stdin must come out of cs_difference_order as
//       recorded, and wherever beam_route_lanes (csrc/pcb_routing.h) would take the register fast path --
//       !((m >> 2) > popcount(visited)) and at most 4 points left -- cs_small_difference_order on a table built by
//       cs_build_points must give the same order;
//   (b) the intersection test: a seeded sweep of segment pairs whose end points are grid cells or centroids of 2-16 cells
//       (what the routes consist of), all inside [0, side - 1], with shared end points and parallel pairs mixed in;
//       slots_intersect on slots hoisted by prepare_slot must equal the reference's is_intersect, and extents_overlap
//       must reject no pair that is_intersect accepts.
// stdin, one case per line:   H x y hash            tuple_hash2(x, y) == hash
//                             S n x0 y0 .. mask k o0 ..   n points, visited mask, the k point indices in iteration order
//                             G seed pairs          run sweep (b)
// Build and run (tests/test_kernel_models.py does that):
//   g++ -std=c++17 -O1 -g -Wall -Wextra -Werror -ffp-contract=off -fsanitize=address,undefined,float-cast-overflow
//       -fno-sanitize-recover=all -Iinclude -Irl-environment-for-component-placement_amd/csrc
//       -o kernel_models_check tools/kernel_models_check.cpp && ./kernel_models_check < cases
#include "pcb_geometry.h"
#include "pcb_setmodel.h"

#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#define FAIL(...) do { fprintf(stderr, "kernel_models_check: " __VA_ARGS__); fprintf(stderr, "\n"); exit(1); } while (0)

static long long g_hashes = 0, g_orders = 0, g_fast = 0, g_pairs = 0, g_hits = 0, g_rejected = 0;

static void check_order(int n, const int *xs, const int *ys, unsigned visited, int k, const int *want) {
    PinRec pins[16];
    memset(pins, 0, sizeof pins);
    for (int i = 0; i < n; i++) { pins[i].abs_x = (signed char)xs[i]; pins[i].abs_y = (signed char)ys[i]; }
    const NetPts pt = NetPts::load(pins, n, -1);  // no start pin to leave out: the case's points are the points to visit
    alignas(16) CSet A, R;
    unsigned char order[16];
    const int got = cs_difference_order(&A, &R, n, visited, pt, order);
    bool same = got == k;
    for (int i = 0; same && i < k; i++) same = order[i] == want[i];
    if (!same) FAIL("cs_difference_order: order case %lld (%d points, visited %#x) differs", g_orders, n, visited);
    const int seen = __builtin_popcount(visited);
    if (!((n >> 2) > seen) && n - seen <= 4) {  // the preconditions of beam_route_lanes' fast path
        unsigned hs[16], packed = 0;
        cs_build_points(&A, &R, hs, n, pt);
        const int ns = cs_small_difference_order(&A, hs, visited, pt, &packed);
        same = ns == k;
        for (int i = 0; same && i < k; i++) same = (int)((packed >> (8 * i)) & 0xFFu) == want[i];
        if (!same) FAIL("cs_small_difference_order: order case %lld (%d points, visited %#x) differs", g_orders, n, visited);
        g_fast++;
    }
    g_orders++;
}

// ---- (b) -----------------------------------------------------------------------------------------------------------
static unsigned long long g_rng;
static unsigned rnd(unsigned n) {  // splitmix64, reduced to [0, n)
    unsigned long long z = (g_rng += 0x9E3779B97F4A7C15ull);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return (unsigned)(((z ^ (z >> 31)) >> 32) * n >> 32);
}
struct Pt { double x, y; };
static Pt point(int side) {  // a pin on its cell, or a net's centroid: (exact integer sum, as float64) / count
    if (rnd(2)) return Pt{(double)rnd(side), (double)rnd(side)};
    const int cnt = 2 + (int)rnd(15);
    int sx = 0, sy = 0;
    for (int i = 0; i < cnt; i++) { sx += (int)rnd(side); sy += (int)rnd(side); }
    return Pt{(double)sx / (double)cnt, (double)sy / (double)cnt};
}
static bool inside(Pt p, int side) { return p.x >= 0.0 && p.x <= side - 1 && p.y >= 0.0 && p.y <= side - 1; }

static void sweep(unsigned long long seed, long long pairs) {
    g_rng = seed;
    const int P = 2, N = 1;
    alignas(16) static unsigned char zone[SEG_LDS_BYTES(P, N, 1, 0)];
    const SegView v = seg_view((double *)zone, P, N);
    v.act[0] = v.act[1] = 1;
    for (long long it = 0; it < pairs; it++) {
        const int side = rnd(4) ? 6 + (int)rnd(10) : 128;
        Pt p[4] = {point(side), point(side), point(side), point(side)};
        const unsigned mix = rnd(8);
        if (mix == 0) p[2 + rnd(2)] = p[rnd(2)];  // a shared end point
        else if (mix <= 2) {                      // parallel (up to the rounding of a centroid), kept inside the grid
            const double dx = p[1].x - p[0].x, dy = p[1].y - p[0].y, f = mix == 1 ? 1.0 : 0.5;
            const Pt up{p[2].x + f * dx, p[2].y + f * dy}, down{p[2].x - f * dx, p[2].y - f * dy};
            if (inside(up, side)) p[3] = up; else if (inside(down, side)) p[3] = down;
        } else if (mix == 3) {                    // on one line with the first segment
            const double t = (double)rnd(5) / 4.0;
            const Pt on{p[0].x + t * (p[1].x - p[0].x), p[0].y + t * (p[1].y - p[0].y)};
            if (inside(on, side)) p[2] = on;  // (rounding can put it an ulp outside)
        }
        for (int s = 0; s < 2; s++) {
            v.X1[s] = p[2 * s].x; v.Y1[s] = p[2 * s].y; v.X2[s] = p[2 * s + 1].x; v.Y2[s] = p[2 * s + 1].y;
            prepare_slot(v, s);
        }
        const bool want = is_intersect(p[0].x, p[0].y, p[1].x, p[1].y, p[2].x, p[2].y, p[3].x, p[3].y);
        if (slots_intersect(v, 0, 1) != want)
            FAIL("slots_intersect != is_intersect (%d) for (%a, %a)-(%a, %a) x (%a, %a)-(%a, %a)", (int)want, p[0].x, p[0].y, p[1].x,
                 p[1].y, p[2].x, p[2].y, p[3].x, p[3].y);
        const bool pass = extents_overlap(v.bbox[0], v.bbox[1]);
        if (want && !pass)
            FAIL("extents_overlap rejects an intersecting pair: (%a, %a)-(%a, %a) x (%a, %a)-(%a, %a)", p[0].x, p[0].y, p[1].x, p[1].y,
                 p[2].x, p[2].y, p[3].x, p[3].y);
        g_pairs++; g_hits += want; g_rejected += !pass;
    }
}

int main() {
    char tag[8];
    while (scanf("%7s", tag) == 1) {
        if (!strcmp(tag, "H")) {
            int x, y; unsigned long long h;
            if (scanf("%d %d %llu", &x, &y, &h) != 3) FAIL("malformed H line");
            if (tuple_hash2(x, y) != h) FAIL("tuple_hash2(%d, %d) = %llu, recorded %llu", x, y, tuple_hash2(x, y), h);
            g_hashes++;
        } else if (!strcmp(tag, "S")) {
            int n, k, xs[16], ys[16], want[16]; unsigned visited;
            if (scanf("%d", &n) != 1 || n < 1 || n > 15) FAIL("malformed S line: 1..15 points");
            for (int i = 0; i < n; i++) if (scanf("%d %d", &xs[i], &ys[i]) != 2 || (xs[i] | ys[i]) < 0 || (xs[i] | ys[i]) > 127) FAIL("malformed S line: point");
            if (scanf("%u %d", &visited, &k) != 2 || visited >> n || k < 0 || k > n) FAIL("malformed S line: mask / count");
            for (int i = 0; i < k; i++) if (scanf("%d", &want[i]) != 1) FAIL("malformed S line: order");
            check_order(n, xs, ys, visited, k, want);
        } else if (!strcmp(tag, "G")) {
            unsigned long long seed; long long pairs;
            if (scanf("%llu %lld", &seed, &pairs) != 2) FAIL("malformed G line");
            sweep(seed, pairs);
        } else FAIL("unknown case tag %s", tag);
    }
    printf("kernel_models_check ok: %lld tuple hashes, %lld set orders (%lld on the fast path), %lld segment pairs (%lld intersect, %lld rejected by their extents)\n",
           g_hashes, g_orders, g_fast, g_pairs, g_hits, g_rejected);
    return 0;
}
