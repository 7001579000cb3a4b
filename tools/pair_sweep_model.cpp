// pair_sweep_model.cpp -- the pair sweep of the routing reward (count_finish, csrc/pcb_reward.h) restated on the CPU over the very
// geometry the kernels compile (csrc/pcb_geometry.h: prepare_slot, extents_overlap, slots_intersect): for the segment slots of one
// environment it deals the sweep steps to `nparts` teams of `nwaves` wavefronts as the kernel does and reports what each wavefront
// meets -- the block sizes R, the pairs that pass the integer extent filter, the dense batches of 128 it runs out of its compaction
// buffer and the intersections counted.  tests/routing_layouts.py uses it to assert that its layouts reach the dense-batch path
// and the path where no pair passes; it also checks the sweep's `magic` division and the buffer bound on every input it sees.
// stdin:   nwaves nparts np nn / nstart[0..nn] / np lines "act x1 y1 x2 y2"
// stdout:  R of nets 1..nn-1 / passes hits / dense batches per (part, wave)
// Build:   g++ -std=c++17 -O1 -Wall -Wextra -Werror -ffp-contract=off -Iinclude -Irl-environment-for-component-placement_amd/csrc
//              -o pair_sweep_model tools/pair_sweep_model.cpp
#include "pcb_geometry.h"

#include <stdio.h>
#include <stdlib.h>

#include <vector>

#define FAIL(...) do { fprintf(stderr, "pair_sweep_model: " __VA_ARGS__); fprintf(stderr, "\n"); exit(1); } while (0)

int main() {
    int nwaves, nparts, np, nn;
    if (scanf("%d %d %d %d", &nwaves, &nparts, &np, &nn) != 4 || (nwaves != 1 && nwaves != 4) || nparts < 1 || np < 0 || np > 256 || nn < 1 || nn > 32)
        FAIL("bad header");
    std::vector<int> nstart(nn + 1);
    for (int &s : nstart) if (scanf("%d", &s) != 1) FAIL("bad nstart");
    if (nstart[0] != 0 || nstart[nn] != np) FAIL("nstart does not cover the slots");
    std::vector<double> X1(np + 1), Y1(np + 1), X2(np + 1), Y2(np + 1), A(np + 1), DX(np + 1), DY(np + 1);
    std::vector<int> act(np + 1);
    std::vector<unsigned> bbox(np + 1);
    SegView v{};
    v.X1 = X1.data(); v.Y1 = Y1.data(); v.X2 = X2.data(); v.Y2 = Y2.data(); v.A = A.data(); v.DX = DX.data(); v.DY = DY.data();
    v.act = act.data(); v.bbox = bbox.data();
    for (int q = 0; q < np; q++) {
        if (scanf("%d %lf %lf %lf %lf", &act[q], &X1[q], &Y1[q], &X2[q], &Y2[q]) != 5) FAIL("bad slot %d", q);
        prepare_slot(v, q);
    }
    for (int n = 1; n < nn; n++) printf("%d%c", nstart[n] * (nstart[n + 1] - nstart[n]), n + 1 < nn ? ' ' : '\n');
    if (nn == 1) printf("\n");
    long long passes = 0, hits = 0;
    std::vector<int> dense((size_t)nparts * nwaves, 0);
    for (int part = 0; part < nparts; part++)
        for (int wave = 0; wave < nwaves; wave++) {
            std::vector<unsigned short> buf;
            int pm = 0, pq = 0;
            for (int n = 1; n < nn; n++) {
                const int s = nstart[n], c = nstart[n + 1] - s, R = s * c;
                const unsigned magic = (65536u + (unsigned)c - 1u) / (unsigned)(c > 1 ? c : 1);
                for (int base = 0; base < R; base += 4 * WAVE) {
                    const bool mine = pm == part && (pq & (nwaves - 1)) == wave;
                    if (++pm == nparts) { pm = 0; pq++; }
                    if (!mine) continue;
                    for (int u = 0; u < 4; u++)
                        for (int lane = 0; lane < WAVE; lane++) {
                            const int r = base + u * WAVE + lane;
                            if (r >= R) continue;
                            const int pi = (int)(((unsigned)r * magic) >> 16), pj = s + (r - pi * c);
                            if (pi != r / c || pj < s || pj >= s + c) FAIL("magic division: r %d c %d", r, c);
                            if (extents_overlap(bbox[pi], bbox[pj])) { buf.push_back((unsigned short)(pi | (pj << 8))); passes++; }
                        }
                    if (buf.size() > (size_t)PAIR_ENTRIES_PER_WAVE) FAIL("compaction buffer: %zu entries", buf.size());
                    while (buf.size() >= 2 * (size_t)WAVE) {
                        for (int i = 0; i < 2 * WAVE; i++) hits += slots_intersect(v, buf[i] & 0xFF, buf[i] >> 8);
                        buf.erase(buf.begin(), buf.begin() + 2 * WAVE);
                        dense[(size_t)part * nwaves + wave]++;
                    }
                }
            }
            for (unsigned short p : buf) hits += slots_intersect(v, p & 0xFF, p >> 8);
        }
    printf("%lld %lld\n", passes, hits);
    for (size_t i = 0; i < dense.size(); i++) printf("%d%c", dense[i], i + 1 < dense.size() ? ' ' : '\n');
    return 0;
}
