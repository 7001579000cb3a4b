// axis_set_check.cpp -- CPU guard of the per-axis legal set (csrc/pcb_axis_set.h, the header the axis kernels compile).
// Reads geometries and bit rows from stdin (tests/test_axis_set_model.py writes the mask classes of
// tests/logits_cases.py, each clean row followed by its dirty twin), unpacks the clean row into a dense mask with the
// definition written out here, and compares pcb_axis::legal_set -- on the clean row and on the twin -- with a brute-force
// scan of that dense mask for every (axis, given) pair, every valid combination of given values and out-of-range ones.
//   G <O> <H> <W> <rows>          then per row two lines of 2*H*WW hexadecimal words: clean, dirty
// Build and run (the test does that):
//   g++ -std=c++17 -fsanitize=address,undefined -Iinclude -Irl-environment-for-component-placement_amd/csrc
//       -o axis_set_check tools/axis_set_check.cpp && ./axis_set_check < rows.txt
#include "pcb_axis_set.h"

#include <stdio.h>
#include <stdlib.h>

#include <vector>

using namespace pcb_axis;

static long long g_queries = 0;

static void fail(const char *what, const Geom &g, int axis, unsigned given, const int vals[3], Set128 got, Set128 want) {
    fprintf(stderr, "axis_set_check: %s: O %d H %d W %d axis %d given %u vals (%d, %d, %d): got %016llx%016llx want %016llx%016llx\n",
            what, g.O, g.H, g.W, axis, given, vals[0], vals[1], vals[2], got.hi, got.lo, want.hi, want.lo);
    exit(1);
}

// the definition, on the dense mask: scan every (o, x, y) that agrees with the given values
static Set128 brute(const std::vector<unsigned char> &dense, const Geom &g, int axis, unsigned given, const int vals[3]) {
    Set128 s{0ull, 0ull};
    const int n[3] = {g.O, g.H, g.W};
    for (int a = 0; a < 3; a++)
        if (((given >> a) & 1u) && (vals[a] < 0 || vals[a] >= n[a])) return s;
    int c[3], lo[3], hi[3];  // a given axis is scanned at its value alone
    for (int a = 0; a < 3; a++) {
        lo[a] = ((given >> a) & 1u) ? vals[a] : 0;
        hi[a] = ((given >> a) & 1u) ? vals[a] + 1 : n[a];
    }
    for (c[0] = lo[0]; c[0] < hi[0]; c[0]++)
        for (c[1] = lo[1]; c[1] < hi[1]; c[1]++)
            for (c[2] = lo[2]; c[2] < hi[2]; c[2]++)
                if (dense[((size_t)c[0] * g.H + c[1]) * g.W + c[2]]) {
                    if (c[axis] < 64) s.lo |= 1ull << c[axis];
                    else s.hi |= 1ull << (c[axis] - 64);
                }
    return s;
}

static void query(const std::vector<unsigned char> &dense, const word_t *clean, const word_t *dirty, const Geom &g, int axis,
                  unsigned given, const int vals[3]) {
    const Set128 want = brute(dense, g, axis, given, vals);
    const Set128 a = legal_set(clean, g, axis, given, vals), b = legal_set(dirty, g, axis, given, vals);
    if (a.lo != want.lo || a.hi != want.hi) fail("clean row", g, axis, given, vals, a, want);
    if (b.lo != want.lo || b.hi != want.hi) fail("dirty twin", g, axis, given, vals, b, want);
    const Set128 range = first_n(axis_size(g, axis));
    if ((a.lo & ~range.lo) || (a.hi & ~range.hi)) fail("value beyond the axis", g, axis, given, vals, a, want);
    g_queries++;
}

int main() {
    int O, H, W, rows, geoms = 0, total_rows = 0;
    while (scanf(" G %d %d %d %d", &O, &H, &W, &rows) == 4) {
        const Geom g{O, H, W, (W + 63) / 64};
        const size_t words = (size_t)2 * H * g.WW;
        // The square kind's rows carry plane 0 only in the arrays handed over: a read of plane 1 is a heap overflow the
        // sanitizer reports.
        const size_t held = O == 1 ? words / 2 : words;
        const int n[3] = {O, H, W};
        for (int r = 0; r < rows; r++) {
            std::vector<word_t> in[2];
            for (int k = 0; k < 2; k++) {
                std::vector<word_t> all(words);
                for (size_t i = 0; i < words; i++)
                    if (scanf("%llx", &all[i]) != 1) { fprintf(stderr, "axis_set_check: short input\n"); return 1; }
                in[k].assign(all.begin(), all.begin() + held);
            }
            std::vector<unsigned char> dense((size_t)O * H * W);
            for (int o = 0; o < O; o++)
                for (int x = 0; x < H; x++)
                    for (int y = 0; y < W; y++)
                        dense[((size_t)o * H + x) * W + y] = (in[0][((size_t)(o & 1) * H + x) * g.WW + y / 64] >> (y % 64)) & 1ull;
            for (int axis = 0; axis < 3; axis++) {
                const int a1 = (axis + 1) % 3, a2 = (axis + 2) % 3;
                for (unsigned pick = 0; pick < 4; pick++) {
                    const unsigned given = ((pick & 1u) ? 1u << a1 : 0u) | ((pick & 2u) ? 1u << a2 : 0u);
                    // out-of-range values sit next to the valid ones: -1, n, n + 5 and a large one
                    const int extra1[4] = {-1, n[a1], n[a1] + 5, 1 << 30}, extra2[4] = {-1, n[a2], n[a2] + 5, 1 << 30};
                    const int n1 = (pick & 1u) ? n[a1] + 4 : 1, n2 = (pick & 2u) ? n[a2] + 4 : 1;
                    for (int i = 0; i < n1; i++)
                        for (int j = 0; j < n2; j++) {
                            int vals[3] = {-7, -7, -7};  // an axis that is not given must not be read as a value
                            vals[a1] = (pick & 1u) ? (i < n[a1] ? i : extra1[i - n[a1]]) : -7;
                            vals[a2] = (pick & 2u) ? (j < n[a2] ? j : extra2[j - n[a2]]) : -7;
                            query(dense, in[0].data(), in[1].data(), g, axis, given, vals);
                        }
                }
            }
            total_rows++;
        }
        geoms++;
    }
    if (!geoms) { fprintf(stderr, "axis_set_check: no input\n"); return 1; }
    printf("axis_set_check ok: %d geometries, %d rows, %lld queries\n", geoms, total_rows, g_queries);
    return 0;
}
