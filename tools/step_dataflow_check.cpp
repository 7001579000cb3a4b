// step_dataflow_check.cpp -- CPU check of the register forms the geometry-fixed step builds take on a 64 x 64 grid with one
// row per lane (Team<>::plain_transition_from_rows, csrc/pcb_step.h), compiled from the header the kernels compile
// (csrc/pcb_transition.h):
//   (a) row_after_update1, a lane's occupancy row after update_grid as an expression of its old row and the action, against
//       occupy_row applied to the rows x..x+ph-1 of the grid in LDS order: exhaustively over (x, ph, y, pw, lane) with ph, pw
//       in [1, 64] and the rectangle inside the grid on empty and full old rows, and over every (y, pw) on both sides of the
//       row range for `rows` random old rows;
//   (b) the value-taking window fold -- row1_hfold, rows_vfold with the 64 lanes' values side by side and a `down` that
//       shifts them the way lane_down does, row1_free_below, put together as Team<>::window_mask_row does -- against the
//       definition of the legal-placement mask (vm[r] bit j = 1 iff r <= H - ph', j <= W - pw' and the cells r..r+ph'-1 x
//       j..j+pw'-1 are empty), on grids that an update has just been applied to: every (ph', pw') with ph' * pw' <=
//       PCBENV_MAX_PINS_PER_COMPONENT (what a component of a pin kind can be, ph' == pw' included) and the (ph', pw')
//       given on the F line, on sparse, dense and full grids, so that windows with no legal cell left are met.
// stdin:
//   U rows seed            part (a)
//   F grids seed n (ph pw) * n     part (b), the extra windows
// Build and run (tests/test_step_dataflow.py does that):
//   g++ -std=c++17 -O1 -g -Wall -Wextra -Werror -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=all
//       -Iinclude -Irl-environment-for-component-placement_amd/csrc -o step_dataflow_check tools/step_dataflow_check.cpp
#include "pcb_transition.h"

#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <utility>
#include <vector>

#define FAIL(...) do { fprintf(stderr, "step_dataflow_check: " __VA_ARGS__); fprintf(stderr, "\n"); exit(1); } while (0)

static const int N = 64;  // H = W = lanes of a wavefront
static long long g_rows = 0, g_folds = 0, g_equal_sides = 0, g_no_legal_cell = 0;

static u64 g_rng = 0;
static u64 rnd() {  // splitmix64
    u64 z = (g_rng += 0x9E3779B97F4A7C15ull);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}
static u64 random_row(int density_16ths) {
    u64 r = 0;
    for (int b = 0; b < 64; b++) if ((int)(rnd() & 15) < density_16ths) r |= 1ull << b;
    return r;
}
static int read_int() {
    int v;
    if (scanf("%d", &v) != 1) FAIL("malformed input: integer expected");
    return v;
}

// ---- (a) ----------------------------------------------------------------------------------------------------------------
// the grid's rows after update_grid the way Team<>::transition drives it for a team of 64 lanes
static void update_in_lds_order(u64 *occ, int x, int ph, int y, int pw) {
    for (int lane = 0; lane < N; lane++)
        for (int r = x + lane; r < x + ph && r < N; r += N) occupy_row(occ + r, 1, y, pw);
}
static void check_update(const u64 *old, int x, int ph, int y, int pw) {
    u64 want[N];
    memcpy(want, old, sizeof want);
    update_in_lds_order(want, x, ph, y, pw);
    for (int lane = 0; lane < N; lane++) {
        const u64 got = row_after_update1(old[lane], lane, x, ph, y, pw);
        if (got != want[lane]) FAIL("row_after_update1(%016llx, lane %d, x %d, ph %d, y %d, pw %d) = %016llx, occupy_row leaves %016llx", old[lane], lane, x, ph, y, pw, got, want[lane]);
        g_rows++;
    }
}
static void update_sweep() {
    const int rows = read_int();
    g_rng = (u64)read_int();
    u64 old[N];
    for (int fill = 0; fill < 2; fill++) {
        for (int r = 0; r < N; r++) old[r] = fill ? ~0ull : 0ull;
        for (int x = 0; x < N; x++)
            for (int ph = 1; x + ph <= N; ph++)
                for (int y = 0; y < N; y++)
                    for (int pw = 1; y + pw <= N; pw++) check_update(old, x, ph, y, pw);
    }
    // random old rows: every column range, with the lane first, inside, last, just above and just below the row range
    for (int k = 0; k < rows; k += N) {
        for (int r = 0; r < N; r++) old[r] = random_row(1 + (int)(rnd() % 15));
        const int x = (int)(rnd() % N), ph = 1 + (int)(rnd() % (N - x));
        for (int y = 0; y < N; y++)
            for (int pw = 1; y + pw <= N; pw++) check_update(old, x, ph, y, pw);
    }
}

// ---- (b) ----------------------------------------------------------------------------------------------------------------
struct Wave {  // one u64 per lane
    u64 v[N];
    Wave operator|(const Wave &o) const { Wave r; for (int i = 0; i < N; i++) r.v[i] = v[i] | o.v[i]; return r; }
};
// lane_down (csrc/pcb_device.h): the value held by lane + s, 0 beyond the wavefront
static Wave down(const Wave &a, int s) { Wave r; for (int i = 0; i < N; i++) r.v[i] = i + s < N ? a.v[i + s] : 0ull; return r; }

static bool check_fold(const u64 *occ, int ph, int pw) {
    Wave a;
    for (int lane = 0; lane < N; lane++) a.v[lane] = row1_hfold(occ[lane], pw);
    a = rows_vfold(a, ph, down);
    bool any = false;
    for (int lane = 0; lane < N; lane++) {
        const u64 got = lane + ph <= N ? row1_free_below(a.v[lane], N - pw + 1) : 0ull;
        u64 want = 0ull;
        if (lane + ph <= N) {
            u64 acc = 0ull;
            for (int r = lane; r < lane + ph; r++) acc |= occ[r];
            for (int j = 0; j + pw <= N; j++) {
                const u64 cells = (pw >= 64 ? ~0ull : ((1ull << pw) - 1ull)) << j;
                if (!(acc & cells)) want |= 1ull << j;
            }
        }
        if (got != want) FAIL("window %d x %d, row %d: the fold of the register rows gives %016llx, the definition %016llx", ph, pw, lane, got, want);
        any |= got != 0ull;
    }
    g_folds++;
    if (ph == pw) g_equal_sides++;
    if (!any) g_no_legal_cell++;
    return any;
}
static void fold_sweep() {
    const int grids = read_int();
    g_rng = (u64)read_int();
    std::vector<std::pair<int, int> > windows;
    for (int ph = 1; ph <= PCBENV_MAX_PINS_PER_COMPONENT && ph <= N; ph++)
        for (int pw = 1; ph * pw <= PCBENV_MAX_PINS_PER_COMPONENT && pw <= N; pw++) windows.push_back(std::make_pair(ph, pw));
    for (int n = read_int(); n > 0; n--) {
        const int ph = read_int(), pw = read_int();
        if (ph < 1 || ph > N || pw < 1 || pw > N) FAIL("malformed F line");
        windows.push_back(std::make_pair(ph, pw));
    }
    for (int g = 0; g < grids; g++) {
        u64 occ[N];
        // empty, full, then densities from one cell in sixteen to fifteen: from "fits almost anywhere" to "fits nowhere"
        for (int r = 0; r < N; r++) occ[r] = g == 0 ? 0ull : g == 1 ? ~0ull : random_row(1 + (g - 2) % 15);
        if (g == 2) for (int r = 0; r < N; r++) occ[r] = ~(r == N - 1 ? 1ull << 63 : 0ull);  // one free cell, in the corner
        if (g > 2 && (g & 1)) {  // every other grid: a handful of occupied cells, so that large windows fit somewhere
            for (int r = 0; r < N; r++) occ[r] = 0ull;
            for (int k = 0; k < 1 + g % 7; k++) occ[rnd() % N] |= 1ull << (rnd() % N);
        }
        const int x = (int)(rnd() % N), ph = 1 + (int)(rnd() % (N - x)), y = (int)(rnd() % N), pw = 1 + (int)(rnd() % (N - y));
        u64 updated[N];
        for (int lane = 0; lane < N; lane++) updated[lane] = row_after_update1(occ[lane], lane, x, ph, y, pw);
        for (size_t i = 0; i < windows.size(); i++) check_fold(updated, windows[i].first, windows[i].second);
    }
}

int main() {
    char tag[8];
    while (scanf("%7s", tag) == 1) {
        if (!strcmp(tag, "U")) update_sweep();
        else if (!strcmp(tag, "F")) fold_sweep();
        else FAIL("unknown case tag %s", tag);
    }
    printf("step_dataflow_check ok: %lld rows after an update, %lld window folds (%lld with equal sides, %lld with no legal cell left)\n",
           g_rows, g_folds, g_equal_sides, g_no_legal_cell);
    return 0;
}
