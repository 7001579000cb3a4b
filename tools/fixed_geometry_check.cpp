// fixed_geometry_check.cpp -- CPU check of the predicate that chooses the geometry-fixed build of k_step
// (csrc/pcb_layout.h fixed_geometry_applies, the only header included): the 64 x 64 pin and spatial kinds on one
// wavefront, in place, one transition per launch select it; every near miss does not; and the constants the fixed build
// writes over its parameter block are what state_layout gives a real 64 x 64 configuration.
// Build and run (tests/test_fixed_geometry_predicate.py does that):
//   g++ -std=c++17 -fsanitize=address,undefined -Iinclude -Irl-environment-for-component-placement_amd/csrc
//       -o fixed_geometry_check tools/fixed_geometry_check.cpp && ./fixed_geometry_check
#include "pcb_layout.h"

#include <stdio.h>
#include <stdlib.h>

#include <initializer_list>

using namespace pcb_layout;

static int g_checks = 0;
#define CHECK(cond)                                                                             \
    do {                                                                                        \
        g_checks++;                                                                             \
        if (!(cond)) { fprintf(stderr, "fixed_geometry_check: %s fails (line %d)\n", #cond, __LINE__); exit(1); } \
    } while (0)

// a launch the fixed build serves: kind, 64 x 64, four orientations, one word per bit row, one wavefront, in place, one transition
static StepShape good(int kind) { return StepShape{kind, 64, 64, 4, 1, WAVE, 1, 1, false, true, true}; }

int main() {
    for (int kind : {PCBENV_PIN, PCBENV_SPATIAL}) {
        CHECK(fixed_geometry_applies(good(kind)));
        StepShape s = good(kind);
        s.H = 64; s.W = 48; CHECK(!fixed_geometry_applies(s));                 // 64 x 48
        s = good(kind); s.H = 48; s.W = 64; CHECK(!fixed_geometry_applies(s));  // 48 x 64
        s = good(kind); s.H = 32; s.W = 32; CHECK(!fixed_geometry_applies(s));  // 32 x 32
        s = good(kind); s.H = 128; s.W = 128; s.WW = 2; CHECK(!fixed_geometry_applies(s));  // 128 x 128
        s = good(kind); s.H = 128; s.W = 128; CHECK(!fixed_geometry_applies(s));             // (whatever WW says)
        s = good(kind); s.WW = 2; CHECK(!fixed_geometry_applies(s));
        s = good(kind); s.threads = MAX_NT; CHECK(!fixed_geometry_applies(s));  // four wavefronts
        s = good(kind); s.num_slots = 2; CHECK(!fixed_geometry_applies(s));     // trajectory layout
        s = good(kind); s.num_slots = 17; CHECK(!fixed_geometry_applies(s));
        s = good(kind); s.num_steps = 2; CHECK(!fixed_geometry_applies(s));     // persistent rollout
        s = good(kind); s.num_steps = 16; CHECK(!fixed_geometry_applies(s));
        s = good(kind); s.cells_aligned16 = false; CHECK(!fixed_geometry_applies(s));  // a misaligned cell tensor
        s = good(kind); s.enabled = false; CHECK(!fixed_geometry_applies(s));   // PCBENV_OPT_FIXED_GEOMETRY = 0
        s = good(kind); s.routes = true; CHECK(!fixed_geometry_applies(s));     // beam / both rewards: the routed builds
        s = good(kind); s.O = 2; CHECK(!fixed_geometry_applies(s));
        // the constants of the fixed build against the layout of real configurations of that grid
        const FixedGeometry f = fixed_geometry(kind);
        CHECK(f.H == 64 && f.W == 64 && f.O == 4 && f.WW == 1);
        for (int C : {1, 8, 16, PCBENV_MAX_COMPONENTS}) for (int N : {1, 8, PCBENV_MAX_NETS}) for (int m : {1, 3, 8}) {
            int P = N * PCBENV_MAX_PINS_PER_NET < C * m * m ? N * PCBENV_MAX_PINS_PER_NET : C * m * m;
            if (P > PCBENV_MAX_PINS) P = PCBENV_MAX_PINS;
            const Layout l = state_layout(Geometry{kind, 64, 64, C, P, N, m, m, WAVE, PCBENV_REWARD_CENTROID, 1});
            CHECK(l.WW == f.WW && l.offOcc == f.offOcc && l.offVm == f.offVm && l.offComps == f.offComps);
            CHECK(fold_across_lanes(l.WW, WAVE, f.H));  // window_mask of the fixed build never stages rows at hf
        }
    }
    for (int kind : {PCBENV_SQUARE, PCBENV_RECT}) {  // the kinds without pins: never, whatever else holds
        StepShape s = good(kind);
        CHECK(!fixed_geometry_applies(s));
        s.O = kind == PCBENV_SQUARE ? 1 : 2;
        CHECK(!fixed_geometry_applies(s));
    }
    // the alignment test behind cells_aligned16
    alignas(16) static unsigned char buf[64];
    CHECK(aligned16(buf) && aligned16(buf + 16) && aligned16(nullptr));
    for (int k = 1; k < 16; k++) CHECK(!aligned16(buf + k));
    printf("fixed_geometry_check ok: %d checks\n", g_checks);
    return 0;
}
