// pcb_puct_noise.hip -- k_puct_root_noise and its entry point pcbenv_puct_root_noise (include/pcbenv_noise.h): a draw
// from Dir(alpha) mixed into the priors of every root's children, on the device (what pcbenv/search.py:puct_root_noise does
// with 32 masked rounds of tensor code over [P, C]).  Part of libpcbenv.so (CDNA4 / gfx950 only); a translation unit of its
// own, host side included, so that nothing here can change the builds of the other kernels or of the other entry points.
//
// The noise of one root is pcb_puct_noise.h (noise_root: the text tools/puct_noise_check.cpp runs on the CPU); the kernel
// composes the same pieces on pcb_group.h's mapping: G = group_lanes(C) lanes per root, lane c at child c, 256 / G roots
// per workgroup.  Groups share nothing: no LDS, no barrier.  Every lane runs the rejection loop of its own child -- the
// loop diverges, at most 32 rounds of some 60 double operations, and is left as the compiler makes it.  S is formed by
// every lane of the group with the same loop over a lane shuffle of g, child after child: the order of the sum is the
// contract, so there is no tree reduction, and all lanes hold the same bits.
#include <hip/hip_runtime.h>

#include "pcb_group.h"
#include "pcb_tree_host.h"
#include "pcbenv_noise.h"
#include "pcb_puct_noise.h"

static_assert(PCBENV_MAX_TREE_CHILDREN == pcb_noise::MAX_CHILDREN, "pcbenv_noise.h and pcb_puct_noise.h name the same bound");
static_assert(sizeof(pcbenv_puct_noise_request) == 104 && offsetof(pcbenv_puct_noise_request, stream) == 96 &&
              offsetof(pcbenv_puct_noise_request, seed) == 24 && offsetof(pcbenv_puct_noise_request, alpha) == 40,
              "pcbenv/_noise_lib.py:PcbenvPuctNoiseRequest");

namespace {

using namespace pcb_noise;

// what the kernel needs of a request
struct NoiseArgs {
    int P, N, C, first_root;
    uint64_t seed, step_index;
    Params q;
    const int *num_children, *first_child;
    double *prior;
    int *noised;
    unsigned *errors;
};

template <int G> __global__ __launch_bounds__(pcb_group::BLOCK) void k_puct_root_noise(const NoiseArgs a) {
    PCB_GROUP_ENTER(G, a);
    (void)base;
    const long long row = (long long)p * a.N;
    const int k = a.num_children[row], fc = a.first_child[row];
    if (!due(a.noised[p], k)) return;  // the whole group
    if (!children_ok(fc, k, a.N, a.C)) {
        if (lane == 0 && a.errors) atomicOr(a.errors, ERR_TREE);
        return;
    }
    const bool mine = lane < k;
    const double g = mine ? gamma_draw(draw_base(a.seed, a.first_root + (int)p, a.step_index), lane, a.q) : 0.0;
    double S = 0.0;
    #pragma unroll
    for (int c = 0; c < G; c++) {
        const double gc = __shfl(g, c, G);
        S = c < k ? S + gc : S;
    }
    if (mine) {
        double *prior = a.prior + row + fc + lane;
        *prior = mixed(*prior, share(g, S, k), a.q);
    }
    if (lane == 0) a.noised[p] = 1;
}

}  // namespace

// ---- pcbenv_puct_root_noise ----------------------------------------------------------------------------------------
// As pcbenv_puct_move: every argument check before a device is touched, the null handle last; then one launch.
extern "C" int pcbenv_puct_root_noise(const pcbenv *cenv, const pcbenv_puct_noise_request *q) {
    using namespace pcb_tree_host;
    pcbenv *env = const_cast<pcbenv *>(cenv);  // the error text only
    PCB_TRY(check_request(env, q, "pcbenv_puct_noise_request"));
    PCB_TRY(check_extents(env, q));
    if (q->reserved != 0) return fail(env, PCBENV_EINVAL, "reserved must be 0");
    if (!(q->alpha >= ALPHA_MIN && q->alpha <= ALPHA_MAX)) return fail(env, PCBENV_EINVAL, "alpha must be in [0.01, 100]");
    if (!(q->eps >= 0.0 && q->eps <= 1.0)) return fail(env, PCBENV_EINVAL, "eps must be in [0, 1]");
    if (!q->num_children || !q->first_child || !q->prior || !q->noised) return fail(env, PCBENV_EINVAL, "null tree tensor");
    if (((uintptr_t)q->prior & 7u) != 0) return fail(env, PCBENV_EINVAL, "the float64 tensors must be 8-byte aligned");
    PCB_TREE_CHECKS_END(env, q);
    NoiseArgs a;
    a.P = q->num_roots; a.N = q->capacity; a.C = q->max_children; a.first_root = q->first_root;
    a.seed = q->seed; a.step_index = q->step_index; a.q = noise_params(q->alpha, q->eps);
    a.num_children = q->num_children; a.first_child = q->first_child; a.prior = q->prior; a.noised = q->noised;
    a.errors = (unsigned *)q->errors_dev;
    PCB_GROUP_LAUNCH(k_puct_root_noise, a, (hipStream_t)q->stream);
    HIP_TRY(env, hipGetLastError());
    return PCBENV_OK;
}
