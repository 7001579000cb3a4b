// pcb_puct.hip -- k_puct_advance and its entry point pcbenv_puct_advance (include/pcbenv_search.h): PUCT selection,
// expansion and backup of a batch of search trees on the device (what pcbenv/search.py:puct_search does with some
// hundred tensor operations per iteration).  Part of libpcbenv.so (CDNA4 / gfx950 only); a translation unit of its own,
// host side included, so that nothing here can change the builds of the other kernels or of the other entry points.
//
// The step of one root is pcb_puct.h (puct_init, puct_select, puct_absorb: the text tools/puct_model_check.cpp replays
// on the CPU); the kernel composes the same pieces with a group of G lanes per root: the mapping, the phases and the
// fence between them are pcb_group.h's.  The absorb and the descent of the select are pcb_puct_group.h's, which says what
// a lane loads and stores in them (k_gumbel_advance runs the same two); init is here: the slots of a root are contiguous,
// the lanes stride them.
#include <hip/hip_runtime.h>

#include "pcb_group.h"
#include "pcb_tree_host.h"
#include "pcbenv_search.h"
#include "pcb_puct_group.h"

static_assert(PCBENV_TREE_INIT == pcb_puct::PHASE_INIT && PCBENV_TREE_ABSORB == pcb_puct::PHASE_ABSORB &&
              PCBENV_TREE_SELECT == pcb_puct::PHASE_SELECT && PCBENV_MAX_TREE_CHILDREN == pcb_puct::MAX_CHILDREN,
              "pcbenv.h and pcb_puct.h name the same phases");
static_assert(sizeof(pcbenv_puct_request) == 224 && offsetof(pcbenv_puct_request, stream) == 216, "pcbenv/_search_lib.py:PcbenvPuctRequest");

namespace {

using namespace pcb_puct;
using pcb_group::BLOCK;

// what the kernel needs of a request
struct PuctArgs {
    int phases, P, N, C, T, K;
    double c_puct;
    int *num_nodes, *parent, *depth, *visits, *num_children, *first_child, *node_action;
    double *prior, *value_sum, *value_max;
    uint8_t *terminal;
    double *lo, *hi;
    int *selected, *path_len, *paths;
    const double *value;
    const uint8_t *leaf_terminal;
    const int *cand_count, *cand_actions;
    const float *cand_prior;
    unsigned *errors;
};

template <int G> __device__ inline void init_phase(const Root &r, int lane) {
    for (int s = lane; s < r.N; s += G) init_slot(r, s);
    if (lane == 0) init_scalars(r);
}

// puct_select, child first_child + c of the current node in lane c
template <int G> __device__ inline unsigned select_phase(const Root &r, const PuctArgs &a, int lane, int base) {
    unsigned err = 0u;
    const double lo = *r.lo, hi = *r.hi;
    int node = 0, d = 0;
    PCB_PUCT_DESCEND(G, r, a, lane, base, lo, hi, node, d, err)
    if (lane == 0) { a.selected[r.p] = node; a.path_len[r.p] = d; }
    return err;
}

template <int G> __global__ __launch_bounds__(BLOCK) void k_puct_advance(const PuctArgs a) {
    PCB_GROUP_ENTER(G, a);
    const Root r = root_of_group(a, (int)p, a.T);
    PCB_GROUP_PHASES(a, init_phase<G>(r, lane), absorb_phase<G>(r, a, lane, base), select_phase<G>(r, a, lane, base));
}

}  // namespace

// ---- pcbenv_puct_advance -----------------------------------------------------------------------------------------
// As pcbenv_tree_advance: every argument check before a device is touched, the null handle last; then one launch.
extern "C" int pcbenv_puct_advance(const pcbenv *cenv, const pcbenv_puct_request *q) {
    using namespace pcb_tree_host;
    pcbenv *env = const_cast<pcbenv *>(cenv);  // the error text only
    PCB_TRY(check_search_request(env, q, "pcbenv_puct_request"));
    const Phases ph = phases_of(q->phases);
    PCB_TRY(check_puct_candidates(env, q, ph));
    if (q->reserved != 0) return fail(env, PCBENV_EINVAL, "reserved must be 0");
    PCB_TRY(check_puct_tree(env, q));
    PCB_TRY(check_exchange(env, q, ph));
    PCB_TRY(check_puct_inputs(env, q, ph));
    PCB_TRY(check_puct_doubles(env, q, ph.absorb ? q->value : 0));
    PCB_TRY(check_cand_prior(env, q, ph));
    PCB_TREE_CHECKS_END(env, q);
    PuctArgs a;
    puct_search_args(a, q);
    PCB_GROUP_LAUNCH(k_puct_advance, a, (hipStream_t)q->stream);
    HIP_TRY(env, hipGetLastError());
    return PCBENV_OK;
}
