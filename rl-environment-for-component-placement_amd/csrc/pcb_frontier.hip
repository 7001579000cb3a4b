// pcb_frontier.hip -- k_frontier_advance and its entry point pcbenv_frontier_advance (include/pcbenv_frontier.h): one depth
// of a beam search over partial placements -- per root, the best finished row recorded, the W best of the F = W * K
// evaluated rows kept, and the paths of their children written (what pcbenv/search.py:frontier_advance does in tensor
// code).  Part of libpcbenv.so (CDNA4 / gfx950 only); a translation unit of its own, host side included, so that nothing
// here can change the build of the other entry points.
//
// The step of one root is pcb_frontier.h (the text tools/frontier_check.cpp replays on the CPU); the kernel composes the
// same pieces with ONE WAVEFRONT per root, four roots per 256-thread workgroup, row i = j * 64 + lane of the root in
// register j of its lane: R = ceil(F / 64) registers per lane, rounded up to a power of two, a template argument, so the
// register arrays are indexed by constants only.  Wavefronts share nothing: no LDS, no barrier, no atomics but the error
// word's, and a wavefront whose root does not exist exits whole.
//   steps 1-3  one coalesced load round per register: path_len, then leaf_terminal, value, cand_count and cum_logp of the
//              live rows.  The best finished row is a wave argmax of (value, i); the order of the expandable rows is W
//              rounds of the same argmax over the scores in registers -- a lane's best first, then a shuffle butterfly
//              whose order is total (score descending, the lower i), so every lane ends with the same row and the result
//              is the serial model's whatever the lanes did.  Lane w keeps i_w.
//   step 4     lanes go along the out slots: slot j * 64 + lane = w * K + c takes i_w from lane w by a shuffle, and for a
//              fixed path row d the 64 stores of a register round are 64 consecutive rows of paths_out.  The K children of
//              a parent read the same words of paths_in in the same instruction: one fetch.
// The in and out sets are different memory (the entry point compares their byte ranges), so no phase reads what another
// lane has stored and there is no fence.
#include <hip/hip_runtime.h>

#include "pcb_tree_host.h"
#include "pcbenv_frontier.h"
#include "pcb_frontier.h"

static_assert(PCBENV_FRONTIER_INIT == pcb_frontier::PHASE_INIT && PCBENV_FRONTIER_ADVANCE == pcb_frontier::PHASE_ADVANCE &&
              PCBENV_MAX_FRONTIER_WIDTH == pcb_frontier::MAX_WIDTH && PCBENV_MAX_FRONTIER_CANDIDATES == pcb_frontier::MAX_CANDIDATES &&
              PCBENV_MAX_FRONTIER_ROWS == pcb_frontier::MAX_ROWS, "pcbenv_frontier.h and pcb_frontier.h name the same phases and bounds");
static_assert(sizeof(pcbenv_frontier_request) == 184 && offsetof(pcbenv_frontier_request, stream) == 176 &&
              offsetof(pcbenv_frontier_request, paths_in) == 40, "pcbenv/_frontier_lib.py:PcbenvFrontierRequest");

namespace {

using namespace pcb_frontier;

constexpr int BLOCK = 256, LANES = 64, ROOTS_PER_BLOCK = BLOCK / LANES;
constexpr int NONE = 0x7fffffff;  // the row of a lane that has none: it loses against any row, whatever its score
static_assert(MAX_WIDTH <= LANES, "lane w keeps the kept row of rank w");

// The row that goes before all others, over the lanes of a wavefront: every lane ends with the same (s, i).
__device__ inline void wave_first(double &s, int &i) {
#pragma unroll
    for (int o = LANES / 2; o > 0; o >>= 1) {
        const double so = __shfl_xor(s, o);
        const int io = __shfl_xor(i, o);
        const bool other = io != NONE && (i == NONE || goes_before(so, io, s, i));
        s = other ? so : s;
        i = other ? io : i;
    }
}

template <int R> __global__ __launch_bounds__(BLOCK) void k_frontier_advance(const Frontier f) {
    const unsigned p = blockIdx.x * ROOTS_PER_BLOCK + threadIdx.x / LANES;
    if (p >= (unsigned)f.P) return;
    const int lane = threadIdx.x % LANES;
    const int F = rows_of(f.W, f.K), rows = f.P * F;
    const long long row0 = (long long)p * F;
    if (f.phases & PHASE_INIT) {
        for (int i = lane; i < F; i += LANES) init_row(f, row0 + i, i);
        if (lane == 0) init_scalars(f, (int)p);
        return;
    }
    // steps 1 to 3: the rows into registers
    double key[R];
    bool open[R];  // expandable and not yet kept
    bool damaged = false;
    double fin_v = 0.0;
    int fin_i = NONE, fin_len = 0;
#pragma unroll
    for (int j = 0; j < R; j++) {
        const int i = j * LANES + lane;
        double s = 0.0;
        bool expandable = false;
        const long long r = row0 + i;
        const int len = i < F ? f.path_len_in[r] : -1;
        damaged = damaged || is_damaged(len, f.T);
        if (is_live(len, f.T)) {
            const double value = f.value[r];
            if (f.leaf_terminal[r] != 0) {
                const double v = not_nan(value);
                if (fin_i == NONE || v > fin_v) { fin_v = v; fin_i = i; fin_len = len; }  // a lane's rows come in increasing i
            } else if (is_expandable(len, f.T, kept_candidates(f.cand_count[r], f.K))) {
                s = score_of(value, f.prior_weight, &f.cum_logp_in[r]);
                expandable = true;
            }
        }
        key[j] = s;  // one store per element, outside the branches: the arrays stay single registers
        open[j] = expandable;
    }
    // step 2: the first of the finished rows with the largest value is the one the serial walk ends with
    wave_first(fin_v, fin_i);
    if (fin_i != NONE) {
        fin_len = __shfl(fin_len, fin_i % LANES);
        if (is_better(fin_v, f.best_value[p], f.best_len[p])) {
            const int src = (int)(row0 + fin_i);
            for (int x = lane; x < 3 * fin_len; x += LANES) f.best_path[step_major(x / 3, f.P, (int)p, x % 3)] = f.paths_in[step_major(x / 3, rows, src, x % 3)];
            if (lane == 0) { f.best_value[p] = fin_v; f.best_len[p] = fin_len; }
        }
    }
    // step 3: W rounds
    int kept_row = 0, n = 0;
    for (; n < f.W; n++) {
        double s = 0.0;
        int i = NONE;
#pragma unroll
        for (int j = 0; j < R; j++)
            if (open[j] && (i == NONE || key[j] > s)) { s = key[j]; i = j * LANES + lane; }
        wave_first(s, i);
        if (i == NONE) break;
#pragma unroll
        for (int j = 0; j < R; j++) open[j] = open[j] && j * LANES + lane != i;
        if (lane == n) kept_row = i;
    }
    // step 4: lanes along the out slots
    int live = 0;
#pragma unroll 1  // no register array in here: one copy of the body
    for (int j = 0; j < R; j++) {
        const int slot = j * LANES + lane;
        const int w = slot / f.K, c = slot - w * f.K;
        const int i_w = __shfl(kept_row, w % LANES);
        bool child = false;
        if (slot < F) {
            const long long row = row0 + slot;
            long long parent = 0;
            int len = 0;
            if (w < n) {
                parent = row0 + i_w;
                len = f.path_len_in[parent];
                child = c < kept_candidates(f.cand_count[parent], f.K);
            }
            if (child) {
                make_child(f, row, parent, i_w, len, c);
                for (int d = 0; d <= len; d++) {
                    const int a0 = child_path(f, rows, parent, len, c, d, 0), a1 = child_path(f, rows, parent, len, c, d, 1), a2 = child_path(f, rows, parent, len, c, d, 2);
                    int *const dst = f.paths_out + step_major(d, rows, (int)row, 0);
                    dst[0] = a0; dst[1] = a1; dst[2] = a2;
                }
            } else {
                no_child(f, row);
            }
        }
        live += __popcll(__ballot(child));
    }
    if (lane == 0) {
        f.live[p] = live;
    }
    if (__ballot(damaged) != 0ull && lane == 0 && f.errors) atomicOr(f.errors, (unsigned)ERR_ROW);
}

// the byte ranges [a, a + na) and [b, b + nb) share a byte
inline bool overlap(const void *a, unsigned long long na, const void *b, unsigned long long nb) {
    const uintptr_t x = (uintptr_t)a, y = (uintptr_t)b;
    return x < y + nb && y < x + na;
}

}  // namespace

// ---- pcbenv_frontier_advance ---------------------------------------------------------------------------------------
// As pcbenv_puct_advance_leaves: every argument check before a device is touched, the null handle last; then one launch.
extern "C" int pcbenv_frontier_advance(const pcbenv *cenv, const pcbenv_frontier_request *q) {
    using namespace pcb_tree_host;
    pcbenv *env = const_cast<pcbenv *>(cenv);  // the error text only
    PCB_TRY(check_request(env, q, "pcbenv_frontier_request"));
    if (q->phases == 0 || (q->phases & ~(PCBENV_FRONTIER_INIT | PCBENV_FRONTIER_ADVANCE)) != 0) return fail(env, PCBENV_EINVAL, "phases must be INIT or ADVANCE");
    if (q->phases == (PCBENV_FRONTIER_INIT | PCBENV_FRONTIER_ADVANCE)) return fail(env, PCBENV_EINVAL, "phases: INIT cannot be combined with ADVANCE");
    const bool advance = q->phases == PCBENV_FRONTIER_ADVANCE;
    if (q->num_roots < 0) return fail(env, PCBENV_EINVAL, "num_roots must not be negative");
    if (q->width < 1 || q->width > PCBENV_MAX_FRONTIER_WIDTH) return fail(env, PCBENV_EINVAL, "width must be in [1, 64]");
    if (q->num_candidates < 1 || q->num_candidates > PCBENV_MAX_FRONTIER_CANDIDATES) return fail(env, PCBENV_EINVAL, "num_candidates must be in [1, 64]");
    const long long F = (long long)q->width * q->num_candidates;
    if (F > PCBENV_MAX_FRONTIER_ROWS) return fail(env, PCBENV_EINVAL, "width * num_candidates must not exceed 1024");
    if (q->max_steps < 1) return fail(env, PCBENV_EINVAL, "max_steps must be at least 1");
    if ((long long)q->num_roots * F > 0x7fffffffLL) return fail(env, PCBENV_EINVAL, "num_roots * width * num_candidates must not exceed 2^31 - 1");
    if (!(q->prior_weight - q->prior_weight == 0.0)) return fail(env, PCBENV_EINVAL, "prior_weight must be finite");
    if (q->reserved != 0 || q->reserved2 != 0) return fail(env, PCBENV_EINVAL, "reserved and reserved2 must be 0");
    if (!q->paths_out || !q->path_len_out || !q->cum_logp_out || !q->parent_row || !q->live || !q->best_value || !q->best_len)
        return fail(env, PCBENV_EINVAL, "null paths_out, path_len_out, cum_logp_out, parent_row, live, best_value or best_len");
    if (advance && (!q->paths_in || !q->path_len_in || !q->cum_logp_in || !q->best_path || !q->value || !q->leaf_terminal || !q->cand_count ||
                    !q->cand_actions || !q->cand_prior))
        return fail(env, PCBENV_EINVAL, "null paths_in, path_len_in, cum_logp_in, best_path, value, leaf_terminal, cand_count, cand_actions or cand_prior with ADVANCE");
    const uintptr_t doubles = (uintptr_t)q->cum_logp_out | (uintptr_t)q->best_value | (advance ? (uintptr_t)q->cum_logp_in | (uintptr_t)q->value : 0);
    if ((doubles & 7u) != 0) return fail(env, PCBENV_EINVAL, "the float64 tensors must be 8-byte aligned");
    if (advance && ((uintptr_t)q->cand_prior & 3u) != 0) return fail(env, PCBENV_EINVAL, "cand_prior must be 4-byte aligned");
    const unsigned long long R = (unsigned long long)q->num_roots * (unsigned long long)F;
    if (advance && (overlap(q->paths_in, R * q->max_steps * 12ull, q->paths_out, R * q->max_steps * 12ull) || overlap(q->path_len_in, R * 4ull, q->path_len_out, R * 4ull) ||
                    overlap(q->cum_logp_in, R * 8ull, q->cum_logp_out, R * 8ull)))
        return fail(env, PCBENV_EINVAL, "an in tensor overlaps its out twin");
    PCB_TREE_CHECKS_END(env, q);
    Frontier f;
    f.phases = q->phases; f.P = q->num_roots; f.W = q->width; f.K = q->num_candidates; f.T = q->max_steps; f.prior_weight = q->prior_weight;
    f.paths_in = q->paths_in; f.path_len_in = q->path_len_in; f.cum_logp_in = q->cum_logp_in;
    f.paths_out = q->paths_out; f.path_len_out = q->path_len_out; f.cum_logp_out = q->cum_logp_out;
    f.parent_row = q->parent_row; f.live = q->live; f.best_value = q->best_value; f.best_len = q->best_len; f.best_path = q->best_path;
    f.value = q->value; f.leaf_terminal = q->leaf_terminal; f.cand_count = q->cand_count; f.cand_actions = q->cand_actions; f.cand_prior = q->cand_prior;
    f.errors = (unsigned *)q->errors_dev;
    const dim3 grid((unsigned)(((long long)f.P + ROOTS_PER_BLOCK - 1) / ROOTS_PER_BLOCK)), block(BLOCK);
    hipStream_t stream = (hipStream_t)q->stream;
    const int per_lane = (int)((F + LANES - 1) / LANES);
    if (per_lane <= 1) hipLaunchKernelGGL(k_frontier_advance<1>, grid, block, 0, stream, f);
    else if (per_lane <= 2) hipLaunchKernelGGL(k_frontier_advance<2>, grid, block, 0, stream, f);
    else if (per_lane <= 4) hipLaunchKernelGGL(k_frontier_advance<4>, grid, block, 0, stream, f);
    else if (per_lane <= 8) hipLaunchKernelGGL(k_frontier_advance<8>, grid, block, 0, stream, f);
    else hipLaunchKernelGGL(k_frontier_advance<16>, grid, block, 0, stream, f);
    HIP_TRY(env, hipGetLastError());
    return PCBENV_OK;
}
