// pcb_frontier_sample.hip -- k_frontier_sample and its entry point pcbenv_frontier_sample
// (include/pcbenv_frontier_sample.h): one depth of a stochastic beam search over partial placements -- per root, the best
// finished row recorded, the W contenders with the largest perturbed log-probability G kept (set entries, finished rows,
// which enter the set, and expandable rows, whose children are written with their own G), what
// pcbenv/search.py:frontier_sample_advance does in tensor code.  Part of libpcbenv.so (CDNA4 / gfx950 only); a translation
// unit of its own, host side included, so that nothing here can change the build of the other entry points.
//
// The step of one root is pcb_frontier_sample.h (the text tools/frontier_sample_check.cpp replays on the CPU); the kernel
// composes the same pieces with the mapping of pcb_frontier.hip: ONE WAVEFRONT per root, four roots per 256-thread
// workgroup, row i = j * 64 + lane of the root in register j of its lane, R registers per lane a template argument.  No
// LDS, no barrier, no atomics but the error word's.
//   steps 1-3  one coalesced load round per register: path_len, then leaf_terminal, value, cand_count and gumbel_in of the
//              live rows.  Lane j < W additionally holds set slot j, one more contender.
//   step 4     W rounds of the shuffle argmax of pcb_frontier.hip over (key, id): a lane's best first, then the butterfly,
//              whose order is total, so every lane ends with the same winner.  Its owner says what it is: a set entry
//              survives in its lane, a finished row of rank m is noted in lane m, an expandable row of rank w in lane w.
//              The slots without a surviving entry are a ballot; a lane's rank among them is the finished row it takes.
//   step 5     lanes go along the out slots as in pcb_frontier.hip.  The K children of a parent sit in consecutive lanes:
//              Z, the largest phi_c + g_c of a parent, is a segmented shuffle maximum (a scan up and a scan down that stop
//              at a segment's ends), and a parent whose children straddle two register rounds takes the other round's part
//              from lane 63 or lane 0.  K <= 64, so a segment touches two rounds at the most.
// The in and out sets are different memory (the entry point compares their byte ranges); a lane reads its set slot before
// any lane writes one, and writes no other.
#include <hip/hip_runtime.h>

#include "pcb_tree_host.h"
#include "pcbenv_frontier_sample.h"
#include "pcb_frontier_sample.h"

static_assert(sizeof(pcbenv_frontier_sample_request) == 248 && offsetof(pcbenv_frontier_sample_request, stream) == 240 &&
              offsetof(pcbenv_frontier_sample_request, paths_in) == 48 && offsetof(pcbenv_frontier_sample_request, seed) == 24 &&
              offsetof(pcbenv_frontier_sample_request, first_root) == 40, "pcbenv/_frontier_sample_lib.py:PcbenvFrontierSampleRequest");

namespace {

using namespace pcb_frontier_sample;

constexpr int BLOCK = 256, LANES = 64, ROOTS_PER_BLOCK = BLOCK / LANES;
constexpr int NONE = 0x7fffffff;  // the id of a lane that has no contender: it loses against any, whatever its key
static_assert(MAX_WIDTH <= LANES, "lane j holds set slot j and the winners of rank j");

// The contender that goes before all others, over the lanes of a wavefront: every lane ends with the same (s, i).
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

// The largest x over the lanes around this one that hold the same w (consecutive lanes): -inf where a lane has nothing.
__device__ inline double segment_max(double x, int w, int lane) {
    double up = x, down = x;
#pragma unroll
    for (int o = 1; o < LANES; o <<= 1) {
        const double xu = __shfl_up(up, o), xd = __shfl_down(down, o);
        const int wu = __shfl_up(w, o), wd = __shfl_down(w, o);
        if (lane >= o && wu == w) up = larger(up, xu);
        if (lane + o < LANES && wd == w) down = larger(down, xd);
    }
    return larger(up, down);
}

template <int R> __global__ __launch_bounds__(BLOCK) void k_frontier_sample(const Sample q) {
    const Frontier &f = q.f;
    const unsigned p = blockIdx.x * ROOTS_PER_BLOCK + threadIdx.x / LANES;
    if (p >= (unsigned)f.P) return;
    const int lane = threadIdx.x % LANES;
    const int W = f.W, F = rows_of(f.W, f.K), rows = f.P * F, slots = f.P * W;
    const long long row0 = (long long)p * F, slot0 = (long long)p * W;
    if (f.phases & PHASE_INIT) {
        for (int i = lane; i < F; i += LANES) { init_row(f, row0 + i, i); init_gumbel(q, row0 + i, i); }
        if (lane < W) q.set_len[slot0 + lane] = -1;
        if (lane == 0) init_scalars(f, (int)p);
        return;
    }
    // step 3: set slot `lane`
    const int entry_len = lane < W ? q.set_len[slot0 + lane] : -1;
    const bool set_damaged = is_damaged(entry_len, f.T), entry = is_entry(entry_len, f.T);
    const double entry_key = entry ? not_nan(q.set_gumbel[slot0 + lane]) : 0.0;
    bool entry_open = entry;
    // steps 1 to 3: the rows into registers
    double key[R];
    bool open[R];      // a contender not yet taken
    bool finished[R];  // a finished row (open or taken)
    bool damaged = false;
    double fin_v = 0.0;
    int fin_i = NONE, fin_len = 0;
#pragma unroll
    for (int j = 0; j < R; j++) {
        const int i = j * LANES + lane;
        bool contender = false, over = false;
        const long long r = row0 + i;
        const int len = i < F ? f.path_len_in[r] : -1;
        damaged = damaged || is_damaged(len, f.T);
        if (is_live(len, f.T)) {
            if (f.leaf_terminal[r] != 0) {
                const double v = not_nan(f.value[r]);
                if (fin_i == NONE || v > fin_v) { fin_v = v; fin_i = i; fin_len = len; }  // a lane's rows come in increasing i
                contender = over = true;
            } else {
                contender = is_expandable(len, f.T, kept_candidates(f.cand_count[r], f.K));
            }
        }
        key[j] = contender ? not_nan(q.gumbel_in[r]) : 0.0;  // one store per element, outside the branches
        open[j] = contender;
        finished[j] = over;
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
    // step 4: W rounds over (key, id), id = j for set slot j and W + i for row i
    int kept_row = 0, n = 0;          // lane w: the kept parent of rank w
    int entered_row = 0, entered = 0; // lane m: the finished winner of rank m
    double entered_key = 0.0;
    for (int round = 0; round < W; round++) {
        double s = entry_key;
        int id = entry_open ? lane : NONE;
#pragma unroll
        for (int j = 0; j < R; j++)
            if (open[j] && (id == NONE || goes_before(key[j], W + j * LANES + lane, s, id))) { s = key[j]; id = W + j * LANES + lane; }
        wave_first(s, id);
        if (id == NONE) break;
        bool mine_finished = false;
        entry_open = entry_open && id != lane;
#pragma unroll
        for (int j = 0; j < R; j++) {
            const bool mine = W + j * LANES + lane == id;
            mine_finished = mine_finished || (mine && finished[j]);
            open[j] = open[j] && !mine;
        }
        if (id < W) continue;  // a set entry survives in its lane: entry && !entry_open
        const int i = id - W;
        if (__shfl((int)mine_finished, i % LANES) != 0) {
            if (lane == entered) { entered_row = i; entered_key = s; }
            entered++;
        } else {
            if (lane == n) kept_row = i;
            n++;
        }
    }
    // the set: entries that did not win are freed; finished winners go, in rank order, to the lowest slots without a survivor
    {
        const bool survivor = entry && !entry_open;
        const bool vacant = lane < W && !survivor;
        const unsigned long long vacancies = __ballot(vacant);
        const int rank = __popcll(vacancies & ((1ull << lane) - 1ull));
        const int i = __shfl(entered_row, rank % LANES);
        const double k = __shfl(entered_key, rank % LANES);
        if (vacant && rank < entered) {
            const long long r = row0 + i, s = slot0 + lane;
            const int len = f.path_len_in[r];
            enter_set(q, s, r, len, k);
            for (int d = 0; d < len; d++) {
                const int *const src = f.paths_in + step_major(d, rows, (int)r, 0);
                int *const dst = q.set_path + step_major(d, slots, (int)s, 0);
                const int a0 = src[0], a1 = src[1], a2 = src[2];
                dst[0] = a0; dst[1] = a1; dst[2] = a2;
            }
        } else if (entry && !survivor) {
            q.set_len[slot0 + lane] = -1;
        }
    }
    // step 5: lanes along the out slots.  First pcb_frontier.hip's step 4 ...
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
    if (lane == 0) f.live[p] = live;
    // ... then G of the children: phi_c + g_c into registers (a lane reads back the cum_logp_out it stored itself), Z by
    // segments, and the truncated Gumbel
    const uint64_t base = pcb_noise::draw_base(q.seed, q.first_root + (int)p, q.step_index);
    double Gc[R], Z[R];
#pragma unroll
    for (int j = 0; j < R; j++) {
        const int slot = j * LANES + lane;
        const int w = slot / f.K, c = slot - w * f.K;
        const int i_w = __shfl(kept_row, w % LANES);
        double g = neg_inf();
        if (slot < F && w < n && f.path_len_out[row0 + slot] >= 0) {
            const double phi = f.cum_logp_out[row0 + slot];
            if (is_finite(phi)) g = phi + gumbel_of(base, c, i_w);
        }
        Gc[j] = g;
        Z[j] = segment_max(g, w, lane);
    }
#pragma unroll
    for (int j = 0; j + 1 < R; j++) {  // a parent whose children end round j and begin round j + 1
        const int w_tail = (j * LANES + LANES - 1) / f.K, w_head = ((j + 1) * LANES) / f.K;
        const double tail = __shfl(Z[j], LANES - 1), head = __shfl(Z[j + 1], 0);
        if (w_tail == w_head) {
            if ((j * LANES + lane) / f.K == w_tail) Z[j] = larger(Z[j], head);
            if (((j + 1) * LANES + lane) / f.K == w_head) Z[j + 1] = larger(Z[j + 1], tail);
        }
    }
#pragma unroll
    for (int j = 0; j < R; j++) {
        const int slot = j * LANES + lane;
        const int w = slot / f.K;
        const int i_w = __shfl(kept_row, w % LANES);
        if (slot < F && w < n && f.path_len_out[row0 + slot] >= 0) {
            const double G_S = not_nan(q.gumbel_in[row0 + i_w]);
            const double phi = f.cum_logp_out[row0 + slot];
            q.gumbel_out[row0 + slot] = child_gumbel(G_S, phi, Gc[j], Z[j]);
        }
    }
    const unsigned err = (__ballot(damaged) != 0ull ? (unsigned)ERR_ROW : 0u) | (__ballot(set_damaged) != 0ull ? (unsigned)ERR_SET : 0u);
    if (err != 0u && lane == 0 && f.errors) atomicOr(f.errors, err);
}

// the byte ranges [a, a + na) and [b, b + nb) share a byte
inline bool overlap(const void *a, unsigned long long na, const void *b, unsigned long long nb) {
    const uintptr_t x = (uintptr_t)a, y = (uintptr_t)b;
    return x < y + nb && y < x + na;
}

}  // namespace

// ---- pcbenv_frontier_sample ----------------------------------------------------------------------------------------
// As pcbenv_frontier_advance: every argument check before a device is touched, the null handle last; then one launch.
extern "C" int pcbenv_frontier_sample(const pcbenv *cenv, const pcbenv_frontier_sample_request *q) {
    using namespace pcb_tree_host;
    pcbenv *env = const_cast<pcbenv *>(cenv);  // the error text only
    PCB_TRY(check_request(env, q, "pcbenv_frontier_sample_request"));
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
    if (q->first_root < 0 || (long long)q->first_root + q->num_roots > 0x7fffffffLL) return fail(env, PCBENV_EINVAL, "first_root must not be negative and first_root + num_roots must not exceed 2^31 - 1");
    if (q->reserved != 0) return fail(env, PCBENV_EINVAL, "reserved must be 0");
    if (!q->paths_out || !q->path_len_out || !q->cum_logp_out || !q->gumbel_out || !q->parent_row || !q->live || !q->best_value || !q->best_len ||
        !q->set_len || !q->set_gumbel || !q->set_logp || !q->set_value || !q->set_path)
        return fail(env, PCBENV_EINVAL, "null paths_out, path_len_out, cum_logp_out, gumbel_out, parent_row, live, best_value, best_len, set_len, set_gumbel, set_logp, set_value or set_path");
    if (advance && (!q->paths_in || !q->path_len_in || !q->cum_logp_in || !q->gumbel_in || !q->best_path || !q->value || !q->leaf_terminal || !q->cand_count ||
                    !q->cand_actions || !q->cand_prior))
        return fail(env, PCBENV_EINVAL, "null paths_in, path_len_in, cum_logp_in, gumbel_in, best_path, value, leaf_terminal, cand_count, cand_actions or cand_prior with ADVANCE");
    const uintptr_t doubles = (uintptr_t)q->cum_logp_out | (uintptr_t)q->gumbel_out | (uintptr_t)q->best_value | (uintptr_t)q->set_gumbel | (uintptr_t)q->set_logp |
                              (uintptr_t)q->set_value | (advance ? (uintptr_t)q->cum_logp_in | (uintptr_t)q->gumbel_in | (uintptr_t)q->value : 0);
    if ((doubles & 7u) != 0) return fail(env, PCBENV_EINVAL, "the float64 tensors must be 8-byte aligned");
    if (advance && ((uintptr_t)q->cand_prior & 3u) != 0) return fail(env, PCBENV_EINVAL, "cand_prior must be 4-byte aligned");
    const unsigned long long R = (unsigned long long)q->num_roots * (unsigned long long)F;
    if (advance && (overlap(q->paths_in, R * q->max_steps * 12ull, q->paths_out, R * q->max_steps * 12ull) || overlap(q->path_len_in, R * 4ull, q->path_len_out, R * 4ull) ||
                    overlap(q->cum_logp_in, R * 8ull, q->cum_logp_out, R * 8ull) || overlap(q->gumbel_in, R * 8ull, q->gumbel_out, R * 8ull)))
        return fail(env, PCBENV_EINVAL, "an in tensor overlaps its out twin");
    PCB_TREE_CHECKS_END(env, q);
    Sample s;
    Frontier &f = s.f;
    f.phases = q->phases; f.P = q->num_roots; f.W = q->width; f.K = q->num_candidates; f.T = q->max_steps; f.prior_weight = 0.0;
    f.paths_in = q->paths_in; f.path_len_in = q->path_len_in; f.cum_logp_in = q->cum_logp_in;
    f.paths_out = q->paths_out; f.path_len_out = q->path_len_out; f.cum_logp_out = q->cum_logp_out;
    f.parent_row = q->parent_row; f.live = q->live; f.best_value = q->best_value; f.best_len = q->best_len; f.best_path = q->best_path;
    f.value = q->value; f.leaf_terminal = q->leaf_terminal; f.cand_count = q->cand_count; f.cand_actions = q->cand_actions; f.cand_prior = q->cand_prior;
    f.errors = (unsigned *)q->errors_dev;
    s.seed = q->seed; s.step_index = q->step_index; s.first_root = q->first_root; s.gumbel_in = q->gumbel_in; s.gumbel_out = q->gumbel_out;
    s.set_len = q->set_len; s.set_gumbel = q->set_gumbel; s.set_logp = q->set_logp; s.set_value = q->set_value; s.set_path = q->set_path;
    const dim3 grid((unsigned)(((long long)f.P + ROOTS_PER_BLOCK - 1) / ROOTS_PER_BLOCK)), block(BLOCK);
    hipStream_t stream = (hipStream_t)q->stream;
    const int per_lane = (int)((F + LANES - 1) / LANES);
    if (per_lane <= 1) hipLaunchKernelGGL(k_frontier_sample<1>, grid, block, 0, stream, s);
    else if (per_lane <= 2) hipLaunchKernelGGL(k_frontier_sample<2>, grid, block, 0, stream, s);
    else if (per_lane <= 4) hipLaunchKernelGGL(k_frontier_sample<4>, grid, block, 0, stream, s);
    else if (per_lane <= 8) hipLaunchKernelGGL(k_frontier_sample<8>, grid, block, 0, stream, s);
    else hipLaunchKernelGGL(k_frontier_sample<16>, grid, block, 0, stream, s);
    HIP_TRY(env, hipGetLastError());
    return PCBENV_OK;
}
