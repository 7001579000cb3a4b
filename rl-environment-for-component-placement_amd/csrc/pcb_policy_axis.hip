// pcb_policy_axis.hip -- k_sample_axis, k_evaluate_axis and k_evaluate_axis_backward: one stage of a factorised policy
// (pcbenv_sample_axis, pcbenv_evaluate_axis, pcbenv_evaluate_axis_backward).  Part of libpcbenv.so (CDNA4 / gfx950
// only); a translation unit of its own, so that nothing here can change the builds of the other kernels.
//
// The reference's factorised distributions (utils/agent/factorized_action_distributions.py:107-818: p(o) p(x|o) p(y|o,x)
// and p(x) p(y|x) p(o|x,y)) draw one action coordinate at a time from a masked Categorical over O, H or W logits, the
// mask being a reduce_max / gather of the uint8 action_mask.  Here a stage's legal set L comes from the bit rows
// (pcb_axis_set.h: the derivation the CPU check compiles too), and a logit is read only where its value is in L.
//
// One wavefront per row (an environment, or a stored step), four rows per 256-thread workgroup; the wavefronts of a
// workgroup share nothing: no LDS, no barrier, and a wavefront whose row does not exist exits whole.  Lane k owns the
// candidates k and k + 64 (n <= 128 = PCBENV_MAX_SIDE).
//   legal set     target y, x given: one row of one or two planes; target x: lane k reads rows k and k + 64; target
//                 orientation, or x not given: lanes stride the rows, OR them, and the wavefront reduces.
//   distribution  M by wave_max; weights by seg_weight (the one place a weight is computed); an inclusive float32 scan
//                 per half of 64 gives the prefix sums, the halves are joined in float64 (Z, the threshold u * Z).
//   backward      recomputes M, Z and the entropy from the <= 128 logits: no statistics buffer.
// A row that is not a distribution (a NaN / +inf in L, or every logit of L -inf) is handled as constant logits over L:
// the same code then gives the uniform pick, log_prob = -log |L| and entropy = log |L|.
#include <hip/hip_runtime.h>

#include "pcbenv.h"
#include "pcb_axis_set.h"
#include "pcb_sampler.h"
#include "pcb_launch.h"
#include "pcb_policy_common.h"

namespace {

using pcb_axis::Geom;
using pcb_axis::Set128;

constexpr int ROWS_PER_GROUP = 4;
constexpr unsigned ERR_GIVEN = 8u;  // bit 3: a given value outside its axis

__device__ inline u64 wave_or(u64 v) { for (int o = 32; o > 0; o >>= 1) v |= __shfl_xor(v, o); return v; }
// this wavefront's row, or -1 where it does not exist (compared unsigned: within 3 rows of INT32_MAX the count of the last
// workgroup's missing rows does not fit an int)
__device__ inline int wave_row(int rows) {
    const unsigned r = blockIdx.x * ROWS_PER_GROUP + (threadIdx.x >> 6);
    return r < (unsigned)rows ? __builtin_amdgcn_readfirstlane((int)r) : -1;
}

// the given columns of a row's (o, x, y); a column that is not given is not read
__device__ inline void given_values(const int *actions, size_t r, unsigned given, int vals[3]) {
    #pragma unroll
    for (int a = 0; a < 3; a++) vals[a] = ((given >> a) & 1u) ? actions[3 * r + a] : 0;
}

// pcb_axis::legal_set with the rows spread over the wavefront; the result is the same in every lane
__device__ inline Set128 wave_legal_set(const u64 *bits, const Geom &g, const AxisStage &s, const int vals[3], int lane) {
    using namespace pcb_axis;
    const unsigned planes = planes_read(g, s.given, vals);
    const Set128 cols = cols_read(g, s.given, vals);
    int x0, x1;
    rows_read(g, s.given, vals, &x0, &x1);
    const bool one_row = (s.given >> AXIS_X) & 1u;
    if (s.axis == AXIS_Y) {
        if (one_row) return rows_or(bits, g, planes, x0, x1, 1);
        const Set128 mine = rows_or(bits, g, planes, lane, g.H, WAVE);
        return Set128{wave_or(mine.lo), wave_or(mine.hi)};
    }
    if (s.axis == AXIS_X)
        return Set128{__ballot(row_open(bits, g, planes, cols, lane)), __ballot(row_open(bits, g, planes, cols, lane + WAVE))};
    bool open[2] = {false, false};
    #pragma unroll
    for (int p = 0; p < 2; p++)
        if (p < g.O) {  // O == 1: plane 1 is never read
            const Set128 mine = one_row ? rows_or(bits, g, 1u << p, x0, x1, 1) : rows_or(bits, g, 1u << p, lane, g.H, WAVE);
            open[p] = __ballot((mine & cols).any()) != 0;
        }
    return orientations_open(g, open[0], open[1]);
}

// A row's masked categorical, lane k holding candidates k (suffix 0) and k + 64 (suffix 1).
struct AxisDist {
    int n;          // |L|
    unsigned bits;  // 0; 1 a NaN / +inf in L; 2 every logit of L -inf (0 when L is empty)
    bool in0, in1;  // this lane's candidates are in L
    float l0, l1, w0, w1, c0, c1;  // logit, weight and inclusive prefix within the half (bits != 0: l = 0, w = 1 on L)
    float M, tot0;  // tot0: the sum of the first half's weights
    double Z, logZ, ent;
};
template <typename T> __device__ inline AxisDist axis_dist(const T *row, const Set128 &L, int lane) {
    AxisDist d;
    d.n = __popcll(L.lo) + __popcll(L.hi);
    d.in0 = (L.lo >> lane) & 1ull; d.in1 = (L.hi >> lane) & 1ull;
    d.l0 = d.in0 ? to_f32(row[lane]) : -INFINITY;
    d.l1 = d.in1 ? to_f32(row[lane + WAVE]) : -INFINITY;
    const bool bad = __ballot((d.in0 && !(d.l0 < INFINITY)) || (d.in1 && !(d.l1 < INFINITY))) != 0;
    d.M = wave_max(fmaxf(d.l0, d.l1));
    d.bits = d.n == 0 ? 0u : bad ? 1u : d.M == -INFINITY ? 2u : 0u;
    if (d.bits) { d.M = 0.f; d.l0 = d.in0 ? 0.f : -INFINITY; d.l1 = d.in1 ? 0.f : -INFINITY; }
    d.w0 = d.l0 > -INFINITY ? seg_weight(d.l0, d.M) : 0.f;
    d.w1 = d.l1 > -INFINITY ? seg_weight(d.l1, d.M) : 0.f;
    d.c0 = wave_scan(d.w0, lane); d.c1 = wave_scan(d.w1, lane);
    d.tot0 = __shfl(d.c0, WAVE - 1);
    d.Z = (double)d.tot0 + (double)__shfl(d.c1, WAVE - 1);
    // a zero weight contributes 0: l - M may be -inf, and 0 * -inf is NaN
    const double tl = wave_sum((d.w0 > 0.f ? (double)d.w0 * (double)(d.l0 - d.M) : 0.0) + (d.w1 > 0.f ? (double)d.w1 * (double)(d.l1 - d.M) : 0.0));
    d.logZ = d.n ? log(d.Z) : 0.0;
    d.ent = d.n ? d.logZ - tl / d.Z : 0.0;
    return d;
}
__device__ inline float logit_of(const AxisDist &d, int v) { return v < WAVE ? __shfl(d.l0, v) : __shfl(d.l1, v - WAVE); }
__device__ inline int first_lane(u64 m) { return __ffsll((long long)m) - 1; }
__device__ inline int last_lane(u64 m) { return 63 - __clzll((long long)m); }

template <typename T>
__global__ __launch_bounds__(64 * ROWS_PER_GROUP) void k_sample_axis(DevParams p, AxisStage s, SampleAxisArgs g) {
    const int e = wave_row(p.B), lane = threadIdx.x & (WAVE - 1);
    if (e < 0) return;
    const Geom q{p.O, p.H, p.W, p.WW};
    const int n = pcb_axis::axis_size(q, s.axis);
    int vals[3];
    given_values(g.actions, (size_t)e, s.given, vals);
    const bool given_ok = pcb_axis::given_in_range(q, s.given, vals);
    Set128 L{0ull, 0ull};
    if (given_ok) L = wave_legal_set((const u64 *)(p.state + (size_t)e * p.stateStride + p.offVm), q, s, vals, lane);
    const AxisDist d = axis_dist((const T *)g.logits + (size_t)e * (size_t)n, L, lane);
    int v = 0;
    double logp = 0.0;
    if (d.n > 0) {
        if (g.greedy && !d.bits) {
            const u64 top0 = __ballot(d.in0 && d.l0 == d.M), top1 = __ballot(d.in1 && d.l1 == d.M);
            v = top0 ? first_lane(top0) : WAVE + first_lane(top1);
        } else {
            const u64 rnd = mix64(draw_bits(g.seed, (int)g.first_env + e, g.step_index) + 0x9E3779B97F4A7C15ull * (u64)(s.axis + 1));
            const double uz = (double)(unsigned)(rnd >> 32) * 0x1p-32 * d.Z;
            const u64 live0 = __ballot(d.w0 > 0.f), live1 = __ballot(d.w1 > 0.f);
            const u64 hit0 = __ballot(d.w0 > 0.f && (double)d.c0 > uz);
            const u64 hit1 = __ballot(d.w1 > 0.f && (double)d.tot0 + (double)d.c1 > uz);
            // rounding can leave no prefix above the threshold: then the last value with weight
            v = hit0 ? first_lane(hit0) : hit1 ? WAVE + first_lane(hit1) : live1 ? WAVE + last_lane(live1) : last_lane(live0);
        }
        logp = (double)logit_of(d, v) - (double)d.M - d.logZ;
    }
    if (lane == 0) {
        g.actions[3 * (size_t)e + s.axis] = v;
        if (g.log_prob) g.log_prob[e] = (float)logp;
        if (g.entropy) g.entropy[e] = (float)d.ent;
        const unsigned bits = d.bits | (given_ok ? 0u : ERR_GIVEN);
        if (bits && g.errors) atomicOr(g.errors, bits);
    }
}

// what the two evaluate kernels do first: the row's legal set, its distribution and the stored value
struct EvalRow { AxisDist d; int a; bool given_ok, a_in; };
template <typename T>
__device__ inline EvalRow eval_row(const EvalGeom &q, const AxisStage &s, const void *logits, const u64 *mask_bits, const int *actions, int r, int lane) {
    const Geom geo{q.O, q.H, q.W, q.WW};
    const int n = pcb_axis::axis_size(geo, s.axis);
    int vals[3];
    given_values(actions, (size_t)r, s.given, vals);
    EvalRow row;
    row.given_ok = pcb_axis::given_in_range(geo, s.given, vals);
    Set128 L{0ull, 0ull};
    if (row.given_ok) L = wave_legal_set(mask_bits + (size_t)r * (size_t)(2 * q.H * q.WW), geo, s, vals, lane);
    row.d = axis_dist((const T *)logits + (size_t)r * (size_t)n, L, lane);
    row.a = actions[3 * (size_t)r + s.axis];
    row.a_in = L.has(row.a);
    return row;
}

template <typename T>
__global__ __launch_bounds__(64 * ROWS_PER_GROUP) void k_evaluate_axis(EvalGeom q, AxisStage s, EvalAxisArgs g) {
    const int r = wave_row(q.rows), lane = threadIdx.x & (WAVE - 1);
    if (r < 0) return;
    const EvalRow row = eval_row<T>(q, s, g.logits, g.mask_bits, g.actions, r, lane);
    const AxisDist &d = row.d;
    unsigned bits = d.bits | (row.given_ok ? 0u : ERR_GIVEN);
    double logp = 0.0;
    if (d.n > 0 && d.bits) logp = -d.logZ;  // -log |L|, whatever was stored
    else if (d.n > 0 && row.a_in) logp = (double)logit_of(d, row.a) - (double)d.M - d.logZ;
    else if (d.n > 0) bits |= 4u;
    if (lane == 0) {
        if (g.log_prob) g.log_prob[r] = (float)logp;
        if (g.entropy) g.entropy[r] = (float)d.ent;
        if (bits && g.errors) atomicOr(g.errors, bits);
    }
}

template <typename T>
__global__ __launch_bounds__(64 * ROWS_PER_GROUP) void k_evaluate_axis_backward(EvalGeom q, AxisStage s, EvalAxisBackwardArgs g) {
    const int r = wave_row(q.rows), lane = threadIdx.x & (WAVE - 1);
    if (r < 0) return;
    const EvalRow row = eval_row<T>(q, s, g.logits, g.mask_bits, g.actions, r, lane);
    const AxisDist &d = row.d;
    const int n = pcb_axis::axis_size(Geom{q.O, q.H, q.W, q.WW}, s.axis);
    const bool live = d.n > 0 && !d.bits;  // otherwise the gradient row is zero
    const float glp = g.grad_log_prob ? g.grad_log_prob[r] : 0.f, gH = g.grad_entropy ? g.grad_entropy[r] : 0.f;
    const float logZ = (float)d.logZ, Hrow = (float)d.ent;
    const int a = row.a_in ? row.a : -1;  // not in L: the one-hot term is dropped
    T *out = (T *)g.grad_logits + (size_t)r * (size_t)n;
    if (lane < n) store1(out + lane, live && d.in0 ? grad_one(d.l0, d.M, logZ, Hrow, glp, gH, lane == a) : 0.f);
    if (lane + WAVE < n) store1(out + lane + WAVE, live && d.in1 ? grad_one(d.l1, d.M, logZ, Hrow, glp, gH, lane + WAVE == a) : 0.f);
}

template <typename F> void with_dtype(int dtype, F &&f) {
    if (dtype == PCBENV_LOGITS_F32) f(type_tag<float>());
    else f(type_tag<bf16_bits>());
}
inline dim3 axis_grid(int rows) { return dim3((unsigned)(((long long)rows + ROWS_PER_GROUP - 1) / ROWS_PER_GROUP)); }

}  // namespace

int pcb_launch_sample_axis(const SampleAxisLaunch &a) {
    with_dtype(a.dtype, [&](auto t) {
        hipLaunchKernelGGL((k_sample_axis<typename decltype(t)::type>), axis_grid(a.d.B), dim3(64 * ROWS_PER_GROUP), 0, a.stream, a.d, a.s, a.g);
    });
    return 0;
}

int pcb_launch_evaluate_axis(const EvalAxisLaunch &a) {
    with_dtype(a.dtype, [&](auto t) {
        hipLaunchKernelGGL((k_evaluate_axis<typename decltype(t)::type>), axis_grid(a.q.rows), dim3(64 * ROWS_PER_GROUP), 0, a.stream, a.q, a.s, a.g);
    });
    return 0;
}

int pcb_launch_evaluate_axis_backward(const EvalAxisBackwardLaunch &a) {
    with_dtype(a.dtype, [&](auto t) {
        hipLaunchKernelGGL((k_evaluate_axis_backward<typename decltype(t)::type>), axis_grid(a.q.rows), dim3(64 * ROWS_PER_GROUP), 0, a.stream, a.q, a.s, a.g);
    });
    return 0;
}
