// pcb_puct_noise.h -- the exploration noise of pcbenv_puct_root_noise (include/pcbenv_noise.h), stated once: a draw from
// Dir(alpha) over the k children of a root, mixed into their priors, for ONE root.  Plain C++17 that compiles alone, on the
// host and on the device: k_puct_root_noise (pcb_puct_noise.hip) composes the pieces below with child c of the root in
// lane c of a group, and tools/puct_noise_check.cpp -- a CPU program -- composes them serially (noise_root).
// pcbenv/search.py:puct_root_noise is the specification: the same operations in the same association, so the three agree
// bit for bit.  Every floating-point operation is + - * / or a comparison (pcb_ieee_math.h supplies ln, exp and the square
// root in those terms); the build passes -ffp-contract=off.
//
// The uniform stream.  base = the 64 bits behind the library's draw for (seed, first_root + p, step_index); draw number t
// of child c is mix64(base + GOLDEN * (64 t + c + 1)), and u = ((w >> 12) + 0.5) * 2^-52: exact, strictly inside (0, 1).
// A value depends on (seed, global root index, step_index, c, t) alone.
//
// Gamma(alpha), Marsaglia and Tsang, at most ATTEMPTS rejection rounds (a constant, not data): a = alpha >= 1 ? alpha :
// alpha + 1, d = a - 1/3, cc = (1/3) / sqrt(d), both computed once by the host (noise_params).  Attempt t takes draws
// 3 t, 3 t + 1, 3 t + 2: a normal deviate by the polar method (it fails if s >= 1), v = (1 + cc x)^3 (it fails if
// v <= 0), accepted if ln u3 < x^2 / 2 + d - d v + d ln v; then g = d v.  No attempt accepted: g = d.  alpha < 1: g *=
// exp(ln(u) / alpha) with draw BOOST_DRAW.
//
// The promise of pcb_puct.h holds here too: k and fc are compared with C and N before they address anything.
#pragma once
#include "pcb_ieee_math.h"
#include "pcb_puct_move.h"

namespace pcb_noise {

using pcb_ieee::ieee_exp;
using pcb_ieee::ieee_ln;
using pcb_ieee::ieee_sqrt;
using pcb_move::mix64;
using pcb_puct::children_ok;
using pcb_tree::ERR_TREE;
using pcb_tree::MAX_CHILDREN;

enum { ATTEMPTS = 32, BOOST_DRAW = 3 * ATTEMPTS };
constexpr uint64_t GOLDEN = 0x9E3779B97F4A7C15ull;
constexpr double ALPHA_MIN = 0.01, ALPHA_MAX = 100.0;
constexpr double TWO_M52 = 1.0 / 4503599627370496.0;

// what a launch needs of (alpha, eps): computed once, on the host
struct Params { double alpha, eps, keep /*1 - eps*/, d, cc; };
PCB_TREE_HD inline Params noise_params(double alpha, double eps) {
    const double a = alpha >= 1.0 ? alpha : alpha + 1.0;
    const double d = a - 1.0 / 3.0;
    return Params{alpha, eps, 1.0 - eps, d, (1.0 / 3.0) / ieee_sqrt(d)};
}

// ---- the uniform stream ----------------------------------------------------------------------------------------------
PCB_TREE_HD inline uint64_t draw_base(uint64_t seed, int genv, uint64_t step_index) {
    return mix64(mix64(seed ^ GOLDEN * ((uint64_t)(int64_t)genv + 1)) + step_index);
}
PCB_TREE_HD inline double uniform(uint64_t base, int c, int t) {
    const uint64_t w = mix64(base + GOLDEN * (uint64_t)(64 * t + c + 1));
    return ((double)(w >> 12) + 0.5) * TWO_M52;
}

// ---- Gamma(alpha) for child c ------------------------------------------------------------------------------------------
// one attempt: true and *g = d v if it accepts
PCB_TREE_HD inline bool gamma_attempt(uint64_t base, int c, int t, double d, double cc, double *g) {
    const double v1 = 2.0 * uniform(base, c, 3 * t) - 1.0, v2 = 2.0 * uniform(base, c, 3 * t + 1) - 1.0;
    const double s = v1 * v1 + v2 * v2;
    if (s >= 1.0) return false;
    const double x = v1 * ieee_sqrt((-2.0 * ieee_ln(s)) / s);
    const double w = 1.0 + cc * x;
    const double v = (w * w) * w;
    if (v <= 0.0) return false;
    if (!(ieee_ln(uniform(base, c, 3 * t + 2)) < ((0.5 * (x * x) + d) - d * v) + d * ieee_ln(v))) return false;
    *g = d * v;
    return true;
}
// *exhausted: no attempt accepted (the table of tests/puct_noise_cases.py has no such draw)
PCB_TREE_HD inline double gamma_draw(uint64_t base, int c, const Params &q, bool *exhausted = nullptr) {
    double g = q.d;
    bool done = false;
    for (int t = 0; t < ATTEMPTS && !done; t++) done = gamma_attempt(base, c, t, q.d, q.cc, &g);
    if (exhausted) *exhausted = !done;
    if (q.alpha < 1.0) g = g * ieee_exp(ieee_ln(uniform(base, c, BOOST_DRAW)) / q.alpha);
    return g;
}

// ---- the mix ---------------------------------------------------------------------------------------------------------
// the root is due: it has not been noised in this move and it has children
PCB_TREE_HD inline bool due(int noised, int k) { return noised == 0 && k >= 1; }
PCB_TREE_HD inline bool sum_ok(double S) { return S > 0.0 && S <= 1.7976931348623157e308; }
PCB_TREE_HD inline double share(double g, double S, int k) { return sum_ok(S) ? g / S : 1.0 / (double)k; }
// a prior is a float32 value, as every prior an evaluator gives is
PCB_TREE_HD inline double mixed(double prior, double eta, const Params &q) { return (double)(float)(q.keep * prior + q.eps * eta); }

// num_children, first_child, prior: the [N] rows of root p; noised: its element.  Stores nothing but prior of the k
// children and *noised.
PCB_TREE_HD inline unsigned noise_root(int N, int C, int genv, uint64_t seed, uint64_t step_index, const Params &q, const int *num_children,
                                       const int *first_child, double *prior, int *noised) {
    const int k = num_children[0], fc = first_child[0];
    if (!due(*noised, k)) return 0u;
    if (!children_ok(fc, k, N, C)) return ERR_TREE;
    const uint64_t base = draw_base(seed, genv, step_index);
    double g[MAX_CHILDREN], S = 0.0;
    for (int c = 0; c < k; c++) { g[c] = gamma_draw(base, c, q); S = S + g[c]; }
    for (int c = 0; c < k; c++) prior[fc + c] = mixed(prior[fc + c], share(g[c], S, k), q);
    *noised = 1;
    return 0u;
}

}  // namespace pcb_noise
