// frontier_sample_check.cpp -- csrc/pcb_frontier_sample.h on the CPU.  Mode 0 replays a sequence of pcbenv_frontier_sample
// calls through sample_init / sample_advance, root by root, and writes the state after every call
// (tests/test_frontier_sample_model.py compares every one with pcbenv/search.py:frontier_sample_advance, the specification,
// tests/test_frontier_sample_gpu.py with the kernel's); mode 1 evaluates child_gumbel, the truncated Gumbel, on a table.
// A stand-alone program:
//   g++ -std=c++17 -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=all -I rl-environment-for-component-placement_amd/csrc
//
// stdin and stdout are streams of little-endian int64 words (a float64 travels as its bits, a float32 as its bits in the
// low half of a word; "word_stream.h").  R = P * W * K rows, S = P * W set slots.
//   in:   0 P W K T calls seed first_root | per call: phases swap step_index
//           [LOADED: path_len[R] cum_logp[R] gumbel[R] paths[T R 3] best_value[P] best_len[P] set_len[S] set_gumbel[S]
//            set_logp[S] set_value[S] set_path[T S 3] -- the in set, the accumulators and the sample set]
//           [ADVANCE: value[R] leaf_terminal[R] cand_count[R] cand_actions[R K 3] cand_prior[R K]]
//         phases: PHASE_INIT = 1 or PHASE_ADVANCE = 2 of csrc/pcb_frontier.h, LOADED = 8 if the call brings a state of the
//         caller's making.  swap: 0 reads set 0 and writes set 1, 1 the other way round.
//   out:  per call: errors | paths_0[T R 3] path_len_0[R] cum_logp_0[R] gumbel_0[R] paths_1 path_len_1 cum_logp_1 gumbel_1 |
//           parent_row[R] live[P] best_value[P] best_len[P] best_path[T P 3] set_len[S] set_gumbel[S] set_logp[S]
//           set_value[S] set_path[T S 3]
//   in:   1 n | n times G_S phi_c G_c Z        out: n times child_gumbel(G_S, phi_c, G_c, Z)
// Before the first call every int32 tensor holds -7 and every float64 tensor -7.5.
#include <stdio.h>

#include <vector>

#include "pcb_frontier_sample.h"
#include "word_stream.h"

using namespace word_stream;

static int table() {
    using namespace pcb_frontier_sample;
    bool ok = true;
    const long long n = read_word(&ok);
    if (!ok || n < 0) { fprintf(stderr, "bad table\n"); return 2; }
    for (long long i = 0; i < n; i++) {
        const double G_S = as_double(read_word(&ok)), phi = as_double(read_word(&ok)), G_c = as_double(read_word(&ok)), Z = as_double(read_word(&ok));
        if (!ok) { fprintf(stderr, "input ends early\n"); return 2; }
        out.push_back(as_bits(child_gumbel(G_S, phi, G_c, Z)));
    }
    return flush();
}

int main() {
    using namespace pcb_frontier_sample;
    bool ok = true;
    if (read_word(&ok) == 1) return table();
    const int P = (int)read_word(&ok), W = (int)read_word(&ok), K = (int)read_word(&ok), T = (int)read_word(&ok), calls = (int)read_word(&ok);
    const uint64_t seed = (uint64_t)read_word(&ok);
    const long long first_root = read_word(&ok);
    if (!ok || P < 0 || W < 1 || W > MAX_WIDTH || K < 1 || K > MAX_CANDIDATES || W * K > MAX_ROWS || T < 1 || calls < 0 ||
        (long long)P * W * K > 0x7fffffffLL || first_root < 0 || first_root + P > 0x7fffffffLL) { fprintf(stderr, "bad header\n"); return 2; }
    const int F = W * K;
    const size_t R = (size_t)P * F, TR3 = (size_t)T * R * 3, S = (size_t)P * W;
    std::vector<int> paths[2] = {std::vector<int>(TR3, -7), std::vector<int>(TR3, -7)};
    std::vector<int> path_len[2] = {std::vector<int>(R, -7), std::vector<int>(R, -7)};
    std::vector<double> cum_logp[2] = {std::vector<double>(R, -7.5), std::vector<double>(R, -7.5)};
    std::vector<double> gumbel[2] = {std::vector<double>(R, -7.5), std::vector<double>(R, -7.5)};
    std::vector<int> parent_row(R, -7), live(P, -7), best_len(P, -7), best_path((size_t)T * P * 3, -7);
    std::vector<double> best_value(P, -7.5);
    std::vector<int> set_len(S, -7), set_path((size_t)T * S * 3, -7);
    std::vector<double> set_gumbel(S, -7.5), set_logp(S, -7.5), set_value(S, -7.5);
    std::vector<double> value(R);
    std::vector<uint8_t> leaf_terminal(R);
    std::vector<int> cand_count(R), cand_actions(R * K * 3);
    std::vector<float> cand_prior(R * K);
    std::vector<unsigned char> kind(W + F);
    std::vector<int> won(W), kept(W);
    enum { LOADED = 8 };
    unsigned errors = 0u;
    for (int call = 0; call < calls; call++) {
        const int word = (int)read_word(&ok), swap = (int)read_word(&ok);
        const uint64_t step_index = (uint64_t)read_word(&ok);
        const int phases = word & ~LOADED;
        if (!ok || (phases != PHASE_INIT && phases != PHASE_ADVANCE) || swap < 0 || swap > 1) { fprintf(stderr, "call %d: bad phases or swap\n", call); return 2; }
        const int in = swap ? 1 : 0, to = 1 - in;
        if (word & LOADED)
            ok = ok && read_ints(path_len[in]) && read_doubles(cum_logp[in]) && read_doubles(gumbel[in]) && read_ints(paths[in]) && read_doubles(best_value) &&
                 read_ints(best_len) && read_ints(set_len) && read_doubles(set_gumbel) && read_doubles(set_logp) && read_doubles(set_value) && read_ints(set_path);
        if (phases == PHASE_ADVANCE)
            ok = ok && read_doubles(value) && read_ints(leaf_terminal) && read_ints(cand_count) && read_ints(cand_actions) && read_floats(cand_prior);
        if (!ok) { fprintf(stderr, "call %d: input ends early\n", call); return 2; }
        Sample q;
        Frontier &f = q.f;
        f.phases = phases; f.P = P; f.W = W; f.K = K; f.T = T; f.prior_weight = 0.0;
        f.paths_in = paths[in].data(); f.path_len_in = path_len[in].data(); f.cum_logp_in = cum_logp[in].data();
        f.paths_out = paths[to].data(); f.path_len_out = path_len[to].data(); f.cum_logp_out = cum_logp[to].data();
        f.parent_row = parent_row.data(); f.live = live.data(); f.best_value = best_value.data(); f.best_len = best_len.data(); f.best_path = best_path.data();
        f.value = value.data(); f.leaf_terminal = leaf_terminal.data(); f.cand_count = cand_count.data(); f.cand_actions = cand_actions.data();
        f.cand_prior = cand_prior.data(); f.errors = nullptr;
        q.seed = seed; q.step_index = step_index; q.first_root = (int)first_root; q.gumbel_in = gumbel[in].data(); q.gumbel_out = gumbel[to].data();
        q.set_len = set_len.data(); q.set_gumbel = set_gumbel.data(); q.set_logp = set_logp.data(); q.set_value = set_value.data(); q.set_path = set_path.data();
        for (int p = 0; p < P; p++) {
            if (phases == PHASE_INIT) sample_init(q, p);
            else errors |= sample_advance(q, p, kind.data(), won.data(), kept.data());
        }
        out.push_back((int64_t)errors);
        for (int s = 0; s < 2; s++) { put(paths[s]); put(path_len[s]); put_bits(cum_logp[s]); put_bits(gumbel[s]); }
        put(parent_row); put(live); put_bits(best_value); put(best_len); put(best_path);
        put(set_len); put_bits(set_gumbel); put_bits(set_logp); put_bits(set_value); put(set_path);
    }
    return flush();
}
