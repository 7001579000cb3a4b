// frontier_check.cpp -- csrc/pcb_frontier.h on the CPU: replays a sequence of pcbenv_frontier_advance calls through
// frontier_init / frontier_advance, root by root, and writes the state after every call (tests/test_frontier_model.py
// compares every one with pcbenv/search.py:frontier_advance, the specification, tests/test_frontier_gpu.py with the
// kernel's).  A stand-alone program:
//   g++ -std=c++17 -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=all -I rl-environment-for-component-placement_amd/csrc
//
// stdin and stdout are streams of little-endian int64 words (a float64 travels as its bits, a float32 as its bits in the
// low half of a word; "word_stream.h").  R = P * W * K rows, row p * W * K + i the slot i of root p.
//   in:   P W K T calls prior_weight | per call: phases swap
//           [LOADED: the in set and the accumulators -- path_len[R] cum_logp[R] paths[T R 3] best_value[P] best_len[P]]
//           [ADVANCE: value[R] leaf_terminal[R] cand_count[R] cand_actions[R K 3] cand_prior[R K]]
//         phases: PHASE_INIT = 1 or PHASE_ADVANCE = 2 of csrc/pcb_frontier.h, LOADED = 8 if the call brings a frontier of
//         the caller's making, stored into the in set before the phase runs.  swap: 0 reads set 0 and writes set 1, 1 the
//         other way round.
//   out:  per call: errors | paths_0[T R 3] path_len_0[R] cum_logp_0[R] paths_1 path_len_1 cum_logp_1 | parent_row[R] live[P]
//           best_value[P] best_len[P] best_path[T P 3]
// Before the first call every int32 tensor holds -7 and every float64 tensor -7.5 (what a test puts into the device
// tensors the kernel must leave alone).
#include <stdio.h>

#include <vector>

#include "pcb_frontier.h"
#include "word_stream.h"

using namespace word_stream;

int main() {
    using namespace pcb_frontier;
    bool ok = true;
    const int P = (int)read_word(&ok), W = (int)read_word(&ok), K = (int)read_word(&ok), T = (int)read_word(&ok), calls = (int)read_word(&ok);
    const double prior_weight = as_double(read_word(&ok));
    if (!ok || P < 0 || W < 1 || W > MAX_WIDTH || K < 1 || K > MAX_CANDIDATES || W * K > MAX_ROWS || T < 1 || calls < 0 ||
        (long long)P * W * K > 0x7fffffffLL) { fprintf(stderr, "bad header\n"); return 2; }
    const int F = W * K;
    const size_t R = (size_t)P * F, TR3 = (size_t)T * R * 3;
    std::vector<int> paths[2] = {std::vector<int>(TR3, -7), std::vector<int>(TR3, -7)};
    std::vector<int> path_len[2] = {std::vector<int>(R, -7), std::vector<int>(R, -7)};
    std::vector<double> cum_logp[2] = {std::vector<double>(R, -7.5), std::vector<double>(R, -7.5)};
    std::vector<int> parent_row(R, -7), live(P, -7), best_len(P, -7), best_path((size_t)T * P * 3, -7);
    std::vector<double> best_value(P, -7.5);
    std::vector<double> value(R);
    std::vector<uint8_t> leaf_terminal(R);
    std::vector<int> cand_count(R), cand_actions(R * K * 3);
    std::vector<float> cand_prior(R * K);
    std::vector<unsigned char> taken(F);
    std::vector<int> kept(W);
    enum { LOADED = 8 };
    unsigned errors = 0u;
    for (int call = 0; call < calls; call++) {
        const int word = (int)read_word(&ok), swap = (int)read_word(&ok);
        const int phases = word & ~LOADED;
        if (!ok || (phases != PHASE_INIT && phases != PHASE_ADVANCE) || swap < 0 || swap > 1) { fprintf(stderr, "call %d: bad phases or swap\n", call); return 2; }
        const int in = swap ? 1 : 0, to = 1 - in;
        if (word & LOADED) ok = ok && read_ints(path_len[in]) && read_doubles(cum_logp[in]) && read_ints(paths[in]) && read_doubles(best_value) && read_ints(best_len);
        if (phases == PHASE_ADVANCE)
            ok = ok && read_doubles(value) && read_ints(leaf_terminal) && read_ints(cand_count) && read_ints(cand_actions) && read_floats(cand_prior);
        if (!ok) { fprintf(stderr, "call %d: input ends early\n", call); return 2; }
        Frontier f;
        f.phases = phases; f.P = P; f.W = W; f.K = K; f.T = T; f.prior_weight = prior_weight;
        f.paths_in = paths[in].data(); f.path_len_in = path_len[in].data(); f.cum_logp_in = cum_logp[in].data();
        f.paths_out = paths[to].data(); f.path_len_out = path_len[to].data(); f.cum_logp_out = cum_logp[to].data();
        f.parent_row = parent_row.data(); f.live = live.data(); f.best_value = best_value.data(); f.best_len = best_len.data(); f.best_path = best_path.data();
        f.value = value.data(); f.leaf_terminal = leaf_terminal.data(); f.cand_count = cand_count.data(); f.cand_actions = cand_actions.data();
        f.cand_prior = cand_prior.data(); f.errors = nullptr;
        for (int p = 0; p < P; p++) {
            if (phases == PHASE_INIT) frontier_init(f, p);
            else errors |= frontier_advance(f, p, taken.data(), kept.data());
        }
        out.push_back((int64_t)errors);
        for (int s = 0; s < 2; s++) { put(paths[s]); put(path_len[s]); put_bits(cum_logp[s]); }
        put(parent_row); put(live); put_bits(best_value); put(best_len); put(best_path);
    }
    return flush();
}
