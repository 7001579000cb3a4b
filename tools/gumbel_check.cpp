// gumbel_check.cpp -- csrc/pcb_gumbel.h on the CPU: runs a sequence of pcbenv_gumbel_advance calls through gumbel_begin /
// puct_absorb / gumbel_select / gumbel_choose, root by root, on the tensors it is handed, and writes the state after every
// call (tests/test_gumbel_model.py compares it with pcbenv/search.py's specification, tests/test_gumbel_gpu.py with the
// kernel's); or writes a row of the table of considered visits.  A stand-alone program:
//   g++ -std=c++17 -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=all -I rl-environment-for-component-placement_amd/csrc
//
// stdin and stdout are streams of little-endian int64 words (a float64 travels as its bits, a float32 as its bits in the
// low half of a word).  The first word is the mode.
//   mode 0, calls.
//     in:   P N C T K n Mc calls | c_puct c_visit c_scale | considered [Mc + 1, n] | the state (below)
//           per call: phases seed step_index first_root pokes | pokes x (tensor, flat index, value)
//             [ABSORB: value[P] leaf_terminal[P] cand_count[P] cand_actions[P K 3] cand_prior[P K]]
//           A poke stores `value` into one element of the state before the phases of its call run -- the damage a caller
//           can do.  tensor: 0 selected, 1 num_nodes, 2 parent, 3 num_children, 4 first_child, 5 sim_index, 6 sim_visits
//           (tests/gumbel_cases.py:POKED).
//     out:  per call: the error bits of that call | the state | move_slot[P] move_action[P 3] child_weights[P C]
//           child_policy[P C] child_actions[P C 3] root_value[P]
//     the state: selected[P] path_len[P] paths[T P 3] | num_nodes[P] parent depth visits num_children first_child [P N]
//           node_action[P N 3] prior value_sum value_max terminal [P N] reward_lo reward_hi [P] | sim_index[P] sim_visits[P C]
//     Before the first CHOOSE the six outputs hold -7 (what a test puts into the device tensors the kernel must leave alone).
//   mode 1, the table.
//     in:   m n      out:  considered_row(m, n), n words
#include "pcb_gumbel.h"
#include "puct_state.h"

using namespace puct_state;

namespace {

int table() {
    bool ok = true;
    const int64_t m = read_word(&ok), n = read_word(&ok);
    if (!ok || m < 0 || m > pcb_gumbel::MAX_CONSIDERED || n < 1 || n > (1 << 20)) { fprintf(stderr, "bad header\n"); return 2; }
    std::vector<int> row((size_t)n, -1);
    pcb_gumbel::considered_row((int)m, (int)n, row.data());
    put(row);
    return 0;
}

int calls() {
    using namespace pcb_gumbel;
    bool ok = true;
    const int P = (int)read_word(&ok), N = (int)read_word(&ok), C = (int)read_word(&ok), T = (int)read_word(&ok), K = (int)read_word(&ok),
              n = (int)read_word(&ok), Mc = (int)read_word(&ok), calls = (int)read_word(&ok);
    const double c_puct = as_double(read_word(&ok)), c_visit = as_double(read_word(&ok)), c_scale = as_double(read_word(&ok));
    if (!ok || P < 0 || N < 1 || C < 1 || C > MAX_CHILDREN || T < 1 || K < 1 || n < 1 || Mc < 1 || Mc > MAX_CONSIDERED || calls < 0) { fprintf(stderr, "bad header\n"); return 2; }
    const size_t PC = (size_t)P * C;
    std::vector<int> considered((size_t)(Mc + 1) * n), sim_index(P), sim_visits(PC);
    State st(P, N, C, T, (size_t)P);
    if (!(read_ints(considered) && st.read_search() && st.read_tree() && read_ints(sim_index) && read_ints(sim_visits))) { fprintf(stderr, "the state ends early\n"); return 2; }
    std::vector<int> &selected = st.selected, &path_len = st.path_len, &paths = st.paths;
    const int FILL = -7;
    std::vector<int> move_slot(P, FILL), move_action((size_t)P * 3, FILL), child_weights(PC, FILL), child_actions(PC * 3, FILL);
    std::vector<float> child_policy(PC, -7.0f);
    std::vector<double> root_value(P, -7.0);
    Evaluation<> ev((size_t)P, K);
    std::vector<int> *const poked[] = {&selected, &st.num_nodes, &st.parent, &st.num_children, &st.first_child, &sim_index, &sim_visits};
    for (int call = 0; call < calls; call++) {
        const int phases = (int)read_word(&ok);
        const uint64_t seed = (uint64_t)read_word(&ok), step_index = (uint64_t)read_word(&ok);
        const int first_root = (int)read_word(&ok);
        const int64_t pokes = read_word(&ok);
        if (!poke(poked, pokes, &ok, call)) return 2;
        if (!ok || pokes < 0 || phases <= 0 || phases > 15 || ((phases & PHASE_SELECT) && (phases & PHASE_CHOOSE))) { fprintf(stderr, "call %d: bad phases\n", call); return 2; }
        if (phases & PHASE_ABSORB) ok = ok && ev.read();
        if (!ok) { fprintf(stderr, "call %d: input ends early\n", call); return 2; }
        const Rule q{c_puct, c_visit, c_scale, seed, step_index, first_root, n, Mc};
        unsigned errors = 0u;
        for (int p = 0; p < P; p++) {
            const size_t row = (size_t)p * C;
            const Root r = st.root(p);
            if (phases & PHASE_BEGIN) gumbel_begin(C, &sim_index[p], &sim_visits[row]);
            if (phases & PHASE_ABSORB) errors |= ev.absorb(r, selected[p], (size_t)p);
            if (phases & PHASE_SELECT) errors |= gumbel_select(r, q, considered.data(), &sim_index[p], &sim_visits[row], paths.data(), &path_len[p], &selected[p]);
            if (phases & PHASE_CHOOSE)
                errors |= gumbel_choose(r, q, &sim_visits[row], &move_slot[p], &move_action[(size_t)p * 3], &child_weights[row], &child_policy[row],
                                        &child_actions[3 * row], &root_value[p]);
        }
        out.push_back((int64_t)errors);
        st.put_search(); st.put_tree(); put(sim_index); put(sim_visits);
        put(move_slot); put(move_action); put(child_weights); put_bits(child_policy); put(child_actions); put_bits(root_value);
    }
    return 0;
}

}  // namespace

int main() {
    bool ok = true;
    const int64_t mode = read_word(&ok);
    if (!ok || mode < 0 || mode > 1) { fprintf(stderr, "bad mode\n"); return 2; }
    const int rc = mode == 0 ? calls() : table();
    return rc != 0 ? rc : flush();
}
