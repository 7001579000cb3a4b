// gumbel_tree_leaves_check.cpp -- csrc/pcb_gumbel_tree_leaves.h on the CPU: runs a sequence of
// pcbenv_gumbel_tree_advance_leaves calls through gumbel_begin / leaves_absorb / tree_leaves_select / tree_choose, root by
// root, on the tensors it is handed, and writes the state after every call (tests/test_gumbel_tree_leaves_model.py compares it
// with pcbenv/search.py's specification and with tools/gumbel_tree_check.cpp, tests/test_gumbel_tree_leaves_gpu.py with the
// kernel's).  A stand-alone program:
//   g++ -std=c++17 -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=all -I rl-environment-for-component-placement_amd/csrc
//
// stdin and stdout: the wire format of tools/gumbel_leaves_check.cpp, word for word (c_puct travels and is not read) -- streams
// of little-endian int64 words, a float64 as its bits, a float32 as its bits in the low half of a word; R = P * L rows, row
// p * L + l the leaf l of root p.
//   in:   P N C T K n Mc L calls | c_puct c_visit c_scale | considered [Mc + 1, n] | the state (below)
//         per call: phases seed step_index first_root pokes | pokes x (tensor, flat index, value)
//           [ABSORB: value[R] leaf_terminal[R] cand_count[R] cand_actions[R K 3] cand_prior[R K]]
//         tensor of a poke: 0 selected, 1 num_nodes, 2 parent, 3 num_children, 4 first_child, 5 sim_index, 6 sim_visits,
//         7 pending (tests/gumbel_tree_leaves_cases.py:POKED).
//   out:  per call: the error bits of that call | the state | move_slot[P] move_action[P 3] child_weights[P C]
//         child_policy[P C] child_actions[P C 3] root_value[P]
//   the state: selected[R] path_len[R] paths[T R 3] | num_nodes[P] parent depth visits num_children first_child [P N]
//         node_action[P N 3] prior value_sum value_max terminal [P N] reward_lo reward_hi [P] | sim_index[P] sim_visits[P C]
//         | pending[P N]
//   Before the first CHOOSE the six outputs hold -7.
#include "pcb_gumbel_tree_leaves.h"
#include "puct_state.h"

using namespace puct_state;

int main() {
    using namespace pcb_gumbel_tree_leaves;
    using pcb_puct_leaves::leaves_absorb;
    bool ok = true;
    const int P = (int)read_word(&ok), N = (int)read_word(&ok), C = (int)read_word(&ok), T = (int)read_word(&ok), K = (int)read_word(&ok),
              n = (int)read_word(&ok), Mc = (int)read_word(&ok), L = (int)read_word(&ok), calls = (int)read_word(&ok);
    const double c_puct = as_double(read_word(&ok)), c_visit = as_double(read_word(&ok)), c_scale = as_double(read_word(&ok));
    if (!ok || P < 0 || N < 1 || C < 1 || C > MAX_CHILDREN || T < 1 || K < 1 || n < 1 || Mc < 1 || Mc > MAX_CONSIDERED || L < 1 || L > MAX_LEAVES ||
        calls < 0) { fprintf(stderr, "bad header\n"); return 2; }
    const size_t PC = (size_t)P * C, R = (size_t)P * L;
    std::vector<int> considered((size_t)(Mc + 1) * n), sim_index(P), sim_visits(PC), pending((size_t)P * N);
    State st(P, N, C, T, R);
    if (!(read_ints(considered) && st.read_search() && st.read_tree() && read_ints(sim_index) && read_ints(sim_visits) && read_ints(pending))) {
        fprintf(stderr, "the state ends early\n");
        return 2;
    }
    const int FILL = -7;
    std::vector<int> move_slot(P, FILL), move_action((size_t)P * 3, FILL), child_weights(PC, FILL), child_actions(PC * 3, FILL);
    std::vector<float> child_policy(PC, -7.0f);
    std::vector<double> root_value(P, -7.0);
    Evaluation<uint8_t> ev(R, K);
    std::vector<int> *const poked[] = {&st.selected, &st.num_nodes, &st.parent, &st.num_children, &st.first_child, &sim_index, &sim_visits, &pending};
    for (int call = 0; call < calls; call++) {
        const int phases = (int)read_word(&ok);
        const uint64_t seed = (uint64_t)read_word(&ok), step_index = (uint64_t)read_word(&ok);
        const int first_root = (int)read_word(&ok);
        const int64_t pokes = read_word(&ok);
        if (!poke(poked, pokes, &ok, call)) return 2;
        if (!ok || pokes < 0 || phases <= 0 || phases > 15 || ((phases & pcb_gumbel::PHASE_SELECT) && (phases & pcb_gumbel::PHASE_CHOOSE))) {
            fprintf(stderr, "call %d: bad phases\n", call);
            return 2;
        }
        if (phases & pcb_gumbel::PHASE_ABSORB) ok = ok && ev.read();
        if (!ok) { fprintf(stderr, "call %d: input ends early\n", call); return 2; }
        (void)c_puct;  // the rule has no exploration constant
        const Rule q{0.0, c_visit, c_scale, seed, step_index, first_root, n, Mc};
        unsigned errors = 0u;
        for (int p = 0; p < P; p++) {
            const size_t row = (size_t)p * C;
            const Root r = st.root(p);
            int *const pend = &pending[(size_t)p * N];
            if (phases & pcb_gumbel::PHASE_BEGIN) pcb_gumbel::gumbel_begin(C, &sim_index[p], &sim_visits[row]);
            if (phases & pcb_gumbel::PHASE_ABSORB)
                errors |= leaves_absorb(r, pend, L, st.selected.data(), ev.value.data(), ev.leaf_terminal.data(), ev.cand_count.data(), K, ev.cand_actions.data(),
                                        ev.cand_prior.data());
            if (phases & pcb_gumbel::PHASE_SELECT)
                errors |= tree_leaves_select(r, q, pend, L, considered.data(), &sim_index[p], &sim_visits[row], st.paths.data(), st.path_len.data(),
                                               st.selected.data());
            if (phases & pcb_gumbel::PHASE_CHOOSE)
                errors |= tree_choose(r, q, &sim_visits[row], &move_slot[p], &move_action[(size_t)p * 3], &child_weights[row], &child_policy[row],
                                                    &child_actions[3 * row], &root_value[p]);
        }
        out.push_back((int64_t)errors);
        st.put_search(); st.put_tree(); put(sim_index); put(sim_visits); put(pending);
        put(move_slot); put(move_action); put(child_weights); put_bits(child_policy); put(child_actions); put_bits(root_value);
    }
    return flush();
}
