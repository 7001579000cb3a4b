// puct_move_check.cpp -- csrc/pcb_puct_move.h on the CPU: runs a sequence of pcbenv_puct_move calls through move_choose /
// move_reroot, root by root, on a tree it is handed, and writes the state after every call (tests/test_puct_move_model.py
// compares it with pcbenv/search.py:puct_choose / puct_reroot, the specification, tests/test_puct_move_gpu.py with the
// kernel's).  A stand-alone program:
//   g++ -std=c++17 -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=all -I rl-environment-for-component-placement_amd/csrc
//
// stdin and stdout are streams of little-endian int64 words (a float64 travels as its bits).
//   in:   P N C calls | the tree: num_nodes[P] parent depth visits num_children first_child [P N] node_action[P N 3]
//           prior value_sum value_max terminal [P N] reward_lo reward_hi [P]
//         per call: phases mode seed step_index first_root has_move has_reset pokes | pokes x (tensor, flat index, value)
//           [has_move: move_slot[P]] [has_reset: reset[P]]
//         phases, mode: the enums of csrc/pcb_puct_move.h.  has_move: the caller writes move_slot before the call.  A poke
//         stores `value` into one element of the state before the phases of its call run -- the damage a caller can do to a
//         tree.  tensor: 0 move_slot, 1 num_nodes, 2 parent, 3 num_children, 4 first_child (tests/puct_move_cases.py:POKED).
//   out:  per call: the error bits of that call | move_slot[P] move_action[P 3] child_visits[P C] child_actions[P C 3]
//           root_value[P] remap[P N] | the tree, in the order above
// Before the first call every int32 output tensor holds -7 and root_value -7.0 (what a test puts into the device tensors
// the kernel must leave alone).
#include "pcb_puct_move.h"
#include "puct_state.h"

using namespace puct_state;

int main() {
    using namespace pcb_move;
    bool ok = true;
    const int P = (int)read_word(&ok), N = (int)read_word(&ok), C = (int)read_word(&ok), calls = (int)read_word(&ok);
    if (!ok || P < 0 || N < 1 || C < 1 || C > MAX_CHILDREN || calls < 0) { fprintf(stderr, "bad header\n"); return 2; }
    const size_t PN = (size_t)P * N, PC = (size_t)P * C;
    const int FILL = -7;
    State st(P, N, C, 0, 0);  // the tree alone
    if (!st.read_tree()) { fprintf(stderr, "the tree ends early\n"); return 2; }
    std::vector<int> move_slot(P, FILL), move_action((size_t)P * 3, FILL), child_visits(PC, FILL), child_actions(PC * 3, FILL), remap(PN, FILL), reset(P, 0);
    std::vector<double> root_value(P, -7.0);
    std::vector<int> *const poked[] = {&move_slot, &st.num_nodes, &st.parent, &st.num_children, &st.first_child};
    for (int call = 0; call < calls; call++) {
        const int phases = (int)read_word(&ok), mode = (int)read_word(&ok);
        const uint64_t seed = (uint64_t)read_word(&ok), step_index = (uint64_t)read_word(&ok);
        const int first_root = (int)read_word(&ok), has_move = (int)read_word(&ok), has_reset = (int)read_word(&ok);
        const int64_t pokes = read_word(&ok);
        if (!ok || pokes < 0 || phases < 1 || phases > 3 || (mode != MODE_GREEDY && mode != MODE_PROPORTIONAL)) { fprintf(stderr, "call %d: bad phases or mode\n", call); return 2; }
        if (!poke(poked, pokes, &ok, call)) return 2;
        if (has_move) ok = ok && read_ints(move_slot);
        if (has_reset) ok = ok && read_ints(reset);
        if (!ok) { fprintf(stderr, "call %d: input ends early\n", call); return 2; }
        unsigned errors = 0u;
        for (int p = 0; p < P; p++) {
            const Root r = st.root(p);
            if (phases & PHASE_CHOOSE)
                errors |= move_choose(r, mode, seed, step_index, first_root, &child_visits[(size_t)p * C], &child_actions[(size_t)p * C * 3], &root_value[p],
                                      &move_slot[p], &move_action[(size_t)p * 3]);
            if (phases & PHASE_REROOT) errors |= move_reroot(r, move_slot[p], has_reset ? reset[p] : 0, &remap[(size_t)p * N]);
        }
        out.push_back((int64_t)errors);
        put(move_slot); put(move_action); put(child_visits); put(child_actions); put_bits(root_value); put(remap);
        st.put_tree();
    }
    return flush();
}
