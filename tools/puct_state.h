// puct_state.h -- the state the PUCT model programs keep between calls, stated once: the thirteen tree tensors of
// csrc/pcb_puct.h plus selected, path_len and paths, in the order they travel on the wire (tools/word_stream.h); the pokes
// a call may bring; and the evaluation an ABSORB call brings.  puct_model_check, puct_leaves_check, puct_move_check,
// puct_game_check and gumbel_check include it with quotes and keep what is their own: header words, further tensors,
// the dispatch of the phases and the checks of a selection.
//   the search part:  selected[R] path_len[R] paths[T R 3]       (R rows: P, or P * L for leaves; none for puct_move_check)
//   the tree:         num_nodes[P] parent depth visits num_children first_child [P N] node_action[P N 3]
//                     prior value_sum value_max terminal [P N] reward_lo reward_hi [P]
#pragma once
#include "pcb_puct.h"
#include "word_stream.h"

namespace puct_state {

using namespace word_stream;

struct State {
    int P, N, C, T;
    std::vector<int> selected, path_len, paths;
    std::vector<int> num_nodes, parent, depth, visits, num_children, first_child, node_action;
    std::vector<double> prior, value_sum, value_max;
    std::vector<uint8_t> terminal;
    std::vector<double> lo, hi;

    // all zero; T = 0 and R = 0 for a tool without the search part
    State(int P, int N, int C, int T, size_t R)
        : P(P), N(N), C(C), T(T), selected(R), path_len(R), paths((size_t)T * R * 3), num_nodes(P), parent((size_t)P * N), depth(parent.size()),
          visits(parent.size()), num_children(parent.size()), first_child(parent.size()), node_action(parent.size() * 3), prior(parent.size()),
          value_sum(parent.size()), value_max(parent.size()), terminal(parent.size()), lo(P), hi(P) {}

    // what a test puts into the device tensors the kernel must leave alone: -7, -7.0, 0xf9
    void fill() {
        for (std::vector<int> *v : {&selected, &path_len, &paths, &num_nodes, &parent, &depth, &visits, &num_children, &first_child, &node_action})
            v->assign(v->size(), -7);
        for (std::vector<double> *v : {&prior, &value_sum, &value_max, &lo, &hi}) v->assign(v->size(), -7.0);
        terminal.assign(terminal.size(), 0xf9);
    }

    bool read_search() { return read_ints(selected) && read_ints(path_len) && read_ints(paths); }
    bool read_tree() {
        return read_ints(num_nodes) && read_ints(parent) && read_ints(depth) && read_ints(visits) && read_ints(num_children) && read_ints(first_child) &&
               read_ints(node_action) && read_doubles(prior) && read_doubles(value_sum) && read_doubles(value_max) && read_ints(terminal) &&
               read_doubles(lo) && read_doubles(hi);
    }
    void put_search() const { put(selected); put(path_len); put(paths); }
    void put_tree() const {
        put(num_nodes); put(parent); put(depth); put(visits); put(num_children); put(first_child); put(node_action);
        put_bits(prior); put_bits(value_sum); put_bits(value_max); put(terminal); put_bits(lo); put_bits(hi);
    }

    // root p's slabs
    pcb_puct::Root root(int p) {
        const size_t s = (size_t)p * N;
        return pcb_puct::Root{N, C, T, P, p, &num_nodes[p], &parent[s], &depth[s], &visits[s], &num_children[s], &first_child[s], &node_action[3 * s],
                              &prior[s], &value_sum[s], &value_max[s], &terminal[s], &lo[p], &hi[p]};
    }
};

// `pokes` x (tensor, flat index, value): stores value into element `flat index` of table[tensor], the damage a caller can
// do to a tree.  Reads nothing once *ok is false; false, with its message on stderr, on a poke that names no element.
template <size_t n> bool poke(std::vector<int> *const (&table)[n], int64_t pokes, bool *ok, int call) {
    for (int64_t i = 0; *ok && i < pokes; i++) {
        const int64_t tensor = read_word(ok), at = read_word(ok), v = read_word(ok);
        if (!*ok || tensor < 0 || tensor >= (int64_t)n || at < 0 || (uint64_t)at >= table[tensor]->size() || v != (int)v) { fprintf(stderr, "call %d: bad poke\n", call); return false; }
        (*table[tensor])[(size_t)at] = (int)v;
    }
    return true;
}

// What an ABSORB call brings for R rows: value[R] leaf_terminal[R] cand_count[R] cand_actions[R K 3] cand_prior[R K].
// Flag: the element type of leaf_terminal (pcb_puct_leaves.h takes the tensor as the kernel does, uint8).
template <class Flag = int> struct Evaluation {
    int K;
    std::vector<double> value;
    std::vector<Flag> leaf_terminal;
    std::vector<int> cand_count, cand_actions;
    std::vector<float> cand_prior;
    Evaluation(size_t R, int K) : K(K), value(R), leaf_terminal(R), cand_count(R), cand_actions(R * K * 3), cand_prior(R * K) {}
    bool read() { return read_doubles(value) && read_ints(leaf_terminal) && read_ints(cand_count) && read_ints(cand_actions) && read_floats(cand_prior); }
    // pcb_puct.h's absorb of row `row` into root r
    unsigned absorb(const pcb_puct::Root &r, int selected, size_t row) const {
        return pcb_puct::puct_absorb(r, selected, value[row], leaf_terminal[row], cand_count[row], K, &cand_actions[row * K * 3], &cand_prior[row * K]);
    }
};

}  // namespace puct_state
