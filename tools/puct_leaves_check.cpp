// puct_leaves_check.cpp -- csrc/pcb_puct_leaves.h on the CPU: replays a recorded sequence of pcbenv_puct_advance_leaves
// calls through leaves_init / leaves_absorb / leaves_select, root by root, checks every selection against the one
// pcbenv/search.py:puct_search(leaves=L) made when the sequence was recorded, and writes the state after every call
// (tests/test_puct_leaves_model.py compares the last one with puct_search's result, tests/test_puct_leaves_gpu.py every
// one with the kernel's).  A stand-alone program:
//   g++ -std=c++17 -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=all -I rl-environment-for-component-placement_amd/csrc
//
// stdin and stdout are streams of little-endian int64 words (a float64 travels as its bits, a float32 as its bits in the
// low half of a word).  R = P * L rows, row p * L + l the leaf l of root p.
//   in:   P N C T K L via calls c_puct | per call: phases check [LOADED: the tree, in the order of `out` from num_nodes to
//           reward_hi] [POKED: pokes | pokes x (tensor, flat index, value)]
//           [ABSORB: value[R] leaf_terminal[R] cand_count[R] cand_actions[R K 3] cand_prior[R K]]
//           [SELECT and check: path_len[R] paths[T R 3] as recorded]
//         via: 0 = through csrc/pcb_puct_leaves.h; 1 = through csrc/pcb_puct.h (puct_init / puct_absorb / puct_select,
//         L == 1 only; pending is then never touched after its zero fill).
//         phases: the PHASE_ bits of csrc/pcb_tree.h, POKED = 8 if the call brings pokes and LOADED = 16 if it brings a
//         tree: the tree tensors are replaced by it and pending is set to zero before the phases run (a tree that
//         pcbenv/search.py:puct_reroot made of an earlier one).  A poke stores `value` into
//         one element of the state before the phases of its call run -- the damage a caller can do to a tree.  tensor:
//         0 selected, 1 num_nodes, 2 parent, 3 num_children, 4 first_child, 5 pending (tests/puct_leaves_cases.py:POKED).
//         From the first poke on path_len == depth(selected) is no longer checked.
//   out:  per call: errors | selected[R] path_len[R] paths[T R 3] | num_nodes[P] parent depth visits num_children first_child
//           [P N] node_action[P N 3] prior value_sum value_max terminal [P N] reward_lo reward_hi [P] | pending[P N]
// Before the first call every int32 tensor holds -7 (what a test puts into the device tensors the kernel must leave alone).
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <vector>

#include "pcb_puct_leaves.h"

namespace {

bool read_words(int64_t *dst, size_t n) { return fread(dst, sizeof(int64_t), n, stdin) == n; }
int64_t read_word(bool *ok) { int64_t v = 0; *ok = *ok && read_words(&v, 1); return v; }
double as_double(int64_t bits) { double d; memcpy(&d, &bits, 8); return d; }
float as_float(int64_t bits) { const uint32_t b = (uint32_t)bits; float f; memcpy(&f, &b, 4); return f; }
int64_t as_bits(double d) { int64_t b; memcpy(&b, &d, 8); return b; }

std::vector<int64_t> out;
template <class V> void put(const V &v) { for (auto x : v) out.push_back((int64_t)x); }
void put_bits(const std::vector<double> &v) { for (double x : v) out.push_back(as_bits(x)); }

template <class I> bool read_ints(std::vector<I> &dst) {
    std::vector<int64_t> w(dst.size());
    if (!read_words(w.data(), w.size())) return false;
    for (size_t i = 0; i < w.size(); i++) dst[i] = (I)w[i];
    return true;
}

}  // namespace

int main() {
    using namespace pcb_puct_leaves;
    bool ok = true;
    const int P = (int)read_word(&ok), N = (int)read_word(&ok), C = (int)read_word(&ok), T = (int)read_word(&ok), K = (int)read_word(&ok),
              L = (int)read_word(&ok), via = (int)read_word(&ok), calls = (int)read_word(&ok);
    const double c_puct = as_double(read_word(&ok));
    if (!ok || P < 0 || N < 1 || C < 1 || C > MAX_CHILDREN || T < 1 || K < 1 || L < 1 || L > MAX_LEAVES || calls < 0 || via < 0 || via > 1 ||
        (via == 1 && L != 1)) { fprintf(stderr, "bad header\n"); return 2; }
    const size_t PN = (size_t)P * N, R = (size_t)P * L, TR3 = (size_t)T * R * 3, RK = R * K;
    const int FILL = -7;
    std::vector<int> num_nodes(P, FILL), parent(PN, FILL), depth(PN, FILL), visits(PN, FILL), num_children(PN, FILL), first_child(PN, FILL),
        node_action(PN * 3, FILL), pending(PN, FILL), selected(R, FILL), path_len(R, FILL), paths(TR3, FILL);
    std::vector<double> prior(PN, -7.0), value_sum(PN, -7.0), value_max(PN, -7.0), lo(P, -7.0), hi(P, -7.0);
    std::vector<uint8_t> terminal(PN, 0xf9), leaf_terminal(R);
    std::vector<double> value(R);
    std::vector<int> cand_count(R), cand_actions(RK * 3), want_len(R), want_paths(TR3);
    std::vector<float> cand_prior(RK);
    std::vector<int> *const poked[] = {&selected, &num_nodes, &parent, &num_children, &first_child, &pending};
    enum { POKED = 8, LOADED = 16 };
    unsigned errors = 0u;
    bool damaged = false;
    for (int call = 0; call < calls; call++) {
        const int word = (int)read_word(&ok), check = (int)read_word(&ok);
        const int phases = word & ~(POKED | LOADED);
        if (word & LOADED) {
            ok = ok && read_ints(num_nodes) && read_ints(parent) && read_ints(depth) && read_ints(visits) && read_ints(num_children) &&
                 read_ints(first_child) && read_ints(node_action);
            for (std::vector<double> *v : {&prior, &value_sum, &value_max}) for (double &x : *v) x = as_double(read_word(&ok));
            ok = ok && read_ints(terminal);
            for (std::vector<double> *v : {&lo, &hi}) for (double &x : *v) x = as_double(read_word(&ok));
            for (int &x : pending) x = 0;
        }
        const int64_t pokes = (word & POKED) ? read_word(&ok) : 0;
        for (int64_t i = 0; ok && i < pokes; i++) {
            const int64_t tensor = read_word(&ok), at = read_word(&ok), v = read_word(&ok);
            if (!ok || tensor < 0 || tensor >= 6 || at < 0 || (uint64_t)at >= poked[tensor]->size() || v != (int)v) { fprintf(stderr, "call %d: bad poke\n", call); return 2; }
            (*poked[tensor])[(size_t)at] = (int)v;
            damaged = true;
        }
        if (!ok || pokes < 0 || phases <= 0 || phases > 7 || ((phases & PHASE_INIT) && (phases & PHASE_ABSORB))) { fprintf(stderr, "call %d: bad phases\n", call); return 2; }
        if (phases & PHASE_ABSORB) {
            for (double &x : value) x = as_double(read_word(&ok));
            ok = ok && read_ints(leaf_terminal) && read_ints(cand_count) && read_ints(cand_actions);
            for (float &x : cand_prior) x = as_float(read_word(&ok));
        }
        if ((phases & PHASE_SELECT) && check) ok = ok && read_ints(want_len) && read_ints(want_paths);
        if (!ok) { fprintf(stderr, "call %d: input ends early\n", call); return 2; }
        for (int p = 0; p < P; p++) {
            const size_t s = (size_t)p * N;
            const Root r{N, C, T, P, p, &num_nodes[p], &parent[s], &depth[s], &visits[s], &num_children[s], &first_child[s], &node_action[3 * s],
                         &prior[s], &value_sum[s], &value_max[s], &terminal[s], &lo[p], &hi[p]};
            int *const pend = &pending[s];
            if (via == 1) {  // L == 1: row p
                if (phases & PHASE_INIT) { puct_init(r); for (int i = 0; i < N; i++) pend[i] = 0; }
                if (phases & PHASE_ABSORB)
                    errors |= puct_absorb(r, selected[p], value[p], leaf_terminal[p], cand_count[p], K, &cand_actions[(size_t)p * K * 3], &cand_prior[(size_t)p * K]);
                if (phases & PHASE_SELECT) errors |= puct_select(r, c_puct, paths.data(), &path_len[p], &selected[p]);
            } else {
                if (phases & PHASE_INIT) leaves_init(r, pend);
                if (phases & PHASE_ABSORB)
                    errors |= leaves_absorb(r, pend, L, selected.data(), value.data(), leaf_terminal.data(), cand_count.data(), K, cand_actions.data(), cand_prior.data());
                if (phases & PHASE_SELECT) errors |= leaves_select(r, pend, L, c_puct, paths.data(), path_len.data(), selected.data());
            }
            if (!(phases & PHASE_SELECT)) continue;
            for (int l = 0; l < L; l++) {
                const int row = leaf_row(p, L, l);
                if ((selected[row] == -1) != (path_len[row] == -1)) { fprintf(stderr, "call %d row %d: selected %d with path_len %d\n", call, row, selected[row], path_len[row]); return 1; }
                if (!damaged && selected[row] != -1 && path_len[row] != r.depth[selected[row]]) { fprintf(stderr, "call %d row %d: path_len %d, depth of the selected node %d\n", call, row, path_len[row], r.depth[selected[row]]); return 1; }
                if (!check) continue;
                if (path_len[row] != want_len[row]) { fprintf(stderr, "call %d row %d: path_len %d, recorded %d\n", call, row, path_len[row], want_len[row]); return 1; }
                for (int d = 0; d < path_len[row]; d++)
                    for (int k = 0; k < 3; k++)
                        if (paths[step_major(d, (int)R, row, k)] != want_paths[step_major(d, (int)R, row, k)]) { fprintf(stderr, "call %d row %d: path row %d differs from the recorded one\n", call, row, d); return 1; }
            }
        }
        out.push_back((int64_t)errors);
        put(selected); put(path_len); put(paths); put(num_nodes); put(parent); put(depth); put(visits); put(num_children); put(first_child);
        put(node_action); put_bits(prior); put_bits(value_sum); put_bits(value_max); put(terminal); put_bits(lo); put_bits(hi); put(pending);
    }
    if (fwrite(out.data(), sizeof(int64_t), out.size(), stdout) != out.size()) { fprintf(stderr, "short write\n"); return 2; }
    return 0;
}
