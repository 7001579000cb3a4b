"""Cases, recordings and the CPU model of pcbenv_puct_advance (plain module, no test; needs no GPU).

The specification is pcbenv/search.py:puct_search.  `record` runs it on the CPU with an evaluator that writes down, per
iteration, the `paths` and `path_len` it was asked for and the evaluation it gave back; `search_calls` turns such a
recording into the sequence of pcbenv_puct_advance calls that `puct_search_device` makes (INIT|SELECT, then ABSORB|SELECT
per evaluation, ABSORB alone for the last), and `replay` feeds a sequence to tools/puct_model_check.cpp -- csrc/pcb_puct.h
compiled for the CPU with AddressSanitizer and UBSan, a program of its own -- which checks every selection against the
recorded one and returns the state after every call.  The GPU tests compare the kernel with those states.

`synthetic_evaluator` is a seeded hash of (root, path): values from {0.25, 0.5, 0.75}, priors from a small set with
repeats -- so that equal scores occur -- candidate counts over 0 .. K, a leaf terminal by hash and always at depth T; root
p % 7 == 6 is terminal at the root and root p % 7 == 5 never has a candidate.  `real_evaluator` is its real-valued twin: values
whose sums depend on the order of the additions, softmax priors (tests/near_tie_cases.py records searches with it).

`exact_ties` walks the selections of a replay again in Python floats -- the operations of csrc/pcb_puct.h:puct_score one
by one, each a single IEEE operation -- and counts the levels at which the best score occurs twice.

`WIDTHS` / `width_case` are synthetic searches at every group width of the kernel over three blocks; `damaged` continues a
healthy search with one call before which the caller has written out-of-range values into the tree (`pokes`), the cases of
csrc/pcb_puct.h's promise that such a tree stops the walk and reports ERR_TREE."""
import functools
import math
from types import SimpleNamespace

import numpy as np
import torch

import model_harness as mh
import tree_cases
from model_harness import REPO, flat, same_bits, words as _words  # noqa: F401  (the other case modules and the tests take them from here)
from pcbenv.search import Evaluation, puct_search

INIT, ABSORB, SELECT = 1, 2, 4
ERR_FULL, ERR_TREE = 1, 2  # the bits of the error word
FILL = -7  # what the model's int32 tensors hold before the first call
TREE_FIELDS = ("num_nodes", "parent", "depth", "visits", "num_children", "first_child", "node_action", "prior", "value_sum", "value_max",
               "terminal", "reward_lo", "reward_hi")
STATE_FIELDS = ("selected", "path_len", "paths") + TREE_FIELDS
FLOATS = ("prior", "value_sum", "value_max", "reward_lo", "reward_hi")
INPUTS = ("value", "leaf_terminal", "cand_count", "cand_actions", "cand_prior")
POKED_CALL = 8  # next to the phases of a call in the model's input: pokes follow
POKED = ("selected", "num_nodes", "parent", "num_children", "first_child")  # the tensors a call's pokes may name, by number


def shapes(P, N, T):
    s = {"selected": (P,), "path_len": (P,), "paths": (T, P, 3), "num_nodes": (P,), "node_action": (P, N, 3), "reward_lo": (P,), "reward_hi": (P,)}
    s.update({n: (P, N) for n in ("parent", "depth", "visits", "num_children", "first_child", "prior", "value_sum", "value_max", "terminal")})
    return s


def program():
    """tools/puct_model_check.cpp as tests/model_harness.py:tool builds it; None without g++."""
    return mh.tool("puct_model_check")


def record(P, T, iterations, c_puct, max_children, evaluate, step_index=0, capacity=None, cfg=None, tree=None):
    """puct_search on the CPU -> (its result, [(paths, path_len, value float64 [P], leaf_terminal uint8 [P], cand_count int32
    [P], cand_actions int32 [P, K, 3], cand_prior float32 [P, K])]).  tree: the search goes on in that tree."""
    calls = []

    def recording(paths, path_len, s):
        ev = evaluate(paths, path_len, s)
        calls.append((paths.clone().numpy(), path_len.clone().numpy(), ev.value.to(torch.float64).numpy().copy(),
                      ev.terminal.to(torch.uint8).numpy().copy(), ev.cand_count.to(torch.int32).numpy().copy(),
                      ev.cand_actions.to(torch.int32).numpy().copy(), ev.cand_prior.to(torch.float32).numpy().copy()))
        return ev
    root = SimpleNamespace(num_envs=P, device="cpu", cfg=cfg)
    ps = puct_search(root, iterations, step_index, recording, c_puct=c_puct, max_children=max_children, max_steps=T, capacity=capacity, tree=tree)
    return ps, calls


def search_calls(calls, split=False):
    """The pcbenv_puct_advance calls of a search: dicts with phases, the evaluation absorbed (or None) and the recorded
    selection to check (or None).  split: every phase in a call of its own."""
    out = []
    for m in range(len(calls) + 1):
        absorbed = None if m == 0 else calls[m - 1][2:]
        chosen = None if m == len(calls) else calls[m][:2]
        first = INIT if m == 0 else ABSORB
        if split:
            out.append(dict(phases=first, evaluation=absorbed, expect=None))
            if chosen is not None:
                out.append(dict(phases=SELECT, evaluation=None, expect=chosen))
        else:
            out.append(dict(phases=first | (SELECT if chosen is not None else 0), evaluation=absorbed, expect=chosen))
    return out


def replay(P, N, C, T, K, c_puct, seq):
    """-> [state after call i]: dicts of STATE_FIELDS (int64; FLOATS as float64) and `errors`.  Raises if the program
    reports a selection that differs from the recorded one, or anything on stderr.  A call may carry `pokes`, a list of
    (tensor of POKED, flat index, value) stored into the state before its phases run."""
    parts = [np.array([P, N, C, T, K, len(seq), mh.bits(c_puct)], np.int64)]
    for c in seq:
        pokes = c.get("pokes", ())
        parts.append(np.array([c["phases"] | (POKED_CALL if pokes else 0), int(c["expect"] is not None)] +
                              ([len(pokes)] + [w for name, at, value in pokes for w in (POKED.index(name), at, value)] if pokes else []), np.int64))
        if c["phases"] & ABSORB:
            value, over, count, actions, prior = c["evaluation"]
            assert actions.shape == (P, K, 3) and prior.shape == (P, K) and prior.dtype == np.float32
            parts += [_words(value, True), _words(over), _words(count), _words(actions), mh.float32_words(prior)]
        if c["expect"] is not None:
            parts += [_words(c["expect"][1]), _words(c["expect"][0])]
    return mh.cut(mh.run_words(program(), parts), len(seq), STATE_FIELDS, shapes(P, N, T), FLOATS)


def compare_with_search(state, ps):
    """The model's final state against puct_search's result, field by field, floats by their bits."""
    for f in TREE_FIELDS:
        t = getattr(ps, f).numpy()
        if f in FLOATS:
            assert same_bits(state[f], t), f
        else:
            assert np.array_equal(state[f], t.astype(np.int64)), f
    assert state["errors"] == int(ps.errors)


def kept(cand_count, K, C):
    """csrc/pcb_puct.h:kept_candidates."""
    return min(max(int(cand_count), 0), min(K, C))


def _scores(state, p, node, c_puct):
    lo, hi = float(state["reward_lo"][p]), float(state["reward_hi"][p])
    fc, k = int(state["first_child"][p, node]), int(state["num_children"][p, node])
    out = []
    for c in range(k):
        ch = fc + c
        n_c = int(state["visits"][p, ch])
        q = (float(state["value_sum"][p, ch]) / float(n_c) - lo) / (hi - lo) if n_c > 0 and hi > lo else 0.0
        out.append(q + c_puct * float(state["prior"][p, ch]) * math.sqrt(float(max(int(state["visits"][p, node]), 1))) / (1.0 + float(n_c)))
    return fc, out


def exact_ties(state, c_puct, T):
    """The selections of `state` (a healthy state dumped after a call with SELECT) redone in Python floats; checks the model's
    choice on the way.  -> the levels of the descents at which the best score occurs twice."""
    n = 0
    for p in range(state["num_nodes"].shape[0]):
        node, d = 0, 0
        while d < T and not state["terminal"][p, node] and state["num_children"][p, node] != 0:
            fc, sc = _scores(state, p, node, c_puct)
            n += sc.count(max(sc)) > 1
            node, d = fc + sc.index(max(sc)), d + 1
        assert node == state["selected"][p] and d == state["path_len"][p], (p, node, d)
    return n


def ties(case):
    return sum(exact_ties(s, case.c_puct, case.T) for s, c in zip(case.states, case.seq) if c["phases"] & SELECT)


# ---- the synthetic evaluator ----------------------------------------------------------------------------------------
def _mix(*xs):
    h = 0x9E3779B97F4A7C15
    for x in xs:
        h = ((h ^ (int(x) & 0xFFFFFFFF)) * 0xBF58476D1CE4E5B9) & 0xFFFFFFFFFFFFFFFF
        h ^= h >> 29
    return h


PRIORS = (0.5, 0.25, 0.25, 0.125, 0.0625, 0.25)  # float32 holds each exactly


def synthetic_evaluator(P, T, K, seed):
    """A function of (root, path).  Candidate c of a node is the action ((h + c) % 2, 0, c), h the node's hash."""
    def evaluate(paths, path_len, step_index0):
        paths, path_len = paths.numpy(), path_len.numpy()
        value, over, count = np.zeros(P), np.zeros(P, np.uint8), np.zeros(P, np.int32)
        actions, prior = np.zeros((P, K, 3), np.int32), np.zeros((P, K), np.float32)
        for p in range(P):
            h = _mix(seed, p)
            for t in range(int(path_len[p])):
                h = _mix(h, paths[t, p, 0], paths[t, p, 2])
            value[p] = (0.25, 0.5, 0.75)[(h >> 16) % 3]
            over[p] = p % 7 == 6 or path_len[p] == T or (path_len[p] > 0 and (h >> 24) % 5 == 0)
            count[p] = 0 if p % 7 == 5 else (h >> 32) % (K + 1) if (h >> 40) % 4 == 0 else K
            for c in range(K):  # all K rows are filled in whatever the count says: a clamped count reads them
                actions[p, c] = ((h + c) % 2, 0, c)
                prior[p, c] = PRIORS[_mix(h, c) % len(PRIORS)]
        return Evaluation(torch.from_numpy(value), torch.from_numpy(over), torch.from_numpy(count), torch.from_numpy(actions), torch.from_numpy(prior))
    return evaluate


ONE_ULP_APART = (0.7310585786300049, math.nextafter(0.7310585786300049, 1.0))


def real_evaluator(P, T, K, seed):
    """A function of (root, path) as synthetic_evaluator, with real-valued evaluations: value sums depend on the order of
    the additions, the range is no power of two and a prior times a root is rounded.  The values, by root p % 5:
      0  -4 +- 1, all 53 mantissa bits hashed           1  1e9 plus multiples of 1e-3, which cancel in the normalisation
      2  both signs over magnitudes 1e-12 .. 1e6        3  -3.57 always: reward_hi == reward_lo for the whole search
      4  two values one ulp apart: the range is one ulp
    The priors are the float32 softmax of hashed logits in [-12, 12] over the K candidates; every seventh node carries one
    prior that is exactly 0 and one that is denormal (1e-40), and every third node's row is scaled by 1.7 and left
    unnormalised.  A leaf is terminal by hash (one in five below the root) and always at depth T; one node in eight gets
    fewer than K candidates."""
    def evaluate(paths, path_len, step_index0):
        paths, path_len = paths.numpy(), path_len.numpy()
        value, over, count = np.zeros(P), np.zeros(P, np.uint8), np.zeros(P, np.int32)
        actions, prior = np.zeros((P, K, 3), np.int32), np.zeros((P, K), np.float32)
        for p in range(P):
            h = _mix(seed, p)
            for t in range(int(path_len[p])):
                h = _mix(h, paths[t, p, 0], paths[t, p, 2])
            frac = float(_mix(h, 1) >> 11) / 9007199254740992.0  # 53 hashed bits in [0, 1)
            value[p] = (-5.0 + 2.0 * frac, 1e9 + 1e-3 * float((h >> 16) % 7), (1.0 if (h >> 20) & 1 else -1.0) * (1.0 + frac) * 10.0 ** ((h >> 24) % 19 - 12),
                        -3.57, ONE_ULP_APART[(h >> 16) & 1])[p % 5]
            over[p] = path_len[p] == T or (path_len[p] > 0 and (h >> 44) % 5 == 0)
            count[p] = (h >> 32) % (K + 1) if (h >> 40) % 8 == 0 else K
            logits = np.array([24.0 * float(_mix(h, 2, c) >> 11) / 9007199254740992.0 - 12.0 for c in range(K)], np.float32)
            e = np.exp(logits - logits.max())
            row = e / e.sum(dtype=np.float32)
            if (h >> 48) % 3 == 0:
                row = row * np.float32(1.7)
            if (h >> 52) % 7 == 0 and K >= 2:
                row[(h >> 56) % K], row[((h >> 56) + 1) % K] = 0.0, 1e-40
            for c in range(K):  # all K rows are filled in whatever the count says: a clamped count reads them
                actions[p, c] = ((h + c) % 2, 0, c)
            prior[p] = row
        return Evaluation(torch.from_numpy(value), torch.from_numpy(over), torch.from_numpy(count), torch.from_numpy(actions), torch.from_numpy(prior))
    return evaluate


@functools.lru_cache(maxsize=None)
def synthetic(P, T, C, K, iterations, c_puct=1.25, seed=11, capacity=None, split=False):
    """-> SimpleNamespace(P, N, C, T, K, c_puct, ps, seq, states): a recorded search with the synthetic evaluator and its replay."""
    ps, calls = record(P, T, iterations, c_puct, C, synthetic_evaluator(P, T, K, seed), step_index=100, capacity=capacity)
    N = 1 + iterations * C if capacity is None else capacity
    seq = search_calls(calls, split)
    return SimpleNamespace(P=P, N=N, C=C, T=T, K=K, c_puct=c_puct, ps=ps, seq=seq, states=replay(P, N, C, T, K, c_puct, seq))


# ---- every group width, more than one block ------------------------------------------------------------------------
group_lanes = tree_cases.group_lanes  # csrc/pcb_group.h:group_lanes -- the lanes per root of the k_puct_advance<G> the host picks for max_children = C


BLOCK = 256  # threads of a k_puct_advance workgroup: 256 / G roots
# P, C, K, iterations of synthetic(P, 5, C, K, iterations); then the G and the blocks the row is there for.  C == G (every
# lane may own a child) and C == G / 2 + 1 (the most idle lanes of a width) at each width; three blocks, the last partly
# filled, and from G = 16 on an odd P: the last wavefront in use is partly filled too.  K is C but for one row above it
# (truncated to C) and one below (never more than K children); the single root of G64_C64_P1 has all 64 lanes at work.
WIDTHS = {
    "G4_C3_P130": (130, 3, 3, 10, 4, 3),
    "G4_C4_P130": (130, 4, 4, 10, 4, 3),
    "G8_C5_P67": (67, 5, 5, 10, 8, 3),
    "G8_C8_P70": (70, 8, 8, 10, 8, 3),
    "G16_C9_P35": (35, 9, 12, 10, 16, 3),
    "G16_C16_P35": (35, 16, 16, 10, 16, 3),
    "G32_C17_P19": (19, 17, 17, 10, 32, 3),
    "G32_C32_P19": (19, 32, 20, 10, 32, 3),
    "G64_C33_P9": (9, 33, 33, 10, 64, 3),
    "G64_C63_P9": (9, 63, 63, 10, 64, 3),
    "G64_C64_P1": (1, 64, 64, 10, 64, 1),
}
WIDTH_T = 5


def width_case(name):
    """synthetic() of a row of WIDTHS, after the checks that the row still exercises what it is there for: the width, the
    blocks, the partly filled tail, a descent through an expanded node in the first and in the last block, exact ties, no
    error."""
    P, C, K, iterations, G, blocks = WIDTHS[name]
    per_block, per_wave = BLOCK // G, 64 // G
    assert group_lanes(C) == G and (C == G or C == G // 2 + 1 or (G, C) == (64, 63)), name
    assert -(-P // per_block) == blocks and (P % per_block != 0 or blocks == 1), name
    assert G < 16 or P % 2 == 1 and (per_wave == 1 or P % per_wave != 0), name
    case = synthetic(P, WIDTH_T, C, K, iterations)
    first, last = slice(0, per_block), slice((blocks - 1) * per_block, P)
    assert any((s["path_len"][first] > 0).any() for s in case.states) and any((s["path_len"][last] > 0).any() for s in case.states), name
    assert int(case.states[-1]["num_children"].max()) == min(K, C), name  # a node with every child the row allows
    assert case.states[-1]["errors"] == 0, name
    assert ties(case) > 0, name
    return case


# ---- trees the caller has damaged -----------------------------------------------------------------------------------
# G: P, T, C, K, iterations of the healthy search, and the roots a scenario may damage: 0 < p < P - 1 (a check that failed
# to hold would then show in a neighbouring root's rows of the same tensor, which every comparison covers), not the root
# without candidates (p % 7 == 5) nor the terminal one (p % 7 == 6).
DAMAGE_GAMES = {4: (9, 5, 3, 3, 12, (1, 2, 3)), 16: (7, 5, 9, 9, 12, (1, 2, 3)), 64: (3, 5, 33, 33, 12, (1,))}
DAMAGE = ("selected_N", "selected_minus_1", "num_nodes_0", "num_nodes_N_plus_1", "first_child_0", "first_child_N", "first_child_plus_k_over_N",
          "num_children_minus_1", "num_children_C_plus_5", "parent_N", "parent_self", "cand_count_minus_3", "cand_count_K_plus_5")
DAMAGE_CASES = [(G, n) for G in DAMAGE_GAMES for n in DAMAGE]


@functools.lru_cache(maxsize=None)
def damaged(G, name):
    """-> SimpleNamespace(P, N, C, T, K, c_puct, seq, states, base, k, p, node, ...): a healthy prefix seq[:k] of the search
    of width G, after which root p is expanded and its selected node is a fresh leaf below the root that the evaluation of
    call k does not call terminal; call k with the pokes (or, for the cand_count scenarios, with that count in its
    evaluation: data, not damage); then two more ABSORB|SELECT calls with the evaluations the healthy search got.  `base` is
    the healthy search: its states are those of the roots nothing was done to.  node: the node call k's ABSORB is about."""
    P, T, C, K, iterations, roots = DAMAGE_GAMES[G]
    base = synthetic(P, T, C, K, iterations)
    N, shp = base.N, shapes(P, base.N, T)
    p = roots[DAMAGE.index(name) % len(roots)]
    for k in range(1, len(base.seq) - 3):
        st = base.states[k - 1]
        node = int(st["selected"][p])
        if node != 0 and st["num_children"][p, node] == 0 and not st["terminal"][p, node] and st["num_nodes"][p] + C <= N and \
                all(base.seq[i]["phases"] == ABSORB | SELECT for i in range(k, k + 3)) and not base.seq[k]["evaluation"][1][p]:
            break
    else:
        raise AssertionError(f"no call of the healthy search after which root {p} suits {name}")
    assert st["errors"] == 0 and st["num_children"][p, 0] >= 1
    nch = int(st["num_children"][p, 0])
    pokes = []
    poke = lambda f, value, *index: pokes.append((f, flat(shp[f], *index), int(value)))
    evaluation = base.seq[k]["evaluation"]
    if name.startswith("selected_"):
        poke("selected", N if name == "selected_N" else -1, p)
    elif name.startswith("num_nodes_"):
        poke("num_nodes", 0 if name == "num_nodes_0" else N + 1, p)
    elif name.startswith("first_child_"):
        poke("first_child", {"first_child_0": 0, "first_child_N": N, "first_child_plus_k_over_N": N - nch + 1}[name], p, 0)
    elif name.startswith("num_children_"):
        poke("num_children", -1 if name == "num_children_minus_1" else C + 5, p, 0)
    elif name.startswith("parent_"):
        poke("parent", N if name == "parent_N" else node, p, node)
    else:
        evaluation = tuple(np.array(a, copy=True) for a in evaluation)
        evaluation[2][p] = -3 if name == "cand_count_minus_3" else K + 5
    seq = base.seq[:k] + [dict(phases=ABSORB | SELECT, evaluation=evaluation, expect=None, pokes=pokes)] + \
        [dict(phases=ABSORB | SELECT, evaluation=base.seq[i]["evaluation"], expect=None) for i in (k + 1, k + 2)]
    return SimpleNamespace(P=P, N=N, C=C, T=T, K=K, c_puct=base.c_puct, seq=seq, states=replay(P, N, C, T, K, base.c_puct, seq), base=base, k=k,
                           p=p, node=node, name=name)
