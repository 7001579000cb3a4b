"""Cases, recordings and the CPU model of pcbenv_tree_advance (plain module, no test; needs no GPU).

The specification is pcbenv/search.py:tree_search.  `record` runs it on the CPU with a backend that writes down, per
iteration, the `paths` and `path_len` it was asked for and the reward, length and actions it gave back; `search_calls` turns
such a recording into the sequence of pcbenv_tree_advance calls that `tree_search_device` makes (INIT|SELECT, then
ABSORB|SELECT per playout, ABSORB alone for the last), and `replay` feeds a sequence to tools/tree_model_check.cpp --
csrc/pcb_tree.h compiled for the CPU with AddressSanitizer and UBSan, a program of its own -- which checks every selection
against the recorded one and returns the state after every call.  The GPU tests compare the kernel with those states.

`synthetic_backend` is a seeded game over a small action set whose rewards come from {0.25, 0.5, 0.75}, so that equal
means, and with equal visits equal scores, occur; root p % 7 == 5 is refused by every playout (length 0) and the episode
of root p % 7 == 6 is over after its first transition (length 1, the root's children are terminal).

`score_gaps` walks the selections of a replay again in Python floats -- the operations of csrc/pcb_tree.h:uct_score one by
one, each a single IEEE operation -- and returns the distances between the best and the second-best score.

`WIDTHS` / `width_case` are synthetic searches at every group width of the kernel over three blocks; `damaged` continues a
healthy search with one call before which the caller has written out-of-range values into the tree (`pokes`), the cases of
csrc/pcb_tree.h's promise that such a tree stops the walk and reports ERR_TREE."""
import functools
import math
from types import SimpleNamespace

import numpy as np
import torch

import model_harness as mh
from model_harness import REPO, flat, same_bits, words as _words  # noqa: F401  (the tests take them from here)
from pcbenv.batched_env import Playout
from pcbenv.search import ln_table, tree_search

INIT, ABSORB, SELECT = 1, 2, 4
ERR_FULL, ERR_TREE = 1, 2  # the bits of the error word
FILL = -7  # what the model's int32 tensors hold before the first call
TREE_FIELDS = ("num_nodes", "parent", "depth", "visits", "num_children", "node_action", "children", "value_sum", "value_max", "terminal",
               "reward_lo", "reward_hi", "best_reward", "best_length", "best_actions")
STATE_FIELDS = ("selected", "path_len", "paths") + TREE_FIELDS
FLOATS = ("value_sum", "value_max", "reward_lo", "reward_hi", "best_reward")
ITERATIONS, STEP_INDEX, C_UCT, MAX_CHILDREN = 24, 5000, 0.7, 3          # of the searches on real roots (tests/test_tree_search_gpu.py's)
ORACLE_CASES = (("small_pin", ITERATIONS), ("c3_centroid", ITERATIONS), ("spatial_7x100_t256", 12))
POKED_CALL = 8  # next to the phases of a call in the model's input: pokes follow
POKED = ("selected", "num_nodes", "parent", "depth", "num_children", "children")  # the tensors a call's pokes may name, by number
GAP_BOUND = 1e-12  # a last-bit difference between two implementations of log moves a score by some 1e-16


def shapes(P, N, C, T):
    s = {"selected": (P,), "path_len": (P,), "paths": (T, P, 3), "num_nodes": (P,), "node_action": (P, N, 3), "children": (P, N, C),
         "reward_lo": (P,), "reward_hi": (P,), "best_reward": (P,), "best_length": (P,), "best_actions": (T, P, 3)}
    s.update({n: (P, N) for n in ("parent", "depth", "visits", "num_children", "value_sum", "value_max", "terminal")})
    return s


def program():
    """tools/tree_model_check.cpp as tests/model_harness.py:tool builds it; None without g++."""
    return mh.tool("tree_model_check")


def record(P, T, iterations, c_uct, max_children, backend, step_index=0, cfg=None):
    """tree_search on the CPU -> (its result, [(paths, path_len, reward float64, length int32, actions int32 [T, P, 3])])."""
    calls = []

    def recording(paths, path_len, s):
        po = backend(paths, path_len, s)
        acts = torch.zeros((T, P, 3), dtype=torch.int32)
        acts[:po.actions.shape[0]] = po.actions[:T]
        calls.append((paths.clone().numpy(), path_len.clone().numpy(), po.reward.to(torch.float64).numpy().copy(),
                      po.length.to(torch.int32).numpy().copy(), acts.numpy()))
        return po
    root = SimpleNamespace(num_envs=P, device="cpu", cfg=cfg)
    ts = tree_search(root, iterations, step_index, c_uct=c_uct, max_children=max_children, backend=recording, max_steps=T)
    return ts, calls


def search_calls(calls, split=False):
    """The pcbenv_tree_advance calls of a search: dicts with phases, the playout absorbed (or None) and the recorded
    selection to check (or None).  split: every phase in a call of its own."""
    out = []
    for m in range(len(calls) + 1):
        absorbed = None if m == 0 else calls[m - 1][2:]
        chosen = None if m == len(calls) else calls[m][:2]
        first = INIT if m == 0 else ABSORB
        if split:
            out.append(dict(phases=first, playout=absorbed, expect=None))
            if chosen is not None:
                out.append(dict(phases=SELECT, playout=None, expect=chosen))
        else:
            out.append(dict(phases=first | (SELECT if chosen is not None else 0), playout=absorbed, expect=chosen))
    return out


def replay(P, N, C, T, c_uct, seq):
    """-> [state after call i]: dicts of STATE_FIELDS (int64; FLOATS as float64) and `errors`.  Raises if the program
    reports a selection that differs from the recorded one, or anything on stderr.  A call may carry `pokes`, a list of
    (tensor of POKED, flat index, value) stored into the state before its phases run."""
    parts = [np.array([P, N, C, T, len(seq), mh.bits(c_uct)], np.int64), _words(ln_table(N).numpy(), True)]
    for c in seq:
        pokes = c.get("pokes", ())
        parts.append(np.array([c["phases"] | (POKED_CALL if pokes else 0), int(c["expect"] is not None)] +
                              ([len(pokes)] + [w for name, at, value in pokes for w in (POKED.index(name), at, value)] if pokes else []), np.int64))
        if c["phases"] & ABSORB:
            r, L, a = c["playout"]
            parts += [_words(r, True), _words(L), _words(a)]
        if c["expect"] is not None:
            parts += [_words(c["expect"][1]), _words(c["expect"][0])]
    return mh.cut(mh.run_words(program(), parts), len(seq), STATE_FIELDS, shapes(P, N, C, T), FLOATS)


def compare_with_search(state, ts, N):
    """The model's final state against tree_search's result (whose tensors have N = iterations + 1 slots), field by field."""
    L = ts.best_length.numpy()
    pairs = dict(num_nodes=ts.num_nodes, parent=ts.parent, depth=ts.depth, visits=ts.visits, node_action=ts.node_action,
                 children=ts.children, terminal=ts.terminal, best_length=ts.best_length)
    for f, t in pairs.items():
        assert np.array_equal(state[f], t.numpy().astype(np.int64)), f
    for f, t in dict(value_sum=ts.value_sum, value_max=ts.value_max, best_reward=ts.best_reward).items():
        assert same_bits(state[f], t.numpy()), f
    assert np.array_equal(state["num_children"], (ts.children.numpy() >= 0).sum(axis=2)), "num_children"
    for p in range(len(L)):
        assert np.array_equal(state["best_actions"][:L[p], p], ts.best_actions[:L[p], p].numpy()), p


def score_gaps(state, C, c_uct, N):
    """The selections of `state` (a state dumped after a call with SELECT) redone in Python floats: the non-zero distances
    between the best and the second-best score of every level of every root's descent; checks the model's choice on the way."""
    ln = ln_table(N).numpy()
    gaps = []
    for p in range(state["num_nodes"].shape[0]):
        lo, hi = float(state["reward_lo"][p]), float(state["reward_hi"][p])
        node, d = 0, 0
        while not state["terminal"][p, node] and state["num_children"][p, node] == C:
            scores = []
            for c in range(C):
                ch = int(state["children"][p, node, c])
                n_c = float(max(int(state["visits"][p, ch]), 1))
                mean = float(state["value_sum"][p, ch]) / n_c
                q = (mean - lo) / (hi - lo) if hi > lo else 0.0
                scores.append(q + c_uct * math.sqrt(float(ln[min(max(int(state["visits"][p, node]), 1), N)]) / n_c))
            best = scores.index(max(scores))
            if C > 1:
                gap = scores[best] - max(s for c, s in enumerate(scores) if c != best)
                if gap != 0.0:
                    gaps.append(gap)
            node, d = int(state["children"][p, node, best]), d + 1
        assert node == state["selected"][p] and d == state["path_len"][p], (p, node, d)
    return gaps


def min_gap(states, seq, C, c_uct, N):
    gaps = [g for st, c in zip(states, seq) if c["phases"] & SELECT for g in score_gaps(st, C, c_uct, N)]
    return min(gaps) if gaps else math.inf


def exact_ties(state, C, c_uct, N):
    """Levels of the descents of `state` at which the best score occurs twice."""
    n = 0
    ln = ln_table(N).numpy()
    for p in range(state["num_nodes"].shape[0]):
        lo, hi, node = float(state["reward_lo"][p]), float(state["reward_hi"][p]), 0
        while not state["terminal"][p, node] and state["num_children"][p, node] == C:
            sc = []
            for c in range(C):
                ch = int(state["children"][p, node, c])
                n_c = float(max(int(state["visits"][p, ch]), 1))
                q = (float(state["value_sum"][p, ch]) / n_c - lo) / (hi - lo) if hi > lo else 0.0
                sc.append(q + c_uct * math.sqrt(float(ln[min(max(int(state["visits"][p, node]), 1), N)]) / n_c))
            n += sc.count(max(sc)) > 1
            node = int(state["children"][p, node, sc.index(max(sc))])
    return n


def ties(case):
    return sum(exact_ties(s, case.C, case.c_uct, case.N) for s, c in zip(case.states, case.seq) if c["phases"] & SELECT)


# ---- the synthetic game ---------------------------------------------------------------------------------------------
def _mix(*xs):
    h = 0x9E3779B97F4A7C15
    for x in xs:
        h = ((h ^ (int(x) & 0xFFFFFFFF)) * 0xBF58476D1CE4E5B9) & 0xFFFFFFFFFFFFFFFF
        h ^= h >> 29
    return h


def synthetic_backend(P, T, seed, orientations=2, cells=3):
    """A game over actions (o, 0, y), o < orientations, y < cells.  The action drawn at transition t is a function of
    (seed, root, step index); an episode ends after transition t if a hash of its actions so far says so (one in three) or at
    t = T - 1; its reward is one of 0.25, 0.5, 0.75 by a hash of all its actions."""
    def backend(paths, path_len, step_index0):
        paths, path_len = paths.numpy(), path_len.numpy()
        acts, reward, length = np.zeros((T, P, 3), np.int32), np.zeros(P), np.zeros(P, np.int32)
        for p in range(P):
            if p % 7 == 5:
                continue  # a refused row: length 0, reward 0.0, no action
            h = _mix(seed, p)
            for t in range(T):
                if t < path_len[p]:
                    a = paths[t, p]
                else:
                    u = _mix(seed, p, step_index0 + t)
                    a = np.array([u % orientations, 0, (u >> 8) % cells], np.int32)
                acts[t, p] = a
                h = _mix(h, a[0], a[2])
                length[p] = t + 1
                if p % 7 == 6 or h % 3 == 0:
                    break
            reward[p] = (0.25, 0.5, 0.75)[(h >> 16) % 3]
        return Playout(torch.from_numpy(reward), torch.from_numpy((length > 0).astype(np.uint8)), torch.from_numpy(length), None,
                       torch.from_numpy(acts))
    return backend


@functools.lru_cache(maxsize=None)
def synthetic(P, T, C, iterations, c_uct=0.9, seed=11, capacity=None, split=False, cells=3):
    """-> SimpleNamespace(P, N, C, T, c_uct, ts, seq, states): a recorded search on the synthetic game and its replay."""
    ts, calls = record(P, T, iterations, c_uct, C, synthetic_backend(P, T, seed, cells=cells), step_index=100)
    N = iterations + 1 if capacity is None else capacity
    seq = search_calls(calls, split)
    if capacity is not None:  # a smaller tree selects differently once it is full: nothing recorded to check against
        for c in seq:
            c["expect"] = None
    return SimpleNamespace(P=P, N=N, C=C, T=T, c_uct=c_uct, ts=ts, seq=seq, states=replay(P, N, C, T, c_uct, seq))


# ---- every group width, more than one block ------------------------------------------------------------------------
def group_lanes(C):
    """csrc/pcb_group.h:group_lanes -- the lanes per root of the kernel<G> the host picks for max_children = C (every tree step)."""
    g = 4
    while g < C:
        g <<= 1
    return g


BLOCK = 256  # threads of a k_tree_advance workgroup: 256 / G roots
# P, C, iterations, cells of synthetic(P, 5, C, iterations, cells=cells); then the G and the blocks the row is there for.
# C == G (every lane owns a child) and C == G / 2 + 1 (the most idle lanes of a width) at each width but 64, whose C == G
# case is the single root of test_tree_advance_gpu.REPLAYS["C64_P1"]; three blocks, the last partly filled, and from
# G = 16 on an odd P: the last wavefront in use is partly filled too.
WIDTHS = {
    "G4_C4_P130": (130, 4, 40, 3, 4, 3),
    "G8_C8_P70": (70, 8, 48, 6, 8, 3),
    "G16_C9_P35": (35, 9, 56, 8, 16, 3),
    "G16_C16_P35": (35, 16, 72, 12, 16, 3),
    "G32_C17_P19": (19, 17, 80, 14, 32, 3),
    "G32_C32_P19": (19, 32, 120, 24, 32, 3),
    "G64_C33_P9": (9, 33, 130, 26, 64, 3),
    "G64_C63_P9": (9, 63, 110, 100, 64, 3),  # 200 actions: a root has its 63 children after some 76 playouts
}
WIDTH_T = 5


def width_case(name):
    """synthetic() of a row of WIDTHS, after the checks that the row still exercises what it is there for: the width, the
    blocks, the partly filled tail, a descent through a full node in the first and in the last block, exact ties, no error."""
    P, C, iterations, cells, G, blocks = WIDTHS[name]
    per_block, per_wave = BLOCK // G, 64 // G
    assert group_lanes(C) == G and (C == G or C == G // 2 + 1 or (G, C) == (64, 63)), name
    assert -(-P // per_block) == blocks and P % per_block != 0, name
    assert G < 16 or P % 2 == 1 and (per_wave == 1 or P % per_wave != 0), name
    case = synthetic(P, WIDTH_T, C, iterations, cells=cells)
    first, last = slice(0, per_block), slice((blocks - 1) * per_block, P)
    assert any((s["path_len"][first] > 0).any() for s in case.states) and any((s["path_len"][last] > 0).any() for s in case.states), name
    assert case.states[-1]["errors"] == 0, name
    assert ties(case) > 0, name
    return case


# ---- trees the caller has damaged -----------------------------------------------------------------------------------
# G: P, T, C, iterations, cells of the healthy game, and the roots a scenario may damage: 0 < p < P - 1 (a check that
# failed to hold would then show in a neighbouring root's rows of the same tensor, which every comparison covers), not
# a refused root (p % 7 == 5) nor one whose children are all terminal (p % 7 == 6), and at G < 64 not at the bottom of
# its wavefront: the groups sit at lanes 16 ... 48.
DAMAGE_GAMES = {4: (9, 5, 3, 40, 3, (4, 7)), 16: (7, 5, 9, 56, 8, (1, 2, 3)), 64: (3, 5, 33, 130, 26, (1,))}
NO_ACTION = (0, 1, 0)  # the second coordinate of every action of the game is 0: no node has this one
DAMAGE = ("selected_N", "selected_minus_1", "num_nodes_0", "num_nodes_N_plus_1",
          "last_child_bad_match_below", "first_child_bad", "middle_child_bad_no_match",
          "last_child_bad_match_below_absorb_alone", "first_child_bad_absorb_alone", "middle_child_bad_no_match_absorb_alone",
          "parent_N", "parent_self", "root_its_own_child",
          "depth_minus_1", "depth_T", "depth_T_plus_3", "num_children_minus_1", "num_children_C_plus_5")
DAMAGE_CASES = ([(4, n) for n in DAMAGE] + [(16, n) for n in DAMAGE[4:] if not n.endswith("absorb_alone")] +
                [(64, n) for n in ("last_child_bad_match_below", "first_child_bad", "middle_child_bad_no_match")])


@functools.lru_cache(maxsize=None)
def damaged(G, name):
    """-> SimpleNamespace(P, N, C, T, c_uct, seq, states, base, k, p, node, ...): a healthy prefix seq[:k] of the game of
    width G, after which root p is full; call k with the pokes and, where the scenario needs a particular playout, a
    hand-written one for root p; then two more ABSORB|SELECT calls with the playouts the healthy search got.  `base` is
    the healthy search: its states are those of the roots nothing was done to.  node: the node call k's ABSORB is about."""
    P, T, C, iterations, cells, roots = DAMAGE_GAMES[G]
    base = synthetic(P, T, C, iterations, cells=cells)
    N, shp = base.N, shapes(P, base.N, C, T)
    p = roots[DAMAGE.index(name) % len(roots)]
    makes_child = name.startswith("depth_")  # the node selected by the healthy search must be able to take a child
    for k in range(1, len(base.seq) - 3):
        st = base.states[k - 1]
        node = int(st["selected"][p])
        if st["num_children"][p, 0] == C and st["num_nodes"][p] < N and all(base.seq[i]["phases"] == ABSORB | SELECT for i in range(k, k + 3)) and \
                (not makes_child or (node != 0 and not st["terminal"][p, node] and st["num_children"][p, node] < C)):
            break
    else:
        raise AssertionError(f"no call of the healthy search after which root {p} suits {name}")
    assert st["errors"] == 0
    child = [int(c) for c in st["children"][p, 0]]
    pokes, hand = [], None  # hand: reward, length, the action of row `row` of root p's playout
    poke = lambda f, value, *index: pokes.append((f, flat(shp[f], *index), int(value)))
    if name in ("selected_N", "selected_minus_1"):
        poke("selected", N if name == "selected_N" else -1, p)
    elif name in ("num_nodes_0", "num_nodes_N_plus_1"):
        poke("num_nodes", 0 if name == "num_nodes_0" else N + 1, p)
    elif "_child_bad" in name:
        c, drawn = {"l": (C - 1, child[0]), "f": (0, child[1]), "m": (C // 2, None)}[name[0]]
        node = 0
        poke("selected", 0, p)
        poke("children", N, p, 0, c)
        hand = (0.5, 1, 0, NO_ACTION if drawn is None else tuple(int(a) for a in st["node_action"][p, drawn]))
    elif name in ("parent_N", "parent_self"):
        node = child[0]  # a playout of length 1 from a node of depth 1 draws nothing: it ends in the node
        poke("selected", node, p)
        poke("parent", N if name == "parent_N" else node, p, node)
        hand = (0.5, 1, 0, NO_ACTION)
    elif name == "root_its_own_child":
        for c in range(C):
            poke("children", 0, p, 0, c)
        poke("num_children", C, p, 0)
    elif name.startswith("depth_"):
        poke("depth", {"depth_minus_1": -1, "depth_T": T, "depth_T_plus_3": T + 3}[name], p, node)
        hand = (0.5, T + 4, T - 1 if name != "depth_minus_1" else 0, NO_ACTION)  # longer than any depth: an action was drawn
    else:
        node = 0
        poke("selected", 0, p)
        poke("num_children", -1 if name == "num_children_minus_1" else C + 5, p, 0)
        hand = (0.5, 1, 0, NO_ACTION)
    playout = base.seq[k]["playout"]
    if hand is not None:
        reward, length, actions = (np.array(a, copy=True) for a in playout)
        reward[p], length[p] = hand[0], hand[1]
        actions[:, p] = (1, 0, 0)  # rows the scenario must not read: an action of the game, and not the drawn one
        actions[hand[2], p] = hand[3]
        playout = (reward, length, actions)
    alone = name.endswith("absorb_alone")
    seq = base.seq[:k] + [dict(phases=ABSORB if alone else ABSORB | SELECT, playout=playout, expect=None, pokes=pokes)] + \
        [dict(phases=ABSORB | SELECT, playout=base.seq[i]["playout"], expect=None) for i in (k + 1, k + 2)]
    return SimpleNamespace(P=P, N=N, C=C, T=T, c_uct=base.c_uct, seq=seq, states=replay(P, N, C, T, base.c_uct, seq), base=base, k=k, p=p,
                           node=node, child=child, hand=hand, name=name)


# ---- searches on real roots (the CPU oracle plays the playouts) ---------------------------------------------------
@functools.lru_cache(maxsize=None)
def oracle_case(name, iterations):
    """-> SimpleNamespace(roots, P, N, C, T, c_uct, ts, seq, states) of tree_search on path_cases.Plan(name)'s roots with
    the playouts of tests/test_tree_search_gpu.py:oracle_backend, and the model's replay of it."""
    import path_cases as pa
    import playout_cases as pc
    from test_tree_search_gpu import oracle_backend
    roots = pa.Plan(name).roots
    T = pc.max_steps(roots.cfg)
    ts, calls = record(roots.P, T, iterations, C_UCT, MAX_CHILDREN, oracle_backend(roots, T, []), step_index=STEP_INDEX, cfg=roots.cfg)
    N, seq = iterations + 1, search_calls(calls)
    return SimpleNamespace(roots=roots, P=roots.P, N=N, C=MAX_CHILDREN, T=T, c_uct=C_UCT, ts=ts, seq=seq,
                           states=replay(roots.P, N, MAX_CHILDREN, T, C_UCT, seq))
