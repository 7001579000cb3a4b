"""A searched game, call by call: cases and the CPU model (plain module, no test; needs no GPU).

A game is J = 3 moves of M iterations on ONE tree that is kept from move to move -- the loop of pcbenv/search.py:
puct_selfplay.  The specification records it on the CPU: per move `puct_search(tree=)` with a recording evaluator
(tests/puct_cases.py:synthetic_evaluator, a seed per move), `puct_choose` (greedy, proportional, greedy), a synthetic `done`
from a hash of (root, move) -- no environment -- and `puct_reroot(reset=done)`.  `calls` turns the recording into the
sequence of pcbenv_puct_advance and pcbenv_puct_move calls that puct_selfplay makes (INIT | SELECT, or SELECT alone on a
kept tree; ABSORB | SELECT per evaluation, ABSORB alone for the last; CHOOSE; REROOT with reset), and `run` feeds it to
tools/puct_game_check.cpp -- csrc/pcb_puct.h and csrc/pcb_puct_move.h compiled for the CPU with AddressSanitizer and UBSan,
a program of its own -- which checks every selection against the recorded one and returns the state after every call.
The GPU test compares the kernels with those states.

The draws are keyed by first_root + p with first_root = 3 (the handle of the GPU test has first_env_index = 3).

GAMES: one per group width of k_puct_advance that tests/puct_cases.py:damaged knows (G = 4, 16, 64), P and C from the matching
rows of puct_cases.WIDTHS, T = 5; and a C = 1 chain, T = 70, whose kept tree passes slot 64.  The capacity is chosen so that
the tree fills: see `check_game` for what each game has to reach."""
import functools
from types import SimpleNamespace

import numpy as np
import torch

import model_harness as mh
import puct_cases as pc
import puct_move_cases as mc
from pcbenv.search import puct_choose, puct_reroot, search_tree

REPO = pc.REPO
ADVANCE, MOVE = 0, 1
J = 3
SEED, STEP, FIRST_ROOT = mc.SEED, 500, 3
C_PUCT = 1.25
MOVE_FIELDS = mc.MOVE_FIELDS
STATE_FIELDS = ("selected", "path_len", "paths") + MOVE_FIELDS + pc.TREE_FIELDS
FLOATS = mc.FLOATS

# name: the row of puct_cases.WIDTHS (or None), P, T, C, K, M iterations per move, N the capacity
# The capacity starts at 1 + M * C.  There no root of the G = 4 and G = 64 games is refused children, keeps a tree and grows it
# again (check_game's third assertion), so theirs is 1 + 8 * C.  The chain game -- recorded in under three seconds, so it is
# in -- ends every chain at depth T: its capacity is what fills it, at the slot behind the first chunk.
GAMES = {
    "G4": ("G4_C3_P130", 130, 5, 3, 3, 12, 1 + 8 * 3),
    "G16": ("G16_C16_P35", 35, 5, 16, 16, 10, 1 + 10 * 16),
    "G64": ("G64_C33_P9", 9, 5, 33, 33, 10, 1 + 8 * 33),
    "chain": (None, 3, 70, 1, 1, 70, 66),
}


def shapes(P, N, C, T):
    return dict(pc.shapes(P, N, T), **mc.shapes(P, N, C))


def program():
    """tools/puct_game_check.cpp as tests/model_harness.py:tool builds it; None without g++."""
    return mh.tool("puct_game_check")


def done_of(P, j):
    """The synthetic `done` of move j: a hash of (root, move)."""
    return np.array([pc._mix(0xD09E, p, j) % 3 == 0 for p in range(P)], np.uint8)


def evaluator(name, P, T, K, j):
    return mc.chain_evaluator(P, T) if name.startswith("chain") else pc.synthetic_evaluator(P, T, K, 11 + j)


@functools.lru_cache(maxsize=None)
def recorded(name):
    """The game as the specification plays it -> SimpleNamespace(P, N, C, T, K, M, moves): per move the search's result `ps`,
    the evaluator's `calls`, `mode`, puct_choose's `chosen`, `done`, and puct_reroot's `tree` and `remap`."""
    _, P, T, C, K, M, N = GAMES[name]
    tree, moves = None, []
    for j in range(J):
        ps, calls = pc.record(P, T, M, C_PUCT, C, evaluator(name, P, T, K, j), step_index=STEP + j * M * T, capacity=N, tree=tree)
        mode = mc.PROPORTIONAL if j % 2 else mc.GREEDY
        chosen = puct_choose(search_tree(ps), C, mode, SEED, STEP + j, FIRST_ROOT)
        done = done_of(P, j)
        tree, remap = puct_reroot(search_tree(ps), chosen["move_slot"], torch.from_numpy(done))
        moves.append(SimpleNamespace(ps=ps, calls=calls, mode=mode, chosen=chosen, done=done, tree=tree, remap=remap))
    return SimpleNamespace(name=name, P=P, N=N, C=C, T=T, K=K, M=M, c_puct=C_PUCT, moves=moves)


def calls(game):
    """The calls of the game as puct_selfplay makes them: dicts with kind, phases, move (the move they belong to) and, by kind,
    evaluation / expect, or mode / step_index / reset."""
    seq = []
    for j, mv in enumerate(game.moves):
        for m in range(len(mv.calls) + 1):
            chosen = None if m == len(mv.calls) else mv.calls[m][:2]
            first = (pc.INIT if j == 0 else 0) if m == 0 else pc.ABSORB
            seq.append(dict(kind=ADVANCE, move=j, phases=first | (pc.SELECT if chosen is not None else 0), evaluation=None if m == 0 else mv.calls[m - 1][2:],
                            expect=chosen))
        seq.append(dict(kind=MOVE, move=j, phases=mc.CHOOSE, mode=mv.mode, seed=SEED, step_index=STEP + j, first_root=FIRST_ROOT, reset=None))
        seq.append(dict(kind=MOVE, move=j, phases=mc.REROOT, mode=mv.mode, seed=SEED, step_index=STEP + j, first_root=FIRST_ROOT, reset=mv.done))
    return seq


def run(P, N, C, T, K, c_puct, seq):
    """-> [state after call i]: dicts of STATE_FIELDS (int64; FLOATS as float64) and `errors`, the error bits of that call.
    Raises if the program reports a selection that differs from the recorded one, or anything on stderr."""
    w = mh.words
    parts = [np.array([P, N, C, T, K, len(seq), mh.bits(c_puct)], np.int64)]
    for c in seq:
        if c["kind"] == ADVANCE:
            parts.append(np.array([ADVANCE, c["phases"], int(c["expect"] is not None)], np.int64))
            if c["phases"] & pc.ABSORB:
                value, over, count, actions, prior = c["evaluation"]
                assert actions.shape == (P, K, 3) and prior.shape == (P, K) and prior.dtype == np.float32
                parts += [w(value, True), w(over), w(count), w(actions), mh.float32_words(prior)]
            if c["expect"] is not None:
                parts += [w(c["expect"][1]), w(c["expect"][0])]
        else:
            parts.append(np.array([MOVE, c["phases"], c["mode"], mh.u64(c["seed"]), c["step_index"], c["first_root"],
                                   int(c["reset"] is not None)], np.int64))
            if c["reset"] is not None:
                parts.append(w(c["reset"]))
    return mh.cut(mh.run_words(program(), parts), len(seq), STATE_FIELDS, shapes(P, N, C, T), FLOATS)


@functools.lru_cache(maxsize=None)
def modelled(name):
    """-> SimpleNamespace(game, seq, states): the game, its calls, and the model's state after every one."""
    g = recorded(name)
    seq = calls(g)
    return SimpleNamespace(game=g, seq=seq, states=run(g.P, g.N, g.C, g.T, g.K, g.c_puct, seq))


# ---- what a game has to reach ---------------------------------------------------------------------------------------
def refused(game, seq, states, i):
    """The roots whose expansion call i (with ABSORB) refuses for want of slots: csrc/pcb_puct.h:puct_absorb, from the state before."""
    before, (value, over, count, _, _) = states[i - 1], seq[i]["evaluation"]
    out = []
    for p in range(game.P):
        node, n = int(before["selected"][p]), int(before["num_nodes"][p])
        k = pc.kept(int(count[p]), game.K, game.C)
        if not over[p] and before["num_children"][p, node] == 0 and not before["terminal"][p, node] and k > 0 and n + k > game.N:
            out.append(p)
    return out


def kept_roots(state):
    """After a REROOT: the roots that kept a tree with visits."""
    return [p for p in range(state["visits"].shape[0]) if state["visits"][p, 0] > 0]


def _only(state, roots):
    return {f: (v if f in ("paths", "errors") else np.take(v, roots, 0)) for f, v in state.items()}


def check_game(name):
    """What a game is there for, asserted on the CPU from the model's states and the recording.  -> the counts, for profiles/."""
    m = modelled(name)
    g, seq, states = m.game, m.seq, m.states
    P, C = g.P, g.C
    G = pc.group_lanes(C)
    per_wave = 64 // G
    row = GAMES[name][0]
    if row is not None:
        assert pc.WIDTHS[row][:2] == (P, C) and pc.WIDTHS[row][4] == G
        assert G == 64 or (-(-P // (pc.BLOCK // G)) > 1 and P % (pc.BLOCK // G) != 0)  # more than one workgroup, the last partly filled
    reroots = [i for i, c in enumerate(seq) if c["kind"] == MOVE and c["phases"] & mc.REROOT]
    assert len(reroots) == J and all(seq[i + 1]["phases"] == pc.SELECT for i in reroots[:-1])
    out = SimpleNamespace(name=name, P=P, N=g.N, C=C, T=g.T, M=g.M, calls=len(seq), deep_first_selects=0, deepest_first_select=0, shared_waves=0,
                          refused_roots=set(), regrown=[], ties_on_kept=0, modes=sorted({mv.mode for mv in g.moves}), first_root_matters=0,
                          kept_nodes=[], resets=[], errors=[])
    # 1. the first SELECT after a REROOT descends two or more levels, through kept nodes: nothing else is in the tree yet
    for i in reroots[:-1]:
        kept = kept_roots(states[i])
        deep = [p for p in kept if states[i + 1]["path_len"][p] >= 2]
        assert all(states[i + 1]["selected"][p] < states[i]["num_nodes"][p] for p in deep)
        out.deep_first_selects += len(deep)
        out.deepest_first_select = max([out.deepest_first_select] + [int(states[i + 1]["path_len"][p]) for p in kept])
    assert out.deep_first_selects > 0, name
    # 2. a reset root and a kept root in one wavefront
    for i in reroots:
        kept = set(kept_roots(states[i]))
        gone = {p for p in range(P) if p not in kept and (seq[i]["reset"][p] or states[i]["move_slot"][p] < 0)}
        out.shared_waves += len({p // per_wave for p in kept} & {p // per_wave for p in gone})
        out.kept_nodes.append(int(sum(states[i]["num_nodes"][p] for p in kept)))
        out.resets.append(len(gone))
    assert out.shared_waves > 0 or per_wave == 1, name
    # 3. a root is refused children (ERR_FULL), is compacted, and later expands into slots REROOT gave up
    for j, r in enumerate(reroots[:-1]):
        first = reroots[j - 1] + 1 if j else 0
        full = {p for i in range(first, r) if seq[i]["kind"] == ADVANCE and seq[i]["phases"] & pc.ABSORB for p in refused(g, seq, states, i)}
        assert all(states[i]["errors"] & pc.ERR_FULL for i in range(first, r) if seq[i]["kind"] == ADVANCE and seq[i]["phases"] & pc.ABSORB and refused(g, seq, states, i))
        out.refused_roots |= {(j, p) for p in full}
        for p in sorted(full):
            n_before, count = int(states[r - 1]["num_nodes"][p]), int(states[r]["num_nodes"][p])
            if p not in kept_roots(states[r]) or not 1 < count < n_before:
                continue  # reset, or nothing given up
            for i in range(r + 1, reroots[j + 1]):
                grew = range(int(states[i - 1]["num_nodes"][p]), int(states[i]["num_nodes"][p]))
                if len(grew) and grew[0] < n_before:
                    out.regrown.append((j, p, count, n_before, grew[0]))
                    break
    assert out.regrown, name
    # 4. exact ties at a selection in a kept tree
    for i, c in enumerate(seq):
        if c["kind"] == ADVANCE and c["phases"] & pc.SELECT and c["move"] > 0:
            kept = kept_roots(states[reroots[c["move"] - 1]])
            out.ties_on_kept += pc.exact_ties(_only(states[i], kept), g.c_puct, g.T)
    assert out.ties_on_kept > 0 or C == 1, name  # a node with one child has no tie
    # 5. both modes; and first_root = 3 draws what first_root = 0 would not have
    assert out.modes == [mc.GREEDY, mc.PROPORTIONAL]
    for j, mv in enumerate(g.moves):
        if mv.mode != mc.PROPORTIONAL:
            continue
        for p in range(P):
            k, fc = int(mv.ps.num_children[p, 0]), int(mv.ps.first_child[p, 0])
            visits = mv.ps.visits[p, fc:fc + k].numpy()
            if k and visits.sum() > 0:
                mine, theirs = (mc.proportional_pick(visits, SEED, first + p, STEP + j) for first in (FIRST_ROOT, 0))
                assert int(mv.chosen["move_slot"][p]) == fc + mine
                out.first_root_matters += mine != theirs
    assert out.first_root_matters > 0 or C == 1, name
    out.errors = sorted({s["errors"] for s in states})
    return out


def report(name):
    v = check_game(name)
    return [f"{name}: P {v.P} N {v.N} C {v.C} T {v.T} M {v.M}, {v.calls} calls; first SELECTs after a REROOT two or more levels deep {v.deep_first_selects} "
            f"(deepest {v.deepest_first_select}); wavefronts with a reset and a kept root {v.shared_waves}; (move, root) refused children {len(v.refused_roots)}, "
            f"of them compacted and grown again into slots given up {len(v.regrown)}; exact ties in kept trees {v.ties_on_kept}; modes {v.modes}; "
            f"proportional picks that first_root = 0 would have drawn otherwise {v.first_root_matters}; nodes kept per move {v.kept_nodes}, roots emptied {v.resets}; "
            f"error words {v.errors}"]
