"""Cases and the CPU model of pcbenv_puct_move (plain module, no test; needs no GPU).

A case is the final tree of a recorded search of tests/puct_cases.py -- `synthetic(...)`, or for the chain the evaluator
below -- and, per root, a move of one of eight kinds by p % 8 (KINDS).  `run` feeds a tree and a sequence of calls to
tools/puct_move_check.cpp -- csrc/pcb_puct_move.h compiled for the CPU with AddressSanitizer and UBSan, a program of its
own -- and returns the state after every call.  `ways` are the three call sequences every case is run in; `damaged` are the
trees a caller has written out-of-range values into.  The GPU tests compare the kernel with the model's states.

Shapes (SHAPES): N = 31 is less than a 64-slot chunk; N = 161 and N = 331 have a ragged last chunk at C = 16 and C = 33; C =
64 with one root has N = 641, more than ten chunks; the chain is a C = 1 tree, T = 70, 80 iterations: every parent is the
previous slot (the previous lane of the kernel) and the chain crosses a chunk boundary; P = 9, 35 and 130 are several
workgroups of four roots with the last partly filled."""
import functools
import os
import shutil
import subprocess
import tempfile
from types import SimpleNamespace

import numpy as np
import torch

import puct_cases as pc
import sampling_contract as sc
from pcbenv.search import Evaluation

REPO = pc.REPO
CHOOSE, REROOT = 1, 2
GREEDY, PROPORTIONAL = 0, 1
ERR_TREE = 2
FILL = -7  # what the model's output tensors hold before the first call
TREE_FIELDS = pc.TREE_FIELDS
MOVE_FIELDS = ("move_slot", "move_action", "child_visits", "child_actions", "root_value", "remap")
STATE_FIELDS = MOVE_FIELDS + TREE_FIELDS
FLOATS = pc.FLOATS + ("root_value",)
POKED = ("move_slot", "num_nodes", "parent", "num_children", "first_child")  # the tensors a call's pokes may name, by number
KINDS = ("most_visited", "zero_visits", "grandchild", "slot_0", "minus_1", "reset", "last_slot", "proportional")
SEED, STEP, FIRST_ROOT = 0x5EED0123456789AB, 77, 3


def shapes(P, N, C):
    s = {"move_slot": (P,), "move_action": (P, 3), "child_visits": (P, C), "child_actions": (P, C, 3), "root_value": (P,), "remap": (P, N),
         "num_nodes": (P,), "node_action": (P, N, 3), "reward_lo": (P,), "reward_hi": (P,)}
    s.update({n: (P, N) for n in ("parent", "depth", "visits", "num_children", "first_child", "prior", "value_sum", "value_max", "terminal")})
    return s


@functools.lru_cache(maxsize=None)
def program():
    """tools/puct_move_check.cpp built with the sanitizers, a program of its own; None without g++."""
    if shutil.which("g++") is None:
        return None
    exe = os.path.join(tempfile.mkdtemp(prefix="puct_move_"), "puct_move_check")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-ffp-contract=off",
                    "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-I", os.path.join(REPO, "rl-environment-for-component-placement_amd", "csrc"),
                    "-o", exe, os.path.join(REPO, "tools", "puct_move_check.cpp")], check=True)
    return exe


def _words(a, floats=False):
    a = np.ascontiguousarray(a)
    return (a.astype(np.float64).view(np.int64) if floats else a.astype(np.int64)).ravel()


def call(phases, mode=GREEDY, move_slot=None, reset=None, pokes=(), seed=SEED, step_index=STEP, first_root=FIRST_ROOT):
    return dict(phases=phases, mode=mode, move_slot=move_slot, reset=reset, pokes=tuple(pokes), seed=seed, step_index=step_index, first_root=first_root)


def run(tree, C, seq):
    """tree: dict of TREE_FIELDS (numpy).  -> [state after call i]: dicts of STATE_FIELDS (int64; FLOATS as float64) and
    `errors`, the error bits of that call.  Raises on anything on stderr."""
    P, N = tree["parent"].shape
    parts = [np.array([P, N, C, len(seq)], np.int64)] + [_words(tree[f], f in FLOATS) for f in TREE_FIELDS]
    for c in seq:
        parts.append(np.array([c["phases"], c["mode"], np.uint64(c["seed"]).astype(np.int64), c["step_index"], c["first_root"], int(c["move_slot"] is not None),
                               int(c["reset"] is not None), len(c["pokes"])] + [w for name, at, value in c["pokes"] for w in (POKED.index(name), at, value)], np.int64))
        parts += [_words(c[f]) for f in ("move_slot", "reset") if c[f] is not None]
    done = subprocess.run([program()], input=np.concatenate(parts).tobytes(), capture_output=True)
    assert done.returncode == 0 and done.stderr == b"", done.stderr.decode()
    words = np.frombuffer(done.stdout, np.int64)
    shp = shapes(P, N, C)
    per_call = 1 + sum(int(np.prod(shp[f])) for f in STATE_FIELDS)
    assert len(words) == per_call * len(seq)
    states = []
    for i in range(len(seq)):
        w = words[i * per_call:(i + 1) * per_call]
        st, at = {"errors": int(w[0])}, 1
        for f in STATE_FIELDS:
            n = int(np.prod(shp[f]))
            st[f] = (w[at:at + n].view(np.float64) if f in FLOATS else w[at:at + n]).reshape(shp[f])
            at += n
        states.append(st)
    return states


# ---- the trees -----------------------------------------------------------------------------------------------------
def chain_evaluator(P, T):
    """One candidate per node and no end before depth T: the tree of every root is a chain."""
    def evaluate(paths, path_len, step_index0):
        plen = path_len.numpy()
        value = np.array([(0.25, 0.5, 0.75)[pc._mix(5, p, plen[p]) % 3] for p in range(P)])
        actions = np.zeros((P, 1, 3), np.int32)
        actions[:, 0, 2] = plen % 7
        return Evaluation(torch.from_numpy(value), torch.from_numpy((plen == T).astype(np.uint8)), torch.ones(P, dtype=torch.int32),
                          torch.from_numpy(actions), torch.full((P, 1), 0.5, dtype=torch.float32))
    return evaluate


# name: P, T, C, K, iterations (synthetic), or "chain"
SHAPES = {
    "G4_C3_P130": (130, pc.WIDTH_T, 3, 3, 10),     # N = 31: less than a chunk; 33 workgroups, the last half filled
    "G16_C16_P35": (35, pc.WIDTH_T, 16, 16, 10),   # N = 161: ragged last chunk
    "G64_C33_P9": (9, pc.WIDTH_T, 33, 33, 10),     # N = 331
    "G64_C64_P1": (1, pc.WIDTH_T, 64, 64, 10),     # N = 641: more than ten chunks, one root
    "chain_C1_T70": (3, 70, 1, 1, 80),             # N = 81: every parent is the previous slot, across the chunk boundary at 64
}


@functools.lru_cache(maxsize=None)
def searched(name):
    """-> (the PuctSearch of the shape's recorded search, C)."""
    P, T, C, K, iterations = SHAPES[name]
    if name.startswith("chain"):
        ps, _ = pc.record(P, T, iterations, 1.25, C, chain_evaluator(P, T), step_index=100)
        return ps, C
    return pc.synthetic(P, T, C, K, iterations).ps, C


def tree_of(ps):
    return {f: getattr(ps, f).numpy().copy() for f in TREE_FIELDS}


def subtree(tree, p, m):
    """The slots of the subtree of m in root p, in slot order (a walk over the child ranges)."""
    todo, out = [m], []
    while todo:
        s = todo.pop()
        out.append(s)
        todo += [int(tree["first_child"][p, s]) + c for c in range(int(tree["num_children"][p, s]))]
    return sorted(out)


def proportional_pick(visits, seed, genv, step):
    """The contract's draw restated with tests/sampling_contract.py: the least c whose inclusive prefix sum exceeds (hi32 * total) >> 32."""
    total = int(sum(int(v) for v in visits))
    at = (sc.hi32(seed, genv, step) * total) >> 32
    prefix = 0
    for c, v in enumerate(visits):
        prefix += int(v)
        if prefix > at:
            return c
    raise AssertionError("no visits to draw from")


def greedy_pick(visits):
    return int(np.argmax(np.asarray(visits)))  # the first maximum


def assign(tree, p, C):
    """-> (kind, move_slot, reset) of root p: the kind p % 8 asks for where the tree has such a node, most_visited (or -1
    for a root without children) otherwise."""
    n, k, fc = int(tree["num_nodes"][p]), int(tree["num_children"][p, 0]), int(tree["first_child"][p, 0])
    if k == 0:
        kind = KINDS[p % 8] if KINDS[p % 8] in ("slot_0", "minus_1", "reset") else "minus_1"
        return kind, 0 if kind != "minus_1" else -1, int(kind == "reset")
    visits = tree["visits"][p, fc:fc + k]
    best = fc + greedy_pick(visits)
    kind = KINDS[p % 8]
    if kind == "zero_visits":
        zero = [s for s in range(1, n) if tree["visits"][p, s] == 0]
        if zero:
            return kind, zero[0], 0
    elif kind == "grandchild":
        if tree["num_children"][p, best] > 0:
            return kind, int(tree["first_child"][p, best]), 0
    elif kind == "slot_0":
        return kind, 0, 0
    elif kind == "minus_1":
        return kind, -1, 0
    elif kind == "reset":
        return kind, best, 1
    elif kind == "last_slot":
        return kind, n - 1, 0
    elif kind == "proportional" and visits.sum() > 0:
        return kind, fc + proportional_pick(visits, SEED, FIRST_ROOT + p, STEP), 0
    return "most_visited", best, 0


@functools.lru_cache(maxsize=None)
def case(name):
    """-> SimpleNamespace(name, P, N, C, tree, kinds, move_slot int32 [P], reset uint8 [P], kept [P]: nodes each root keeps, mode)."""
    ps, C = searched(name)
    tree = tree_of(ps)
    P, N = tree["parent"].shape
    assert N == 1 + SHAPES[name][4] * C and int(ps.errors) == 0
    kinds, move, reset = zip(*(assign(tree, p, C) for p in range(P)))
    kept = [0 if reset[p] or move[p] < 0 else len(subtree(tree, p, move[p])) for p in range(P)]
    mode = PROPORTIONAL if list(SHAPES).index(name) % 2 else GREEDY
    return SimpleNamespace(name=name, P=P, N=N, C=C, tree=tree, kinds=kinds, move_slot=np.array(move, np.int32), reset=np.array(reset, np.uint8),
                           kept=kept, mode=mode)


def check_cases():
    """What the set of cases is there for: every kind of move occurs, one root keeps more than 1 + C nodes and one exactly 1;
    the shapes are the ones the module's docstring names."""
    cases = [case(n) for n in SHAPES]
    assert {k for c in cases for k in c.kinds} == set(KINDS)
    assert any(k > 1 + c.C for c in cases for k in c.kept) and any(k == 1 for c in cases for k in c.kept)
    assert [c.N for c in cases] == [31, 161, 331, 641, 81] and [c.P for c in cases] == [130, 35, 9, 1, 3]
    chain = case("chain_C1_T70")
    n = int(chain.tree["num_nodes"][0])
    assert n > 64 and (chain.tree["parent"][0, 1:n] == np.arange(n - 1)).all()  # every parent is the previous slot, past slot 64
    assert any(k > 64 for k in chain.kept)  # and a kept chain crosses the chunk boundary
    assert {c.mode for c in cases} == {GREEDY, PROPORTIONAL}
    return cases


WAYS = ("one_launch", "two_launches", "given_move")


def ways(c, reset=True):
    """The three call sequences of a case, each from the case's tree: CHOOSE | REROOT in one call, CHOOSE and REROOT in two,
    REROOT alone with the caller's move_slot."""
    r = c.reset if reset else None
    return {"one_launch": [call(CHOOSE | REROOT, c.mode, reset=r)],
            "two_launches": [call(CHOOSE, c.mode), call(REROOT, reset=r)],
            "given_move": [call(REROOT, move_slot=c.move_slot, reset=r)]}


@functools.lru_cache(maxsize=None)
def modelled(name, way, reset=True):
    c = case(name)
    return run(c.tree, c.C, ways(c, reset)[way])


# ---- trees the caller has damaged -----------------------------------------------------------------------------------
DAMAGE_SHAPE = "G16_C16_P35"
DAMAGE = ("num_nodes_0", "num_nodes_N_plus_1", "move_slot_N", "move_slot_minus_2", "parent_self", "parent_N", "num_children_minus_1",
          "num_children_C_plus_5", "first_child_0", "first_child_n", "child_range_not_kept")


def flat(shape, *index):
    return int(np.ravel_multi_index(index, shape))


@functools.lru_cache(maxsize=None)
def damaged(name):
    """-> SimpleNamespace(case, p, m, seq, states, healthy): REROOT alone with the caller's moves, root p (with neighbours on
    both sides) moving to its most-visited child m, which has at least two children of its own, after the pokes of `name`;
    `healthy` is the same call without them."""
    c = case(DAMAGE_SHAPE)
    t, shp = c.tree, shapes(c.P, c.N, c.C)
    for p in range(1, c.P - 1):
        k, fc = int(t["num_children"][p, 0]), int(t["first_child"][p, 0])
        if k:
            m = fc + greedy_pick(t["visits"][p, fc:fc + k])
            if m != 1 and t["num_children"][p, m] >= 2:
                break
    else:
        raise AssertionError("no root suits")
    n = int(t["num_nodes"][p])
    move = c.move_slot.copy()
    move[p] = m
    reset = c.reset.copy()
    reset[p] = 0
    last_kept = subtree(t, p, m)[-1]
    poke = {"num_nodes_0": ("num_nodes", 0, p), "num_nodes_N_plus_1": ("num_nodes", c.N + 1, p), "move_slot_N": ("move_slot", c.N, p),
            "move_slot_minus_2": ("move_slot", -2, p), "parent_self": ("parent", n - 1, p, n - 1), "parent_N": ("parent", c.N, p, 2),
            "num_children_minus_1": ("num_children", -1, p, last_kept), "num_children_C_plus_5": ("num_children", c.C + 5, p, m),
            "first_child_0": ("first_child", 0, p, m), "first_child_n": ("first_child", n, p, m),
            "child_range_not_kept": ("first_child", 1, p, m)}[name]  # the root's own children: m's siblings are not kept
    f, value, *index = poke
    if f == "move_slot":  # the caller's move_slot is written after the pokes: an out-of-range move goes into that tensor itself
        move[p] = value
        pokes = ()
    else:
        pokes = ((f, flat(shp[f], *index), int(value)),)
    seq = [call(REROOT, move_slot=move, reset=reset, pokes=pokes)]
    healthy = run(t, c.C, [call(REROOT, move_slot=np.where(np.arange(c.P) == p, m, move).astype(np.int32), reset=reset)])
    return SimpleNamespace(case=c, p=p, m=m, n=n, seq=seq, pokes=pokes, move_slot=move, reset=reset, states=run(t, c.C, seq), healthy=healthy)
