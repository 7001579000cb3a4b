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
one, each a single IEEE operation -- and returns the distances between the best and the second-best score."""
import functools
import math
import os
import shutil
import struct
import subprocess
import tempfile
from types import SimpleNamespace

import numpy as np
import torch

from pcbenv.batched_env import Playout
from pcbenv.search import ln_table, tree_search

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INIT, ABSORB, SELECT = 1, 2, 4
FILL = -7  # what the model's int32 tensors hold before the first call
TREE_FIELDS = ("num_nodes", "parent", "depth", "visits", "num_children", "node_action", "children", "value_sum", "value_max", "terminal",
               "reward_lo", "reward_hi", "best_reward", "best_length", "best_actions")
STATE_FIELDS = ("selected", "path_len", "paths") + TREE_FIELDS
FLOATS = ("value_sum", "value_max", "reward_lo", "reward_hi", "best_reward")
ITERATIONS, STEP_INDEX, C_UCT, MAX_CHILDREN = 24, 5000, 0.7, 3          # of the searches on real roots (tests/test_tree_search_gpu.py's)
ORACLE_CASES = (("small_pin", ITERATIONS), ("c3_centroid", ITERATIONS), ("spatial_7x100_t256", 12))
GAP_BOUND = 1e-12  # a last-bit difference between two implementations of log moves a score by some 1e-16


def shapes(P, N, C, T):
    s = {"selected": (P,), "path_len": (P,), "paths": (T, P, 3), "num_nodes": (P,), "node_action": (P, N, 3), "children": (P, N, C),
         "reward_lo": (P,), "reward_hi": (P,), "best_reward": (P,), "best_length": (P,), "best_actions": (T, P, 3)}
    s.update({n: (P, N) for n in ("parent", "depth", "visits", "num_children", "value_sum", "value_max", "terminal")})
    return s


@functools.lru_cache(maxsize=None)
def program():
    """tools/tree_model_check.cpp built as tests/test_kernel_models.py builds its tool; None without g++."""
    if shutil.which("g++") is None:
        return None
    exe = os.path.join(tempfile.mkdtemp(prefix="tree_model_"), "tree_model_check")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-ffp-contract=off",
                    "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-I", os.path.join(REPO, "rl-environment-for-component-placement_amd", "csrc"),
                    "-o", exe, os.path.join(REPO, "tools", "tree_model_check.cpp")], check=True)
    return exe


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


def _words(a, floats=False):
    a = np.ascontiguousarray(a)
    return (a.astype(np.float64).view(np.int64) if floats else a.astype(np.int64)).ravel()


def replay(P, N, C, T, c_uct, seq):
    """-> [state after call i]: dicts of STATE_FIELDS (int64; FLOATS as float64) and `errors`.  Raises if the program
    reports a selection that differs from the recorded one, or anything on stderr."""
    parts = [np.array([P, N, C, T, len(seq), struct.unpack("<q", struct.pack("<d", float(c_uct)))[0]], np.int64), _words(ln_table(N).numpy(), True)]
    for c in seq:
        parts.append(np.array([c["phases"], int(c["expect"] is not None)], np.int64))
        if c["phases"] & ABSORB:
            r, L, a = c["playout"]
            parts += [_words(r, True), _words(L), _words(a)]
        if c["expect"] is not None:
            parts += [_words(c["expect"][1]), _words(c["expect"][0])]
    run = subprocess.run([program()], input=np.concatenate(parts).tobytes(), capture_output=True)
    assert run.returncode == 0 and run.stderr == b"", run.stderr.decode()
    words = np.frombuffer(run.stdout, np.int64)
    shp = shapes(P, N, C, T)
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


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


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
