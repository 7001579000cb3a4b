"""Cases, recordings and the CPU model of pcbenv_frontier_advance (plain module, no test; needs no GPU).

The specification is pcbenv/search.py:frontier_advance.  `record` runs a search on it on the CPU -- INIT, then per depth
an evaluation and ADVANCE with the sets swapped -- and writes the calls down; `replay` feeds such a sequence to
tools/frontier_check.cpp -- csrc/pcb_frontier.h compiled for the CPU with AddressSanitizer and UBSan, a program of its own
-- which returns every tensor after every call; `specify` runs the same sequence through the specification from the same
sentinel-filled tensors.  The GPU tests compare the kernel with the model's states.

The evaluators are tests/puct_cases.py's `synthetic_evaluator` and `real_evaluator` at P * F rows (the "root" of their
hash is the row), and `poisoned` puts what an evaluator should never give on top of one: NaN, +-inf and +-0.0 values, counts
below 0 and above K, priors that are 0, denormal, negative, inf, NaN and above 1.  A call may also bring a frontier made by
hand (`load`): `hand_made` is a table of such calls, one per arm of the rule a search does not reach by itself.

`facts` walks the ADVANCE calls of a case again in plain Python and counts the arms of the rule they reach; `assert_reach`
holds the table of cases to every arm, so that a test that compares two implementations on it cannot be vacuous."""
import functools
import math
import struct
from types import SimpleNamespace

import numpy as np
import torch

import model_harness as mh
import puct_cases as pc
from model_harness import same_bits  # noqa: F401  (the tests take it from here)
from pcbenv import search
from pcbenv.search import Evaluation

INIT, ADVANCE, LOADED = 1, 2, 8
ERR_ROW = 2
FILL, FILL_F = -7, -7.5  # what the model's int32 and float64 tensors hold before the first call
STATE_FIELDS = ("paths_0", "path_len_0", "cum_logp_0", "paths_1", "path_len_1", "cum_logp_1", "parent_row", "live", "best_value", "best_len", "best_path")
FLOATS = ("cum_logp_0", "cum_logp_1", "best_value")
ROOTS_PER_BLOCK = 4  # csrc/pcb_frontier.hip: one wavefront per root, 256 threads per workgroup


def shapes(P, W, K, T):
    R = P * W * K
    s = {"parent_row": (R,), "live": (P,), "best_value": (P,), "best_len": (P,), "best_path": (T, P, 3)}
    for i in (0, 1):
        s.update({f"paths_{i}": (T, R, 3), f"path_len_{i}": (R,), f"cum_logp_{i}": (R,)})
    return s


def program():
    """tools/frontier_check.cpp as tests/model_harness.py:tool builds it; None without g++."""
    return mh.tool("frontier_check")


def new_state(P, W, K, T, device="cpu"):
    """The tensors of `search.new_frontier_tensors`, sentinel-filled as the model's are before its first call."""
    ft = search.new_frontier_tensors(P, W, K, T, device)
    for n, t in ft.items():
        if n != "errors_dev":
            t.fill_(FILL_F if t.dtype == torch.float64 else FILL)
    return ft


def _numpy_evaluation(ev):
    return (ev.value.to(torch.float64).numpy().copy(), ev.terminal.to(torch.uint8).numpy().copy(), ev.cand_count.to(torch.int32).numpy().copy(),
            ev.cand_actions.to(torch.int32).numpy().copy(), ev.cand_prior.to(torch.float32).numpy().copy())


def _torch_evaluation(e, device="cpu"):
    return Evaluation(*(torch.from_numpy(np.ascontiguousarray(a)).to(device) for a in e))


def apply_load(ft, load, swap):
    """A hand-made frontier into the in set of a call and into the accumulators."""
    s = 1 if swap else 0
    for n, t in ((f"path_len_{s}", load["path_len"]), (f"cum_logp_{s}", load["cum_logp"]), (f"paths_{s}", load["paths"]), ("best_value", load["best_value"]),
                 ("best_len", load["best_len"])):
        ft[n].copy_(torch.from_numpy(np.ascontiguousarray(t)).to(ft[n].dtype))


def dump(ft):
    """A state of the specification in the form of the model's: int64, FLOATS as float64, and the error word."""
    st = {"errors": int(ft["errors_dev"][0])}
    for f in STATE_FIELDS:
        t = ft[f].cpu()
        st[f] = t.numpy().copy() if f in FLOATS else t.to(torch.int64).numpy()
    return st


def record(P, W, K, T, prior_weight, evaluate, depth=None, step_index=100):
    """A search on the specification -> the sequence of its calls: dicts of phases, swap, evaluation (numpy) and load."""
    ft = new_state(P, W, K, T)
    seq = [dict(phases=INIT, swap=1, evaluation=None, load=None)]
    search.frontier_advance(ft, INIT, W, K, prior_weight, swap=True)
    for d in range(T + 1 if depth is None else depth):
        cur = d % 2
        ev = evaluate(ft[f"paths_{cur}"].clone(), ft[f"path_len_{cur}"].clone(), step_index + d * T)
        seq.append(dict(phases=ADVANCE, swap=cur, evaluation=_numpy_evaluation(ev), load=None))
        search.frontier_advance(ft, ADVANCE, W, K, prior_weight, ev, swap=cur == 1)
    return seq


def specify(P, W, K, T, prior_weight, seq, device="cpu"):
    """The sequence through pcbenv/search.py:frontier_advance from sentinel-filled tensors -> [state after call i]."""
    ft = new_state(P, W, K, T, device)
    states = []
    for c in seq:
        if c["load"] is not None:
            apply_load(ft, c["load"], c["swap"])
        ev = None if c["evaluation"] is None else _torch_evaluation(c["evaluation"], device)
        search.frontier_advance(ft, c["phases"], W, K, prior_weight, ev, swap=bool(c["swap"]))
        states.append(dump(ft))
    return states


def replay(P, W, K, T, prior_weight, seq):
    """The sequence through tools/frontier_check.cpp -> [state after call i]: dicts of STATE_FIELDS (int64; FLOATS as float64)
    and `errors`.  Raises on anything on stderr."""
    parts = [np.array([P, W, K, T, len(seq), mh.bits(prior_weight)], np.int64)]
    R = P * W * K
    for c in seq:
        parts.append(np.array([c["phases"] | (LOADED if c["load"] is not None else 0), int(c["swap"])], np.int64))
        if c["load"] is not None:
            ld = c["load"]
            assert ld["path_len"].shape == (R,) and ld["cum_logp"].shape == (R,) and ld["paths"].shape == (T, R, 3)
            parts += [mh.words(ld["path_len"]), mh.words(ld["cum_logp"], True), mh.words(ld["paths"]), mh.words(ld["best_value"], True), mh.words(ld["best_len"])]
        if c["phases"] == ADVANCE:
            value, over, count, actions, prior = c["evaluation"]
            assert actions.shape == (R, K, 3) and prior.shape == (R, K) and prior.dtype == np.float32
            parts += [mh.words(value, True), mh.words(over), mh.words(count), mh.words(actions), mh.float32_words(prior)]
    return mh.cut(mh.run_words(program(), parts), len(seq), STATE_FIELDS, shapes(P, W, K, T), FLOATS)


# ---- what an evaluator should never give ------------------------------------------------------------------------------
BAD_PRIORS = (0.0, 1e-40, -0.25, float("inf"), float("nan"), 1.5)


def poisoned(evaluate, K, seed):
    """`evaluate` with, by a hash of (row, step index): one row in 16 each with a value NaN, +inf, -inf, -0.0, +0.0 and a
    count of -3 and of K + 5; and in three rows of four one prior replaced by one of BAD_PRIORS."""
    def poisoning(paths, path_len, s):
        value, over, count, actions, prior = _numpy_evaluation(evaluate(paths, path_len, s))
        for r in range(value.shape[0]):
            h = pc._mix(seed, r, s)
            m = h % 16
            if m < 5:
                value[r] = (float("nan"), float("inf"), float("-inf"), -0.0, 0.0)[m]
            elif m < 7:
                count[r] = -3 if m == 5 else K + 5
            g = (h >> 8) % 8
            if g < len(BAD_PRIORS):
                prior[r, (h >> 16) % K] = np.float32(BAD_PRIORS[g])
        return _torch_evaluation((value, over, count, actions, prior))
    return poisoning


# ---- frontiers made by hand ------------------------------------------------------------------------------------------
def blank(P, W, K, T):
    """A call with an empty frontier (no row, best_len -1) and an evaluation of zeros, to be filled in by `put_row`."""
    R = P * W * K
    load = dict(path_len=np.full(R, -1, np.int32), cum_logp=np.zeros(R), paths=np.zeros((T, R, 3), np.int32), best_value=np.full(P, -np.inf),
                best_len=np.full(P, -1, np.int32))
    ev = (np.zeros(R), np.zeros(R, np.uint8), np.zeros(R, np.int32), np.zeros((R, K, 3), np.int32), np.zeros((R, K), np.float32))
    return dict(phases=ADVANCE, swap=0, evaluation=ev, load=load)


def put_row(call, r, length, value, terminal=0, count=0, cum_logp=0.0, priors=None, tag=0):
    """Row r of a `blank` call: its path is (tag, d, r) at step d, candidate c is the action (tag, 100 + c, r)."""
    ld, (v, over, cnt, actions, prior) = call["load"], call["evaluation"]
    T, K = ld["paths"].shape[0], prior.shape[1]
    ld["path_len"][r], ld["cum_logp"][r] = length, cum_logp
    for d in range(max(0, min(length, T))):
        ld["paths"][d, r] = (tag, d, r)
    v[r], over[r], cnt[r] = value, terminal, count
    for c in range(K):
        actions[r, c] = (tag, 100 + c, r)
        prior[r, c] = np.float32(0.5 if priors is None else priors[c % len(priors)])


HAND_P, HAND_W, HAND_K, HAND_T = 3, 2, 3, 4


def hand_made(prior_weight):
    """Calls on frontiers made by hand, P = 3, W = 2, K = 3 (F = 6), T = 4: one per arm of the rule.  Root 1 is the one
    things are done to; roots 0 and 2 hold an ordinary row each, so that a stray write would show."""
    P, W, K, T = HAND_P, HAND_W, HAND_K, HAND_T
    F = W * K
    nan, inf = float("nan"), float("inf")
    calls = []

    def call(rows, best=None):
        c = blank(P, W, K, T)
        put_row(c, 0 * F + 1, 1, 0.5, count=2, tag=1)
        put_row(c, 2 * F + 4, 2, 0.25, count=K, tag=1)
        for i, kw in rows.items():
            put_row(c, F + i, **kw)
        if best is not None:
            c["load"]["best_value"][1], c["load"]["best_len"][1] = best
        calls.append(c)
    # exact ties: -0.0 in slot 1 against +0.0 in slot 4 (the lower slot goes first); then three rows at 0.5, of which the cut takes the two lower slots
    call({1: dict(length=2, value=-0.0, count=3), 4: dict(length=2, value=0.0, count=3), 0: dict(length=1, value=-1.0, count=3)})
    call({2: dict(length=2, value=0.5, count=1), 5: dict(length=3, value=0.5, count=2), 3: dict(length=1, value=0.5, count=3)})
    # NaN and +-inf values among the expandable rows: +inf first, then the finite one; NaN and -inf tie at the bottom
    call({0: dict(length=1, value=nan, count=3), 1: dict(length=1, value=-inf, count=3), 2: dict(length=1, value=inf, count=3), 3: dict(length=1, value=0.0, count=3)})
    call({0: dict(length=1, value=nan, count=2), 1: dict(length=1, value=-inf, count=3)})
    # a NaN final: it is the best while there is none, and no later NaN or -inf replaces it
    call({0: dict(length=2, value=nan, terminal=1), 1: dict(length=3, value=-inf, terminal=1), 2: dict(length=1, value=nan, terminal=7)})
    # fewer expandable rows than W; zero expandable rows (a final, a row at T, a row without candidates)
    call({3: dict(length=2, value=0.75, count=3)})
    call({0: dict(length=2, value=0.75, terminal=1), 1: dict(length=T, value=0.9, count=3), 2: dict(length=1, value=0.9, count=0)})
    # rows at length T: one final, one not (dropped); counts below 0 and above K
    call({0: dict(length=T, value=0.75, terminal=1), 1: dict(length=T, value=0.8, count=3), 2: dict(length=T - 1, value=0.1, count=-3), 3: dict(length=T - 1, value=0.2, count=K + 5)})
    # priors: 0, denormal, negative | inf, NaN, above 1
    call({0: dict(length=1, value=0.5, count=3, cum_logp=-1.5, priors=(0.0, 1e-40, -0.25)), 1: dict(length=1, value=0.5, count=3, cum_logp=-0.5, priors=(inf, nan, 1.5))})
    # a path_len out of range on either side (bit 1), next to a healthy row
    call({0: dict(length=T + 1, value=0.9, count=3), 1: dict(length=-2, value=0.9, count=3), 2: dict(length=1, value=0.1, count=2)})
    # a later final that is better, one that is equal, one that is worse than the best so far
    call({0: dict(length=2, value=0.5, terminal=1), 1: dict(length=3, value=0.75, terminal=1), 2: dict(length=1, value=0.75, terminal=1)}, best=(0.25, 4))
    call({0: dict(length=2, value=0.25, terminal=1), 1: dict(length=1, value=0.125, terminal=1)}, best=(0.25, 4))
    # cum_logp decides with a prior weight: -inf in it, and a weight of 0 does not read it
    call({0: dict(length=1, value=0.5, count=1, cum_logp=-inf), 1: dict(length=1, value=0.25, count=1, cum_logp=-0.125), 2: dict(length=1, value=0.5, count=1, cum_logp=-2.0)})
    return calls


# ---- the table of cases ----------------------------------------------------------------------------------------------
# name: P, W, K, T, prior_weight, the evaluator, its seed, depths (None: T + 1).  What each row is there for is in
# tests/test_frontier_gpu.py; P = 6 fills one workgroup of four roots, starts a second and leaves it half filled.
CASES = {
    "W1_K1": (6, 1, 1, 5, 0.0, "synthetic", 11, None),
    "W3_K5": (6, 3, 5, 5, 0.5, "poisoned", 12, None),
    "W4_K16": (6, 4, 16, 5, 0.0, "real", 13, None),
    "W5_K13": (6, 5, 13, 5, 1.0, "poisoned", 14, None),
    "W16_K64": (6, 16, 64, 5, 0.0, "poisoned", 15, 3),
    "W64_K16": (1, 64, 16, 5, 0.25, "synthetic", 16, 4),
    "T1": (6, 3, 5, 1, 0.0, "poisoned", 17, None),
    "P1": (1, 3, 5, 5, -0.75, "poisoned", 18, None),
    "P23": (23, 2, 3, 4, 0.0, "poisoned", 19, None),
    "hand_0": (HAND_P, HAND_W, HAND_K, HAND_T, 0.0, "hand", 0, 0),
    "hand_1": (HAND_P, HAND_W, HAND_K, HAND_T, 1.0, "hand", 0, 0),
}
SMALL = tuple(n for n in CASES if CASES[n][1] * CASES[n][2] <= 65)


def evaluator(kind, rows, T, K, seed):
    base = (pc.real_evaluator if kind == "real" else pc.synthetic_evaluator)(rows, T, K, seed)
    return poisoned(base, K, seed) if kind == "poisoned" else base


@functools.lru_cache(maxsize=None)
def case(name):
    """-> SimpleNamespace(name, P, W, K, T, prior_weight, seq, states): a sequence of calls and the model's state after each."""
    P, W, K, T, pw, kind, seed, depth = CASES[name]
    if kind == "hand":
        seq = [dict(phases=INIT, swap=1, evaluation=None, load=None)] + hand_made(pw)
    else:
        seq = record(P, W, K, T, pw, evaluator(kind, P * W * K, T, K, seed), depth)
    return SimpleNamespace(name=name, P=P, W=W, K=K, T=T, prior_weight=pw, seq=seq, states=replay(P, W, K, T, pw, seq))


# ---- the arms of the rule a case reaches ------------------------------------------------------------------------------
def _f32_bits(x):
    return struct.unpack("<I", struct.pack("<f", float(x)))[0]


def prior_kind(x):
    """The arm of csrc/pcb_frontier.h:log_prior a float32 prior takes."""
    b = _f32_bits(x)
    e = (b >> 23) & 0xff
    if math.isnan(x):
        return "prior_nan"
    if b >> 31:
        return "prior_negative" if (b & 0x7fffffff) else "prior_zero"
    if e == 0:
        return "prior_denormal" if b else "prior_zero"
    if e == 255:
        return "prior_inf"
    return "prior_above_1" if x > 1.0 else "prior_ok"


def facts(c):
    """The ADVANCE calls of a case walked again in plain Python -> {arm: times reached}.  The in set of call i is the model's
    state after call i - 1 with the call's load on top."""
    P, W, K, T, pw = c.P, c.W, c.K, c.T, c.prior_weight
    F = W * K
    out = {}

    def hit(k, n=1):
        out[k] = out.get(k, 0) + n
    hit("weight_zero" if pw == 0.0 else "weight_non_zero")
    for i, call in enumerate(c.seq):
        if call["phases"] != ADVANCE:
            continue
        s = 1 if call["swap"] else 0
        before = c.states[i - 1]
        length, best_len, best_value = before[f"path_len_{s}"], before["best_len"].copy(), before["best_value"].copy()
        cum = before[f"cum_logp_{s}"]
        if call["load"] is not None:
            length, cum, best_len, best_value = call["load"]["path_len"], call["load"]["cum_logp"], call["load"]["best_len"].copy(), call["load"]["best_value"].copy()
        value, over, count, _, prior = call["evaluation"]
        for p in range(P):
            scores, live = [], 0
            for j in range(F):
                r = p * F + j
                ln = int(length[r])
                if ln < -1 or ln > T:
                    hit("bad_len")
                if not 0 <= ln <= T:
                    continue
                live += 1
                hit("row_at_T", ln == T)
                v = float(value[r])
                if over[r]:
                    hit("nan_final", math.isnan(v))
                    hit("first_evaluation_terminal", i == 1 and j == 0)
                    v = -math.inf if math.isnan(v) else v
                    if best_len[p] != -1:
                        hit("later_final_better", v > best_value[p])
                        hit("later_final_equal", v == best_value[p])
                    if best_len[p] == -1 or v > best_value[p]:
                        best_len[p], best_value[p] = ln, v
                    continue
                hit("count_below_0", int(count[r]) < 0)
                hit("count_above_K", int(count[r]) > K)
                k = min(max(int(count[r]), 0), K)
                if ln < T and k > 0:
                    hit("nan_value", math.isnan(v))
                    hit("inf_value", math.isinf(v))
                    sc = v if pw == 0.0 else v + pw * float(cum[r])
                    scores.append((-math.inf if math.isnan(sc) else sc, math.copysign(1.0, sc), j, k))
            hit("zero_expandable", live > 0 and not scores)
            hit("fewer_than_W", 0 < len(scores) < W)
            hit("more_than_W", len(scores) > W)
            order = sorted(scores, key=lambda t: (-t[0], t[2]))
            for a, b in zip(order, order[1:]):
                hit("tie", a[0] == b[0])
                hit("tie_of_zeros", a[0] == b[0] == 0.0 and a[1] != b[1])
            if len(order) > W:
                hit("tie_at_the_cut", order[W - 1][0] == order[W][0])
            for _, _, j, k in order[:W]:
                for cc in range(k):
                    hit(prior_kind(float(prior[p * F + j, cc])))
    return {k: v for k, v in out.items()}


ARMS = ("tie", "tie_of_zeros", "tie_at_the_cut", "nan_value", "inf_value", "nan_final", "fewer_than_W", "more_than_W", "zero_expandable",
        "first_evaluation_terminal", "row_at_T", "count_below_0", "count_above_K", "prior_zero", "prior_denormal", "prior_negative", "prior_inf",
        "prior_nan", "prior_above_1", "prior_ok", "weight_zero", "weight_non_zero", "bad_len", "later_final_better", "later_final_equal")


def reach(names):
    total = {}
    for n in names:
        for k, v in facts(case(n)).items():
            total[k] = total.get(k, 0) + int(v)
    return total


def assert_reach(names):
    """Every arm of the rule is reached by the cases `names`, and the searches among them reach most without the hand-made calls."""
    total = reach(names)
    missing = [a for a in ARMS if not total.get(a)]
    assert not missing, missing
    assert any(case(n).states[-1]["errors"] & ERR_ROW for n in names) and any(not case(n).states[-1]["errors"] for n in names)
