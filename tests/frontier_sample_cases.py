"""Cases, recordings and the CPU model of pcbenv_frontier_sample (plain module, no test; needs no GPU).

The specification is pcbenv/search.py:frontier_sample_advance.  `record` runs a search on it on the CPU -- INIT, then per
depth an evaluation and ADVANCE with the sets swapped -- and writes the calls down; `replay` feeds such a sequence to
tools/frontier_sample_check.cpp -- csrc/pcb_frontier_sample.h compiled for the CPU with AddressSanitizer and UBSan, a
program of its own -- which returns every tensor after every call; `specify` runs the same sequence through the
specification from the same sentinel-filled tensors.  The GPU tests compare the kernel with the model's states.

The evaluators are tests/puct_cases.py's through tests/frontier_cases.py:evaluator -- synthetic, real and poisoned -- at
P * F rows.  A call may also bring a state made by hand (`load`): `hand_made` is a table of such calls, one per arm of the
rule a search does not reach by itself.  `path_evaluator` is a vectorised evaluator that depends on the path alone.

`facts` walks the ADVANCE calls of a case again in plain Python and counts the arms of the rule they reach; `assert_reach`
holds the table of cases to every arm, so that a test that compares two implementations on it cannot be vacuous."""
import functools
import math
from types import SimpleNamespace

import numpy as np
import torch

import frontier_cases as fc
import model_harness as mh
from model_harness import same_bits  # noqa: F401  (the tests take it from here)
from pcbenv import search
from pcbenv.search import Evaluation

INIT, ADVANCE, LOADED = 1, 2, 8
ERR_ROW, ERR_SET = 2, 4
FILL, FILL_F = -7, -7.5  # what the model's int32 and float64 tensors hold before the first call
ROW_SET = ("paths", "path_len", "cum_logp", "gumbel")
SET_FIELDS = ("set_len", "set_gumbel", "set_logp", "set_value", "set_path")
STATE_FIELDS = tuple(f"{n}_{s}" for s in (0, 1) for n in ROW_SET) + ("parent_row", "live", "best_value", "best_len", "best_path") + SET_FIELDS
FLOATS = ("cum_logp_0", "cum_logp_1", "gumbel_0", "gumbel_1", "best_value", "set_gumbel", "set_logp", "set_value")
LOAD_FIELDS = ("path_len", "cum_logp", "gumbel", "paths", "best_value", "best_len") + SET_FIELDS  # the order of the model's input
ROOTS_PER_BLOCK = 4  # csrc/pcb_frontier_sample.hip: one wavefront per root, 256 threads per workgroup
STEP_INDEX = 100


def shapes(P, W, K, T):
    R, S = P * W * K, P * W
    s = {"parent_row": (R,), "live": (P,), "best_value": (P,), "best_len": (P,), "best_path": (T, P, 3), "set_len": (S,), "set_gumbel": (S,),
         "set_logp": (S,), "set_value": (S,), "set_path": (T, S, 3)}
    for i in (0, 1):
        s.update({f"paths_{i}": (T, R, 3), f"path_len_{i}": (R,), f"cum_logp_{i}": (R,), f"gumbel_{i}": (R,)})
    return s


def program():
    """tools/frontier_sample_check.cpp as tests/model_harness.py:tool builds it; None without g++."""
    return mh.tool("frontier_sample_check")


def new_state(P, W, K, T, device="cpu"):
    """The tensors of `search.new_frontier_sample_tensors`, sentinel-filled as the model's are before its first call."""
    ft = search.new_frontier_sample_tensors(P, W, K, T, device)
    for n, t in ft.items():
        if n != "errors_dev":
            t.fill_(FILL_F if t.dtype == torch.float64 else FILL)
    return ft


def apply_load(ft, load, swap):
    """A hand-made state into the in set of a call, the accumulators and the sample set."""
    s = 1 if swap else 0
    for n in LOAD_FIELDS:
        t = ft[f"{n}_{s}"] if n in ROW_SET else ft[n]
        t.copy_(torch.from_numpy(np.ascontiguousarray(load[n])).to(t.dtype))


def dump(ft):
    """A state of the specification in the form of the model's: int64, FLOATS as float64, and the error word."""
    st = {"errors": int(ft["errors_dev"][0])}
    for f in STATE_FIELDS:
        t = ft[f].cpu()
        st[f] = t.numpy().copy() if f in FLOATS else t.to(torch.int64).numpy()
    return st


def record(P, W, K, T, seed, first_root, evaluate, depth=None, step_index=STEP_INDEX):
    """A search on the specification -> the sequence of its calls: dicts of phases, swap, step_index, evaluation (numpy) and load."""
    ft = new_state(P, W, K, T)
    seq = [dict(phases=INIT, swap=1, step_index=step_index, evaluation=None, load=None)]
    search.frontier_sample_advance(ft, INIT, W, K, seed, step_index, first_root, swap=True)
    for d in range(T + 1 if depth is None else depth):
        cur, s = d % 2, step_index + d * T
        ev = evaluate(ft[f"paths_{cur}"].clone(), ft[f"path_len_{cur}"].clone(), s)
        seq.append(dict(phases=ADVANCE, swap=cur, step_index=s, evaluation=fc._numpy_evaluation(ev), load=None))
        search.frontier_sample_advance(ft, ADVANCE, W, K, seed, s, first_root, ev, swap=cur == 1)
    return seq


def specify(P, W, K, T, seed, first_root, seq, device="cpu"):
    """The sequence through pcbenv/search.py:frontier_sample_advance from sentinel-filled tensors -> [state after call i]."""
    ft = new_state(P, W, K, T, device)
    states = []
    for c in seq:
        if c["load"] is not None:
            apply_load(ft, c["load"], c["swap"])
        ev = None if c["evaluation"] is None else fc._torch_evaluation(c["evaluation"], device)
        search.frontier_sample_advance(ft, c["phases"], W, K, seed, c["step_index"], first_root, ev, swap=bool(c["swap"]))
        states.append(dump(ft))
    return states


def replay(P, W, K, T, seed, first_root, seq):
    """The sequence through tools/frontier_sample_check.cpp -> [state after call i]: dicts of STATE_FIELDS (int64; FLOATS as
    float64) and `errors`.  Raises on anything on stderr."""
    parts = [np.array([0, P, W, K, T, len(seq), mh.u64(seed), first_root], np.int64)]
    R, shp = P * W * K, shapes(P, W, K, T)
    for c in seq:
        parts.append(np.array([c["phases"] | (LOADED if c["load"] is not None else 0), int(c["swap"]), mh.u64(c["step_index"])], np.int64))
        if c["load"] is not None:
            for n in LOAD_FIELDS:
                a = c["load"][n]
                assert a.shape == shp.get(n, shp.get(n + "_0")), n
                parts.append(mh.words(a, a.dtype == np.float64))
        if c["phases"] == ADVANCE:
            value, over, count, actions, prior = c["evaluation"]
            assert actions.shape == (R, K, 3) and prior.shape == (R, K) and prior.dtype == np.float32
            parts += [mh.words(value, True), mh.words(over), mh.words(count), mh.words(actions), mh.float32_words(prior)]
    return mh.cut(mh.run_words(program(), parts), len(seq), STATE_FIELDS, shp, FLOATS)


def truncated_table(rows):
    """child_gumbel of csrc/pcb_frontier_sample.h on rows of (G_S, phi_c, G_c, Z) -> float64 [n], through the same program."""
    a = np.asarray(rows, np.float64).reshape(-1, 4)
    out = mh.run_words(program(), [np.array([1, len(a)], np.int64), mh.words(a, True)])
    return out.view(np.float64).copy()


# ---- an evaluator of the path alone ------------------------------------------------------------------------------------
def _mix_np(h, x):
    h = (h ^ (x.astype(np.uint64) & np.uint64(0xFFFFFFFF))) * np.uint64(0xBF58476D1CE4E5B9)
    return h ^ (h >> np.uint64(29))


def path_evaluator(K, T, seed, early=True):
    """Vectorised, a function of the path alone (not of the row): candidate c is the action (0, 0, c) with a prior picked by
    hash from puct_cases.PRIORS, every node has K candidates, a row is terminal at length T and, with `early`, by hash one
    time in five below the root; the value is hashed into [0, 1)."""
    table = np.array(fc.pc.PRIORS, np.float32)

    def evaluate(paths, path_len, step_index0):
        paths, path_len = paths.numpy(), path_len.numpy()
        R = path_len.shape[0]
        with np.errstate(over="ignore"):
            h = _mix_np(np.full(R, 0x9E3779B97F4A7C15, np.uint64), np.full(R, seed))
            for t in range(T):
                h = np.where(path_len > t, _mix_np(h, paths[t, :, 2] + 1), h)
            value = ((h >> np.uint64(16)) % np.uint64(1000)).astype(np.float64) / 1000.0
            over = (path_len == T) | ((path_len > 0) & ((h >> np.uint64(24)) % np.uint64(5) == 0) & early)
            prior = np.stack([table[(_mix_np(h, np.full(R, c)) >> np.uint64(8)) % np.uint64(len(table))] for c in range(K)], axis=1)
        actions = np.zeros((R, K, 3), np.int32)
        actions[:, :, 2] = np.arange(K)
        return fc._torch_evaluation((value, over.astype(np.uint8), np.full(R, K, np.int32), actions, prior.astype(np.float32)))
    return evaluate


# ---- states made by hand ---------------------------------------------------------------------------------------------
HAND_P, HAND_W, HAND_K, HAND_T = 3, 3, 2, 4


def blank(P, W, K, T):
    """A call with an empty frontier, an empty set and an evaluation of zeros, to be filled in by `put_row` and `put_entry`."""
    c = fc.blank(P, W, K, T)
    S = P * W
    c["load"].update(gumbel=np.zeros(P * W * K), set_len=np.full(S, -1, np.int32), set_gumbel=np.full(S, FILL_F), set_logp=np.full(S, FILL_F),
                     set_value=np.full(S, FILL_F), set_path=np.full((T, S, 3), FILL, np.int32))
    c["step_index"] = STEP_INDEX
    return c


def put_row(call, r, gumbel, **kw):
    fc.put_row(call, r, **kw)
    call["load"]["gumbel"][r] = gumbel


def put_entry(call, s, length, gumbel, logp=-3.0, value=0.125):
    """Slot s of the set: a placement of `length` steps whose path is (9, d, s)."""
    ld = call["load"]
    ld["set_len"][s], ld["set_gumbel"][s], ld["set_logp"][s], ld["set_value"][s] = length, gumbel, logp, value
    for d in range(max(0, min(length, ld["set_path"].shape[0]))):
        ld["set_path"][d, s] = (9, d, s)


def hand_made():
    """Calls on states made by hand, P = 3, W = 3, K = 2 (F = 6), T = 4: one per arm of the rule.  Root 1 is the one things
    are done to; roots 0 and 2 hold an ordinary row and a set entry each, so that a stray write would show."""
    P, W, K, T = HAND_P, HAND_W, HAND_K, HAND_T
    F = W * K
    nan, inf = float("nan"), float("inf")
    calls = []

    def call(rows, entries=None, best=None):
        c = blank(P, W, K, T)
        put_row(c, 0 * F + 1, -0.5, length=1, value=0.5, count=2, tag=1)
        put_row(c, 2 * F + 4, -0.25, length=2, value=0.25, count=K, tag=1)
        put_entry(c, 0 * W + 1, 2, -0.75)
        put_entry(c, 2 * W + 2, 3, -9.0)
        for i, kw in rows.items():
            put_row(c, F + i, **kw)
        for j, kw in (entries or {}).items():
            put_entry(c, W + j, **kw)
        if best is not None:
            c["load"]["best_value"][1], c["load"]["best_len"][1] = best
        calls.append(c)
    # 1: a set entry that survives (slot 0) and one that is dropped (slot 1), next to two expandable rows
    call({0: dict(gumbel=-1.0, length=1, value=0.5, count=2), 3: dict(gumbel=-2.0, length=2, value=0.5, count=1)},
         {0: dict(length=2, gumbel=-0.5), 1: dict(length=3, gumbel=-5.0)})
    # 2: slots 0 and 2 free, slot 1 survives: the finished winners go to slot 0 and slot 2 in rank order (row 4 before row 2)
    call({2: dict(gumbel=-0.3, length=3, value=0.75, terminal=1, cum_logp=-1.25), 4: dict(gumbel=-0.2, length=2, value=0.5, terminal=1, cum_logp=-2.5)},
         {1: dict(length=1, gumbel=-0.1)})
    # 3: ties: a set entry and three rows at -1.0 -- the entry first, then the lower rows, row 5 is cut; 4: -0.0 against +0.0
    call({1: dict(gumbel=-1.0, length=1, value=0.5, count=2), 3: dict(gumbel=-1.0, length=1, value=0.9, terminal=1), 5: dict(gumbel=-1.0, length=1, value=0.5, count=2)},
         {2: dict(length=2, gumbel=-1.0)})
    call({0: dict(gumbel=0.0, length=1, value=0.5, count=2), 1: dict(gumbel=-0.0, length=1, value=0.5, count=2), 2: dict(gumbel=-0.0, length=1, value=0.5, count=2)},
         {1: dict(length=2, gumbel=-0.0)})
    # 5, 6: NaN, -inf and +inf keys: +inf first, then the finite one, NaN and -inf tie at the bottom (the lower id); alone they win
    call({0: dict(gumbel=nan, length=1, value=0.5, count=2), 1: dict(gumbel=-inf, length=1, value=0.5, count=2), 2: dict(gumbel=inf, length=1, value=0.5, count=2),
          3: dict(gumbel=0.5, length=1, value=0.5, count=2)})
    call({0: dict(gumbel=-inf, length=1, value=0.5, count=2), 1: dict(gumbel=nan, length=1, value=0.5, count=1), 4: dict(gumbel=nan, length=2, value=0.5, terminal=1)},
         {0: dict(length=2, gumbel=nan)})
    # 7: a parent whose candidates all have priors without a logarithm, and one with a single good prior
    call({0: dict(gumbel=-1.0, length=1, value=0.5, count=2, priors=(0.0, -0.25)), 1: dict(gumbel=-1.5, length=1, value=0.5, count=2, priors=(nan, 0.25))})
    # 8: cum_logp that is not finite: -inf, NaN and +inf
    call({0: dict(gumbel=-1.0, length=1, value=0.5, count=2, cum_logp=-inf), 1: dict(gumbel=-1.5, length=1, value=0.5, count=2, cum_logp=nan),
          2: dict(gumbel=-1.75, length=1, value=0.5, count=2, cum_logp=inf)})
    # 9: set_len out of range on either side (bit 2): no entries, and slots a finished row may take; 10: path_len out of range (bit 1)
    call({0: dict(gumbel=-1.0, length=2, value=0.5, terminal=1), 1: dict(gumbel=-2.0, length=1, value=0.5, count=2)},
         {0: dict(length=T + 1, gumbel=5.0), 2: dict(length=-2, gumbel=6.0)})
    call({0: dict(gumbel=5.0, length=T + 1, value=0.9, count=2), 1: dict(gumbel=6.0, length=-2, value=0.9, count=2), 2: dict(gumbel=-1.0, length=1, value=0.1, count=2)})
    # 11: more finished contenders than W, the best of them by value is not among the winners; an entry is pushed out
    call({0: dict(gumbel=-4.0, length=2, value=0.99, terminal=1), 1: dict(gumbel=-1.0, length=2, value=0.5, terminal=1), 2: dict(gumbel=-2.0, length=3, value=0.25, terminal=1),
          3: dict(gumbel=-3.0, length=T, value=0.125, terminal=1), 4: dict(gumbel=-0.5, length=1, value=nan, terminal=1)},
         {1: dict(length=2, gumbel=-3.5)}, best=(0.75, 4))
    # 12: rows that are neither finished nor expandable (at T, without candidates) are no contenders whatever their key
    call({0: dict(gumbel=9.0, length=T, value=0.5, count=2), 1: dict(gumbel=9.0, length=1, value=0.5, count=0), 2: dict(gumbel=-1.0, length=1, value=0.5, count=K + 5)})
    return calls


# ---- the table of cases ----------------------------------------------------------------------------------------------
# name: P, W, K, T, the evaluator, seed, first_root, depths (None: T + 1).  What each row is there for is in
# tests/test_frontier_sample_gpu.py; "path_full" rows finish at T alone, so the widest cases fill all F rows and then all W
# slots; P = 5 and 6 fill one workgroup of four roots and leave the second partly empty.
CASES = {
    "W1_K1": (6, 1, 1, 5, "synthetic", 11, 0, None),
    "W3_K5": (6, 3, 5, 5, "poisoned", 12, 3, None),
    "W4_K16": (6, 4, 16, 5, "real", 13, 0, None),
    "W5_K13": (6, 5, 13, 5, "poisoned", 14, 0, None),
    "W16_K64": (2, 16, 64, 3, "path_full", 15, 0, None),
    "W64_K16": (1, 64, 16, 4, "path_full", 16, 7, None),
    "W1_K64": (6, 1, 64, 4, "real", 17, 0, None),
    "W7_K40": (2, 7, 40, 4, "path", 21, 0, None),
    "T1": (6, 3, 5, 1, "poisoned", 18, 0, None),
    "P5": (5, 3, 5, 4, "path", 19, 2 ** 31 - 6, None),
    "P23": (23, 2, 3, 4, "poisoned", 20, 0, None),
    "hand": (HAND_P, HAND_W, HAND_K, HAND_T, "hand", 5, 0, 0),
}


def evaluator(kind, rows, T, K, seed):
    return path_evaluator(K, T, seed, early=kind == "path") if kind in ("path", "path_full") else fc.evaluator(kind, rows, T, K, seed)


@functools.lru_cache(maxsize=None)
def case(name):
    """-> SimpleNamespace(name, P, W, K, T, seed, first_root, seq, states): a sequence of calls and the model's state after each."""
    P, W, K, T, kind, seed, first_root, depth = CASES[name]
    if kind == "hand":
        seq = [dict(phases=INIT, swap=1, step_index=STEP_INDEX, evaluation=None, load=None)] + hand_made()
    else:
        seq = record(P, W, K, T, seed, first_root, evaluator(kind, P * W * K, T, K, seed), depth)
    return SimpleNamespace(name=name, P=P, W=W, K=K, T=T, seed=seed, first_root=first_root, seq=seq, states=replay(P, W, K, T, seed, first_root, seq))


# ---- the arms of the rule a case reaches ------------------------------------------------------------------------------
def _key(x):
    return -math.inf if math.isnan(x) else float(x)


def walk(c):
    """The ADVANCE calls of a case in plain Python: per call and root (i, p, before, after, contenders, winners, parents) with
    contenders = [(key, id, kind)] in the order of the rule, kind one of "entry", "finished", "expandable"."""
    P, W, K, T = c.P, c.W, c.K, c.T
    F = W * K
    for i, call in enumerate(c.seq):
        if call["phases"] != ADVANCE:
            continue
        s = 1 if call["swap"] else 0
        before = {f: c.states[i - 1][f] for f in STATE_FIELDS}
        if call["load"] is not None:
            before.update({(f"{n}_{s}" if n in ROW_SET else n): call["load"][n] for n in LOAD_FIELDS})
        value, over, count, _, prior = call["evaluation"]
        for p in range(P):
            cont = []
            for j in range(W):
                if 0 <= int(before["set_len"][p * W + j]) <= T:
                    cont.append((_key(before["set_gumbel"][p * W + j]), j, "entry"))
            for i_row in range(F):
                r = p * F + i_row
                ln = int(before[f"path_len_{s}"][r])
                if not 0 <= ln <= T:
                    continue
                k = min(max(int(count[r]), 0), K)
                if over[r]:
                    cont.append((_key(before[f"gumbel_{s}"][r]), W + i_row, "finished"))
                elif ln < T and k > 0:
                    cont.append((_key(before[f"gumbel_{s}"][r]), W + i_row, "expandable"))
            cont.sort(key=lambda t: (-t[0], t[1]))
            yield SimpleNamespace(i=i, p=p, s=s, before=before, after=c.states[i], contenders=cont, winners=cont[:W], call=call)


def facts(c):
    """{arm: times reached} over the ADVANCE calls of a case."""
    P, W, K, T = c.P, c.W, c.K, c.T
    F = W * K
    out = {}

    def hit(k, n=1):
        out[k] = out.get(k, 0) + int(n)
    for x in walk(c):
        b, s, p = x.before, x.s, x.p
        value, over, count, _, prior = x.call["evaluation"]
        hit("bad_set_len", sum(1 for j in range(W) if not -1 <= int(b["set_len"][p * W + j]) <= T))
        hit("bad_len", sum(1 for i in range(F) if not -1 <= int(b[f"path_len_{s}"][p * F + i]) <= T))
        kinds = [k for _, _, k in x.contenders]
        won = [k for _, _, k in x.winners]
        hit("more_than_W", len(kinds) > W)
        hit("fewer_than_W", 0 < len(kinds) < W)
        hit("no_contender", not kinds)
        hit("finished_more_than_W", kinds.count("finished") > W)
        hit("entry_survives", won.count("entry"))
        hit("entry_dropped", kinds.count("entry") - won.count("entry"))
        hit("finished_enters", won.count("finished"))
        hit("finished_cut", kinds.count("finished") - won.count("finished"))
        hit("expandable_cut", kinds.count("expandable") - won.count("expandable"))
        survivors = {j for _, j, k in x.winners if k == "entry"}
        free = [j for j in range(W) if j not in survivors]
        hit("enters_behind_a_survivor", sum(1 for m in range(won.count("finished")) if free[m] != m))
        for a, bb in zip(x.contenders, x.contenders[1:]):
            if a[0] == bb[0]:
                hit("tie")
                hit("tie_entry_row", a[2] == "entry" and bb[2] != "entry")
                hit("tie_rows", a[2] != "entry" and bb[2] != "entry")
        if len(x.contenders) > W:
            hit("tie_at_the_cut", x.contenders[W - 1][0] == x.contenders[W][0])
        for key_, id_, _ in x.contenders:
            raw = b["set_gumbel"][p * W + id_] if id_ < W else b[f"gumbel_{s}"][p * F + id_ - W]
            hit("nan_key", math.isnan(raw))
            hit("plus_inf_key", raw == math.inf)
            hit("minus_inf_key", raw == -math.inf)
            hit("tie_of_zeros", raw == 0.0 and math.copysign(1.0, raw) < 0)
        for key_, id_, k in x.winners:
            if k != "expandable":
                continue
            r = p * F + id_ - W
            kk = min(max(int(count[r]), 0), K)
            good = [fc.prior_kind(float(prior[r, cc])) in ("prior_ok", "prior_above_1") for cc in range(kk)]
            hit("parent")
            hit("all_priors_bad", not any(good))
            hit("some_prior_bad", any(good) and not all(good))
            hit("cum_logp_not_finite", not math.isfinite(float(b[f"cum_logp_{s}"][r])))
            hit("parent_key_not_finite", not math.isfinite(key_))
    return out


ARMS = ("bad_set_len", "bad_len", "more_than_W", "fewer_than_W", "no_contender", "finished_more_than_W", "entry_survives", "entry_dropped",
        "finished_enters", "finished_cut", "expandable_cut", "enters_behind_a_survivor", "tie", "tie_entry_row", "tie_rows", "tie_at_the_cut", "nan_key",
        "plus_inf_key", "minus_inf_key", "tie_of_zeros", "parent", "all_priors_bad", "some_prior_bad", "cum_logp_not_finite", "parent_key_not_finite")


def reach(names):
    total = {}
    for n in names:
        for k, v in facts(case(n)).items():
            total[k] = total.get(k, 0) + int(v)
    return total


def assert_reach(names):
    """Every arm of the rule is reached by the cases `names`."""
    total = reach(names)
    missing = [a for a in ARMS if not total.get(a)]
    assert not missing, missing
    errs = [case(n).states[-1]["errors"] for n in names]
    assert any(e & ERR_ROW for e in errs) and any(e & ERR_SET for e in errs) and any(not e for e in errs)


def children_properties(c):
    """Exact maximum on every recorded call: among the children of a kept parent with a finite key and at least one child
    of finite cum_logp, the largest gumbel equals the parent's key bit for bit and no child exceeds it; a parent whose key
    is not finite hands it down.  -> the number of parents checked."""
    F, K = c.W * c.K, c.K
    checked = 0
    for x in walk(c):
        o = 1 - x.s
        for w in range(c.W):
            rows = [x.p * F + w * K + cc for cc in range(K)]
            rows = [r for r in rows if x.after[f"path_len_{o}"][r] >= 0]
            if not rows:
                continue
            parent = int(x.after["parent_row"][rows[0]])
            assert all(int(x.after["parent_row"][r]) == parent for r in rows)
            G_S = _key(x.before[f"gumbel_{x.s}"][x.p * F + parent])
            g = np.array([x.after[f"gumbel_{o}"][r] for r in rows])
            phi = np.array([x.after[f"cum_logp_{o}"][r] for r in rows])
            assert not np.isnan(g).any() and (g <= G_S).all(), (c.name, x.i, x.p, w)
            assert np.isneginf(g[~np.isfinite(phi)]).all()
            if np.isfinite(phi).any():
                assert same_bits(np.float64(g[np.isfinite(phi)].max()) + 0.0, np.float64(G_S) + 0.0), (c.name, x.i, x.p, w)
                checked += 1
    return checked
