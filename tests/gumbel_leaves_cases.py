"""The cases of pcbenv_gumbel_advance_leaves (include/pcbenv_gumbel_leaves.h) and its CPU model: the trees, counters and
calls of tests/gumbel_cases.py -- every kind of root at every group width, the preset sim_index values, the scripted
evaluations, the damage pokes -- with `pending` and L leaves per launch, and tools/gumbel_leaves_check.cpp --
csrc/pcb_gumbel_leaves.h as a program of its own, built with AddressSanitizer and UBSan -- to run them.
tests/test_gumbel_leaves_model.py holds the model to the specification (pcbenv/search.py:gumbel_select_root per leaf,
gumbel_choose, gumbel_search(leaves=L)) and to tools/gumbel_check.cpp at L = 1, tests/test_gumbel_leaves_gpu.py the kernel to the
model.  Plain module, no test; needs no GPU.

A case is gumbel_cases.case(name) with L leaves: the same P roots, T = 3 levels, K = min(C, 3) candidates, the same calls
(SELECT on the preset counters, ABSORB, BEGIN | SELECT, n + 1 times ABSORB | SELECT, ABSORB, CHOOSE), the exchange tensors of
P * L rows, `pending` zero before the first call.  The evaluation of row r in call i is gumbel_cases.evaluation's hash of
(case, call, r): with L = 1 the very evaluations of gumbel_cases.  N is gumbel_cases' at L = 1 -- the two runs are compared
field by field -- and grows by 3 K slots per further leaf up to four, so that the launches of many leaves still reach level 2
before the larger roots run out of slots: ERR_FULL is part of every width.
The preset sim_index values (0, inside a phase, at a halving boundary, n - 1, n, above n) make call 0 cross a phase boundary
and the end of the budget in the middle of its leaves."""
import functools
from types import SimpleNamespace

import numpy as np

import gumbel_cases as gc
import model_harness as mh
import puct_cases as pc
import puct_leaves_cases as plc
from pcbenv.search import considered_visits

BEGIN, ABSORB, SELECT, CHOOSE = gc.BEGIN, gc.ABSORB, gc.SELECT, gc.CHOOSE
ERR_FULL, ERR_TREE = gc.ERR_FULL, gc.ERR_TREE
FILL, T, SEED, BLOCK = gc.FILL, gc.T, gc.SEED, gc.BLOCK
TREE_FIELDS, OUT_FIELDS, FLOATS = gc.TREE_FIELDS, gc.OUT_FIELDS, gc.FLOATS
STATE_FIELDS = gc.STATE_FIELDS + ("pending",)
POKED = gc.POKED + ("pending",)
INT_MAX, INT_MIN = 2 ** 31 - 1, -(2 ** 31)

# L: 1; 2; 3, which divides no round; 4 = Mc of two cases; 8, more than a round, so a child is visited twice in a launch
LEAVES = (1, 2, 3, 4, 8)
# one L above G: the table entries of a launch take more than one per lane
CASES = [(name, L) for name in gc.CASES for L in LEAVES] + [("G4_C4_P131", 9)]
DAMAGE_CASE, DAMAGE_ROOT, DAMAGE_L = gc.DAMAGE_CASE, gc.DAMAGE_ROOT, 3
DAMAGE = dict(gc.DAMAGE)
DAMAGE.update({
    "pending_int_max": (4, "pending", lambda N, k, C: INT_MAX),   # pending is data: it addresses nothing and traps nothing
    "pending_int_min": (4, "pending", lambda N, k, C: INT_MIN),
    "pending_child_int_max": (4, "pending", lambda N, k, C: INT_MAX),
})


def shapes(P, N, C, L, levels=T):
    s = gc.shapes(P, N, C, levels)
    s.update(selected=(P * L,), path_len=(P * L,), paths=(levels, P * L, 3), pending=(P, N))
    return s


def program():
    """tools/gumbel_leaves_check.cpp as tests/model_harness.py:tool builds it; None without g++."""
    return mh.tool("gumbel_leaves_check")


def run(state, C, K, n, Mc, L, rule, seq, levels=T):
    """gumbel_cases.run for L leaves: state has `pending` and exchange tensors of P * L rows; an ABSORB call brings P * L
    rows; pokes name a tensor of POKED.  -> [state after call i]."""
    P, N = state["parent"].shape
    R = P * L
    table = considered_visits(Mc, n).numpy()
    words = [np.array([P, N, C, levels, K, n, Mc, L, len(seq)] + [mh.bits(x) for x in rule], np.int64), table.astype(np.int64).ravel()]
    words += [mh.words(state[f], f in FLOATS) for f in STATE_FIELDS]
    for c in seq:
        words.append(np.array([c["phases"], mh.u64(c["seed"]), mh.u64(c["step_index"]), c["first_root"], len(c["pokes"])] +
                              [w for name, at, value in c["pokes"] for w in (POKED.index(name), at, value)], np.int64))
        if c["phases"] & ABSORB:
            value, over, count, actions, prior = c["evaluation"]
            assert actions.shape == (R, K, 3) and prior.shape == (R, K) and prior.dtype == np.float32
            words += [mh.words(value, True), mh.words(over), mh.words(count), mh.words(actions), mh.float32_words(prior)]
    return mh.cut(mh.run_words(program(), words), len(seq), STATE_FIELDS + OUT_FIELDS, shapes(P, N, C, L, levels), FLOATS, ("child_policy",))


def capacity(base, L):
    """N of case `base` with L leaves."""
    return base.N + 3 * base.K * (min(L, 4) - 1)


def with_leaves(state, P, N, L, levels=T):
    """A state of gumbel_cases (numpy) as one of L leaves and N >= its slots: the new slots as PCBENV_TREE_INIT leaves them,
    the exchange tensors of P * L rows filled with FILL, nothing pending."""
    was = state["parent"].shape[1]
    init = dict(parent=-1, first_child=-1, value_max=-np.inf)
    st = {}
    for f, v in state.items():
        v = np.array(v)
        if v.ndim >= 2 and v.shape[1] == was and f not in ("paths", "sim_visits"):
            wide = np.full((P, N) + v.shape[2:], init.get(f, 0), v.dtype)
            wide[:, :was] = v
            v = wide
        st[f] = v
    i32 = lambda shape, x: np.full(shape, x, np.int32)
    st.update(selected=i32(P * L, FILL), path_len=i32(P * L, FILL), paths=i32((levels, P * L, 3), FILL), pending=i32((P, N), 0))
    return st


@functools.lru_cache(maxsize=None)
def case(name, L):
    """-> SimpleNamespace(name, L, P, N, C, G, K, n, Mc, rule, kinds, k, state, seq, states, base): gumbel_cases.case(name) with L
    leaves and the model's state after every call."""
    base = gc.case(name)
    P, N = base.P, capacity(base, L)
    assert N > base.C + 3  # C != N: no [P, C] tensor is taken for a [P, N] one
    st = with_leaves(base.state, P, N, L)
    seq = [dict(q, evaluation=None if q["evaluation"] is None else gc.evaluation(name, i, P * L, base.K, None)) for i, q in enumerate(base.seq)]
    return SimpleNamespace(name=name, L=L, P=P, N=N, C=base.C, G=base.G, K=base.K, n=base.n, Mc=base.Mc, rule=base.rule, kinds=base.kinds, k=base.k,
                           state=st, seq=seq, states=run(st, base.C, base.K, base.n, base.Mc, L, base.rule, seq), first_root=base.first_root,
                           step_index=base.step_index, table=base.table, base=base)


def before(c, i):
    return c.state if i == 0 else c.states[i - 1]


@functools.lru_cache(maxsize=None)
def damaged(name, L=DAMAGE_L):
    """gumbel_cases.damaged with L leaves -> (the case, the index of the damaged call, its sequence up to and including that
    call with the poke, the model's states of it, the root).  A poke on `selected` hits leaf 0 of the root, one on `pending`
    the root's slot 0, or ("pending_child") its first child."""
    c = case(DAMAGE_CASE, L)
    p = DAMAGE_ROOT
    assert c.kinds[p] == "kept" and 0 < p < c.P - 1
    at, tensor, value = DAMAGE[name]
    at = at % len(c.seq)
    shp = shapes(c.P, c.N, c.C, L)
    was = before(c, at)
    k = int(was["num_children"][p, 0])
    index = (p * L,) if tensor == "selected" else (p,) if len(shp[tensor]) == 1 else (p, int(was["first_child"][p, 0]) if name == "pending_child_int_max" else 0)
    poke = (tensor, pc.flat(shp[tensor], *index), int(value(c.N, k, c.C)))
    seq = list(c.seq[:at]) + [dict(c.seq[at], pokes=(poke,))]
    return c, at, seq, run(c.state, c.C, c.K, c.n, c.Mc, L, c.rule, seq), p


# ---- a launch again, leaf by leaf: the specification's root step and Python floats below it ---------------------------------
def redo_select(c, q, was, st):
    """The SELECT of call q of case c redone from `st`'s tree (SELECT stores nothing to it but pending): level 0 of every leaf
    by pcbenv/search.py:gumbel_select_root on the counters as the leaves before left them, the levels below in Python floats
    with the operations of csrc/pcb_puct_leaves.h:leaves_score.  Healthy trees only.  `was`: the state the call started from,
    for the counters and pending (zero after an ABSORB); st: the state after it.  Checks selected, path_len, the path rows,
    pending, sim_index and sim_visits, and returns the facts of the launch: a Counter of what happened."""
    import collections

    import torch
    from pcbenv.search import gumbel_select_root
    facts = collections.Counter()
    P, L, n = c.P, c.L, c.n
    tree = gc.tree_of(st)
    table = torch.from_numpy(np.ascontiguousarray(c.table))
    begun, absorbed = q["phases"] & BEGIN, q["phases"] & ABSORB
    t = np.zeros(P, np.int32) if begun else np.array(was["sim_index"], np.int32)
    sv = np.zeros((P, c.C), np.int32) if begun else np.array(was["sim_visits"], np.int32)
    pending = [dict() if absorbed else {s: int(x) for s, x in enumerate(was["pending"][p]) if x} for p in range(P)]
    alive = np.ones(P, bool)
    t0 = t.copy()
    for l in range(L):
        sel = gumbel_select_root(tree, torch.from_numpy(t), torch.from_numpy(sv), table, c.C, c.rule[1], c.rule[2], q["seed"], q["step_index"], q["first_root"])
        assert int(sel["errors"]) == 0
        for p in range(P):
            row = p * L + l
            k = int(st["num_children"][p, 0])
            halts = bool(st["terminal"][p, 0]) or k == 0
            sched = bool(sel["scheduled"][p])
            if alive[p] and l > 0 and (halts or not sched):
                alive[p] = False
                facts["budget_ends_inside" if not halts and t[p] != t0[p] else "one_leaf_only"] += 1
            if not alive[p]:
                assert st["selected"][row] == -1 and st["path_len"][row] == -1, (p, l)
                assert (st["paths"][:, row] == was["paths"][:, row]).all(), (p, l)  # the rows behind a -1 are untouched
                continue
            pend = pending[p]
            node, d, passed = 0, 0, [0]
            if sched:
                node, d = int(st["first_child"][p, 0]) + int(sel["child"][p]), 1
                passed.append(node)
                row_phase = c.table[min(c.Mc, k)]
                facts["crosses_a_boundary"] += l > 0 and row_phase[t[p]] != row_phase[t[p] - 1] and t[p] != t0[p]
            elif not halts:
                facts["puct_at_root"] += 1
            while d < T and not st["terminal"][p, node] and st["num_children"][p, node] != 0 and (d > 0 or not sched):
                fc, kk = int(st["first_child"][p, node]), int(st["num_children"][p, node])
                look = {s: pend.get(s, 0) for s in [node] + list(range(fc, fc + kk))}
                sc = [plc._score(st, p, node, fc + ch, look, c.rule[0]) for ch in range(kk)]
                node, d = fc + sc.index(max(sc)), d + 1
                passed.append(node)
            taken = len(passed) - 1
            for lvl in range(taken):  # a repeat's own path rows hold what it passed
                assert (st["paths"][lvl, row] == st["node_action"][p, passed[lvl + 1]]).all(), (p, l, lvl)
            if not st["terminal"][p, node] and st["num_children"][p, node] == 0 and pend.get(node, 0) > 0:
                alive[p] = False
                facts["repeat"] += 1
                facts["repeat_behind_a_leaf"] += l > 0
                assert st["selected"][row] == -1 and st["path_len"][row] == -1, (p, l)
                assert (st["paths"][taken:, row] == was["paths"][taken:, row]).all()
                continue
            assert (node, taken) == (st["selected"][row], st["path_len"][row]), (p, l, node, taken)
            assert (st["paths"][taken:, row] == was["paths"][taken:, row]).all()  # rows >= path_len are untouched
            facts["deeper"] += taken >= 2
            for s in passed:
                pend[s] = pend.get(s, 0) + 1
            if sched:
                facts["twice_in_a_launch"] += sv[p, int(sel["child"][p])] - (0 if begun else was["sim_visits"][p, int(sel["child"][p])]) >= 1
                t[p], sv[p] = int(sel["sim_index"][p]), sel["sim_visits"][p].numpy()
        facts["leaves"] += int(alive.sum())
    for p in range(P):
        want = np.zeros(c.N, np.int64)
        for s, x in pending[p].items():
            want[s] = x
        assert np.array_equal(st["pending"][p], want), p
    assert np.array_equal(st["sim_index"], t) and np.array_equal(st["sim_visits"], sv)
    return facts


@functools.lru_cache(maxsize=None)
def check_cases():
    """The table is what it is there for: every group width at every L, an L above G, roots across workgroups with a partly
    filled last group, and on the model's states every branch of the rule.  -> the facts, summed."""
    import collections
    total = collections.Counter()
    cases = [case(name, L) for name, L in CASES]
    assert {c.G for c in cases} == {4, 8, 16, 32, 64} and {c.L for c in cases} == set(LEAVES) | {9} and any(c.L > c.G for c in cases)
    assert all(c.P > BLOCK // c.G and c.P % (BLOCK // c.G) for c in cases) and any(c.step_index >> 32 for c in cases)
    full = set()
    for c in cases:
        err = 0
        for i, (q, st) in enumerate(zip(c.seq, c.states)):
            err |= st["errors"]
            assert not st["errors"] & ERR_TREE
            if q["phases"] & SELECT:
                facts = redo_select(c, q, before(c, i), st)
                if c.L > 1:
                    total.update(facts)
            if q["phases"] & ABSORB and not q["phases"] & SELECT:
                assert not st["pending"].any()
        if err & ERR_FULL and c.L > 1:
            full.add(c.name)
    assert full == set(gc.CASES), set(gc.CASES) - full  # at every width the larger roots run out of slots
    want = {"repeat", "repeat_behind_a_leaf", "budget_ends_inside", "one_leaf_only", "crosses_a_boundary", "puct_at_root", "deeper", "twice_in_a_launch"}
    assert want <= {f for f, x in total.items() if x > 0}, want - set(total)
    return total


# ---- a launch worked out by hand: the state, and what the rule alone says of the result ----------------------------------------
def hand_state(L, P=3, k=5):
    """P `full` roots with k children, priors 1 / k, no visits below the root; T = 3."""
    N = k + 1
    st = gc.init_state(P, N, k, T)
    st["num_children"][:, 0], st["first_child"][:, 0], st["num_nodes"][:] = k, 1, N
    st["visits"][:, 0], st["value_sum"][:, 0], st["value_max"][:, 0], st["reward_lo"][:], st["reward_hi"][:] = 1, 0.5, 0.5, 0.5, 0.5
    st["parent"][:, 1:], st["depth"][:, 1:], st["prior"][:, 1:] = 0, 1, 1.0 / k
    st["node_action"][:, 1:, 2] = np.arange(k)
    st["node_action"][:, 1:, 1] = 10 + np.arange(k)
    return with_leaves(st, P, N, L)


HAND = dict(k=5, Mc=4, n=8, rule=(1.25, 50.0, 1.0))


def check_hand(L, st, P=3):
    """Mc = 4, n = 8: row 4 of the table is 0 0 0 0 1 1 2 2.  The first four simulations each want a child at count 0 and find
    one, another one every time, for the one before went up to 1; each child is a node without children and nothing pending:
    path_len 1.  Simulation 4 wants a child at count 1: one of the four just visited, which is waiting for its evaluation with
    a pending visit -- a repeat, which consumes nothing and ends the launch of its root."""
    k = HAND["k"]
    assert st["errors"] == 0
    for p in range(P):
        rows = slice(p * L, (p + 1) * L)
        sel, plen = st["selected"][rows], st["path_len"][rows]
        assert len(set(sel[:4])) == 4 and (sel[:4] >= 1).all() and (sel[:4] <= k).all() and (plen[:4] == 1).all()
        assert st["sim_index"][p] == 4 and st["pending"][p, 0] == 4 and sorted(st["sim_visits"][p]) == [0] * (k - 4) + [1] * 4
        assert np.array_equal(st["pending"][p, 1:], st["sim_visits"][p])
        for l in range(4):
            assert (st["paths"][0, p * L + l] == st["node_action"][p, sel[l]]).all() and (st["paths"][1:, p * L + l] == FILL).all()
        if L == 8:
            assert (sel[4:] == -1).all() and (plen[4:] == -1).all()
            went = st["paths"][0, p * L + 4]  # path row 0 of the repeat: the action of the child it went to, one of the four
            assert went[1] - 10 == went[2] and 1 + went[2] in sel[:4] and (st["paths"][1:, p * L + 4] == FILL).all()
            assert (st["paths"][:, p * L + 5:(p + 1) * L] == FILL).all()
