"""The cases of pcbenv_gumbel_tree_advance_leaves (include/pcbenv_gumbel_tree_leaves.h) and its CPU model: the trees, counters
and calls of tests/gumbel_tree_cases.py -- the six widths, roots across workgroups with a partly filled last one, T = 4 levels,
the eleven arms of the node rule below every root child, the preset sim_index values -- with `pending` and L leaves per launch,
and tools/gumbel_tree_leaves_check.cpp -- csrc/pcb_gumbel_tree_leaves.h as a program of its own, built with AddressSanitizer and
UBSan -- to run them.  tests/test_gumbel_tree_leaves_model.py holds the model to the specification (pcbenv/search.py:
gumbel_select_root(full=True) per leaf, gumbel_select_node(pending=) per level, gumbel_choose(full=True),
gumbel_search(node_rule="gumbel", leaves=L)) and to tools/gumbel_tree_check.cpp at L = 1, tests/test_gumbel_tree_leaves_gpu.py the
kernel to the model.  Plain module, no test; needs no GPU.

A case is gumbel_tree_cases.case(name) with L leaves: the same P roots and calls (CHOOSE on the trees as built, SELECT on the
preset counters, ABSORB, BEGIN | SELECT, n + 1 times ABSORB | SELECT, ABSORB, CHOOSE), the exchange tensors of P * L rows,
`pending` zero before the first call.  The evaluation of row r in a call is gumbel_cases.evaluation's hash of (case, call, r):
with L = 1 the very evaluations of gumbel_tree_cases.  N is gumbel_tree_cases' at L = 1 -- the two runs are compared field by
field.  With more leaves it grows as gumbel_leaves_cases.capacity does, per further leaf up to four, but by K slots and from the
fullest root of the case: gumbel_tree_cases sizes N for the widest tree it could build, which at four of the six widths leaves
more room than the calls of a case ever fill, and ERR_FULL is to be part of every width.  The preset sim_index values make call
1 cross a halving boundary and the end of the budget in the middle of its leaves."""
import collections
import functools
from types import SimpleNamespace

import numpy as np
import torch

import gumbel_cases as gc
import gumbel_leaves_cases as glc
import gumbel_tree_cases as gtc
import model_harness as mh
import puct_cases as pc
from pcbenv.search import considered_visits, gumbel_node_scores, gumbel_select_root

BEGIN, ABSORB, SELECT, CHOOSE = gc.BEGIN, gc.ABSORB, gc.SELECT, gc.CHOOSE
ERR_FULL, ERR_TREE = gc.ERR_FULL, gc.ERR_TREE
FILL, T, SEED, BLOCK = gc.FILL, gtc.T, gc.SEED, gc.BLOCK
TREE_FIELDS, OUT_FIELDS, FLOATS = gc.TREE_FIELDS, gc.OUT_FIELDS, gc.FLOATS
STATE_FIELDS, POKED = glc.STATE_FIELDS, glc.POKED

LEAVES = glc.LEAVES  # 1, 2, 3, 4, 8
CASES = [(name, L) for name in gtc.CASES for L in LEAVES] + [("G4_C4_P131", 9)]  # one L above G
DAMAGE_CASE, DAMAGE_ROOT, DAMAGE_L = gtc.DAMAGE_CASE, gtc.DAMAGE_ROOT, glc.DAMAGE_L
MSUM = "msum_minus_1"
# gumbel_tree_cases' damage, the three pending pokes of gumbel_leaves_cases, and counts that add up to -1 at a node below the root
DAMAGE = dict(gtc.DAMAGE)
DAMAGE.update({name: glc.DAMAGE[name] for name in ("pending_int_max", "pending_int_min", "pending_child_int_max")})
DAMAGE[MSUM] = (4, "pending", None)


def shapes(P, N, C, L, levels=T):
    return glc.shapes(P, N, C, L, levels)


def program():
    """tools/gumbel_tree_leaves_check.cpp as tests/model_harness.py:tool builds it; None without g++."""
    return mh.tool("gumbel_tree_leaves_check")


def run(state, C, K, n, Mc, L, rule, seq, levels=T):
    """gumbel_leaves_cases.run on tools/gumbel_tree_leaves_check.cpp: the same wire format, states and outputs."""
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
    return base.N if L == 1 else int(base.state["num_nodes"].max()) + base.K * (2 + min(L, 4) - 1)


def with_leaves(state, P, N, L, levels=T):
    """gumbel_leaves_cases.with_leaves; a state of more than N slots loses the ones behind N, which no root uses."""
    was = state["parent"].shape[1]
    if was > N:
        assert state["num_nodes"].max() <= N
        state = {f: np.array(v)[:, :N] if np.ndim(v) >= 2 and np.shape(v)[1] == was and f not in ("paths", "sim_visits") else v for f, v in state.items()}
    return glc.with_leaves(state, P, N, L, levels)


@functools.lru_cache(maxsize=None)
def case(name, L):
    """-> SimpleNamespace(name, L, P, N, C, G, K, n, Mc, rule, kinds, k, state, seq, states, base, arms): gumbel_tree_cases.case(name)
    with L leaves and the model's state after every call."""
    base = gtc.case(name)
    P, N = base.P, capacity(base, L)
    assert N > base.C + 3  # C != N: no [P, C] tensor is taken for a [P, N] one
    st = with_leaves(base.state, P, N, L)
    # call i of these cases is call i - 1 of gumbel_cases, whose index the evaluations are hashed with
    seq = [dict(q, evaluation=None if q["evaluation"] is None else gc.evaluation(name, i - 1, P * L, base.K, None)) for i, q in enumerate(base.seq)]
    return SimpleNamespace(name=name, L=L, P=P, N=N, C=base.C, G=base.G, K=base.K, n=base.n, Mc=base.Mc, rule=base.rule, kinds=base.kinds, k=base.k,
                           state=st, seq=seq, states=run(st, base.C, base.K, base.n, base.Mc, L, base.rule, seq), first_root=base.first_root,
                           step_index=base.step_index, table=base.table, base=base, arms=base.arms, key=base.key)


def before(c, i):
    return c.state if i == 0 else c.states[i - 1]


def msum_pokes(c, was, p):
    """Under every child a of root p that has children, pending of a's LAST child is set so that the counts of a's children add
    up to -1: Msum == -1 whichever child the root level takes, 1 + Msum == 0, and a first child without a visit or a pending
    visit has t = 0 / 0, a NaN."""
    shp = shapes(c.P, c.N, c.C, c.L)
    k0, fc0 = int(was["num_children"][p, 0]), int(was["first_child"][p, 0])
    pokes = []
    for a in range(fc0, fc0 + k0):
        k, fc = int(was["num_children"][p, a]), int(was["first_child"][p, a])
        if k == 0:
            continue
        rest = int(was["visits"][p, fc:fc + k].astype(np.int64).sum()) + int(was["pending"][p, fc:fc + k - 1].astype(np.int64).sum())
        pokes.append(("pending", pc.flat(shp["pending"], p, fc + k - 1), -1 - rest))
    return tuple(pokes)


@functools.lru_cache(maxsize=None)
def damaged(name, L=DAMAGE_L):
    """-> (the case, the index of the damaged call, its sequence up to and including that call with the pokes, the model's states
    of it, the root, the state a healthy run has behind the same calls).  A poke on `selected` hits leaf 0 of the root, one on
    `pending` the root's slot 0, or ("pending_child") its first child; a `below_` damage pokes every child of the root.  MSUM:
    the damaged call is a SELECT of its own behind the move's first -- whose leaves are still pending -- with `msum_pokes`."""
    c = case(DAMAGE_CASE, L)
    p = DAMAGE_ROOT
    assert c.kinds[p] == "kept" and 0 < p < c.P - 1
    at, tensor, value = DAMAGE[name]
    at = at % len(c.seq)
    shp = shapes(c.P, c.N, c.C, L)
    was = before(c, at)
    k, fc = int(was["num_children"][p, 0]), int(was["first_child"][p, 0])
    if name == MSUM:
        assert c.seq[at - 1]["phases"] == BEGIN | SELECT
        seq = list(c.seq[:at]) + [gc.call(SELECT, pokes=msum_pokes(c, was, p), **c.key)]
        twin = run(c.state, c.C, c.K, c.n, c.Mc, L, c.rule, seq[:at] + [dict(seq[at], pokes=())])[-1]
        return c, at, seq, run(c.state, c.C, c.K, c.n, c.Mc, L, c.rule, seq), p, twin
    if name.startswith("below_"):
        pokes = tuple((tensor, pc.flat(shp[tensor], p, fc + j), int(value(c.N, k, c.C))) for j in range(k))
    else:
        index = (p * L,) if tensor == "selected" else (p,) if len(shp[tensor]) == 1 else (p, fc if name == "pending_child_int_max" else 0)
        pokes = ((tensor, pc.flat(shp[tensor], *index), int(value(c.N, k, c.C))),)
    seq = list(c.seq[:at]) + [dict(c.seq[at], pokes=pokes)]
    return c, at, seq, run(c.state, c.C, c.K, c.n, c.Mc, L, c.rule, seq), p, c.states[at]


# ---- a launch again, leaf by leaf, by the specification --------------------------------------------------------------------
def _t(a):
    return torch.from_numpy(np.array(a))  # a copy: the model's states are views of its output, which is not writable


def redo_select(c, q, was, st):
    """The SELECT of call q of case c redone from `st`'s tree (SELECT stores nothing to it but pending), every root at once:
    level 0 of every leaf by pcbenv/search.py:gumbel_select_root(full=True) on the counters as the leaves before left them, every
    other level -- and level 0 of a spent budget -- by gumbel_node_scores(pending=) on pending as the leaves before left it.
    Healthy trees only.  `was`: the state the call started from, for the counters and pending (zero behind an ABSORB); st: the
    state after it.  Checks selected, path_len, the path rows, pending, sim_index and sim_visits, and returns the facts of the
    launch: a Counter of what happened."""
    facts = collections.Counter()
    P, L, n, C, N = c.P, c.L, c.n, c.C, c.N
    tree = gc.tree_of(st)
    table = _t(c.table)
    begun, absorbed = q["phases"] & BEGIN, q["phases"] & ABSORB
    t = torch.zeros(P, dtype=torch.int32) if begun else _t(was["sim_index"]).to(torch.int32)
    sv = torch.zeros((P, C), dtype=torch.int32) if begun else _t(was["sim_visits"]).to(torch.int32)
    pending = torch.zeros((P, N), dtype=torch.int64) if absorbed else _t(was["pending"]).to(torch.int64).clone()
    rows = torch.arange(P)
    nch, fch, term = tree["num_children"].long(), tree["first_child"].long(), tree["terminal"] != 0
    halts = term[:, 0] | (nch[:, 0] == 0)
    alive = torch.ones(P, dtype=torch.bool)
    t0 = t.clone()
    for l in range(L):
        sel = gumbel_select_root(tree, t, sv, table, C, c.rule[1], c.rule[2], q["seed"], q["step_index"], q["first_root"], full=True)
        assert int(sel["errors"]) == 0
        sched = sel["scheduled"]
        if l > 0:
            ends = alive & (halts | ~sched)
            facts["budget_ends_inside"] += int((ends & ~halts & (t != t0)).sum())
            facts["one_leaf_only"] += int((ends & (halts | (t == t0))).sum())
            alive = alive & ~ends
        took = alive.clone()
        node, plen = torch.zeros(P, dtype=torch.int64), torch.zeros(P, dtype=torch.int64)
        undo = pending.clone()
        passed = []
        for d in range(T):
            stopped = ~took | term[rows, node] | (nch[rows, node] == 0)
            ns = gumbel_node_scores(tree, node, C, c.rule[1], c.rule[2], pending)
            assert bool((ns["ok"] | stopped).all())
            aware = torch.where(ns["mine"], ns["t"], torch.full_like(ns["t"], float("-inf"))).argmax(dim=1)
            blind_t = ns["pi"] - ns["n"].to(torch.float64) / (1.0 + ns["Nsum"].to(torch.float64))[:, None]
            blind = torch.where(ns["mine"], blind_t, torch.full_like(blind_t, float("-inf"))).argmax(dim=1)
            by_rule = ~stopped & ~(sched & (d == 0))
            facts["levels_by_the_rule"] += int(by_rule.sum())
            facts["pending_on_two_children"] += int((by_rule & ((ns["mine"] & (ns["m"] > ns["n"])).sum(dim=1) >= 2)).sum())
            facts["pending_changes_the_child"] += int((by_rule & (aware != blind)).sum())
            facts["spent_at_root"] += int((by_rule & (d == 0)).sum()) if d == 0 else 0
            nxt = fch[rows, node] + aware
            if d == 0:
                nxt = torch.where(sched, fch[:, 0] + sel["child"], nxt)
            go = ~stopped
            pending[rows[go], node[go]] += 1
            node = torch.where(go, nxt, node)
            passed.append(torch.where(go, node, torch.full_like(node, -1)))
            plen = plen + go.long()
        repeat = took & ~term[rows, node] & (nch[rows, node] == 0) & (pending[rows, node] > 0)
        pending[repeat] = undo[repeat]
        facts["repeat"] += int(repeat.sum())
        facts["repeat_behind_a_leaf"] += int(repeat.sum()) if l > 0 else 0
        alive = alive & ~repeat
        leaf = took & ~repeat
        pending[rows[leaf], node[leaf]] += 1
        keep = leaf & sched
        t, sv = torch.where(keep, sel["sim_index"], t), torch.where(keep[:, None], sel["sim_visits"], sv)
        facts["leaves"] += int(leaf.sum())
        facts["deeper"] += int((leaf & (plen >= 3)).sum())
        if l == L - 1:
            facts["all_leaves_taken"] += int(leaf.sum()) if L > 1 else 0
        for p in range(P):
            row = p * L + l
            taken = int(plen[p]) if took[p] else 0
            for lvl in range(taken):  # a repeat's own path rows hold what it passed
                assert (st["paths"][lvl, row] == st["node_action"][p, int(passed[lvl][p])]).all(), (p, l, lvl)
            assert (st["paths"][taken:, row] == was["paths"][taken:, row]).all(), (p, l)  # rows >= path_len and rows behind a -1 are untouched
            want = (int(node[p]), taken) if leaf[p] else (-1, -1)
            assert (int(st["selected"][row]), int(st["path_len"][row])) == want, (p, l, want)
    assert np.array_equal(st["pending"], pending.numpy()) and np.array_equal(st["sim_index"], t.numpy()) and np.array_equal(st["sim_visits"], sv.numpy())
    return facts


WANT = ("all_leaves_taken", "repeat", "repeat_behind_a_leaf", "budget_ends_inside", "one_leaf_only", "pending_on_two_children", "pending_changes_the_child",
        "spent_at_root", "deeper")


@functools.lru_cache(maxsize=None)
def case_facts(name, L):
    """The facts of every SELECT of a case, summed; every launch is held to the specification on the way."""
    c = case(name, L)
    total = collections.Counter()
    for i, (q, st) in enumerate(zip(c.seq, c.states)):
        assert not st["errors"] & ERR_TREE
        total["err_full"] += bool(st["errors"] & ERR_FULL)
        if q["phases"] & SELECT:
            total.update(redo_select(c, q, before(c, i), st))
    return total


def check_cases():
    """The table is what it is there for: every group width at every L, an L above G, roots across workgroups with a partly
    filled last group, ERR_FULL at every width, and on the model's states every branch of the rule -- so that the comparisons
    cannot pass on empty ground.  -> the facts of the launches with L > 1, summed."""
    cases = [case(name, L) for name, L in CASES]
    assert {c.G for c in cases} == {4, 8, 16, 32, 64} and {c.L for c in cases} == set(LEAVES) | {9} and any(c.L > c.G for c in cases)
    assert all(c.P > BLOCK // c.G and c.P % (BLOCK // c.G) for c in cases) and all(c.P == (131 if c.G == 4 else 67) for c in cases)
    assert all(set(gtc.ARMS) <= set(c.arms.values()) or c.C < 4 for c in cases)
    total, full = collections.Counter(), set()
    for c in cases:
        facts = case_facts(c.name, c.L)
        if c.L > 1:
            total.update(facts)
            if facts["err_full"]:
                full.add(c.name)
    assert full == set(gtc.CASES), set(gtc.CASES) - full
    missing = [f for f in WANT if total[f] <= 0]
    assert not missing, missing
    return total


# ---- one node, many descents: a launch worked out by hand, and the counts against the policy --------------------------------
def one_node_state(priors, L, P=2):
    """P roots, each with ONE child A (prior 1) and len(priors) terminal children under A with these priors; no visit below the
    root, reward_lo == reward_hi.  Every scheduled simulation goes root -> A -> a child of A by the node rule; a terminal node is
    no repeat.  node_action[.., 2] is the child's index."""
    k = len(priors)
    N = k + 2
    st = gc.init_state(P, N, k, T)
    st["num_children"][:, 0], st["first_child"][:, 0], st["num_children"][:, 1], st["first_child"][:, 1], st["num_nodes"][:] = 1, 1, k, 2, N
    st["visits"][:, 0], st["value_sum"][:, 0], st["value_max"][:, 0], st["reward_lo"][:], st["reward_hi"][:] = 1, 0.5, 0.5, 0.5, 0.5
    st["parent"][:, 1], st["depth"][:, 1], st["prior"][:, 1] = 0, 1, 1.0
    st["parent"][:, 2:], st["depth"][:, 2:], st["prior"][:, 2:], st["terminal"][:, 2:] = 1, 2, np.asarray(priors), 1
    st["node_action"][:, 1] = (1, 9, 0)
    st["node_action"][:, 2:, 2] = np.arange(k)
    st["node_action"][:, 2:, 1] = 20
    return with_leaves(st, P, N, L)


HAND = dict(priors=(0.5, 0.25, 0.125, 0.125), L=8, Mc=2, n=8, rule=(1.25, 50.0, 0.0))
# c_scale = 0: pi is the prior, to the last bits of ln and exp -- every comparison below has a margin of 0.04 or is a tie of two
# children with the same prior, hence the same bits.  With m the counts of A's children and M their sum, t = pi - m / (1 + M):
#   leaf 0  m = 0 0 0 0   t =  .5    .25   .125  .125   -> 0        leaf 4  m = 2 1 1 0   t =  .1    .05  -.075  .125   -> 3
#   leaf 1  m = 1 0 0 0   t =  0     .25   .125  .125   -> 1        leaf 5  m = 2 1 1 1   t =  .167  .083 -.042 -.042   -> 0
#   leaf 2  m = 1 1 0 0   t =  .167 -.083  .125  .125   -> 0        leaf 6  m = 3 1 1 1   t =  .071  .107 -.018 -.018   -> 1
#   leaf 3  m = 2 1 0 0   t =  0     0     .125  .125   -> 2 (tie)  leaf 7  m = 3 2 1 1   t =  .125  0     0     0      -> 0
# A rule that did not count pending visits would send all eight to child 0.
HAND_CHILDREN = (0, 1, 0, 2, 3, 0, 1, 0)


def check_hand(st, P=2):
    L, k = HAND["L"], len(HAND["priors"])
    assert st["errors"] == 0
    for p in range(P):
        rows = slice(p * L, (p + 1) * L)
        assert st["selected"][rows].tolist() == [2 + c for c in HAND_CHILDREN] and (st["path_len"][rows] == 2).all()
        assert (st["paths"][0, rows] == (1, 9, 0)).all() and st["paths"][1, rows, 2].tolist() == list(HAND_CHILDREN) and (st["paths"][2:, rows] == FILL).all()
        assert st["pending"][p].tolist() == [L, L] + [HAND_CHILDREN.count(c) for c in range(k)]
        assert st["sim_index"][p] == L and st["sim_visits"][p].tolist() == [L] + [0] * (k - 1)
