"""Witnesses of the score arithmetic of the search kernels (plain module, no test; needs no GPU).

The kernels, their CPU models and the torch specification are held together bit for bit, but on dyadic inputs a score
computed another way gives the same bits.  A WITNESS is a root with two contending children a < b whose scores nearly tie:
the documented arithmetic (`score`, `gumbel_score`: Python floats, one IEEE operation per written operator) goes to one of
them and a named wrong arithmetic -- a VARIANT, what a refactor or a build flag could make of the formula -- to the other.
All other children are far below both.  A kernel, a model or a specification that computes a variant selects another node
on its witnesses than the reference.

Variants (VARIANTS says which score each applies to):
  reciprocal_range      (mean - lo) * (1 / (hi - lo))                      puct, leaves, gumbel's completed_q
  reciprocal_mean       value_sum * (1 / n)                                puct, leaves, gumbel's completed_q
  reassociated_u        c_puct * (prior * root) / (1 + n)                  puct, leaves
  reassociated_u_ratio  (c_puct * prior) * (root / (1 + n))                puct, leaves
  heron_root            pcb_ieee::ieee_sqrt for the correctly rounded root puct, leaves (at parent counts where the two differ)
  fused                 one rounding of a * b + c (fractions.Fraction)     leaves: q * (visits / n_c) + u; gumbel: (g + logit) + s * qhat
  leaves_ratio          q * visits / n_c left to right                     leaves
  gumbel_reassociated   g + (logit + sigma)                                gumbel
"puct" is csrc/pcb_puct.h:puct_score, which pcbenv_puct_advance, the Gumbel kernel's levels below the root and its root
level once the budget is spent all call; "leaves" is csrc/pcb_puct_leaves.h:leaves_score with pending visits; "gumbel" is
csrc/pcb_gumbel.h:score at the root.

A TABLE is one hand-built state of P roots for one kernel and one group width: T = 2 levels, N = 1 + 2 C slots, the
smallest tree with a level below the root.  Root p holds witness p.  Its level is 0 (the contenders are root children) or
1 (they are the children of a root child that wins clearly); the pair sits at lanes PLACEMENTS of the width: (0, 1),
(0, k - 1), (k - 2, k - 1) and one pair (j, j + o) per butterfly stride o = 1 .. G / 2.  Widths: G = 4 (C = 3), 16, 64.
Leaves tables (L = 2 descents) preset `pending` by PENDING kind: none; on the node; on the node and both children;
"natural", what a first descent to a leaves (node 1, a 1) -- the one kind with pending that the specification, which
starts from nothing pending, reaches: as the second leaf of a launch.  All leaf nodes of a leaves table are terminal, so
that a descent to a node with a pending visit is no repeat.  Gumbel tables hold root-score witnesses (sim_index 0, every
sim_visits 0: both contenders stand at the considered count and at the most sim_visits, so the same pair decides SELECT's
node and CHOOSE's move_slot), PUCT witnesses at the root (sim_index == n) and PUCT witnesses at level 1.

The generator is seeded: per witness it draws non-dyadic lo < hi, visit counts, float32 priors and b's value_sum, solves
for the value_sum of a that equalises the two scores, and scans +-SCAN ulps of it for an ordering that differs.
`tables()` and the `choose_table`s take about MEASURED_SECONDS of one CPU together; both are cached per process."""
import functools
import math
import random
import time
from fractions import Fraction
from types import SimpleNamespace

import numpy as np
import torch

import gumbel_cases as gc
import puct_cases as pc
import puct_leaves_cases as lc
from pcbenv import search

MEASURED_SECONDS = 15  # tables() 5 s and the three choose_table() 8 to 11 s, one CPU (profiles/near_ties.txt)
FLOOR = 8              # witnesses per variant x kernel x level, and per lane placement of a table
SCAN = 100
T = 2
L = 2                  # descents per root of a leaves table
WIDTHS = {4: 3, 16: 16, 64: 64}  # G: C
C_PUCT = {4: 1.25, 16: 1.7, 64: 0.9}
KERNELS = ("puct", "leaves", "gumbel")
PUCT_VARIANTS = ("reciprocal_range", "reciprocal_mean", "reassociated_u", "reassociated_u_ratio", "heron_root")
LEAVES_VARIANTS = PUCT_VARIANTS + ("fused", "leaves_ratio")
GUMBEL_VARIANTS = ("reciprocal_range", "reciprocal_mean", "fused", "gumbel_reassociated")
VARIANTS = {"puct": PUCT_VARIANTS, "leaves": LEAVES_VARIANTS, "gumbel": GUMBEL_VARIANTS}
PENDING = {"none": (0, 0, 0), "node": (2, 0, 0), "both": (3, 1, 2), "natural": (1, 1, 0)}  # kind: pending of the node, of a, of b
NEEDS_CHILD_PENDING = ("fused", "leaves_ratio")  # the factor visits / n_c is exactly 1 without
# the Gumbel rule of the tables: non-dyadic, and a sigma small enough for the means to stay inside [lo, hi]
GUMBEL_N, GUMBEL_RULE = 4, (None, 20.0, 0.7)  # c_puct is the width's
GUMBEL_KEY = dict(seed=gc.SEED, step_index=(1 << 33) + 9, first_root=5)
# the prior of a child that is no contender (its one visit returned reward_lo, so q is 0): tiny for PUCT, and 0 under the
# Gumbel rule, whose logit is then ln 2^-149 = -103 -- no draw of g makes that up
FAR_PRIOR = {"puct": 2.0 ** -20, "leaves": 2.0 ** -20, "gumbel": 0.0}
GUMBEL_LEVELS = gc.T  # the rows of `paths` of a Gumbel table: what tests/test_gumbel_gpu.py's harness builds its request for


# ---- the reference arithmetic and its variants ------------------------------------------------------------------------
def heron(x):
    """csrc/pcb_ieee_math.h:ieee_sqrt."""
    m, e = math.frexp(x)
    if e & 1:
        m, e = 2.0 * m, e - 1
    y = 1.0
    for _ in range(6):
        y = 0.5 * (y + m / y)
    return y * 2.0 ** (e // 2)


HERON_COUNTS = tuple(n for n in range(1, 2000) if heron(float(n)) != math.sqrt(float(n)))  # parent counts whose root the two round differently


def fma(a, b, c):
    """a * b + c rounded once."""
    return float(Fraction(a) * Fraction(b) + Fraction(c))


def score(value_sum, visits, pending, prior, lo, hi, c_puct, visits_node, pending_node, variant=None):
    """csrc/pcb_puct_leaves.h:leaves_score -- csrc/pcb_puct.h:puct_score bit for bit with nothing pending -- or `variant` of it."""
    n_c = float(visits + pending)
    n_p = visits_node + pending_node
    root = (heron if variant == "heron_root" else math.sqrt)(float(n_p if n_p >= 1 else 1))
    if variant == "reassociated_u":
        u = c_puct * (prior * root) / (1.0 + n_c)
    elif variant == "reassociated_u_ratio":
        u = (c_puct * prior) * (root / (1.0 + n_c))
    else:
        u = c_puct * prior * root / (1.0 + n_c)
    if not (visits > 0 and hi > lo):
        return 0.0 + u
    mean = value_sum * (1.0 / float(visits)) if variant == "reciprocal_mean" else value_sum / float(visits)
    q = (mean - lo) * (1.0 / (hi - lo)) if variant == "reciprocal_range" else (mean - lo) / (hi - lo)
    if variant == "leaves_ratio":
        return q * float(visits) / n_c + u
    ratio = float(visits) / n_c
    return fma(q, ratio, u) if variant == "fused" else q * ratio + u


def completed_q(value_sum, visits, vbar, lo, hi, variant=None):
    """csrc/pcb_gumbel.h:completed_q."""
    if not hi > lo:
        return 0.0
    mean = vbar if visits <= 0 else value_sum * (1.0 / float(visits)) if variant == "reciprocal_mean" else value_sum / float(visits)
    return (mean - lo) * (1.0 / (hi - lo)) if variant == "reciprocal_range" else (mean - lo) / (hi - lo)


def sigma_scale(most_visits, c_visit, c_scale):
    return (c_visit + float(most_visits)) * c_scale


def gumbel_score(g, logit, qhat, scale, variant=None):
    """csrc/pcb_gumbel.h:score of sigma = scale * qhat.  -> (score, improved)."""
    if variant == "fused":
        return fma(scale, qhat, g + logit), fma(scale, qhat, logit)
    sg = scale * qhat
    return (g + (logit + sg) if variant == "gumbel_reassociated" else (g + logit) + sg), logit + sg


def first_max(scores):
    """csrc/pcb_tree.h:beats over the children in order: the first maximum."""
    return scores.index(max(scores))


# ---- one witness ------------------------------------------------------------------------------------------------------
def _near(x):
    """x and the floats within SCAN ulps of it, the nearest first."""
    ulp = math.ulp(x)
    return [x + s * k * ulp for k in range(SCAN + 1) for s in ((1,) if k == 0 else (1, -1))]


def _puct_duel(rng, variant, c_puct, pending):
    """-> dict(lo, hi, n_p, a, b, ref, var) or None: a, b = (value_sum, visits, prior); ref / var: 0 if a wins, 1 if b does."""
    pn, pa, pb = pending
    lo = rng.uniform(-5.0, -3.0)
    hi = lo + rng.uniform(0.3, 2.0)
    n_a, n_b = rng.randint(1, 40), rng.randint(1, 40)
    p_a, p_b = float(np.float32(rng.uniform(0.02, 0.6))), float(np.float32(rng.uniform(0.02, 0.6)))
    n_p = rng.choice(HERON_COUNTS) - pn if variant == "heron_root" else rng.randint(1, 1500)
    if n_p < 1:
        return None
    vs_b = (lo + (hi - lo) * rng.uniform(0.15, 0.85)) * n_b
    args = (lo, hi, c_puct, n_p, pn)
    s_b, s_b_var = score(vs_b, n_b, pb, p_b, *args), score(vs_b, n_b, pb, p_b, *args, variant)
    u_a = score(0.0, 0, pa + n_a, p_a, *args)  # the exploration term of a alone
    mean_a = (s_b - u_a) / (n_a / (n_a + pa)) * (hi - lo) + lo
    if not lo + 0.02 * (hi - lo) < mean_a < hi - 0.02 * (hi - lo):
        return None
    for vs_a in _near(mean_a * n_a):
        ref = int(not score(vs_a, n_a, pa, p_a, *args) >= s_b)
        var = int(not score(vs_a, n_a, pa, p_a, *args, variant) >= s_b_var)
        if ref != var:
            return dict(lo=lo, hi=hi, n_p=n_p, a=(vs_a, n_a, p_a), b=(vs_b, n_b, p_b), ref=ref, var=var)
    return None


def _gumbel_duel(rng, variant, g_a, g_b, c_visit, c_scale):
    """As _puct_duel for the root score of the Gumbel rule; a, b = (value_sum, visits, prior); vbar is not used: both have visits."""
    lo = rng.uniform(-5.0, -3.0)
    hi = lo + rng.uniform(0.3, 2.0)
    n_a, n_b = rng.randint(1, 40), rng.randint(1, 40)
    p_a, p_b = float(np.float32(rng.uniform(0.2, 0.5))), float(np.float32(rng.uniform(0.2, 0.5)))
    lg_a, lg_b = (float(x) for x in search.ieee_ln(torch.tensor([p_a, p_b], dtype=torch.float64)))
    scale = sigma_scale(max(n_a, n_b), c_visit, c_scale)
    vs_b = (lo + (hi - lo) * rng.uniform(0.15, 0.85)) * n_b
    s_b = gumbel_score(g_b, lg_b, completed_q(vs_b, n_b, 0.0, lo, hi), scale)[0]
    s_b_var = gumbel_score(g_b, lg_b, completed_q(vs_b, n_b, 0.0, lo, hi, variant), scale, variant)[0]
    mean_a = (s_b - (g_a + lg_a)) / scale * (hi - lo) + lo
    if not lo + 0.02 * (hi - lo) < mean_a < hi - 0.02 * (hi - lo):
        return None
    for vs_a in _near(mean_a * n_a):
        ref = int(not gumbel_score(g_a, lg_a, completed_q(vs_a, n_a, 0.0, lo, hi), scale)[0] >= s_b)
        var = int(not gumbel_score(g_a, lg_a, completed_q(vs_a, n_a, 0.0, lo, hi, variant), scale, variant)[0] >= s_b_var)
        if ref != var:
            return dict(lo=lo, hi=hi, n_p=1 + n_a + n_b, a=(vs_a, n_a, p_a), b=(vs_b, n_b, p_b), ref=ref, var=var)
    return None


def placements(G, k):
    """The lane pairs (a, b), a < b < k, of the width: the ends, and per butterfly stride o one pair of lanes that the
    shuffle of that stride exchanges."""
    out = [(0, 1), (0, k - 1), (k - 2, k - 1)]
    o = 1
    while o <= G // 2 and o < k:
        j = 2 * o if 3 * o < k else 0  # bit o of j is clear: lanes j and j + o = j ^ o are partners at stride o
        out.append((j, j + o))
        o *= 2
    return sorted(set(out))


# ---- the tables -------------------------------------------------------------------------------------------------------
def _empty(P, N, C):
    i32 = lambda shape, v: np.full(shape, v, np.int32)
    return dict(num_nodes=i32(P, 1), parent=i32((P, N), -1), depth=i32((P, N), 0), visits=i32((P, N), 0), num_children=i32((P, N), 0),
                first_child=i32((P, N), -1), node_action=i32((P, N, 3), 0), prior=np.zeros((P, N)), value_sum=np.zeros((P, N)),
                value_max=np.full((P, N), -np.inf), terminal=np.zeros((P, N), np.uint8), reward_lo=np.zeros(P), reward_hi=np.zeros(P),
                pending=i32((P, N), 0))


def _children(st, p, node, first, k, lo, far):
    """k children of `node` in the slots from `first` on, none a contender yet: one visit that returned reward_lo, a tiny prior."""
    st["first_child"][p, node], st["num_children"][p, node], st["num_nodes"][p] = first, k, first + k
    for c in range(k):
        s = first + c
        st["parent"][p, s], st["depth"][p, s], st["node_action"][p, s] = node, st["depth"][p, node] + 1, (s % 2, 0, s)
        st["prior"][p, s], st["visits"][p, s], st["value_sum"][p, s], st["value_max"][p, s] = far, 1, lo, lo


def _contender(st, p, slot, child):
    vs, n, prior = child
    st["value_sum"][p, slot], st["visits"][p, slot], st["prior"][p, slot], st["value_max"][p, slot] = vs, n, prior, st["reward_hi"][p]


def _plan(kernel):
    """The (score, variant, level) of the roots of a table, FLOOR of each in a row.  score: "puct", "leaves" or "gumbel"."""
    if kernel == "gumbel":
        plan = [("gumbel", v, 0) for v in GUMBEL_VARIANTS] + [("puct", v, lv) for v in PUCT_VARIANTS for lv in (0, 1)]
    else:
        plan = [(kernel, v, lv) for v in VARIANTS[kernel] for lv in (0, 1)]
    return [row for row in plan for _ in range(FLOOR)]


@functools.lru_cache(maxsize=None)
def table(kernel, G):
    """-> SimpleNamespace(kernel, G, C, P, N, c_puct, state, rows, ...): the hand-built state (numpy, the fields of
    puct_leaves_cases.STATE_FIELDS' tree and pending; for gumbel also sim_index, sim_visits) and per root the witness:
    dict(score, variant, level, lanes, pending, kind, node, slots, ref, var) -- ref / var: the slot the reference / the variant selects."""
    C, c_puct = WIDTHS[G], C_PUCT[G]
    plan = _plan(kernel)
    P, N, k = len(plan), 1 + 2 * C, C
    rng = random.Random(f"near ties {kernel} {G}")
    st = _empty(P, N, C)
    lanes = placements(G, k)
    kinds = list(PENDING)
    rule = (c_puct,) + GUMBEL_RULE[1:]
    g = None
    if kernel == "gumbel":
        dummy = {f: torch.from_numpy(st[f]) for f in ("num_children", "first_child", "visits", "prior", "value_sum", "reward_lo", "reward_hi")}
        g = search.gumbel_scores(dummy, C, rule[1], rule[2], **GUMBEL_KEY)["g"].numpy()  # the draws depend on the key alone
        st.update(sim_index=np.zeros(P, np.int32), sim_visits=np.zeros((P, C), np.int32))
    rows, tries = [], 0
    for p, (what, variant, level) in enumerate(plan):
        a, b = lanes[p % len(lanes)]
        kind = "none"
        if what == "leaves":
            kind = kinds[(p // 3) % len(kinds)]
            if variant in NEEDS_CHILD_PENDING and kind in ("none", "node"):
                kind = ("both", "natural")[p % 2]
        pending = PENDING[kind]
        while True:
            tries += 1
            assert tries < 400000, (kernel, G, what, variant, level)
            duel = _gumbel_duel(rng, variant, float(g[p, a]), float(g[p, b]), rule[1], rule[2]) if what == "gumbel" else \
                _puct_duel(rng, variant, c_puct, pending)
            if duel is not None:
                break
        lo, hi = duel["lo"], duel["hi"]
        st["reward_lo"][p], st["reward_hi"][p] = lo, hi
        _children(st, p, 0, 1, k, lo, FAR_PRIOR[kernel])
        node = 0
        if level == 1:  # the contenders' parent is a root child that wins clearly: the highest prior there is and the highest mean
            node = 1 + (a + b) % k
            _children(st, p, node, 1 + C, k, lo, FAR_PRIOR[kernel])
            st["prior"][p, node], st["visits"][p, node], st["value_sum"][p, node], st["value_max"][p, node] = 1.0, duel["n_p"], hi * duel["n_p"], hi
            st["visits"][p, 0], st["value_sum"][p, 0] = duel["n_p"] + k, hi * duel["n_p"] + lo * (k - 1)
        else:
            st["visits"][p, 0], st["value_sum"][p, 0] = duel["n_p"], lo * (k - 2) + duel["a"][0] + duel["b"][0]
        st["value_max"][p, 0] = hi
        fc = int(st["first_child"][p, node])
        _contender(st, p, fc + a, duel["a"])
        _contender(st, p, fc + b, duel["b"])
        if what == "leaves":
            st["pending"][p, node], st["pending"][p, fc + a], st["pending"][p, fc + b] = pending
            if level == 1:
                st["pending"][p, 0] = pending[0]
        if kernel == "leaves":  # a descent to a leaf with a pending visit is a repeat unless the leaf is terminal
            for s in range(1, int(st["num_nodes"][p])):
                st["terminal"][p, s] = st["num_children"][p, s] == 0
        if kernel == "gumbel":  # the root level is the rule's while sim_index < n
            st["sim_index"][p] = GUMBEL_N if (what, level) == ("puct", 0) else 0
        rows.append(dict(score=what, variant=variant, level=level, lanes=(a, b), kind=kind, pending=pending, node=node, slots=(fc + a, fc + b),
                         ref=fc + (a, b)[duel["ref"]], var=fc + (a, b)[duel["var"]]))
    return SimpleNamespace(kernel=kernel, G=G, C=C, P=P, N=N, K=C, T=T, L=L if kernel == "leaves" else 1, c_puct=c_puct, rule=rule, n=GUMBEL_N,
                           Mc=min(C, 16), state=st, rows=rows, tries=tries)


def tree_of(t, pending=False):
    """The tree of a table as the dict the specification and the models' `load` take (torch)."""
    d = {f: torch.from_numpy(np.array(t.state[f])) for f in pc.TREE_FIELDS}
    if pending:
        d["pending"] = torch.from_numpy(np.array(t.state["pending"]))
    return d


@functools.lru_cache(maxsize=None)
def gumbel_quantities(G):
    """pcbenv/search.py:gumbel_scores of the Gumbel table of width G: g and logit are taken from there."""
    t = table("gumbel", G)
    return search.gumbel_scores(tree_of(t), t.C, t.rule[1], t.rule[2], **GUMBEL_KEY)


def reference_choice(t, p, variant=None):
    """The slot root p's witness level selects in the first descent, recomputed from the state of the table alone: by the
    reference arithmetic, or by `variant`."""
    st, row = t.state, t.rows[p]
    node = row["node"]
    fc, k = int(st["first_child"][p, node]), int(st["num_children"][p, node])
    lo, hi = float(st["reward_lo"][p]), float(st["reward_hi"][p])
    ch = range(fc, fc + k)
    if row["score"] == "gumbel":
        g = gumbel_quantities(t.G)
        scale = sigma_scale(max(int(st["visits"][p, s]) for s in ch), t.rule[1], t.rule[2])
        vbar = float(st["value_sum"][p, 0]) / float(st["visits"][p, 0])
        sc = [gumbel_score(float(g["g"][p, c]), float(g["logit"][p, c]),
                           completed_q(float(st["value_sum"][p, s]), int(st["visits"][p, s]), vbar, lo, hi, variant), scale, variant)[0]
              for c, s in enumerate(ch)]
    else:
        sc = [score(float(st["value_sum"][p, s]), int(st["visits"][p, s]), int(st["pending"][p, s]), float(st["prior"][p, s]), lo, hi, t.c_puct,
                    int(st["visits"][p, node]), int(st["pending"][p, node]), variant) for s in ch]
    return fc + first_max(sc), sc


# ---- the calls on a table, and the models' states after them -----------------------------------------------------------
def evaluation(t, selected):
    """The scripted evaluation of the nodes `selected` [rows] (the model's first SELECT): a real value around the root's range,
    a little outside it now and then, K = C candidates with hashed float32 priors; terminal at depth T.  A row that is no
    leaf (-1) gets NaN and a count far out of range: it is not read."""
    rows = len(selected)
    per = rows // t.P
    rng = random.Random(f"evaluation {t.kernel} {t.G}")
    value, over, count = np.zeros(rows), np.zeros(rows, np.uint8), np.full(rows, t.K, np.int32)
    actions, prior = np.zeros((rows, t.K, 3), np.int32), np.zeros((rows, t.K), np.float32)
    for r in range(rows):
        p, s = r // per, int(selected[r])
        lo, hi = float(t.state["reward_lo"][p]), float(t.state["reward_hi"][p])
        value[r] = lo + (hi - lo) * rng.uniform(-0.2, 1.2)
        for c in range(t.K):
            actions[r, c], prior[r, c] = (c % 2, 1, c), rng.uniform(0.0, 0.5)
        if s < 0:
            value[r], count[r] = np.nan, t.K + 1000
        else:
            over[r] = t.state["depth"][p, s] >= T or bool(t.state["terminal"][p, s])
    return value, over, count, actions, prior


def _pending_pokes(t):
    shp = lc.shapes(t.P, t.N, T, t.L)["pending"]
    return [("pending", lc.flat(shp, int(p), int(s)), int(t.state["pending"][p, s])) for p, s in zip(*np.nonzero(t.state["pending"]))]


@functools.lru_cache(maxsize=None)
def puct_calls(kernel, G):
    """-> (table, seq, states): SELECT on the loaded table, then ABSORB | SELECT with `evaluation`; the states are those of
    tools/puct_leaves_check.cpp -- through csrc/pcb_puct.h for "puct", through csrc/pcb_puct_leaves.h with the table's pending
    for "leaves"."""
    t = table(kernel, G)
    first = dict(phases=pc.SELECT, load=tree_of(t), expect=None, evaluation=None)
    if kernel == "leaves":
        first["pokes"] = _pending_pokes(t)
    run = lambda seq: lc.replay(t.P, t.N, t.C, T, t.K, t.L, t.c_puct, seq, via=int(kernel == "puct"))
    selected = run([first])[0]["selected"]
    seq = [first, dict(phases=pc.ABSORB | pc.SELECT, evaluation=evaluation(t, selected), expect=None)]
    return t, seq, run(seq)


def gumbel_state(t):
    P, C = t.P, t.C
    st = {f: t.state[f] for f in pc.TREE_FIELDS + ("sim_index", "sim_visits")}
    st.update(selected=np.full(P, gc.FILL, np.int32), path_len=np.full(P, gc.FILL, np.int32), paths=np.full((GUMBEL_LEVELS, P, 3), gc.FILL, np.int32))
    return st


@functools.lru_cache(maxsize=None)
def gumbel_calls(G):
    """-> (case, seq, states) as tests/test_gumbel_gpu.py's harness takes them: CHOOSE on the table (it stores to no state),
    SELECT, then ABSORB | SELECT with `evaluation`; the states are tools/gumbel_check.cpp's."""
    t = table("gumbel", G)
    st = gumbel_state(t)
    key = GUMBEL_KEY
    head = [gc.call(gc.CHOOSE, **key), gc.call(gc.SELECT, **key)]
    run = lambda seq: gc.run(st, t.C, t.K, t.n, t.Mc, t.rule, seq, levels=GUMBEL_LEVELS)
    selected = run(head)[1]["selected"]
    seq = head + [gc.call(gc.ABSORB | gc.SELECT, evaluation(t, selected), **key)]
    case = SimpleNamespace(P=t.P, N=t.N, C=t.C, K=t.K, n=t.n, Mc=t.Mc, rule=t.rule, state=st, table=search.considered_visits(t.Mc, t.n).numpy(), T=T)
    return case, seq, run(seq)


# ---- what the tables are there for -------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def tables():
    """Every table, and the seconds their generation took."""
    t0 = time.perf_counter()
    out = {(kernel, G): table(kernel, G) for kernel in KERNELS for G in WIDTHS}
    return out, time.perf_counter() - t0


def counts():
    """-> {(kernel, score, variant, level): witnesses}, {(kernel, G, lanes): witnesses}, {(variant-needing-pending kind ...)}."""
    by_variant, by_lanes, by_kind = {}, {}, {}
    for (kernel, G), t in tables()[0].items():
        for row in t.rows:
            for d, key in ((by_variant, (kernel, row["score"], row["variant"], row["level"])), (by_lanes, (kernel, G, row["lanes"])),
                           (by_kind, (kernel, row["kind"]))):
                d[key] = d.get(key, 0) + 1
    return by_variant, by_lanes, by_kind


@functools.lru_cache(maxsize=None)
def check_cases():
    """From the tables alone: every variant x kernel x level it applies to and every lane placement of every width has FLOOR
    witnesses; every pending kind occurs; the heron witnesses stand at counts whose roots differ; a table of G = 4 spans
    workgroups; no NaN and nothing infinite but value_max of an unused slot.  -> the tables."""
    all_tables, seconds = tables()
    by_variant, by_lanes, by_kind = counts()
    for kernel in ("puct", "leaves"):
        for v in VARIANTS[kernel]:
            for level in (0, 1):
                assert by_variant.get((kernel, kernel, v, level), 0) >= FLOOR, (kernel, v, level)
    for v in GUMBEL_VARIANTS:
        assert by_variant.get(("gumbel", "gumbel", v, 0), 0) >= FLOOR, v
    for v in PUCT_VARIANTS:  # the Gumbel kernel's PUCT levels: the root once the budget is spent, and below the root
        for level in (0, 1):
            assert by_variant.get(("gumbel", "puct", v, level), 0) >= FLOOR, (v, level)
    for (kernel, G), t in all_tables.items():
        for lanes in placements(G, t.C):
            assert by_lanes.get((kernel, G, lanes), 0) >= FLOOR, (kernel, G, lanes)
        strides = {b - a for a, b in placements(G, t.C)}
        assert all(o in strides for o in (1, 2, 4, 8, 16, 32) if o <= G // 2 and o < t.C), (G, strides)
        assert pc.group_lanes(t.C) == G and (G != 4 or t.P > pc.BLOCK // G)
        for f, a in t.state.items():
            if a.dtype.kind == "f":
                assert not np.isnan(a).any(), (kernel, G, f)
                assert f == "value_max" or np.isfinite(a).all(), (kernel, G, f)
        for p, row in enumerate(t.rows):
            assert row["ref"] != row["var"] and {row["ref"], row["var"]} == set(row["slots"]), (kernel, G, p)
            lo, hi = t.state["reward_lo"][p], t.state["reward_hi"][p]
            for s in row["slots"]:
                assert lo <= t.state["value_sum"][p, s] / t.state["visits"][p, s] <= hi, (kernel, G, p)
            if row["variant"] == "heron_root":
                assert int(t.state["visits"][p, row["node"]]) + int(t.state["pending"][p, row["node"]]) in HERON_COUNTS, (kernel, G, p)
            if row["variant"] in NEEDS_CHILD_PENDING and row["score"] == "leaves":
                assert row["pending"][1] or row["pending"][2]
    for kind in PENDING:
        assert by_kind.get(("leaves", kind), 0) >= FLOOR, kind
    return all_tables


# ---- recorded searches on real-valued evaluations ----------------------------------------------------------------------
# tests/puct_cases.py:real_evaluator in the place of synthetic_evaluator: the recorded searches of the three kernels on
# values whose sums depend on the order of the additions, ranges that are no power of two and priors that are a softmax.
REAL_C_PUCT, REAL_SEED = 1.7, 41
REAL_PUCT = {  # name: (P, T, C, K, iterations, capacity)
    "G4_C4_P130": (130, 5, 4, 4, 10, None),   # three workgroups of 64 roots
    "G64_C64_P5": (5, 5, 64, 64, 8, None),    # one root of every kind of value
    "deep_P4_C4": (4, 8, 4, 4, 400, 128),     # root visit counts in the hundreds: root_of and 1 + n_c far from the 1 .. 14 of the others
}
REAL_LEAVES = {"C5_L3": (10, 5, 5, 5, 3, 6), "C64_L8": (5, 5, 64, 64, 8, 4)}  # name: (P, T, C, K, L, iterations)
REAL_GUMBEL = ("G4_C3_P131", "G64_C64_P67")  # rows of gumbel_cases.CASES: their shapes, rules and keys
DEEP_VISITS = 300


@functools.lru_cache(maxsize=None)
def real_puct(name):
    """-> a case as puct_cases.synthetic makes them: the recorded search and the model's replay of it."""
    P, T_, C, K, iterations, capacity = REAL_PUCT[name]
    ps, calls = pc.record(P, T_, iterations, REAL_C_PUCT, C, pc.real_evaluator(P, T_, K, REAL_SEED), step_index=100, capacity=capacity)
    N = 1 + iterations * C if capacity is None else capacity
    seq = pc.search_calls(calls)
    return SimpleNamespace(P=P, N=N, C=C, T=T_, K=K, c_puct=REAL_C_PUCT, ps=ps, seq=seq, states=pc.replay(P, N, C, T_, K, REAL_C_PUCT, seq))


@functools.lru_cache(maxsize=None)
def real_leaves(name):
    """-> a case as puct_leaves_cases.synthetic makes them."""
    P, T_, C, K, L_, iterations = REAL_LEAVES[name]
    N = 1 + 40 * C
    ps, calls = lc.record(P, T_, L_, iterations, REAL_C_PUCT, C, lc.per_leaf(pc.real_evaluator(P, T_, K, REAL_SEED), P, T_, K, L_), step_index=100, capacity=N)
    seq = pc.search_calls(calls)
    return SimpleNamespace(P=P, N=N, C=C, T=T_, K=K, L=L_, c_puct=REAL_C_PUCT, ps=ps, calls=calls, seq=seq,
                           states=lc.replay(P, N, C, T_, K, L_, REAL_C_PUCT, seq))


@functools.lru_cache(maxsize=None)
def real_gumbel(name):
    """-> (case, seq, states, gs, calls): gumbel_search recorded at the shape of gumbel_cases.CASES[name], the calls of
    gumbel_cases.search_calls and tools/gumbel_check.cpp's states after them; `case` as tests/test_gumbel_gpu.py's harness takes it."""
    C, P, Mc, n, c_visit, c_scale, first_root, step_index = gc.CASES[name]
    K, levels = C, gc.T
    N = 1 + (n + 1) * C
    rule, key = (REAL_C_PUCT, c_visit, c_scale), dict(seed=gc.SEED ^ 9, step_index=step_index, first_root=first_root)
    gs, calls = gc.record_search(P, levels, n, Mc, C, pc.real_evaluator(P, levels, K, REAL_SEED), rule, key, capacity=N)
    seq = gc.search_calls(calls, key)
    start = gc.init_state(P, N, C, levels)
    case = SimpleNamespace(P=P, N=N, C=C, K=K, n=n, Mc=Mc, rule=rule, state=start, table=search.considered_visits(Mc, n).numpy(), T=levels)
    return case, seq, gc.run(start, C, K, n, Mc, rule, seq, levels=levels), gs, calls


# ---- witnesses of CHOOSE's outputs -------------------------------------------------------------------------------------
# A second kind of witness: a root on which some child_weights integer or child_policy float32 differs between the reference
# and a variant of the softmax.  They do not occur by chance: one child's value_sum is bisected until its pi * 2^24 sits at
# an integer plus one half ("weights") or its pi at the boundary between two float32 ("policy"), then its ulps are scanned.
#   z_butterfly   Z summed pairwise in the order of a shuffle butterfly over the G lanes, not child after child
#   reciprocal_z  e * (1 / Z)
#   fused         logit + scale * qhat of `improved` rounded once
CHOOSE_VARIANTS = ("z_butterfly", "reciprocal_z", "fused")
CHOOSE_KINDS = ("weights", "policy")
CHOOSE_PER_WIDTH = 3       # of every variant x kind: 9 over the three widths
CHOOSE_RULE = (None, 0.5, 0.05)  # a sigma so small that one ulp of a value_sum moves pi by about one ulp


def exp_of(x):
    """pcbenv/search.py:ieee_exp in Python floats, -708 <= x <= 0 (check_cases holds the two together)."""
    kf = float(int(x * search._LOG2_E - 0.5))
    r = (x - kf * search._LN2_HI) - kf * search._LN2_LO
    p = (1.0 / 6227020800.0) * r + 1.0 / 479001600.0
    for f in (39916800.0, 3628800.0, 362880.0, 40320.0, 5040.0, 720.0, 120.0, 24.0, 6.0, 2.0, 1.0, 1.0):
        p = p * r + 1.0 / f
    return p * 2.0 ** int(kf)


def policy_of(x, G, variant=None):
    """csrc/pcb_gumbel.h:gumbel_choose's target of the improved logits x [k] -> (child_weights [k], child_policy [k] float32)."""
    mx = max(x)
    e = [exp_of(v - mx) for v in x]
    if variant == "z_butterfly":
        v, o = e + [0.0] * (G - len(e)), G // 2
        while o:
            v, o = [v[i] + v[i ^ o] for i in range(G)], o // 2
        Z = v[0]
    else:
        Z = 0.0
        for v in e:
            Z = Z + v
    pi = [v * (1.0 / Z) for v in e] if variant == "reciprocal_z" else [v / Z for v in e]
    return [int(p * 16777216.0 + 0.5) for p in pi], [np.float32(p) for p in pi]


def improved_of(logit, qhat, scale, variant=None):
    return fma(scale, qhat, logit) if variant == "fused" else logit + scale * qhat


def _choose_root(rng, G, k, variant, kind, c_visit, c_scale):
    """-> dict(lo, hi, children [(value_sum, visits, prior)]) or None: a root whose outputs of `kind` differ under `variant`."""
    lo = rng.uniform(-5.0, -3.0)
    hi = lo + rng.uniform(0.3, 2.0)
    ch = [[(lo + (hi - lo) * rng.uniform(0.1, 0.9)) * n, n, float(np.float32(rng.uniform(0.02, 0.5)))] for n in (rng.randint(1, 3) for _ in range(k))]
    logit = [float(v) for v in search.ieee_ln(torch.tensor([c[2] for c in ch], dtype=torch.float64))]
    scale = sigma_scale(max(c[1] for c in ch), c_visit, c_scale)
    x_of = lambda vs, n, j, var: improved_of(logit[j], completed_q(vs, n, 0.0, lo, hi), scale, var)
    x = [x_of(c[0], c[1], j, None) for j, c in enumerate(ch)]
    j = rng.choice([i for i in range(k) if x[i] < max(x)])  # the child that is moved is not the largest: the others' e stay

    def outputs(vs, var):
        xs = [x_of(c[0], c[1], i, var) for i, c in enumerate(ch)] if var == "fused" else list(x)
        xs[j] = x_of(vs, ch[j][1], j, var)
        return policy_of(xs, G, var)
    w, p32 = outputs(ch[j][0], None)
    # the boundary above the present value, as a predicate that is monotone in the value_sum
    if kind == "weights":
        above = lambda vs: outputs(vs, None)[0][j] > w[j]
    else:
        above = lambda vs: outputs(vs, None)[1][j] > p32[j]
    a, b = ch[j][0], hi * ch[j][1]
    if not above(b) or above(a):
        return None
    while True:
        mid = a + (b - a) / 2.0
        if mid <= a or mid >= b:
            break
        a, b = (a, mid) if above(mid) else (mid, b)
    for vs in _near(b):
        if not lo * ch[j][1] <= vs <= hi * ch[j][1] or x_of(vs, ch[j][1], j, None) >= max(x):
            continue
        ref, var = outputs(vs, None), outputs(vs, variant)
        differs = ref[0] != var[0] if kind == "weights" else [float(v) for v in ref[1]] != [float(v) for v in var[1]]
        if differs:
            ch[j][0] = vs
            return dict(lo=lo, hi=hi, children=[tuple(c) for c in ch])
    return None


@functools.lru_cache(maxsize=None)
def choose_table(G):
    """-> SimpleNamespace as `table`: roots whose k = C children all take part in the softmax; rows: dict(variant, kind)."""
    C, c_puct = WIDTHS[G], C_PUCT[G]
    plan = [(v, kind) for v in CHOOSE_VARIANTS for kind in CHOOSE_KINDS for _ in range(CHOOSE_PER_WIDTH)]
    P, N, k = len(plan), 1 + C, C
    rng = random.Random(f"near ties choose {G}")
    st = _empty(P, N, C)
    st.update(sim_index=np.zeros(P, np.int32), sim_visits=np.zeros((P, C), np.int32))
    rule = (c_puct,) + CHOOSE_RULE[1:]
    rows, tries = [], 0
    for p, (variant, kind) in enumerate(plan):
        while True:
            tries += 1
            assert tries < 20000, (G, variant, kind)
            root = _choose_root(rng, G, k, variant, kind, rule[1], rule[2])
            if root is not None:
                break
        st["reward_lo"][p], st["reward_hi"][p] = root["lo"], root["hi"]
        _children(st, p, 0, 1, k, root["lo"], 0.0)
        for c, child in enumerate(root["children"]):
            _contender(st, p, 1 + c, child)
        st["visits"][p, 0] = 1 + sum(c[1] for c in root["children"])
        st["value_sum"][p, 0], st["value_max"][p, 0] = root["lo"] + sum(c[0] for c in root["children"]), root["hi"]
        rows.append(dict(variant=variant, kind=kind))
    return SimpleNamespace(kernel="gumbel", G=G, C=C, P=P, N=N, K=C, T=T, L=1, c_puct=c_puct, rule=rule, n=GUMBEL_N, Mc=min(C, 16), state=st, rows=rows,
                           tries=tries)


@functools.lru_cache(maxsize=None)
def _choose_quantities(G):
    t = choose_table(G)
    return search.gumbel_scores(tree_of(t), t.C, t.rule[1], t.rule[2], **GUMBEL_KEY)


def choose_outputs(t, p, variant=None):
    """(child_weights, child_policy) of root p of a choose_table, recomputed from its state alone: g plays no part, the
    logit is pcbenv/search.py:gumbel_scores'."""
    st = t.state
    sc = _choose_quantities(t.G)
    lo, hi = float(st["reward_lo"][p]), float(st["reward_hi"][p])
    ch = range(1, 1 + t.C)
    scale = sigma_scale(max(int(st["visits"][p, s]) for s in ch), t.rule[1], t.rule[2])
    x = [improved_of(float(sc["logit"][p, c]), completed_q(float(st["value_sum"][p, s]), int(st["visits"][p, s]), 0.0, lo, hi), scale, variant)
         for c, s in enumerate(ch)]
    return policy_of(x, t.G, variant)


@functools.lru_cache(maxsize=None)
def choose_calls(G):
    """-> (case, seq, states): CHOOSE on the table, as gumbel_calls."""
    t = choose_table(G)
    st = gumbel_state(t)
    seq = [gc.call(gc.CHOOSE, **GUMBEL_KEY)]
    case = SimpleNamespace(P=t.P, N=t.N, C=t.C, K=t.K, n=t.n, Mc=t.Mc, rule=t.rule, state=st, table=search.considered_visits(t.Mc, t.n).numpy(), T=T)
    return case, seq, gc.run(st, t.C, t.K, t.n, t.Mc, t.rule, seq, levels=GUMBEL_LEVELS)


@functools.lru_cache(maxsize=None)
def check_choose_cases():
    """FLOOR roots of every variant x kind over the widths; exp_of is pcbenv/search.py:ieee_exp; no NaN.  -> the tables."""
    out = {G: choose_table(G) for G in WIDTHS}
    count = {}
    for t in out.values():
        for row in t.rows:
            count[(row["variant"], row["kind"])] = count.get((row["variant"], row["kind"]), 0) + 1
        assert not any(np.isnan(a).any() for a in t.state.values() if a.dtype.kind == "f")
    for v in CHOOSE_VARIANTS:
        for kind in CHOOSE_KINDS:
            assert count.get((v, kind), 0) >= FLOOR, (v, kind)
    xs = [-700.0 * random.Random(7).random() ** 4 for _ in range(500)] + [0.0, -1e-300, -708.0]
    assert [exp_of(x) for x in xs] == search.ieee_exp(torch.tensor(xs, dtype=torch.float64)).tolist()
    return out
