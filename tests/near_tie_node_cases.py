"""Witnesses of the arithmetic of the Gumbel node rule and of the leaf kernels' root scores: tests/near_tie_cases.py's method
for pcbenv_gumbel_tree_advance, pcbenv_gumbel_tree_advance_leaves and pcbenv_gumbel_advance_leaves (plain module, no test;
needs no GPU).

`node_rule` restates csrc/pcb_gumbel_tree.h:node_logits + node_policy + excess, and csrc/pcb_gumbel_tree_leaves.h:excess
with pending visits, in Python floats, one IEEE operation per written operator; `variant=` names a wrong arithmetic:
  s_butterfly, wv_butterfly, qv_butterfly  that sum formed pairwise in the order of a shuffle butterfly over the G lanes
  qv_fused              Qv = fma(pr, q, Qv)                       vmix_fused         fma(Nsum / Wv, Qv, vhat)
  vmix_reassociated     (Nsum * Qv) / Wv                          reciprocal_range   (m - lo) * (1 / (hi - lo)) in `completed`
  reciprocal_mean       value_sum * (1 / n) wherever q_c is formed  fused            improved = fma(scale, qhat, logit)
  z_butterfly           Z in butterfly order                      reciprocal_z       e * (1 / Z)
  reciprocal_excess     m_c * (1 / (1 + Msum))
  pending_not_in_msum   m_c / (1 + Nsum)                          pending_in_sigma   max_b (n_b + pn_b) in sigma's scale
A WITNESS is a node with two contending children a < b: the reference goes to one of them and the variant to the other, and
every other child stands at least MARGIN below both in t.  The six variants that act through vmix (VMIX_VARIANTS) reach t only
through a child without a visit: on their witnesses n_a = 0.  For the three butterflies and qv_fused at least three other
children hold visits, non-dyadic value sums and float32 priors of 1e-3 to 1e-2, which enter Wv.  At G = 4 (k = 3) there is
one other child: with a unvisited the sums S, Wv and Qv have two addends that are not 0.0 and every order gives the same bits,
and qv_fused cannot have its three visited others -- NO_WITNESS_AT_K3 have no witness there and take their floor over G = 16
and 64.  Float32 priors between 1e-3 and 1 add up exactly in float64 in every order (24 bits each, within 2^-33 .. 1), so
wv_butterfly has no witness on them at any width: its witnesses carry priors of all 53 bits on the other children, which is what
pcbenv_puct_root_noise leaves on a root's children -- the node of a spent budget.

The generator is seeded.  Per witness it draws the range, the other children, the contenders' counts and a's prior, solves
b's prior for a tie at the middle of b's range, bisects b's value_sum until t_a - t_b changes sign and scans +-SCAN ulps of
it for a value on which reference and variant part.

Tables, one state of P roots per width G = 4 (C = 3), 16, 64, T = 2 levels, N = 1 + 2 C slots, root p holding witness p at the
lanes nt.placements(G, k)[p % ..]; every leaf is terminal, so no descent of a leaves launch is a repeat:
  node_table(G)     the twelve NODE_VARIANTS without pending at level 1 -- the node is a root child that the schedule takes
                    clearly (prior 1 against 0, sim_index 0) -- and at level 0 with the budget spent (sim_index == n).  It
                    serves k_gumbel_tree and, with L = 2 and nothing pending, k_gumbel_tree_leaves.
  pending_table(G)  PENDING_VARIANTS on preset pending visits of nt.PENDING's kinds and on "launched" roots: nothing is preset,
                    both leaves of the launch go to the node (every other root child stands at a count the schedule does not
                    consider), the first goes clearly to a, and the second meets the tie with a's pending visit: the reference
                    then goes to b, where the rule without the pending visit would go to a again.  k_gumbel_tree_leaves only.
  choose_table(G)   CHOOSE witnesses (nt.choose_table's kinds "weights" and "policy") of qv_butterfly and vmix_fused on roots some
                    of whose children have no visit.
The root-score witnesses of the leaf kernels are nt.table("gumbel", G)'s and nt.table("leaves", G)'s: see `gumbel_rows_calls`.
`tables()` takes about MEASURED_SECONDS of one CPU; it is cached per process."""
import functools
import math
import random
import time
from types import SimpleNamespace

import numpy as np
import torch

import gumbel_cases as gc
import gumbel_leaves_cases as glc
import gumbel_tree_cases as gtc
import gumbel_tree_leaves_cases as gtl
import near_tie_cases as nt
import puct_cases as pc
import puct_leaves_cases as lc
from pcbenv import search

MEASURED_SECONDS = 28  # node 10 s, pending 8 s, choose 2 s, root 5 s and the checks, one CPU; G = 64 takes four fifths (profiles/near_ties_node_rule.txt)
FLOOR = nt.FLOOR       # witnesses per variant x level x kernel, summed over the widths
SCAN = 40
MARGIN = 1e-3
T, L = nt.T, nt.L
WIDTHS, C_PUCT = nt.WIDTHS, nt.C_PUCT
N_SIMS = nt.GUMBEL_N
KEY = nt.GUMBEL_KEY
# a sigma so small that one ulp of a value_sum moves pi by a few ulps: the variants move it by about one
NODE_RULE = (None, 0.5, 0.03)
VMIX_VARIANTS = ("s_butterfly", "wv_butterfly", "qv_butterfly", "qv_fused", "vmix_fused", "vmix_reassociated")
NO_WITNESS_AT_K3 = ("s_butterfly", "wv_butterfly", "qv_butterfly", "qv_fused")
NODE_VARIANTS = VMIX_VARIANTS + ("reciprocal_range", "reciprocal_mean", "fused", "z_butterfly", "reciprocal_z", "reciprocal_excess")
PENDING_VARIANTS = ("pending_not_in_msum", "pending_in_sigma", "reciprocal_excess")
PENDING = dict(nt.PENDING, launched=(1, 1, 0))  # "launched": what the first leaf of the launch leaves behind; nothing is preset
NEEDS_CHILD_PENDING = ("pending_not_in_msum", "pending_in_sigma")  # the same bits as the reference while no child has a pending visit
# witnesses per variant x level of a width.  G = 4 takes more: its table is to span two workgroups
PER_WIDTH = {4: 5, 16: 2, 64: 2}
PER_WIDTH_NO_K3 = {4: 0, 16: 4, 64: 4}
PENDING_PER_WIDTH = {4: 12, 16: 3, 64: 3}
CHOOSE_VARIANTS = ("qv_butterfly", "vmix_fused")
CHOOSE_PER_WIDTH = {4: {"qv_butterfly": 0, "vmix_fused": 3}, 16: {"qv_butterfly": 4, "vmix_fused": 3}, 64: {"qv_butterfly": 4, "vmix_fused": 2}}
LEVELS = gtc.T  # the rows of `paths` of a table of the tree kernels: what their GPU harnesses build the request for
OTHERS_SIM_VISITS = 5  # a count that no row of the considered table of n = 4 simulations holds


# ---- the reference arithmetic and its variants ------------------------------------------------------------------------
fma = nt.fma
exp_of = functools.lru_cache(maxsize=1 << 18)(nt.exp_of)


@functools.lru_cache(maxsize=1 << 16)
def ln_of(x):
    """pcbenv/search.py:ieee_ln in Python floats (check_cases holds the two together)."""
    m, e = math.frexp(x)
    if m < search._SQRT_HALF:
        m, e = 2.0 * m, e - 1
    t = (m - 1.0) / (m + 1.0)
    t2 = t * t
    p = (1.0 / 27.0) * t2 + 1.0 / 25.0
    for n in (23.0, 21.0, 19.0, 17.0, 15.0, 13.0, 11.0, 9.0, 7.0, 5.0, 3.0, 1.0):
        p = p * t2 + 1.0 / n
    ef = float(e)
    return ef * search._LN2_HI + (ef * search._LN2_LO + (2.0 * t) * p)


def butterfly(addends, G):
    """The sum a __shfl_xor butterfly over G lanes leaves in lane 0: 0.0 in the lanes without an addend."""
    v, o = list(addends) + [0.0] * (G - len(addends)), G // 2
    while o:
        v, o = [v[i] + v[i ^ o] for i in range(G)], o // 2
    return v[0]


def clamped_prior(prior):
    return (prior if prior < 1.0 else 1.0) if prior > search.GUMBEL_PRIOR_FLOOR else search.GUMBEL_PRIOR_FLOOR


def softmax_of(x, G, variant=None):
    """csrc/pcb_gumbel_tree.h:node_policy."""
    mx = max(x)
    e = [exp_of(v - mx) for v in x]
    if variant == "z_butterfly":
        Z = butterfly(e, G)
    else:
        Z = 0.0
        for v in e:
            Z = Z + v
    if variant == "reciprocal_z":
        r = 1.0 / Z
        return [v * r for v in e]
    return [v / Z for v in e]


def node_rule(ch, vs_node, n_node, lo, hi, c_visit, c_scale, G, variant=None, pending=None):
    """ch: [(value_sum, visits, prior)] of the node's children in order; vs_node, n_node: the node's own; pending: [k] or None.
    -> dict(t, pi, x [k], vmix, scale)."""
    k = len(ch)
    n = [c[1] for c in ch]
    pn = [0] * k if pending is None else list(pending)
    Nsum = sum(n)
    most = max(a + b for a, b in zip(n, pn)) if variant == "pending_in_sigma" else max(n)
    pr = [clamped_prior(c[2]) for c in ch]
    seen = [m > 0 for m in n]
    if variant == "reciprocal_mean":
        q = [c[0] * (1.0 / float(c[1])) if s else None for c, s in zip(ch, seen)]
    else:
        q = [c[0] / float(c[1]) if s else None for c, s in zip(ch, seen)]
    if variant == "s_butterfly":
        S = butterfly([c[0] for c in ch], G)
    else:
        S = 0.0
        for c in ch:
            S = S + c[0]
    if variant == "wv_butterfly":
        Wv = butterfly([p if s else 0.0 for p, s in zip(pr, seen)], G)
    else:
        Wv = 0.0
        for p, s in zip(pr, seen):
            if s:
                Wv = Wv + p
    if variant == "qv_butterfly":
        Qv = butterfly([p * v if s else 0.0 for p, v, s in zip(pr, q, seen)], G)
    else:
        Qv = 0.0
        for p, v, s in zip(pr, q, seen):
            if s:
                Qv = fma(p, v, Qv) if variant == "qv_fused" else Qv + p * v
    own = n_node - Nsum
    vhat = (vs_node - S) / float(own) if own > 0 else (vs_node / float(n_node) if n_node > 0 else lo)
    Nf = float(Nsum)
    if Nsum > 0 and Wv > 0.0:
        if variant == "vmix_fused":
            vmix = fma(Nf / Wv, Qv, vhat) / (1.0 + Nf)
        elif variant == "vmix_reassociated":
            vmix = (vhat + (Nf * Qv) / Wv) / (1.0 + Nf)
        else:
            vmix = (vhat + (Nf / Wv) * Qv) / (1.0 + Nf)
    else:
        vmix = vhat
    scale = (c_visit + float(most)) * c_scale
    x = []
    for c in range(k):
        m = q[c] if seen[c] else vmix
        qhat = 0.0 if not hi > lo else (m - lo) * (1.0 / (hi - lo)) if variant == "reciprocal_range" else (m - lo) / (hi - lo)
        x.append(nt.improved_of(ln_of(pr[c]), qhat, scale, variant))
    pi = softmax_of(x, G, variant)
    Msum = Nsum if variant == "pending_not_in_msum" else Nsum + sum(pn)
    den = 1.0 + float(Msum)
    if variant == "reciprocal_excess":
        r = 1.0 / den
        t = [pi[c] - float(n[c] + pn[c]) * r for c in range(k)]
    else:
        t = [pi[c] - float(n[c] + pn[c]) / den for c in range(k)]
    return dict(t=t, pi=pi, x=x, vmix=vmix, scale=scale)


# ---- one witness ------------------------------------------------------------------------------------------------------
def _near(x):
    ulp = math.ulp(x)
    return [x + s * j * ulp for j in range(SCAN + 1) for s in ((1,) if j == 0 else (1, -1))]


def _f32(x):
    return float(np.float32(x))


def _others(rng, k, a, b, lo, hi, visited_at_least, float32=True, mean_hi=0.3, prior=(1e-3, 1e-2)):
    """The children that are no contenders: float32 priors of 1e-3 to 1e-2, low non-dyadic means, most of them visited.
    float32=False: priors of all 53 bits, as pcbenv_puct_root_noise leaves them."""
    ch = [None] * k
    rest = [c for c in range(k) if c not in (a, b)]
    must = set(rng.sample(rest, min(visited_at_least, len(rest))))
    for c in rest:
        n = rng.randint(1, 3) if c in must or rng.random() < 0.75 else 0
        pr = rng.uniform(*prior)
        ch[c] = ((lo + (hi - lo) * rng.uniform(0.02, mean_hi)) * n, n, _f32(pr) if float32 else pr)
    return ch


def _node_duel(rng, G, k, a, b, variant, c_visit, c_scale, pending=(0, 0, 0), launched=False):
    """-> dict(lo, hi, vs_node, n_node, children [(value_sum, visits, prior)], ref, var) or None; ref / var: 0 if a wins, 1 if b."""
    lo = rng.uniform(-5.0, -3.0)
    hi = lo + rng.uniform(0.3, 2.0)
    ch = _others(rng, k, a, b, lo, hi, 3, variant != "wv_butterfly")
    n_b = rng.randint(1, 12)
    n_a = 0 if variant in VMIX_VARIANTS else rng.randint(1, 12)
    if variant == "pending_in_sigma":  # the most visits with pending is another number than without
        n_a = max(n_a, n_b, 3)
    ch[a] = ((lo + (hi - lo) * rng.uniform(0.15, 0.85)) * n_a, n_a, _f32(rng.uniform(0.15, 0.45)))
    pend = [0] * k
    pend[a], pend[b] = pending[1], pending[2]
    own = rng.randint(1, 3)
    args = (lo, hi, c_visit, c_scale, G)

    def rule(vs_b, p_b, var=None):
        ch[b] = (vs_b, n_b, p_b)
        S = 0.0
        for c in ch:
            S = S + c[0]
        return node_rule(ch, S + own * vhat, n_node, *args, var, pend)
    n_node = sum(c[1] for c in ch if c is not None) + n_b + own
    vhat = lo + (hi - lo) * rng.uniform(0.1, 0.9)
    mid = (lo + (hi - lo) * 0.5) * n_b
    p_b = ch[a][2]
    Msum = n_node - own + sum(pend)
    for _ in range(3):  # b's prior for a tie at the middle of b's range
        r = rule(mid, p_b)
        want = r["pi"][a] - float(n_a + pend[a] - n_b - pend[b]) / (1.0 + Msum)
        if not 0.05 < want < 0.9:
            return None
        p_b = _f32(p_b * want / r["pi"][b])
        if not 0.02 < p_b < 0.9:
            return None

    def a_wins(vs_b, var=None):
        t = rule(vs_b, p_b, var)["t"]
        return t[a] >= t[b]
    x, y = (lo + (hi - lo) * 0.05) * n_b, (lo + (hi - lo) * 0.95) * n_b  # b's value_sum: a wins at x, b at y
    if not a_wins(x) or a_wins(y):
        return None
    while True:
        m = x + (y - x) / 2.0
        if m <= x or m >= y:
            break
        x, y = (m, y) if a_wins(m) else (x, m)
    for vs_b in _near(y):
        ref, var = int(not a_wins(vs_b)), int(not a_wins(vs_b, variant))
        if ref == var or (launched and ref != 1):
            continue
        tv, t = rule(vs_b, p_b, variant)["t"], rule(vs_b, p_b)["t"]
        far = [c for c in range(k) if c not in (a, b)]
        if far and (max(t[c] for c in far) > min(t[a], t[b]) - 2 * MARGIN or max(tv[c] for c in far) > min(tv[a], tv[b]) - 2 * MARGIN):
            return None
        if launched:  # without the pending visit the rule goes to a, clearly
            blind = node_rule(ch, _vs_node(ch, own, vhat), n_node, *args)["t"]
            if not blind[a] > max(blind[c] for c in range(k) if c != a) + 2 * MARGIN:
                return None
        return dict(lo=lo, hi=hi, vs_node=_vs_node(ch, own, vhat), n_node=n_node, children=list(ch), ref=ref, var=var)
    return None


def _vs_node(ch, own, vhat):
    S = 0.0
    for c in ch:
        S = S + c[0]
    return S + own * vhat


# ---- the tables -------------------------------------------------------------------------------------------------------
def _fill(st, p, node, first, children, lo):
    """The children of `node` in the slots from `first` on; every one a terminal leaf."""
    k = len(children)
    st["first_child"][p, node], st["num_children"][p, node], st["num_nodes"][p] = first, k, first + k
    for c, (vs, n, prior) in enumerate(children):
        s = first + c
        st["parent"][p, s], st["depth"][p, s], st["node_action"][p, s] = node, st["depth"][p, node] + 1, (s % 2, 0, s)
        st["prior"][p, s], st["visits"][p, s], st["value_sum"][p, s] = prior, n, vs
        st["value_max"][p, s] = st["reward_hi"][p] if n else -np.inf
        st["terminal"][p, s] = 1


def _place(st, p, C, level, duel, a, b):
    """Witness `duel` into root p at `level` -> (node, fc)."""
    lo, hi = duel["lo"], duel["hi"]
    k = len(duel["children"])
    st["reward_lo"][p], st["reward_hi"][p], st["value_max"][p, 0] = lo, hi, hi
    if level == 0:
        node, fc = 0, 1
        _fill(st, p, 0, 1, duel["children"], lo)
        st["visits"][p, 0], st["value_sum"][p, 0] = duel["n_node"], duel["vs_node"]
        st["sim_index"][p] = N_SIMS
    else:  # the contenders' parent is a root child that the schedule takes clearly: prior 1 against 0
        node, fc = 1 + (a + b) % k, 1 + C
        _fill(st, p, 0, 1, [(lo, 1, 0.0)] * k, lo)
        _fill(st, p, node, fc, duel["children"], lo)
        st["terminal"][p, node] = 0
        st["prior"][p, node], st["visits"][p, node], st["value_sum"][p, node], st["value_max"][p, node] = 1.0, duel["n_node"], duel["vs_node"], hi
        st["visits"][p, 0], st["value_sum"][p, 0] = duel["n_node"] + k, (duel["vs_node"] + lo * (k - 1)) + lo
    return node, fc


def _table(G, plan, name, duel_of):
    C, c_puct = WIDTHS[G], C_PUCT[G]
    P, N, k = len(plan), 1 + 2 * C, C
    rng = random.Random(f"near ties {name} {G}")
    st = nt._empty(P, N, C)
    st.update(sim_index=np.zeros(P, np.int32), sim_visits=np.zeros((P, C), np.int32))
    lanes = nt.placements(G, k)
    rule = (c_puct,) + NODE_RULE[1:]
    rows, tries = [], 0
    for p, item in enumerate(plan):
        a, b = lanes[p % len(lanes)]
        while True:
            tries += 1
            assert tries < 400000, (name, G, item)
            duel = duel_of(rng, item, k, a, b, rule)
            if duel is not None:
                break
        variant, level, kind = item
        node, fc = _place(st, p, C, level, duel, a, b)
        pending = PENDING[kind]
        if kind == "launched":  # both leaves go to the node: no other root child stands at a count the schedule considers
            st["sim_visits"][p, :] = OTHERS_SIM_VISITS
            st["sim_visits"][p, node - 1] = 0
        elif kind != "none":
            st["pending"][p, node], st["pending"][p, fc + a], st["pending"][p, fc + b] = pending
            if level == 1:
                st["pending"][p, 0] = pending[0]
        rows.append(dict(variant=variant, level=level, lanes=(a, b), kind=kind, pending=pending, node=node, slots=(fc + a, fc + b),
                         ref=fc + (a, b)[duel["ref"]], var=fc + (a, b)[duel["var"]]))
    return SimpleNamespace(kernel=name, G=G, C=C, P=P, N=N, K=C, T=T, L=L, c_puct=c_puct, rule=rule, n=N_SIMS, Mc=min(C, 16), state=st, rows=rows,
                           tries=tries)


@functools.lru_cache(maxsize=None)
def node_table(G):
    """-> SimpleNamespace as nt.table: rows dict(variant, level, lanes, kind "none", node, slots, ref, var)."""
    plan = [(v, level, "none") for v in NODE_VARIANTS for level in (0, 1) for _ in range((PER_WIDTH_NO_K3 if v in NO_WITNESS_AT_K3 else PER_WIDTH)[G])]
    return _table(G, plan, "node", lambda rng, item, k, a, b, rule: _node_duel(rng, G, k, a, b, item[0], rule[1], rule[2]))


def _pending_kinds(variant, level):
    kinds = [kd for kd in PENDING if kd != "none" and not (variant in NEEDS_CHILD_PENDING and kd == "node")]
    return [kd for kd in kinds if not (kd == "launched" and level == 0)]  # a spent budget makes one descent


@functools.lru_cache(maxsize=None)
def pending_table(G):
    """-> as node_table, with `pending` preset by kind, but for the "launched" roots."""
    plan = []
    for v in PENDING_VARIANTS:
        for level in (0, 1):
            kinds = _pending_kinds(v, level)
            plan += [(v, level, kinds[(i + level) % len(kinds)]) for i in range(PENDING_PER_WIDTH[G])]
    return _table(G, plan, "pending", lambda rng, item, k, a, b, rule: _node_duel(rng, G, k, a, b, item[0], rule[1], rule[2], PENDING[item[2]],
                                                                                 item[2] == "launched"))


def children_of(t, p, node=None):
    st = t.state
    node = t.rows[p]["node"] if node is None else node
    fc, k = int(st["first_child"][p, node]), int(st["num_children"][p, node])
    return fc, [(float(st["value_sum"][p, s]), int(st["visits"][p, s]), float(st["prior"][p, s])) for s in range(fc, fc + k)]


def reference_choice(t, p, variant=None):
    """The slot root p's witness node goes to, recomputed from the state of the table alone, by the reference arithmetic or by
    `variant`; the pending visits are the table's, or for a "launched" root what the first leaf leaves.  -> (slot, t [k])."""
    st, row = t.state, t.rows[p]
    node = row["node"]
    fc, ch = children_of(t, p)
    pend = [int(st["pending"][p, fc + c]) for c in range(len(ch))]
    if row["kind"] == "launched":
        pend[row["slots"][0] - fc] += 1
    out = node_rule(ch, float(st["value_sum"][p, node]), int(st["visits"][p, node]), float(st["reward_lo"][p]), float(st["reward_hi"][p]),
                    t.rule[1], t.rule[2], t.G, variant, pend)
    return fc + nt.first_max(out["t"]), out["t"]


# ---- CHOOSE witnesses with v_mix ----------------------------------------------------------------------------------------
def choose_of(ch, vs_node, n_node, lo, hi, c_visit, c_scale, G, variant=None):
    """csrc/pcb_gumbel_tree.h:tree_choose's target -> (child_weights [k], child_policy [k] float32)."""
    pi = node_rule(ch, vs_node, n_node, lo, hi, c_visit, c_scale, G, variant)["pi"]
    return [int(p * 16777216.0 + 0.5) for p in pi], [np.float32(p) for p in pi]


def _choose_root(rng, G, k, variant, kind, c_visit, c_scale):
    """nt._choose_root with children that have no visit: one visited child's value_sum is bisected until a child WITHOUT a visit
    -- whose logit is completed with vmix -- has its pi * 2^24 at an integer plus one half, or its pi between two float32."""
    lo = rng.uniform(-5.0, -3.0)
    hi = lo + rng.uniform(0.3, 2.0)
    ch = []
    for c in range(k):
        n = rng.randint(1, 3) if c < 2 or rng.random() < 0.6 else 0
        ch.append([(lo + (hi - lo) * rng.uniform(0.1, 0.9)) * n, n, _f32(rng.uniform(0.02, 0.5))])
    rng.shuffle(ch)
    unseen = [c for c in range(k) if ch[c][1] == 0]
    seen = [c for c in range(k) if ch[c][1] > 0]
    if not unseen or len(seen) < min(3, k - 1):
        return None
    j, u = rng.choice(seen), rng.choice(unseen)  # j is moved; u's output is watched
    own, vhat = rng.randint(1, 3), lo + (hi - lo) * rng.uniform(0.1, 0.9)
    n_node = sum(c[1] for c in ch) + own

    def outputs(vs, var=None):
        moved = [tuple(c) if i != j else (vs, c[1], c[2]) for i, c in enumerate(ch)]
        return choose_of(moved, _vs_node(moved, own, vhat), n_node, lo, hi, c_visit, c_scale, G, var)
    watched = (lambda vs: outputs(vs)[0][u]) if kind == "weights" else (lambda vs: float(outputs(vs)[1][u]))
    x = ch[j][0]
    was = watched(x)  # bisect between a value_sum that gives this output and one that gives another: the boundary of two outputs
    y = next((e for e in (hi * ch[j][1], lo * ch[j][1]) if watched(e) != was), None)
    if y is None:
        return None
    while True:
        m = x + (y - x) / 2.0
        if m == x or m == y:
            break
        x, y = (m, y) if watched(m) == was else (x, m)
    for vs in _near(y):
        if not lo * ch[j][1] <= vs <= hi * ch[j][1]:
            continue
        ref, var = outputs(vs), outputs(vs, variant)
        if (ref[0] != var[0]) if kind == "weights" else ([float(v) for v in ref[1]] != [float(v) for v in var[1]]):
            ch[j][0] = vs
            moved = [tuple(c) for c in ch]
            return dict(lo=lo, hi=hi, children=moved, vs_node=_vs_node(moved, own, vhat), n_node=n_node)
    return None


@functools.lru_cache(maxsize=None)
def choose_table(G):
    """-> SimpleNamespace as nt.choose_table: roots whose k = C children all take part in the softmax, some without a visit; rows
    dict(variant, kind)."""
    C, c_puct = WIDTHS[G], C_PUCT[G]
    plan = [(v, kind) for v in CHOOSE_VARIANTS for kind in nt.CHOOSE_KINDS for _ in range(CHOOSE_PER_WIDTH[G][v])]
    P, N, k = len(plan), 1 + C, C
    rng = random.Random(f"near ties tree choose {G}")
    st = nt._empty(P, N, C)
    st.update(sim_index=np.zeros(P, np.int32), sim_visits=np.zeros((P, C), np.int32))
    rule = (c_puct,) + nt.CHOOSE_RULE[1:]
    rows, tries = [], 0
    for p, (variant, kind) in enumerate(plan):
        while True:
            tries += 1
            assert tries < 20000, (G, variant, kind)
            root = _choose_root(rng, G, k, variant, kind, rule[1], rule[2])
            if root is not None:
                break
        st["reward_lo"][p], st["reward_hi"][p], st["value_max"][p, 0] = root["lo"], root["hi"], root["hi"]
        _fill(st, p, 0, 1, root["children"], root["lo"])
        st["visits"][p, 0], st["value_sum"][p, 0] = root["n_node"], root["vs_node"]
        rows.append(dict(variant=variant, kind=kind))
    return SimpleNamespace(kernel="tree_choose", G=G, C=C, P=P, N=N, K=C, T=T, L=L, c_puct=c_puct, rule=rule, n=N_SIMS, Mc=min(C, 16), state=st, rows=rows,
                           tries=tries)


def choose_outputs(t, p, variant=None):
    """(child_weights, child_policy) of root p of a choose_table, recomputed from its state alone."""
    st = t.state
    fc, ch = children_of(t, p, 0)
    return choose_of(ch, float(st["value_sum"][p, 0]), int(st["visits"][p, 0]), float(st["reward_lo"][p]), float(st["reward_hi"][p]), t.rule[1], t.rule[2],
                     t.G, variant)


# ---- the calls on a table, and the models' states after them -----------------------------------------------------------
def tree_state(t, levels=LEVELS):
    """The state of a table as the one-leaf Gumbel models take it."""
    st = {f: t.state[f] for f in pc.TREE_FIELDS + ("sim_index", "sim_visits")}
    st.update(selected=np.full(t.P, gc.FILL, np.int32), path_len=np.full(t.P, gc.FILL, np.int32), paths=np.full((levels, t.P, 3), gc.FILL, np.int32))
    return st


def leaves_state(t, levels=LEVELS):
    """... as the models of L leaves take it: the table's pending visits where it has any."""
    st = glc.with_leaves(tree_state(t, levels), t.P, t.N, t.L, levels)
    st["pending"] = np.array(t.state["pending"], np.int32)
    return st


def _case(t, st, levels):
    return SimpleNamespace(P=t.P, N=t.N, C=t.C, K=t.K, L=t.L, n=t.n, Mc=t.Mc, rule=t.rule, state=st, table=search.considered_visits(t.Mc, t.n).numpy(),
                           T=T, levels=levels)


RUNS = {  # kernel: (the model of one call sequence, leaves)
    "gumbel_leaves": (lambda t, st, seq, levels: glc.run(st, t.C, t.K, t.n, t.Mc, t.L, t.rule, seq, levels=levels), True),
    "gumbel_tree": (lambda t, st, seq, levels: gtc.run(st, t.C, t.K, t.n, t.Mc, t.rule, seq, levels=levels), False),
    "gumbel_tree_leaves": (lambda t, st, seq, levels: gtl.run(st, t.C, t.K, t.n, t.Mc, t.L, t.rule, seq, levels=levels), True),
}


def _calls(t, kernel, levels, choose_only=False):
    """-> (case, seq, states) as the kernels' GPU harnesses take them: CHOOSE on the table (it stores to no state), SELECT, then
    ABSORB | SELECT with nt.evaluation."""
    run, leaves = RUNS[kernel]
    one = t if leaves else SimpleNamespace(**dict(vars(t), L=1))
    st = leaves_state(one, levels) if leaves else tree_state(one, levels)
    head = [gc.call(gc.CHOOSE, **KEY)] + ([] if choose_only else [gc.call(gc.SELECT, **KEY)])
    if choose_only:
        return _case(one, st, levels), head, run(one, st, head, levels)
    selected = run(one, st, head, levels)[1]["selected"]
    seq = head + [gc.call(gc.ABSORB | gc.SELECT, nt.evaluation(one, selected), **KEY)]
    return _case(one, st, levels), seq, run(one, st, seq, levels)


@functools.lru_cache(maxsize=None)
def node_calls(kernel, G):
    """node_table(G) through "gumbel_tree" or "gumbel_tree_leaves" (L = 2, nothing pending)."""
    return _calls(node_table(G), kernel, LEVELS)


@functools.lru_cache(maxsize=None)
def pending_calls(G):
    return _calls(pending_table(G), "gumbel_tree_leaves", LEVELS)


@functools.lru_cache(maxsize=None)
def choose_calls(kernel, G):
    return _calls(choose_table(G), kernel, LEVELS, choose_only=True)


@functools.lru_cache(maxsize=None)
def root_rule_choose_calls(kernel, G):
    """nt.choose_table(G) -- z_butterfly, reciprocal_z and fused on roots whose children all have a visit -- through the CHOOSE of
    "gumbel_tree" or "gumbel_tree_leaves": nothing is completed with vmix."""
    return _calls(SimpleNamespace(**dict(vars(nt.choose_table(G)), L=L)), kernel, LEVELS, choose_only=True)


# ---- the root-score witnesses of nt.table("gumbel", G) and nt.table("leaves", G) on the leaf kernels ----------------------
# nt.table("gumbel", G) holds the four GUMBEL_VARIANTS' root-score witnesses at sim_index 0; all of its root children have a
# visit, so pcb_gumbel_tree.h:tree_root_scores completes none of them with vmix and gives pcb_gumbel.h:root_scores' bits.
# "first": the table as it is, L = 2: the witness decides leaf 0.  "second": n = 8 simulations over Mc = 2 candidates, whose row
# of the considered table is 0 0 1 1 2 2 3 3; sim_index 1, the contenders at count 1, the child after b (cyclically the next
# that is no contender) at 0 and all others at OTHERS: leaf 0 goes to that child, the only one at 0, and leaf 1 meets the tie at
# count 1 -- decided by scores and counters that the kernel kept in registers.
SECOND = dict(n=8, Mc=2, others=9)


def _second(t):
    st = {f: np.array(v) for f, v in t.state.items()}
    third = {}
    for p, row in enumerate(t.rows):
        if row["score"] != "gumbel":
            st["sim_index"][p] = SECOND["n"]
            continue
        a, b = row["lanes"]
        c3 = next(c for c in ((b + 1 + i) % t.C for i in range(t.C)) if c not in (a, b))
        st["sim_index"][p] = 1
        st["sim_visits"][p, :] = SECOND["others"]
        st["sim_visits"][p, [a, b]], st["sim_visits"][p, c3] = 1, 0
        third[p] = 1 + c3
    return SimpleNamespace(**dict(vars(t), state=st, n=SECOND["n"], Mc=SECOND["Mc"], third=third))


@functools.lru_cache(maxsize=None)
def gumbel_rows_calls(kernel, G, which):
    """nt.table("gumbel", G) through "gumbel_leaves" or "gumbel_tree_leaves" at L = 2 -> (table, case, seq, states); which:
    "first" or "second"."""
    t = nt.table("gumbel", G)
    t = SimpleNamespace(**dict(vars(t), L=L, state=dict(t.state, pending=np.zeros((t.P, t.N), np.int32))))
    if which == "second":
        t = _second(t)
    levels = gc.T if kernel == "gumbel_leaves" else LEVELS
    return (t,) + _calls(t, kernel, levels)


@functools.lru_cache(maxsize=None)
def leaves_rows_calls(G):
    """nt.table("leaves", G) -- the LEAVES_VARIANTS' witnesses with pending visits -- through "gumbel_leaves" with sim_index 0: at
    level 1 they stand below a root level that the schedule takes (the node has prior 1 and the highest mean)."""
    t = nt.table("leaves", G)
    st = dict(t.state, sim_index=np.zeros(t.P, np.int32), sim_visits=np.zeros((t.P, t.C), np.int32))
    t = SimpleNamespace(**dict(vars(t), state=st, rule=(t.c_puct,) + nt.GUMBEL_RULE[1:], n=N_SIMS, Mc=min(t.C, 16)))
    return (t,) + _calls(t, "gumbel_leaves", gc.T)


# ---- root-score witnesses with vmix for k_gumbel_tree_leaves ----------------------------------------------------------------
ROOT_VARIANTS = nt.GUMBEL_VARIANTS + ("vmix_fused", "vmix_reassociated")
ROOT_PER_WIDTH = {4: 11, 16: 3, 64: 3}
ROOT_RULE = (None, 2.0, 0.3)  # a's completion is the mean of mostly low values: under a large sigma no prior makes that up


def root_scores_of(ch, vs_node, n_node, lo, hi, c_visit, c_scale, G, g, variant=None):
    """csrc/pcb_gumbel_tree.h:tree_root_scores' score [k]: (g + logit) + sigma with the completion of node_logits."""
    node_variant = variant if variant in NODE_VARIANTS else None
    k = len(ch)
    # sigma_c = scale * qhat_c is node_rule's x_c - logit_c only up to rounding: restate it from the quantities themselves
    r = node_rule(ch, vs_node, n_node, lo, hi, c_visit, c_scale, G, node_variant)
    out = []
    for c in range(k):
        vs, n, prior = ch[c]
        m = (vs * (1.0 / float(n)) if variant == "reciprocal_mean" else vs / float(n)) if n > 0 else r["vmix"]
        qhat = 0.0 if not hi > lo else (m - lo) * (1.0 / (hi - lo)) if variant == "reciprocal_range" else (m - lo) / (hi - lo)
        out.append(nt.gumbel_score(g[c], ln_of(clamped_prior(prior)), qhat, r["scale"], variant if variant in nt.GUMBEL_VARIANTS else None)[0])
    return out


def _root_duel(rng, G, k, a, b, variant, g, c_visit, c_scale):
    """A root whose contender a has NO visit and is completed with vmix; b's value_sum is bisected.  The other children are
    _others: all visited, priors of 1e-5 to 1e-4, which enter Wv."""
    lo = rng.uniform(-5.0, -3.0)
    hi = lo + rng.uniform(0.3, 2.0)
    ch = _others(rng, k, a, b, lo, hi, k, prior=(1e-5, 1e-4))  # far below whatever a root's draws are: the largest of 62 is about 6
    n_b = rng.randint(1, 12)
    ch[a] = (0.0, 0, _f32(rng.uniform(0.05, 0.5)))
    own, vhat = rng.randint(1, 3), lo + (hi - lo) * rng.uniform(0.1, 0.9)
    n_node = sum(c[1] for c in ch if c is not None) + n_b + own
    args = (lo, hi, c_visit, c_scale, G, g)
    far = [c for c in range(k) if c not in (a, b)]

    def scores(vs_b, var=None):
        ch[b] = (vs_b, n_b, p_b)
        return root_scores_of(ch, _vs_node(ch, own, vhat), n_node, *args, var)
    p_b = _f32(math.exp(rng.uniform(math.log(0.02), math.log(0.5))))
    s = scores((lo + (hi - lo) * 0.5) * n_b)  # a's prior for a tie at the middle of b's range: it enters nothing but a's logit
    p_a = _f32(ch[a][2] * math.exp(max(-20.0, min(20.0, s[b] - s[a]))))
    if not 1e-3 < p_a < 1.0:
        return None
    ch[a] = (0.0, 0, p_a)

    def a_wins(vs_b, var=None):
        s = scores(vs_b, var)
        return s[a] >= s[b]
    x, y = (lo + (hi - lo) * 0.05) * n_b, (lo + (hi - lo) * 0.95) * n_b
    if not a_wins(x) or a_wins(y):
        return None
    s = scores(x)
    if far and max(s[c] for c in far) > min(s[a], s[b]) - 0.1:
        return None
    while True:
        m = x + (y - x) / 2.0
        if m <= x or m >= y:
            break
        x, y = (m, y) if a_wins(m) else (x, m)
    for vs_b in _near(y):
        ref, var = int(not a_wins(vs_b)), int(not a_wins(vs_b, variant))
        if ref != var:
            ch[b] = (vs_b, n_b, p_b)
            return dict(lo=lo, hi=hi, vs_node=_vs_node(ch, own, vhat), n_node=n_node, children=list(ch), ref=ref, var=var)
    return None


@functools.lru_cache(maxsize=None)
def root_table(G):
    """-> as node_table: root-score witnesses (sim_index 0, every sim_visits 0) of the full rule whose contender a has no visit."""
    C, c_puct = WIDTHS[G], C_PUCT[G]
    plan = [v for v in ROOT_VARIANTS for _ in range(ROOT_PER_WIDTH[G])]
    P, N, k = len(plan), 1 + C, C
    rng = random.Random(f"near ties tree root {G}")
    st = nt._empty(P, N, C)
    st.update(sim_index=np.zeros(P, np.int32), sim_visits=np.zeros((P, C), np.int32))
    rule = (c_puct,) + ROOT_RULE[1:]
    dummy = {f: torch.from_numpy(st[f]) for f in ("num_children", "first_child", "visits", "prior", "value_sum", "reward_lo", "reward_hi")}
    g = search.gumbel_scores(dummy, C, rule[1], rule[2], **KEY)["g"].numpy()  # the draws depend on the key alone
    lanes = nt.placements(G, k)
    rows, tries = [], 0
    for p, variant in enumerate(plan):
        at = 0
        while True:
            tries, at = tries + 1, at + 1
            assert tries < 400000, (G, variant)
            a, b = lanes[(p + at // 3000) % len(lanes)]  # the draws g of a root may part two lanes too far for any pair of priors
            duel = _root_duel(rng, G, k, a, b, variant, [float(v) for v in g[p]], rule[1], rule[2])
            if duel is not None:
                break
        st["reward_lo"][p], st["reward_hi"][p], st["value_max"][p, 0] = duel["lo"], duel["hi"], duel["hi"]
        _fill(st, p, 0, 1, duel["children"], duel["lo"])
        st["visits"][p, 0], st["value_sum"][p, 0] = duel["n_node"], duel["vs_node"]
        rows.append(dict(variant=variant, level=0, lanes=(a, b), kind="none", node=0, slots=(1 + a, 1 + b), ref=1 + (a, b)[duel["ref"]],
                         var=1 + (a, b)[duel["var"]]))
    return SimpleNamespace(kernel="tree_root", G=G, C=C, P=P, N=N, K=C, T=T, L=L, c_puct=c_puct, rule=rule, n=N_SIMS, Mc=min(C, 16), state=st, rows=rows,
                           tries=tries, g=g)


def root_choice(t, p, variant=None):
    st = t.state
    fc, ch = children_of(t, p, 0)
    s = root_scores_of(ch, float(st["value_sum"][p, 0]), int(st["visits"][p, 0]), float(st["reward_lo"][p]), float(st["reward_hi"][p]), t.rule[1], t.rule[2],
                       t.G, [float(v) for v in t.g[p]], variant)
    return fc + nt.first_max(s), s


@functools.lru_cache(maxsize=None)
def root_calls(kernel, G):
    return _calls(root_table(G), kernel, LEVELS)


# ---- what the tables are there for -------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def tables():
    """Every table of this module, and the seconds their generation took."""
    t0 = time.perf_counter()
    out = {(name, G): make(G) for name, make in (("node", node_table), ("pending", pending_table), ("choose", choose_table), ("root", root_table))
           for G in WIDTHS}
    return out, time.perf_counter() - t0


def counts():
    """-> {(table, variant, level): witnesses over the widths}, {(table, G, lanes): witnesses}, {kind: witnesses of the pending tables}."""
    by_variant, by_lanes, by_kind = {}, {}, {}
    for (name, G), t in tables()[0].items():
        for row in t.rows:
            keys = [(by_variant, (name, row["variant"], row.get("level", row.get("kind"))))]
            if name != "choose":
                keys.append((by_lanes, (name, G, row["lanes"])))
            if name == "pending":
                keys.append((by_kind, row["kind"]))
            for d, key in keys:
                d[key] = d.get(key, 0) + 1
    return by_variant, by_lanes, by_kind


@functools.lru_cache(maxsize=None)
def check_cases():
    """From the tables alone: every variant x level has FLOOR witnesses over the widths -- NO_WITNESS_AT_K3 over G = 16 and 64 --,
    every lane placement of every width and every pending kind is reached, the vmix witnesses are what they have to be, a table of
    G = 4 with a SELECT spans workgroups, no NaN and nothing infinite but value_max of a slot without a visit; ln_of and exp_of are
    pcbenv/search.py's.  -> the tables."""
    all_tables, seconds = tables()
    by_variant, by_lanes, by_kind = counts()
    for v in NODE_VARIANTS:
        for level in (0, 1):
            assert by_variant.get(("node", v, level), 0) >= FLOOR, (v, level)
    for v in PENDING_VARIANTS:
        for level in (0, 1):
            assert by_variant.get(("pending", v, level), 0) >= FLOOR, (v, level)
    for v in ROOT_VARIANTS:
        assert by_variant.get(("root", v, 0), 0) >= FLOOR, v
    for v in CHOOSE_VARIANTS:
        for kind in nt.CHOOSE_KINDS:
            assert by_variant.get(("choose", v, kind), 0) >= FLOOR, (v, kind)
    for kind in PENDING:
        assert (by_kind.get(kind, 0) >= FLOOR) == (kind != "none"), kind
    for (name, G), t in all_tables.items():
        assert pc.group_lanes(t.C) == G
        for f, arr in t.state.items():
            if arr.dtype.kind == "f":
                assert not np.isnan(arr).any(), (name, G, f)
                assert np.isfinite(arr).all() or (f == "value_max" and (np.isfinite(arr) | ((arr == -np.inf) & (t.state["visits"] == 0))).all()), (name, G, f)  # a slot without a visit
        if name == "choose":
            for p in range(t.P):
                n = t.state["visits"][p, 1:1 + t.C]
                assert (n == 0).any() and (n > 0).sum() >= min(3, t.C - 1), (G, p)  # some children without a visit, and enough addends
            continue
        assert G != 4 or t.P > pc.BLOCK // G
        for lanes in nt.placements(G, t.C):
            assert by_lanes.get((name, G, lanes), 0) >= 1, (name, G, lanes)
        for p, row in enumerate(t.rows):
            assert row["ref"] != row["var"] and {row["ref"], row["var"]} == set(row["slots"]), (name, G, p)
            lo, hi = t.state["reward_lo"][p], t.state["reward_hi"][p]
            fc, ch = children_of(t, p)
            for s in row["slots"]:
                vs, n, prior = ch[s - fc]
                assert n == 0 or lo <= vs / n <= hi, (name, G, p)
            n_a = ch[row["slots"][0] - fc][1]
            others = [c for i, c in enumerate(ch) if fc + i not in row["slots"]]
            own = int(t.state["visits"][p, row["node"]]) - sum(c[1] for c in ch)
            if row["variant"] in VMIX_VARIANTS or name == "root":
                assert n_a == 0, (name, G, p)
            if row["variant"] in NO_WITNESS_AT_K3:
                visited = [c for c in others if c[1] > 0]
                assert len(visited) >= 3 and all(1e-3 <= c[2] <= 1e-2 for c in visited) and G != 4, (name, G, p)
            if row["variant"] == "s_butterfly":
                assert own > 0
            if row["variant"] in NEEDS_CHILD_PENDING:
                assert row["pending"][1] or row["pending"][2]
    xs = [-700.0 * random.Random(7).random() ** 4 for _ in range(500)] + [0.0, -1e-300, -708.0]
    assert [exp_of(x) for x in xs] == search.ieee_exp(torch.tensor(xs, dtype=torch.float64)).tolist()
    ys = [random.Random(8).random() ** 6 for _ in range(500)] + [2.0 ** -149, 1.0, float(np.float32(1e-3)), 0.5, 0.70710678118654752, 0.7071067811865476]
    assert [ln_of(y) for y in ys] == search.ieee_ln(torch.tensor(ys, dtype=torch.float64)).tolist()
    return all_tables


# ---- recorded searches on real-valued evaluations ----------------------------------------------------------------------
# nt.real_gumbel for the three kernels, at the shapes (C, P, the rule and the key) of gumbel_cases.CASES' rows REAL: T = 4 levels,
# n = 16 simulations over Mc = 2 and 4 candidates -- the rows' own n of 4 and 3, and Mc = 64, give no root child a third visit, so
# no search gets below level 2 -- and logits scaled by REAL_LOGIT_SCALE: softmax priors of logits in [-12, 12] keep a search on one
# child per node, and the node rule is to be seen spreading its visits.
REAL = {"G4_C3_P131": (2, 16), "G64_C64_P67": (4, 16)}  # name: (Mc, n)
REAL_LEAVES = {"gumbel_leaves": (3, 8), "gumbel_tree": (1,), "gumbel_tree_leaves": (3, 8)}
REAL_LEVELS = gtc.T
REAL_PRIOR_POWER = 0.125


def flat_evaluator(P, levels, K, seed, power=REAL_PRIOR_POWER):
    """pc.real_evaluator with every positive candidate prior raised to `power`, rounded to float32: the softmax of logits an
    eighth as large, not normalised -- priors are data."""
    base = pc.real_evaluator(P, levels, K, seed)

    def evaluate(paths, path_len, step_index0):
        ev = base(paths, path_len, step_index0)
        pr = ev.cand_prior.to(torch.float64)
        return search.Evaluation(ev.value, ev.terminal, ev.cand_count, ev.cand_actions, torch.where(pr > 0, pr.clamp(min=1e-300) ** power, pr).to(torch.float32))
    return evaluate


@functools.lru_cache(maxsize=None)
def real_search(kernel, name, leaves=1):
    """-> (case, seq, states, gs, calls): the specification's search recorded, the calls of gumbel_cases.search_calls and the
    kernel's model's states after them; `case` as the kernel's GPU harness takes it."""
    C, P, _, _, c_visit, c_scale, first_root, step_index = gc.CASES[name]
    Mc, n = REAL[name]
    K, levels = C, REAL_LEVELS
    rule, key = (nt.REAL_C_PUCT, c_visit, c_scale), dict(seed=gc.SEED ^ 9, step_index=step_index, first_root=first_root)
    base = flat_evaluator(P, levels, K, nt.REAL_SEED)
    if kernel == "gumbel_tree":
        N = 1 + (n + 1) * C
        gs, calls = gtc.record_search(P, levels, n, Mc, C, base, rule, key, capacity=N)
        start = gc.init_state(P, N, C, levels)
    else:
        E = -(-n // leaves) + 1
        N = 1 + E * leaves * C
        calls = []

        def recording(paths, path_len, s):
            ev = lc.per_leaf(base, P, levels, K, leaves)(paths, path_len, s)
            calls.append((paths.clone().numpy(), path_len.clone().numpy(), ev.value.to(torch.float64).numpy().copy(),
                          ev.terminal.to(torch.uint8).numpy().copy(), ev.cand_count.to(torch.int32).numpy().copy(),
                          ev.cand_actions.to(torch.int32).numpy().copy(), ev.cand_prior.to(torch.float32).numpy().copy()))
            return ev
        gs = search.gumbel_search(SimpleNamespace(num_envs=P, device="cpu", cfg=None), n, 100, recording, max_considered=Mc, c_visit=c_visit, c_scale=c_scale,
                                  c_puct=rule[0], max_children=C, max_steps=levels, capacity=N, seed=key["seed"], first_root=first_root,
                                  gumbel_step_index=step_index, leaves=leaves, launches=E, node_rule="gumbel" if kernel == "gumbel_tree_leaves" else "puct")
        start = glc.with_leaves(gc.init_state(P, N, C, levels), P, N, leaves, levels)
    seq = gc.search_calls(calls, key)
    t = SimpleNamespace(P=P, N=N, C=C, K=K, L=leaves, n=n, Mc=Mc, rule=rule)
    states = RUNS[kernel][0](t, start, seq, levels)
    case = SimpleNamespace(P=P, N=N, C=C, K=K, L=leaves, n=n, Mc=Mc, rule=rule, state=start, table=search.considered_visits(Mc, n).numpy(), T=levels,
                           levels=levels)
    return case, seq, states, gs, calls
