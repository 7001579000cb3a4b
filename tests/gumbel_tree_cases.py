"""The cases of pcbenv_gumbel_tree_advance (include/pcbenv_gumbel_tree.h) and its CPU model: the geometry of
tests/gumbel_cases.py -- the six widths, roots across workgroups with a partly filled last one, a step index past 2^32 --
with T = 4 levels and hand-built nodes below every root child, so that levels 1 to 3 run the node rule on every arm of it,
and tools/gumbel_tree_check.cpp -- csrc/pcb_gumbel_tree.h as a program of its own, built with AddressSanitizer and UBSan --
to run them.  tests/test_gumbel_tree_model.py holds the model to the specification (pcbenv/search.py:gumbel_node_scores,
gumbel_select_node, gumbel_select_root and gumbel_choose with full=True), tests/test_gumbel_tree_gpu.py the kernel to the
model.  Plain module, no test; needs no GPU.

A case takes the roots of gumbel_cases.case(name) -- kinds none, term, one, few, full, kept, flat, zero -- and hangs a node of
arm ARMS[(p + c) % len(ARMS)] under child c of root p (the child becomes that node), and two visited children under the first
child of that node.  The arms (n: the visits of the node's children, own = visits(node) - sum n):
  none      no child has a visit, own = 1                      all      every child has one, own = 1
  some      every other child has one, own = 1                 many     as some, own = 3
  own_0     as some, own = 0: vhat is the node's mean          own_neg  as some, own = -1
  blank     no visit at the node or below it: vhat = reward_lo single   k = 1, visited on every other root
  floor     only child 0 has a visit, and its prior is 0: Wv = 2^-149
  big       as some, child 0 with prior 0 and child 1 with prior 1.5
  wide      k = C, as some
The calls are CHOOSE on the trees as built, then gumbel_cases': SELECT alone on preset counters (t >= n among them: the node rule at the root), ABSORB alone,
BEGIN | SELECT, n + 1 times ABSORB | SELECT, ABSORB, CHOOSE.  N leaves room for a few expansions only: ERR_FULL, and then
leaves absorbed more than once (own > 1 the way a search produces it)."""
import functools
from types import SimpleNamespace

import numpy as np
import torch

import gumbel_cases as gc
import model_harness as mh
import puct_cases as pc
from pcbenv.search import considered_visits

BEGIN, ABSORB, SELECT, CHOOSE = gc.BEGIN, gc.ABSORB, gc.SELECT, gc.CHOOSE
ERR_FULL, ERR_TREE = gc.ERR_FULL, gc.ERR_TREE
FILL, SEED, BLOCK = gc.FILL, gc.SEED, gc.BLOCK
T = 4
CASES = gc.CASES
ARMS = ("none", "all", "some", "many", "own_0", "own_neg", "blank", "single", "floor", "big", "wide")
TREE_FIELDS, STATE_FIELDS, OUT_FIELDS, FLOATS, POKED = gc.TREE_FIELDS, gc.STATE_FIELDS, gc.OUT_FIELDS, gc.FLOATS, gc.POKED
DAMAGE_CASE, DAMAGE_ROOT = gc.DAMAGE_CASE, gc.DAMAGE_ROOT
# gumbel_cases' damage at the root, and a child range below the root that fails the check: every child of the root is
# poked, so whichever the root level takes, level 1 meets it
DAMAGE = dict(gc.DAMAGE, below_more_children_than_C=(4, "num_children", lambda N, k, C: C + 1), below_first_child_0=(4, "first_child", lambda N, k, C: 0),
              below_first_child_past_the_end=(4, "first_child", lambda N, k, C: N))

shapes = gc.shapes
call = gc.call
before = gc.before
tree_of = gc.tree_of
init_state = gc.init_state
state_of = gc.state_of
search_calls = gc.search_calls


def program():
    """tools/gumbel_tree_check.cpp as tests/model_harness.py:tool builds it; None without g++."""
    return mh.tool("gumbel_tree_check")


def run(state, C, K, n, Mc, rule, seq, levels=T):
    """gumbel_cases.run on tools/gumbel_tree_check.cpp: the same wire format, states and outputs."""
    P, N = state["parent"].shape
    table = considered_visits(Mc, n).numpy()
    words = [np.array([0, P, N, C, levels, K, n, Mc, len(seq)] + [mh.bits(x) for x in rule], np.int64), table.astype(np.int64).ravel()]
    words += [mh.words(state[f], f in FLOATS) for f in STATE_FIELDS]
    for c in seq:
        words.append(np.array([c["phases"], mh.u64(c["seed"]), mh.u64(c["step_index"]), c["first_root"], len(c["pokes"])] +
                              [w for name, at, value in c["pokes"] for w in (POKED.index(name), at, value)], np.int64))
        if c["phases"] & ABSORB:
            value, over, count, actions, prior = c["evaluation"]
            assert actions.shape == (P, K, 3) and prior.shape == (P, K) and prior.dtype == np.float32
            words += [mh.words(value, True), mh.words(over), mh.words(count), mh.words(actions), mh.float32_words(prior)]
    return mh.cut(mh.run_words(program(), words), len(seq), STATE_FIELDS + OUT_FIELDS, shapes(P, N, C, levels), FLOATS, ("child_policy",))


def node_model(state, node, C, c_visit, c_scale):
    """Mode 1 of the program: the quantities of slot node[p] of every root of `state` -> dict(child, Nsum int64 [P]; logit,
    sigma, pi, t float64 [P, C])."""
    P, N = state["parent"].shape
    words = [np.array([1, P, N, C, mh.bits(c_visit), mh.bits(c_scale)], np.int64)] + [mh.words(state[f], f in FLOATS) for f in TREE_FIELDS]
    out = mh.run_words(program(), words + [mh.words(node)])
    got = dict(child=out[:P], Nsum=out[P:2 * P])
    for i, f in enumerate(("logit", "sigma", "pi", "t")):
        got[f] = out[2 * P + i * P * C:2 * P + (i + 1) * P * C].view(np.float64).reshape(P, C)
    return got


DEEPER = ("all", "some", "many", "own_0", "own_neg", "big", "wide")  # the arms whose child 0 has a visit


def hang(st, p, a, arm, C, free, deepen=False):
    """Makes slot `a` of root p a node of `arm` with its children from slot `free` on -> the next free slot.  deepen: child 0,
    where the arm gives it a visit, becomes a node with two visited children itself."""
    k = {"single": 1, "wide": C}.get(arm, min(C, 2 + (p + a) % 3))
    d = int(st["depth"][p, a])
    for c in range(k):
        s = free + c
        st["parent"][p, s], st["depth"][p, s], st["node_action"][p, s] = a, d + 1, (c % 2, 10 + d, c)
        st["prior"][p, s] = pc.PRIORS[(p + a + c) % len(pc.PRIORS)]
        seen = {"none": False, "blank": False, "all": True, "single": p % 2 == 0, "floor": c == 0}.get(arm, c % 2 == 0)
        n = 1 + (p + c) % 3 if seen else 0
        mean = 0.25 + 0.125 * ((c + p + a) % 5)
        st["visits"][p, s], st["value_sum"][p, s], st["value_max"][p, s] = n, n * mean, mean if n else -np.inf
    if arm == "floor":
        st["prior"][p, free] = 0.0
    if arm == "big" and k >= 2:
        st["prior"][p, free], st["prior"][p, free + 1] = 0.0, 1.5
    end = hang(st, p, free, "all", 2, free + k) if deepen and arm in DEEPER else free + k
    below, S = int(st["visits"][p, free:free + k].sum()), float(st["value_sum"][p, free:free + k].sum())
    own = {"many": 3, "own_0": 0, "own_neg": -1, "blank": 0}.get(arm, 1)
    st["visits"][p, a], st["value_sum"][p, a], st["value_max"][p, a] = below + own, S + max(own, 0) * 0.5, 0.75
    st["num_children"][p, a], st["first_child"][p, a] = k, free
    return end


@functools.lru_cache(maxsize=None)
def case(name):
    """-> SimpleNamespace(name, P, N, C, G, K, n, Mc, rule, kinds, k, state, seq, states, ...) as gumbel_cases.case gives it."""
    g = gc.case(name)
    C, P, K = g.C, g.P, g.K
    used = 4 + 8 * C  # the root's children behind fc <= 3, a node of up to 4 children under each, one of them wide, two below each
    N = used + 2 * K
    i32 = lambda shape, v: np.full(shape, v, np.int32)
    st = dict(selected=i32(P, FILL), path_len=i32(P, FILL), paths=i32((T, P, 3), FILL), num_nodes=i32(P, 1), parent=i32((P, N), -1),
              depth=i32((P, N), 0), visits=i32((P, N), 0), num_children=i32((P, N), 0), first_child=i32((P, N), -1),
              node_action=i32((P, N, 3), 0), prior=np.zeros((P, N)), value_sum=np.zeros((P, N)), value_max=np.full((P, N), -np.inf),
              terminal=np.zeros((P, N), np.uint8), reward_lo=np.array(g.state["reward_lo"]), reward_hi=np.array(g.state["reward_hi"]),
              sim_index=np.array(g.state["sim_index"]), sim_visits=np.array(g.state["sim_visits"]))
    for f in TREE_FIELDS:
        if st[f].ndim >= 2:
            st[f][:, :g.N] = g.state[f]
        else:
            st[f][:] = g.state[f]
    arms = {}
    for p in range(P):
        k, fc = int(st["num_children"][p, 0]), int(st["first_child"][p, 0])
        if k == 0:
            continue
        free = fc + k
        for c in range(k):
            arm = ARMS[(p + c) % len(ARMS)]
            if arm == "wide" and c != 0 and C > 8:
                arm = "some"  # one wide node per root is enough where C is large
            arms[(p, fc + c)] = arm
            free = hang(st, p, fc + c, arm, C, free, deepen=True)
        below = int(st["visits"][p, fc:fc + k].sum())
        own = (1, 1, 2, 0, -1)[p % 5]
        st["visits"][p, 0], st["value_sum"][p, 0] = max(below + own, 1), float(st["value_sum"][p, fc:fc + k].sum()) + max(own, 0) * 0.5
        if g.kinds[p] == "flat":
            st["reward_lo"][p] = st["reward_hi"][p] = 0.5
        elif st["reward_hi"][p] <= st["reward_lo"][p] and p % 3:
            st["reward_lo"][p], st["reward_hi"][p] = 0.125, 0.875
        assert free <= used, (name, p, free, used)
        st["num_nodes"][p] = free
    key = dict(seed=SEED, step_index=g.step_index, first_root=g.first_root)
    seq = [call(CHOOSE, **key)] + [dict(q) for q in g.seq]  # CHOOSE on the hand-built roots too: no child with a visit, no value range
    return SimpleNamespace(name=name, P=P, N=N, C=C, G=g.G, K=K, n=g.n, Mc=g.Mc, rule=g.rule, kinds=g.kinds, k=g.k, state=st, seq=seq, arms=arms,
                           states=run(st, C, K, g.n, g.Mc, g.rule, seq), first_root=g.first_root, step_index=g.step_index, table=g.table, key=key)


def node_arms(st, p, a, C):
    """What the rule meets at node a of root p in state st: the names of the arms of csrc/pcb_gumbel_tree.h it takes."""
    k, fc = int(st["num_children"][p, a]), int(st["first_child"][p, a])
    n = st["visits"][p, fc:fc + k].astype(np.int64)
    pr = st["prior"][p, fc:fc + k]
    own = int(st["visits"][p, a]) - int(n.sum())
    out = {"seen_none" if not (n > 0).any() else "seen_all" if (n > 0).all() else "seen_some",
           "own_1" if own == 1 else "own_many" if own > 1 else "own_0" if own == 0 else "own_negative",
           "flat" if not st["reward_hi"][p] > st["reward_lo"][p] else "range"}
    if own <= 0:
        out.add("vhat_is_the_mean" if st["visits"][p, a] > 0 else "vhat_is_lo")
    if (pr <= 0).any():
        out.add("zero_prior")
    if (pr > 1).any():
        out.add("prior_above_1")
    if k == 1:
        out.add("k_1")
    if k == C:
        out.add("k_C")
    if n.sum() > 0 and ((n > 0) & (pr <= 2.0 ** -149)).any() and ((n > 0) <= (pr <= 2.0 ** -149)).all():
        out.add("Wv_at_the_floor")
    return out


def chain(st, p):
    """The nodes the descent of root p went through in state st, the root first, `selected` not among them."""
    node, out = int(st["selected"][p]), []
    while node > 0:
        node = int(st["parent"][p, node])
        out.append(node)
    return out[::-1]


@functools.lru_cache(maxsize=None)
def damaged(name):
    """gumbel_cases.damaged on these cases; a `below_` damage pokes every child of the root."""
    c = case(DAMAGE_CASE)
    p = DAMAGE_ROOT
    assert c.kinds[p] == "kept" and 0 < p < c.P - 1
    at, tensor, value = DAMAGE[name]
    at = at % len(c.seq)
    shp = shapes(c.P, c.N, c.C, T)
    was = before(c, at)
    k, fc = int(was["num_children"][p, 0]), int(was["first_child"][p, 0])
    if name.startswith("below_"):
        pokes = tuple((tensor, pc.flat(shp[tensor], p, fc + j), int(value(c.N, k, c.C))) for j in range(k))
    else:
        index = (p,) if len(shp[tensor]) == 1 else (p, 0)
        pokes = ((tensor, pc.flat(shp[tensor], *index), int(value(c.N, k, c.C))),)
    seq = list(c.seq[:at]) + [dict(c.seq[at], pokes=pokes)]
    return c, at, seq, run(c.state, c.C, c.K, c.n, c.Mc, c.rule, seq), p


@functools.lru_cache(maxsize=None)
def check_cases():
    """The table is what it is there for: every group width, roots across workgroups with a partly filled last group, and on
    the model's states every arm of the rule, at the root and below it, down to level 3.  -> the cases."""
    cases = [case(name) for name in CASES]
    assert {c.G for c in cases} == {4, 8, 16, 32, 64} and all(c.P == (131 if c.G == 4 else 67) for c in cases)
    assert all(c.P > BLOCK // c.G and c.P % (BLOCK // c.G) for c in cases)
    assert any(c.step_index >> 32 for c in cases) and any(c.first_root for c in cases) and any(c.rule[2] == 0.0 for c in cases)
    below, at_root, levels, seen = set(), set(), set(), set()
    for c in cases:
        assert set(ARMS) <= set(c.arms.values()) or c.C < 4
        for i, (q, st) in enumerate(zip(c.seq, c.states)):
            seen.update({1: "err_full", 2: "err_tree", 3: "err_full"}.get(st["errors"], "ok").split())
            if q["phases"] & CHOOSE:
                for p in range(c.P):
                    if st["num_children"][p, 0] > 0:
                        at_root |= {"choose_" + a for a in node_arms(st, p, 0, c.C)}
            if not q["phases"] & SELECT:
                continue
            was = before(c, i)
            for p in range(c.P):
                t = int(0 if q["phases"] & BEGIN else was["sim_index"][p])
                nodes = chain(st, p)
                assert len(nodes) == st["path_len"][p]
                levels.add(int(st["path_len"][p]))
                for a in nodes:
                    if a == 0 and t < c.n:
                        at_root |= {"scheduled_" + arm for arm in node_arms(st, p, 0, c.C)}
                    elif a == 0:
                        at_root |= {"spent_" + arm for arm in node_arms(st, p, 0, c.C)}
                    else:
                        below |= node_arms(st, p, a, c.C)
        assert c.states[-1]["errors"] == 0
    want = {"seen_none", "seen_all", "seen_some", "own_1", "own_many", "own_0", "own_negative", "flat", "range", "vhat_is_the_mean", "vhat_is_lo",
            "zero_prior", "prior_above_1", "k_1", "k_C", "Wv_at_the_floor"}
    assert want <= below, want - below
    for phase in ("scheduled_", "spent_", "choose_"):
        need = {phase + a for a in ("seen_none", "seen_all", "seen_some", "own_1", "own_many", "own_0", "own_negative", "flat", "range", "zero_prior",
                                    "prior_above_1", "k_1", "k_C")}
        assert need <= at_root, need - at_root
    assert {0, 1, 2, 3, 4} <= levels and {"ok", "err_full"} <= seen
    for name in DAMAGE:
        c, at, seq, states, p = damaged(name)
        if not name.startswith(("sim_visits", "choose_sim_visits")):
            assert states[-1]["errors"] & ERR_TREE, name
    return cases


def record_search(P, levels, n, Mc, C, evaluate, rule, key, tree=None, capacity=None):
    """gumbel_search(full=True) on the CPU -> (its result, the recorded evaluations as gumbel_cases.record_search keeps them)."""
    from pcbenv.search import gumbel_search
    calls = []

    def recording(paths, path_len, s):
        ev = evaluate(paths, path_len, s)
        calls.append((paths.clone().numpy(), path_len.clone().numpy(), ev.value.to(torch.float64).numpy().copy(),
                      ev.terminal.to(torch.uint8).numpy().copy(), ev.cand_count.to(torch.int32).numpy().copy(),
                      ev.cand_actions.to(torch.int32).numpy().copy(), ev.cand_prior.to(torch.float32).numpy().copy()))
        return ev
    root = SimpleNamespace(num_envs=P, device="cpu", cfg=None)
    gs = gumbel_search(root, n, 100, recording, max_considered=Mc, c_visit=rule[1], c_scale=rule[2], c_puct=rule[0], max_children=C, max_steps=levels,
                       capacity=capacity, tree=tree, seed=key["seed"], first_root=key["first_root"], gumbel_step_index=key["step_index"], full=True)
    return gs, calls
