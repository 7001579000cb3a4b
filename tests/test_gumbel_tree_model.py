"""csrc/pcb_gumbel_tree.h -- Gumbel's non-root rule and v_mix as plain C++ -- against its specification in pcbenv/search.py,
on the CPU: tools/gumbel_tree_check.cpp (AddressSanitizer + UBSan, a program of its own, nothing preloaded) runs the cases of
tests/gumbel_tree_cases.py and returns the state after every call.  Level 0 of every SELECT and every CHOOSE must be
gumbel_select_root's and gumbel_choose's with full=True bit for bit, every level below gumbel_select_node's, and the
quantities of a node gumbel_node_scores'; the levels below the root are redone in Python floats; one node is worked out by
hand; the two identities with pcbenv_gumbel_advance; damaged roots; whole searches, gumbel_search(full=True) recorded and
replayed; and the visit counts of the rule against the policy they track."""
import math
import shutil

import numpy as np
import pytest
import torch

import gumbel_tree_cases as gt
import puct_cases as pc
from pcbenv.search import (gumbel_choose, gumbel_node_scores, gumbel_select_node, gumbel_select_root, puct_reroot, search_tree)

pytestmark = pytest.mark.skipif(shutil.which("g++") is None, reason="no g++")


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a))


def _rule(c, q):
    return (c.C, c.rule[1], c.rule[2], q["seed"], q["step_index"], q["first_root"])


def _floats_child(c, st, p, a):
    """The rule at node a of root p in plain Python floats, with math.log and math.exp -> (the child, the margin of its t over
    the next best): an independent restatement, good to the last bits, so only a clear margin is a verdict."""
    k, fc = int(st["num_children"][p, a]), int(st["first_child"][p, a])
    lo, hi = float(st["reward_lo"][p]), float(st["reward_hi"][p])
    n = [int(st["visits"][p, fc + j]) for j in range(k)]
    vs = [float(st["value_sum"][p, fc + j]) for j in range(k)]
    pr = [min(max(float(st["prior"][p, fc + j]), 2.0 ** -149), 1.0) for j in range(k)]
    N, own = sum(n), int(st["visits"][p, a]) - sum(n)
    vhat = (float(st["value_sum"][p, a]) - sum(vs)) / own if own > 0 else float(st["value_sum"][p, a]) / int(st["visits"][p, a]) if st["visits"][p, a] > 0 else lo
    Wv = sum(pr[j] for j in range(k) if n[j] > 0)
    Qv = sum(pr[j] * vs[j] / n[j] for j in range(k) if n[j] > 0)
    vmix = (vhat + N / Wv * Qv) / (1 + N) if N > 0 and Wv > 0 else vhat
    q = [((vs[j] / n[j] if n[j] > 0 else vmix) - lo) / (hi - lo) if hi > lo else 0.0 for j in range(k)]
    x = [math.log(pr[j]) + (c.rule[1] + max(n)) * c.rule[2] * q[j] for j in range(k)]
    e = [math.exp(v - max(x)) for v in x]
    t = [e[j] / sum(e) - n[j] / (1 + N) for j in range(k)]
    best = max(range(k), key=lambda j: (t[j], -j))
    return best, min([t[best] - t[j] for j in range(k) if j != best], default=1.0)


def check_call(c, q, was, st, damaged=()):
    """One call of the model against the specification: `was` the state before it, `st` after it."""
    tree, table, P = gt.tree_of(st), _t(c.table), c.P
    bit, clear = 0, 0
    if q["phases"] & gt.SELECT:
        begun = q["phases"] & gt.BEGIN
        t0, v0 = (np.zeros_like(was["sim_index"]), np.zeros_like(was["sim_visits"])) if begun else (was["sim_index"], was["sim_visits"])
        sel = gumbel_select_root(tree, _t(t0), _t(v0), table, *_rule(c, q), full=True)
        assert np.array_equal(sel["sim_index"].numpy(), st["sim_index"]) and np.array_equal(sel["sim_visits"].numpy(), st["sim_visits"])
        bit |= int(sel["errors"])
        # the descent of every root at once, level by level, as the specification takes it
        rows = torch.arange(P)
        k0, fc0 = tree["num_children"][:, 0].long(), tree["first_child"][:, 0].long()
        ok0 = (k0 >= 1) & (k0 <= c.C) & (fc0 >= 1) & (fc0 <= c.N - k0)
        node, plen = torch.zeros(P, dtype=torch.int64), torch.zeros(P, dtype=torch.int64)
        stopped = (tree["terminal"][:, 0] != 0) | (k0 == 0) | ~ok0 | (_t(t0).long() < 0)
        for d in range(gt.T):
            k = tree["num_children"].long()[rows, node]
            stopped = stopped | (tree["terminal"][rows, node] != 0) | (k == 0)
            rule = gumbel_select_node(tree, node, c.C, c.rule[1], c.rule[2])
            bad = ~stopped & ~rule["ok"]
            bit |= 2 * int(bad.any())
            stopped = stopped | bad
            nxt = tree["first_child"].long()[rows, node] + rule["child"]
            if d == 0:
                nxt = torch.where(sel["scheduled"], fc0 + sel["child"], nxt)
            for p in range(P):
                if not stopped[p]:
                    assert (st["paths"][d, p] == st["node_action"][p, int(nxt[p])]).all(), (d, p)
                    if d > 0 or not sel["scheduled"][p]:
                        child, margin = _floats_child(c, st, p, int(node[p]))
                        if margin > 1e-9:
                            clear += 1
                            assert child == int(rule["child"][p]), (d, p, margin)
            node = torch.where(stopped, node, nxt)
            plen = plen + (~stopped).long()
        assert np.array_equal(node.numpy(), st["selected"]) and np.array_equal(plen.numpy(), st["path_len"])
        for p in range(P):
            assert (st["paths"][int(plen[p]):, p] == was["paths"][int(plen[p]):, p]).all()  # the rows not taken are untouched
        if not q["phases"] & gt.ABSORB:  # SELECT never stores to the tree
            for f in gt.TREE_FIELDS:
                assert pc.same_bits(st[f], was[f].astype(st[f].dtype)), f
    if q["phases"] & gt.CHOOSE:
        ch = gumbel_choose(tree, _t(st["sim_visits"]), *_rule(c, q), full=True)
        bit |= int(ch["errors"])
        for f in gt.OUT_FIELDS:
            got, want = st[f], ch[f].numpy()
            assert pc.same_bits(got, want if f in ("child_policy", "root_value") else want.astype(np.int64)), f
        for f in gt.STATE_FIELDS:
            assert pc.same_bits(st[f], was[f].astype(st[f].dtype)), f
    else:
        for f in gt.OUT_FIELDS:
            assert pc.same_bits(st[f], was[f]) if f in was else (st[f] == gt.FILL).all(), f
    if not q["phases"] & gt.ABSORB:
        assert st["errors"] == bit
    else:
        assert st["errors"] & gt.ERR_TREE == bit or damaged
    return bit, clear


def test_the_cases_are_what_they_are_there_for():
    gt.check_cases()


@pytest.mark.parametrize("name", list(gt.CASES))
def test_the_model_is_the_specification_call_by_call(name):
    c = gt.case(name)
    clear = 0
    for i, (q, st) in enumerate(zip(c.seq, c.states)):
        bit, n = check_call(c, q, dict(gt.before(c, i)), st)
        assert bit == 0
        clear += n
    assert clear >= c.P  # the restatement in floats had its say
    last = c.states[-1]
    for p in range(c.P):
        k = int(last["num_children"][p, 0])
        if k:
            pol = last["child_policy"][p, :k].astype(np.float64)
            assert (pol >= 0).all() and abs(pol.sum() - 1.0) <= k * 2.0 ** -24 and (last["child_policy"][p, k:] == 0).all()
        else:
            assert last["move_slot"][p] == -1 and not last["child_weights"][p].any()


@pytest.mark.parametrize("name", ["G4_C3_P131", "G16_C16_P67", "G64_C64_P67"])
def test_the_quantities_of_a_node_are_the_specifications(name):
    """logit, sigma, pi and t of the root, of a root child and of a node two levels down, per root, bit for bit."""
    c = gt.case(name)
    for st in (c.state, c.states[-2]):
        tree = gt.tree_of(st)
        fc = np.where(st["num_children"][:, 0] > 0, st["first_child"][:, 0], 0).astype(np.int64)
        deep = np.where(st["num_children"][np.arange(c.P), fc] > 0, st["first_child"][np.arange(c.P), fc], 0).astype(np.int64)
        for node in (np.zeros(c.P, np.int64), fc, fc + (st["num_children"][:, 0] > 1), deep):
            got = gt.node_model(st, node, c.C, c.rule[1], c.rule[2])
            want = gumbel_node_scores(tree, _t(node), c.C, c.rule[1], c.rule[2])
            goes = want["ok"].numpy() & (st["terminal"][np.arange(c.P), node] == 0)
            assert goes.any()
            mine = want["mine"].numpy() & goes[:, None]
            for f in ("logit", "sigma", "pi", "t"):
                assert pc.same_bits(np.where(mine, got[f], 0.0), np.where(mine, want[f].numpy(), 0.0)), f
                assert not got[f][~mine].any()
            assert np.array_equal(got["Nsum"][goes], want["Nsum"].numpy()[goes])
            rule = gumbel_select_node(tree, _t(node), c.C, c.rule[1], c.rule[2])
            assert np.array_equal(got["child"][goes], rule["child"].numpy()[goes]) and (got["child"][~goes] == -1).all()


def _node(k, visits, value_sum, prior, node_visits, node_sum, lo, hi):
    st = gt.init_state(1, k + 1, k, gt.T)
    st["num_children"][0, 0], st["first_child"][0, 0], st["num_nodes"][0] = k, 1, k + 1
    st["visits"][0], st["value_sum"][0], st["prior"][0] = [node_visits] + visits, [node_sum] + value_sum, [0.0] + prior
    st["parent"][0, 1:], st["depth"][0, 1:], st["reward_lo"][0], st["reward_hi"][0] = 0, 1, lo, hi
    return st


def test_one_node_by_hand():
    """Two children with priors 1/4 and 3/4, the first visited once with value 3/4; the node has two visits and value_sum 5/4,
    so S = 3/4, own = 1, vhat = 1/2, Wv = 1/4, Qv = 3/16, Nsum = 1 and vmix = (1/2 + (1 / (1/4)) * 3/16) / 2 = 5/8.  With [lo,
    hi] = [0, 1], c_visit = 3 and c_scale = 1/2 the factor is (3 + 1) / 2 = 2: sigma = (3/2, 5/4), every step exact."""
    st = _node(2, [1, 0], [0.75, 0.0], [0.25, 0.75], 2, 1.25, 0.0, 1.0)
    got = gt.node_model(st, np.zeros(1, np.int64), 2, 3.0, 0.5)
    assert got["sigma"][0].tolist() == [1.5, 1.25] and got["Nsum"][0] == 1
    assert np.allclose(got["logit"][0], [math.log(0.25), math.log(0.75)], rtol=0, atol=1e-15)
    e = [math.exp(math.log(0.25) + 1.5), math.exp(math.log(0.75) + 1.25)]
    assert np.allclose(got["pi"][0], [e[0] / sum(e), e[1] / sum(e)], rtol=0, atol=1e-15)
    assert np.allclose(got["t"][0], [e[0] / sum(e) - 0.5, e[1] / sum(e)], rtol=0, atol=1e-15) and got["child"][0] == 1
    want = gumbel_node_scores(gt.tree_of(st), torch.zeros(1, dtype=torch.int64), 2, 3.0, 0.5)
    assert float(want["vhat"][0]) == 0.5 and float(want["vmix"][0]) == 0.625 and want["sigma"][0].tolist() == [1.5, 1.25]
    # equal priors, the visited child's value the node's own: vmix = (1/2 + 2 * 1/4) / 2 = 1/2, sigma equal, pi = (1/2, 1/2)
    # exactly, t = (1/2 - 1/2, 1/2): the unvisited child.  With two visits at child 0 and none at the node beyond them the
    # mean stands in for vhat
    st = _node(2, [1, 0], [0.5, 0.0], [0.5, 0.5], 2, 1.0, 0.0, 1.0)
    got = gt.node_model(st, np.zeros(1, np.int64), 2, 3.0, 0.5)
    assert got["pi"][0].tolist() == [0.5, 0.5] and got["t"][0].tolist() == [0.0, 0.5] and got["child"][0] == 1 and got["sigma"][0].tolist() == [1.0, 1.0]
    st = _node(2, [2, 0], [1.0, 0.0], [0.5, 0.5], 2, 1.5, 0.0, 1.0)  # own = 0: vhat = 3/4, vmix = (3/4 + 4 * 1/4) / 3 = 7/12
    want = gumbel_node_scores(gt.tree_of(st), torch.zeros(1, dtype=torch.int64), 2, 3.0, 0.5)
    assert float(want["vhat"][0]) == 0.75 and float(want["vmix"][0]) == (0.75 + 4.0 * 0.25) / 3.0
    got = gt.node_model(st, np.zeros(1, np.int64), 2, 3.0, 0.5)
    assert pc.same_bits(got["sigma"][0], want["sigma"][0].numpy())


def test_the_two_identities_with_the_root_rule():
    """c_scale == 0: level 0 of a scheduled SELECT and CHOOSE have pcbenv_gumbel_advance's bits.  Any c_scale: the same at a root
    whose children all have a visit, where vmix is not read."""
    c = gt.case("G32_C20_P67")
    assert c.rule[2] == 0.0
    scheduled = 0
    for i in (0, 3, 5, len(c.seq) - 1):
        q, st = c.seq[i], c.states[i]
        tree, args = gt.tree_of(st), _rule(c, q)
        a, b = gumbel_choose(tree, _t(st["sim_visits"]), *args, full=True), gumbel_choose(tree, _t(st["sim_visits"]), *args)
        for f in gt.OUT_FIELDS:
            assert pc.same_bits(a[f].numpy(), b[f].numpy()), f
        was = gt.before(c, i)
        a = gumbel_select_root(tree, _t(was["sim_index"]), _t(was["sim_visits"]), _t(c.table), *args, full=True)
        b = gumbel_select_root(tree, _t(was["sim_index"]), _t(was["sim_visits"]), _t(c.table), *args)
        assert all(pc.same_bits(a[f].numpy(), b[f].numpy()) for f in ("scheduled", "child", "sim_index", "sim_visits"))
        scheduled += int(a["scheduled"].sum())
    assert scheduled >= c.P
    c = gt.case("G8_C8_P67")
    st = {f: np.array(v) for f, v in c.states[-2].items() if f != "errors"}
    for p in range(c.P):  # every child of every root gets a visit
        k, fc = int(st["num_children"][p, 0]), int(st["first_child"][p, 0])
        for s in range(fc, fc + k):
            if st["visits"][p, s] <= 0:
                st["visits"][p, s], st["value_sum"][p, s] = 1 + s % 2, 0.375 * (1 + s % 2)
    tree, args = gt.tree_of(st), _rule(c, c.seq[-1])
    a, b = gumbel_choose(tree, _t(st["sim_visits"]), *args, full=True), gumbel_choose(tree, _t(st["sim_visits"]), *args)
    for f in gt.OUT_FIELDS:
        assert pc.same_bits(a[f].numpy(), b[f].numpy()), f
    model = gt.run(st, c.C, c.K, c.n, c.Mc, c.rule, [c.seq[-1]])[0]
    assert pc.same_bits(model["child_policy"], b["child_policy"].numpy()) and np.array_equal(model["move_slot"], b["move_slot"].numpy())
    # and it is an identity of these roots, not of the rule: as the search left them the two differ
    tree = gt.tree_of(c.states[-2])
    a, b = gumbel_choose(tree, _t(st["sim_visits"]), *args, full=True), gumbel_choose(tree, _t(st["sim_visits"]), *args)
    assert not pc.same_bits(a["child_policy"].numpy(), b["child_policy"].numpy())


@pytest.mark.parametrize("name", list(gt.DAMAGE))
def test_a_damaged_root_stops_where_the_contract_says(name):
    c, at, seq, states, p = gt.damaged(name)
    q, st, healthy = seq[-1], states[-1], c.states[at]
    was = {f: np.array(v) for f, v in gt.before(c, at).items() if f != "errors"}
    for tensor, flat_index, value in q["pokes"]:
        was[tensor].reshape(-1)[flat_index] = value
    counters = name.startswith(("sim_visits", "choose_sim_visits"))  # a counter is only ever compared: data, not damage
    if name.startswith("absorb_"):
        assert st["errors"] & gt.ERR_TREE and not healthy["errors"] & gt.ERR_TREE
        for f in gt.TREE_FIELDS:  # ABSORB stopped before its first store
            assert pc.same_bits(st[f][p], was[f][p].astype(st[f].dtype)), f
    else:
        bit, _ = check_call(c, q, was, st, damaged=() if counters else (p,))
        assert bit == (0 if counters else gt.ERR_TREE)
    if name.startswith("sim_index"):
        assert st["sim_index"][p] == q["pokes"][0][2] and (st["sim_visits"][p] == was["sim_visits"][p]).all() and (st["paths"][:, p] == was["paths"][:, p]).all()
        assert st["selected"][p] == 0 and st["path_len"][p] == 0
    if name.startswith("select_"):
        assert st["selected"][p] == 0 and st["path_len"][p] == 0
    if name.startswith("below_"):  # the descent ends at the damaged node: one level taken
        assert st["path_len"][p] == 1 and st["parent"][p, st["selected"][p]] == 0
    if name.startswith("choose_") and not counters:
        assert st["move_slot"][p] == -1 and not st["move_action"][p].any() and not st["child_weights"][p].any() and not st["child_policy"][p].any() \
            and not st["child_actions"][p].any()
    others = [r for r in range(c.P) if r != p]
    for f in gt.STATE_FIELDS + gt.OUT_FIELDS:  # the neighbours are the healthy run's
        rows = (lambda a: a[:, others]) if f == "paths" else (lambda a: a[others])
        assert pc.same_bits(rows(st[f]), rows(healthy[f])), f


# ---- whole searches ------------------------------------------------------------------------------------------------------
SEARCH = dict(P=9, levels=5, n=8, Mc=4, C=4, K=4, rule=(1.25, 50.0, 1.0), key=dict(seed=gt.SEED ^ 5, step_index=(1 << 33) + 3, first_root=4))


def _replay(gs, calls, start, s=SEARCH):
    seq = gt.search_calls(calls, s["key"])
    states = gt.run(start, s["C"], s["K"], s["n"], s["Mc"], s["rule"], seq, levels=s["levels"])
    for m, st in enumerate(states[:len(calls)]):  # every selection is the recorded one
        want_paths, want_len = calls[m][0], calls[m][1]
        assert np.array_equal(st["path_len"], want_len)
        for p in range(s["P"]):
            assert np.array_equal(st["paths"][:want_len[p], p], want_paths[:want_len[p], p])
    last = states[-1]
    pc.compare_with_search(dict(last, errors=max(st["errors"] for st in states)), gs.search)
    assert np.array_equal(last["sim_index"], gs.sim_index.numpy()) and np.array_equal(last["sim_visits"], gs.sim_visits.numpy())
    for f in gt.OUT_FIELDS:
        want = getattr(gs, f).numpy()
        assert pc.same_bits(last[f], want if f in ("child_policy", "root_value") else want.astype(np.int64)), f
    return states


def test_a_search_and_the_search_that_follows_it_in_the_kept_tree():
    s = SEARCH
    N = 1 + 2 * (s["n"] + 1) * s["C"]
    ev = pc.synthetic_evaluator(s["P"], s["levels"], s["K"], 23)
    gs, calls = gt.record_search(s["P"], s["levels"], s["n"], s["Mc"], s["C"], ev, s["rule"], s["key"], capacity=N)
    assert len(calls) == s["n"] + 1
    states = _replay(gs, calls, gt.init_state(s["P"], N, s["C"], s["levels"]))
    assert max(int(st["path_len"].max()) for st in states[:len(calls)]) >= 2  # the node rule below the root had its say
    tree, _ = puct_reroot(search_tree(gs.search), gs.move_slot)
    key = dict(s["key"], step_index=s["key"]["step_index"] + 1)
    gs2, calls2 = gt.record_search(s["P"], s["levels"], s["n"], s["Mc"], s["C"], pc.synthetic_evaluator(s["P"], s["levels"], s["K"], 29), s["rule"], key,
                                   tree=tree)
    states2 = _replay(gs2, calls2, gt.state_of(tree, s["P"], s["C"], s["levels"]), dict(s, key=key))
    kept = (states2[0]["num_children"][:, 0] > 0) & (states2[0]["terminal"][:, 0] == 0)
    assert kept.any() and (states2[-1]["sim_index"][kept] == s["n"]).all()
    assert (states2[-1]["visits"][kept, 0] - states2[0]["visits"][kept, 0] == s["n"] + 1).all()
    assert max(int(st["path_len"].max()) for st in states2[:len(calls2)]) >= 3


# ---- the visit counts track the policy -------------------------------------------------------------------------------------
def test_the_visits_of_a_node_track_its_policy():
    """c_scale = 0, so pi is the prior: geometric (2^-(c+1), the last doubled) or uniform over k = 4, 8, 16 children.  A root
    whose budget is spent takes the node rule at level 0; its children are leaves that never expand.  After m = 1 .. 256 visits
    through the node |n_c - m * pi_c| < 1.5 for every child (a simulation of the rule gives at most 1.03 for these priors)."""
    ks, C, M = (4, 8, 16), 16, 256
    P, N = 2 * len(ks), C + 1
    st = gt.init_state(P, N, C, gt.T)
    pis = []
    for p in range(P):
        k = ks[p // 2]
        pi = np.full(k, 1.0 / k) if p % 2 else np.array([2.0 ** -(j + 1) for j in range(k - 1)] + [2.0 ** -(k - 1)])
        assert pi.sum() == 1.0
        pis.append(pi)
        st["num_children"][p, 0], st["first_child"][p, 0], st["num_nodes"][p] = k, 1, k + 1
        st["visits"][p, 0], st["value_sum"][p, 0], st["value_max"][p, 0] = 1, 0.5, 0.5
        st["parent"][p, 1:k + 1], st["depth"][p, 1:k + 1], st["prior"][p, 1:k + 1] = 0, 1, pi
        st["node_action"][p, 1:k + 1, 2] = np.arange(k)
    st["reward_lo"][:], st["reward_hi"][:], st["sim_index"][:], st["sim_visits"][:] = 0.5, 0.5, 1, 0
    nothing = (np.full(P, 0.5), np.zeros(P, np.uint8), np.zeros(P, np.int32), np.zeros((P, 1, 3), np.int32), np.zeros((P, 1), np.float32))
    seq = [gt.call(gt.SELECT)] + [gt.call(gt.ABSORB | gt.SELECT, nothing) for _ in range(M)]
    states = gt.run(st, C, 1, 1, 1, (1.25, 50.0, 0.0), seq)
    worst = 0.0
    for m in range(1, M + 1):
        s = states[m]
        assert s["errors"] == 0 and (s["path_len"] == 1).all() and (s["sim_index"] == 1).all()
        for p in range(P):
            n = s["visits"][p, 1:len(pis[p]) + 1]
            assert n.sum() == m
            worst = max(worst, float(np.abs(n - m * pis[p]).max()))
    print(f"largest |n_c - m pi_c| over m = 1 .. {M}: {worst:.3f}")
    assert worst < 1.5
