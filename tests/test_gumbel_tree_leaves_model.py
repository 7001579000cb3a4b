"""csrc/pcb_gumbel_tree_leaves.h -- the full Gumbel rule with L leaves per launch as plain C++ -- against its specification in
pcbenv/search.py, on the CPU: tools/gumbel_tree_leaves_check.cpp (AddressSanitizer + UBSan, a program of its own, nothing
preloaded) runs the cases of tests/gumbel_tree_leaves_cases.py and returns the state after every call.  Every SELECT is redone
leaf by leaf with gumbel_select_root(full=True) at the root and gumbel_node_scores(pending=) below it; CHOOSE is
gumbel_choose(full=True)'s; I1: with L = 1 every tensor is tools/gumbel_tree_check.cpp's; I2: nothing is pending behind an ABSORB;
I3: BEGIN, ABSORB and CHOOSE are those of the functions the header names; the coverage the comparisons stand on; damaged roots,
Msum == -1 among them; whole searches of gumbel_search(node_rule="gumbel", leaves=L) recorded and replayed; a launch worked out by
hand; and the pending visits of one launch against the policy they track."""
import shutil
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import gumbel_cases as gc
import gumbel_leaves_cases as glc
import gumbel_tree_cases as gtc
import gumbel_tree_leaves_cases as gtl
import puct_cases as pc
import puct_leaves_cases as plc
from pcbenv.search import gumbel_choose, gumbel_node_scores, gumbel_search, gumbel_select_node, puct_reroot, search_tree

pytestmark = pytest.mark.skipif(shutil.which("g++") is None, reason="no g++")


def _t(a):
    return torch.from_numpy(np.array(a))  # a copy: the model's states are views of its output, which is not writable


@pytest.mark.parametrize("name,L", gtl.CASES)
def test_the_model_is_the_specification_call_by_call(name, L):
    c = gtl.case(name, L)
    gtl.case_facts(name, L)  # every SELECT, leaf by leaf
    for i, (q, st) in enumerate(zip(c.seq, c.states)):
        was = gtl.before(c, i)
        if q["phases"] & gtl.SELECT and not q["phases"] & gtl.ABSORB:  # SELECT stores nothing to the tree but pending
            for f in gtl.TREE_FIELDS:
                assert pc.same_bits(st[f], was[f].astype(st[f].dtype)), f
        if q["phases"] & gtl.ABSORB and not q["phases"] & gtl.SELECT:  # I2
            assert not st["pending"].any()
        if q["phases"] == gtl.BEGIN | gtl.SELECT:  # BEGIN does not touch pending: it is the SELECT's alone
            assert st["pending"].sum() == (st["path_len"] >= 0).sum() + (st["path_len"].clip(min=0)).sum()
        if q["phases"] & gtl.CHOOSE:
            ch = gumbel_choose(gc.tree_of(st), _t(st["sim_visits"]), c.C, c.rule[1], c.rule[2], q["seed"], q["step_index"], q["first_root"], full=True)
            for f in gtl.OUT_FIELDS:
                want = ch[f].numpy()
                assert pc.same_bits(st[f], want if f in ("child_policy", "root_value") else want.astype(np.int64)), f
            for f in gtl.STATE_FIELDS:  # CHOOSE stores nothing else
                assert pc.same_bits(st[f], was[f].astype(st[f].dtype)), f
        elif i > 0:
            for f in gtl.OUT_FIELDS:
                assert pc.same_bits(st[f], was[f]), f


def test_the_cases_are_what_they_are_there_for():
    """Over the case table some launch takes all L leaves, some root has a repeat, some root runs out of budget at a leaf l >= 1,
    some descent passes a node with pending > 0 on two children, and at some node the pending-aware argmax differs from the
    pending-blind one: gumbel_tree_leaves_cases.WANT, asserted by check_cases on the model's states alone."""
    facts = gtl.check_cases()
    print(dict(facts))
    assert facts["pending_changes_the_child"] > 0 and facts["pending_on_two_children"] > 0 and facts["all_leaves_taken"] > 0


@pytest.mark.parametrize("name", list(gtc.CASES))
def test_I1_one_leaf_is_pcbenv_gumbel_tree_advance(name):
    """L = 1, pending zero: every tensor tools/gumbel_tree_check.cpp writes on gumbel_tree_cases.CASES has the same bits."""
    one, base = gtl.case(name, 1), gtc.case(name)
    assert one.N == base.N and len(one.states) == len(base.states) and (base.state["visits"] >= 0).all()
    for i, (a, b) in enumerate(zip(one.states, base.states)):
        assert a["errors"] == b["errors"], i
        for f in gc.STATE_FIELDS + gc.OUT_FIELDS:
            assert pc.same_bits(a[f], b[f]), (i, f)
        if not one.seq[i]["phases"] & gtl.SELECT:
            assert not a["pending"].any(), i


@pytest.mark.parametrize("name,L", [("G8_C8_P67", 3), ("G64_C64_P67", 8), ("G4_C4_P131", 9)])
def test_I3_begin_absorb_and_choose_are_the_functions_named(name, L):
    """The calls without SELECT of a case, each run on the state it starts from, by both programs: BEGIN and ABSORB against
    tools/gumbel_leaves_check.cpp (gumbel_begin, leaves_absorb), every field; CHOOSE against tools/gumbel_tree_check.cpp
    (tree_choose), which knows no pending and takes the tensors of one leaf."""
    c = gtl.case(name, L)
    seen = set()
    for i, q in enumerate(c.seq):
        start = {f: np.array(v) for f, v in gtl.before(c, i).items() if f in gtl.STATE_FIELDS}
        if q["phases"] & gtl.SELECT:
            if not q["phases"] & gtl.ABSORB:
                continue
            q = dict(q, phases=gtl.ABSORB)  # the ABSORB of an ABSORB | SELECT, alone, on pending as the SELECT before left it
        for phases in ({gtl.ABSORB: (gtl.ABSORB, gtl.BEGIN | gtl.ABSORB)}.get(q["phases"], (q["phases"],))):
            one = dict(q, phases=phases)
            mine = gtl.run(start, c.C, c.K, c.n, c.Mc, L, c.rule, [one])[0]
            if phases & gtl.CHOOSE:
                narrow = dict(start, selected=start["selected"][::L], path_len=start["path_len"][::L], paths=start["paths"][:, ::L])
                theirs = gtc.run(narrow, c.C, c.K, c.n, c.Mc, c.rule, [one])[0]
                fields = gc.TREE_FIELDS + ("sim_index", "sim_visits") + gc.OUT_FIELDS
                seen.add("choose")
            else:
                theirs = glc.run(start, c.C, c.K, c.n, c.Mc, L, c.rule, [one], levels=gtl.T)[0]
                fields = gtl.STATE_FIELDS + gc.OUT_FIELDS
                assert start["pending"].any()  # every ABSORB of a case stands behind a SELECT
                seen.add("begin" if phases & gtl.BEGIN else "absorb")
            assert mine["errors"] == theirs["errors"], (i, phases)
            for f in fields:
                assert pc.same_bits(mine[f], theirs[f]), (i, phases, f)
    assert seen == {"choose", "begin", "absorb"}


@pytest.mark.parametrize("name", list(gtl.DAMAGE))
def test_a_damaged_root_stops_where_the_contract_says(name):
    c, at, seq, states, p, healthy = gtl.damaged(name)
    L = c.L
    q, st = seq[-1], states[-1]
    was = {f: np.array(v) for f, v in gtl.before(c, at).items() if f != "errors"}
    for tensor, flat_index, value in q["pokes"]:
        was[tensor].reshape(-1)[flat_index] = value
    rows = slice(p * L, (p + 1) * L)
    data = name.startswith(("sim_visits", "choose_sim_visits", "pending", "msum"))  # a counter and pending are only ever compared or added: data
    assert bool(st["errors"] & gtl.ERR_TREE) == (not data), name
    if name.startswith("absorb_"):
        assert not healthy["errors"] & gtl.ERR_TREE
        for f in gtl.TREE_FIELDS:  # ABSORB stopped before its first store
            assert pc.same_bits(st[f][p], was[f][p].astype(st[f].dtype)), f
    if name.startswith(("sim_index", "select_")):  # no descent: leaf 0 is the root itself, the others are none, no simulation is consumed
        assert st["selected"][rows].tolist() == [0] + [-1] * (L - 1) and st["path_len"][rows].tolist() == [0] + [-1] * (L - 1)
        assert (st["paths"][:, rows] == was["paths"][:, rows]).all()
        assert st["sim_index"][p] == was["sim_index"][p] and (st["sim_visits"][p] == was["sim_visits"][p]).all()
        assert st["pending"][p, 0] == 1 and not st["pending"][p, 1:].any()
    if name.startswith("below_"):  # every descent ends at the damaged node: one level taken, and the simulation counts
        live = st["selected"][rows] >= 0
        assert live.any() and (st["path_len"][rows][live] == 1).all() and (st["parent"][p, st["selected"][rows][live]] == 0).all()
    if name.startswith("pending"):  # whatever it holds, the stores stay where the healthy run's are and the counters stay counters
        assert (st["selected"][rows] >= -1).all() and (st["selected"][rows] < c.N).all()
        assert np.array_equal(st["sim_visits"][p].sum() - was["sim_visits"][p].sum(), st["sim_index"][p] - was["sim_index"][p])
    if name == gtl.MSUM:
        # leaf 0 of the root went through a child a of the root whose children's counts add up to -1: 1 + Msum == 0, so t is
        # +inf where m_c < 0 -- the poked last child -- -inf where m_c > 0 and NaN, which counts as -inf, where m_c == 0
        assert st["selected"][p * L] >= 1 and st["path_len"][p * L] >= 2
        a = int(st["selected"][p * L])
        while was["parent"][p, was["parent"][p, a]] != 0:
            a = int(was["parent"][p, a])
        node, went = int(was["parent"][p, a]), a
        k, fc = int(was["num_children"][p, node]), int(was["first_child"][p, node])
        m = was["visits"][p, fc:fc + k].astype(np.int64) + was["pending"][p, fc:fc + k]
        assert m.sum() == -1 and m[-1] < 0 and (m[:-1] >= 0).all() and went == fc + k - 1
        ns = gumbel_node_scores(gc.tree_of(was), _t(np.full(c.P, node)), c.C, c.rule[1], c.rule[2], _t(was["pending"]))
        assert int(ns["Msum"][p]) == -1 and float(ns["t"][p, k - 1]) == float("inf") and bool((ns["t"][p, :k - 1] == float("-inf")).all())
        assert int(gumbel_select_node(gc.tree_of(was), _t(np.full(c.P, node)), c.C, c.rule[1], c.rule[2], _t(was["pending"]))["child"][p]) == k - 1
    if name.startswith("choose_") and not data:
        assert st["move_slot"][p] == -1 and not st["move_action"][p].any() and not st["child_weights"][p].any() and not st["child_policy"][p].any() \
            and not st["child_actions"][p].any()
    others = [r for r in range(c.P) if r != p]
    other_rows = [r for r in range(c.P * L) if r // L != p]
    for f in gtl.STATE_FIELDS + gtl.OUT_FIELDS:  # the neighbours are the healthy run's
        take = (lambda a: a[:, other_rows]) if f == "paths" else (lambda a: a[other_rows]) if f in ("selected", "path_len") else (lambda a: a[others])
        assert pc.same_bits(take(st[f]), take(healthy[f])), f


def test_a_nan_counts_as_minus_infinity():
    """One node whose children's counts add up to -1 with the negative count LAST and no count at child 0: t_0 = 0 - 0 / 0 is a
    NaN, t_1 = -inf, t_2 = +inf.  A loop that let the NaN stand would keep child 0, which nothing beats; the order of the
    header takes child 2, in the model and in the specification."""
    st = gtl.one_node_state((0.5, 0.25, 0.25), 1, P=3)
    st["pending"][:, 3], st["pending"][:, 4] = 1, -2
    got = gtl.run(st, 3, 1, 4, 2, 1, (1.25, 50.0, 0.0), [gc.call(gtl.BEGIN | gtl.SELECT)])[0]
    assert got["errors"] == 0 and (got["selected"] == 4).all() and (got["path_len"] == 2).all()
    ns = gumbel_node_scores(gc.tree_of(st), _t(np.ones(3, np.int64)), 3, 50.0, 0.0, _t(st["pending"]))
    assert ns["Msum"].tolist() == [-1] * 3 and ns["t"][0].tolist() == [float("-inf"), float("-inf"), float("inf")]
    blind = gumbel_node_scores(gc.tree_of(st), _t(np.ones(3, np.int64)), 3, 50.0, 0.0)
    assert "Msum" not in blind and blind["t"][0, 0] > 0  # without the argument pending is not read


# ---- a launch worked out by hand -------------------------------------------------------------------------------------------
def test_a_launch_worked_out_by_hand():
    h = gtl.HAND
    st = gtl.one_node_state(h["priors"], h["L"])
    got = gtl.run(st, len(h["priors"]), 1, h["n"], h["Mc"], h["L"], h["rule"], [gc.call(gtl.BEGIN | gtl.SELECT, step_index=3)])[0]
    gtl.check_hand(got)


# ---- the pending visits of one launch track the policy ---------------------------------------------------------------------
def test_the_pending_visits_of_a_launch_track_the_policy():
    """The priors of tests/test_gumbel_tree_model.py -- geometric (2^-(c+1), the last doubled) or uniform over k = 4, 8, 16
    children -- on a hand-made node with no absorbed visit below it, c_scale = 0, so pi is the prior.  One SELECT of L = 64
    leaves sends 64 descents through the node; after the first j = 1 .. 64 of them |pending_c - j * pi_c| <= 1.5 for every child:
    the bound the one-leaf rule keeps for visits."""
    worst = 0.0
    for k in (4, 8, 16):
        for pi in (np.full(k, 1.0 / k), np.array([2.0 ** -(j + 1) for j in range(k - 1)] + [2.0 ** -(k - 1)])):
            assert pi.sum() == 1.0
            st = gtl.one_node_state(pi, 64, P=1)
            got = gtl.run(st, k, 1, 64, 1, 64, (1.25, 50.0, 0.0), [gc.call(gtl.BEGIN | gtl.SELECT)])[0]
            assert got["errors"] == 0 and (got["path_len"] == 2).all() and got["sim_index"][0] == 64
            spec = gumbel_node_scores(gc.tree_of(st), _t(np.ones(1, np.int64)), k, 50.0, 0.0)["pi"][0, :k].numpy()
            assert np.abs(spec - pi).max() < 1e-15
            went = got["paths"][1, :, 2]
            counts = np.zeros(k)
            for j in range(1, 65):
                counts[went[j - 1]] += 1
                worst = max(worst, float(np.abs(counts - j * spec).max()))
            assert np.array_equal(got["pending"][0, 2:], counts.astype(np.int64)) and got["pending"][0, 0] == got["pending"][0, 1] == 64
    print(f"largest |pending_c - j pi_c| over j = 1 .. 64: {worst:.3f}")
    assert worst <= 1.5


# ---- whole searches ------------------------------------------------------------------------------------------------------
SEARCH = dict(P=9, levels=5, n=8, Mc=4, C=4, K=4, rule=(1.25, 50.0, 1.0), key=dict(seed=gc.SEED ^ 5, step_index=(1 << 33) + 3, first_root=4))


def record_search(s, L, evaluate, tree=None, capacity=None, launches=None):
    """gumbel_search(node_rule="gumbel", leaves=L) on the CPU -> (its result, the recorded evaluations)."""
    calls = []

    def recording(paths, path_len, step):
        ev = evaluate(paths, path_len, step)
        calls.append((paths.clone().numpy(), path_len.clone().numpy(), ev.value.to(torch.float64).numpy().copy(),
                      ev.terminal.to(torch.uint8).numpy().copy(), ev.cand_count.to(torch.int32).numpy().copy(),
                      ev.cand_actions.to(torch.int32).numpy().copy(), ev.cand_prior.to(torch.float32).numpy().copy()))
        return ev
    root = SimpleNamespace(num_envs=s["P"], device="cpu", cfg=None)
    gs = gumbel_search(root, s["n"], 100, recording, max_considered=s["Mc"], c_visit=s["rule"][1], c_scale=s["rule"][2], c_puct=s["rule"][0],
                       max_children=s["C"], max_steps=s["levels"], capacity=capacity, tree=tree, seed=s["key"]["seed"], first_root=s["key"]["first_root"],
                       gumbel_step_index=s["key"]["step_index"], leaves=L, launches=launches, node_rule="gumbel")
    return gs, calls


def replay(s, L, gs, calls, start):
    seq = gc.search_calls(calls, s["key"])
    states = gtl.run(start, s["C"], s["K"], s["n"], s["Mc"], L, s["rule"], seq, levels=s["levels"])
    R = s["P"] * L
    for m, st in enumerate(states[:len(calls)]):  # every selection is the recorded one
        want_paths, want_len = calls[m][0], calls[m][1]
        assert np.array_equal(st["path_len"], want_len), m
        for r in range(R):
            assert np.array_equal(st["paths"][:max(want_len[r], 0), r], want_paths[:max(want_len[r], 0), r])
        assert np.array_equal(st["sim_visits"].sum(axis=1), st["sim_index"])
    assert not states[len(calls)]["pending"].any()  # I2: the last ABSORB has taken every leaf
    last = states[-1]
    pc.compare_with_search(dict(last, errors=max(st["errors"] for st in states)), gs.search)
    assert not last["pending"].any()
    assert np.array_equal(last["sim_index"], gs.sim_index.numpy()) and np.array_equal(last["sim_visits"], gs.sim_visits.numpy())
    for f in gtl.OUT_FIELDS:
        want = getattr(gs, f).numpy()
        assert pc.same_bits(last[f], want if f in ("child_policy", "root_value") else want.astype(np.int64)), f
    return states


@pytest.mark.parametrize("L", [2, 3, 4, 8])
def test_a_search_and_the_search_that_follows_it_in_the_kept_tree(L):
    s = SEARCH
    E = -(-s["n"] // L) + 1
    N = 1 + 2 * E * L * s["C"]
    gs, calls = record_search(s, L, plc.leaves_evaluator(s["P"], s["levels"], s["K"], L, 23), capacity=N)
    assert len(calls) == E
    states = replay(s, L, gs, calls, gtl.with_leaves(gc.init_state(s["P"], N, s["C"], s["levels"]), s["P"], N, L, s["levels"]))
    expanded = states[1]["num_children"][:, 0] > 0
    assert expanded.any() and (states[-1]["sim_index"][expanded & (states[-1]["terminal"][:, 0] == 0)] > 0).all()
    tree, _ = puct_reroot(search_tree(gs.search), gs.move_slot)
    s2 = dict(s, key=dict(s["key"], step_index=s["key"]["step_index"] + 1))
    gs2, calls2 = record_search(s2, L, plc.leaves_evaluator(s["P"], s["levels"], s["K"], L, 29), tree=tree)
    states2 = replay(s2, L, gs2, calls2, gtl.with_leaves(gc.state_of(tree, s["P"], s["C"], s["levels"]), s["P"], N, L, s["levels"]))
    kept = (states2[0]["num_children"][:, 0] > 0) & (states2[0]["terminal"][:, 0] == 0)
    assert kept.any() and (states2[-1]["sim_index"][kept] > 0).all()
    assert max(int(st["path_len"].max()) for st in states2[:len(calls2)]) >= 2  # a level below the root's: the node rule had its say


def test_one_leaf_with_launches_is_the_search_of_one_leaf():
    """node_rule="gumbel", leaves=1, launches=n + 1 goes through the leaf loop and pcbenv_gumbel_tree_advance_leaves' model with
    L = 1: the search of full=True, field by field."""
    s = SEARCH
    N = 1 + 2 * (s["n"] + 1) * s["C"]
    gs, calls = record_search(s, 1, pc.synthetic_evaluator(s["P"], s["levels"], s["K"], 23), capacity=N, launches=s["n"] + 1)
    replay(s, 1, gs, calls, gtl.with_leaves(gc.init_state(s["P"], N, s["C"], s["levels"]), s["P"], N, 1, s["levels"]))
    full, _ = gtc.record_search(s["P"], s["levels"], s["n"], s["Mc"], s["C"], pc.synthetic_evaluator(s["P"], s["levels"], s["K"], 23), s["rule"], s["key"],
                                capacity=N)
    for f in ("sim_index", "sim_visits", "move_slot", "move_action", "child_weights", "child_policy", "child_actions", "root_value"):
        assert pc.same_bits(getattr(gs, f).numpy(), getattr(full, f).numpy()), f
    for f in gc.TREE_FIELDS:
        assert pc.same_bits(getattr(gs.search, f).numpy(), getattr(full.search, f).numpy()), f
