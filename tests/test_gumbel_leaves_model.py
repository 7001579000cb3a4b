"""csrc/pcb_gumbel_leaves.h -- the Gumbel root rule with L leaves per launch as plain C++ -- against its specification in
pcbenv/search.py, on the CPU: tools/gumbel_leaves_check.cpp (AddressSanitizer + UBSan, a program of its own, nothing
preloaded) runs the cases of tests/gumbel_leaves_cases.py and returns the state after every call.  Every SELECT is redone leaf
by leaf with gumbel_select_root at the root and Python floats below it; CHOOSE is gumbel_choose's; with L = 1 every tensor is
tools/gumbel_check.cpp's; whole searches of gumbel_search(leaves=L) are recorded and replayed; and a launch worked out by
hand."""
import shutil
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import gumbel_cases as gc
import gumbel_leaves_cases as glc
import puct_cases as pc
import puct_leaves_cases as plc
from pcbenv.search import gumbel_choose, gumbel_search, puct_reroot, search_tree

pytestmark = pytest.mark.skipif(shutil.which("g++") is None, reason="no g++")


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a))


def test_the_cases_are_what_they_are_there_for():
    facts = glc.check_cases()
    print(dict(facts))


def check_counters(c, i, q, st):
    """The counters of a healthy root move together: what a call adds to sim_index it adds to the sum of sim_visits; from the
    BEGIN of the move on the two are equal.  (Call 0 starts from preset counters that say different things on purpose.)"""
    was = glc.before(c, i)
    if q["phases"] & glc.BEGIN or i > 2:
        assert np.array_equal(st["sim_visits"].sum(axis=1), st["sim_index"]), i
    else:
        assert np.array_equal(st["sim_visits"].sum(axis=1) - was["sim_visits"].sum(axis=1), st["sim_index"] - was["sim_index"]), i


@pytest.mark.parametrize("name,L", glc.CASES)
def test_the_model_is_the_specification_call_by_call(name, L):
    c = glc.case(name, L)
    for i, (q, st) in enumerate(zip(c.seq, c.states)):
        was = glc.before(c, i)
        check_counters(c, i, q, st)
        if q["phases"] & glc.SELECT:
            glc.redo_select(c, q, was, st)
            if not q["phases"] & glc.ABSORB:  # SELECT stores nothing to the tree but pending
                for f in glc.TREE_FIELDS:
                    assert pc.same_bits(st[f], was[f].astype(st[f].dtype)), f
        if q["phases"] & glc.ABSORB and not q["phases"] & glc.SELECT:
            assert not st["pending"].any()  # after the ABSORB of every SELECT nothing is pending
        if q["phases"] == glc.BEGIN | glc.SELECT:  # BEGIN does not touch pending: it is the SELECT's alone
            assert st["pending"].sum() == (st["path_len"] >= 0).sum() + (st["path_len"].clip(min=0)).sum()
        if q["phases"] & glc.CHOOSE:
            ch = gumbel_choose(gc.tree_of(st), _t(st["sim_visits"]), c.C, c.rule[1], c.rule[2], q["seed"], q["step_index"], q["first_root"])
            for f in glc.OUT_FIELDS:
                want = ch[f].numpy()
                assert pc.same_bits(st[f], want if f in ("child_policy", "root_value") else want.astype(np.int64)), f
            for f in glc.STATE_FIELDS:  # CHOOSE stores nothing else
                assert pc.same_bits(st[f], was[f].astype(st[f].dtype)), f
        else:
            for f in glc.OUT_FIELDS:
                assert (st[f] == glc.FILL).all(), f
        assert not st["errors"] & glc.ERR_TREE


@pytest.mark.parametrize("name", list(gc.CASES))
def test_one_leaf_is_pcbenv_gumbel_advance(name):
    """L = 1, pending zero: every tensor tools/gumbel_check.cpp writes on gumbel_cases.CASES has the same bits."""
    one, base = glc.case(name, 1), gc.case(name)
    assert one.N == base.N and len(one.states) == len(base.states)
    for i, (a, b) in enumerate(zip(one.states, base.states)):
        assert a["errors"] == b["errors"], i
        for f in gc.STATE_FIELDS + gc.OUT_FIELDS:
            assert pc.same_bits(a[f], b[f]), (i, f)


@pytest.mark.parametrize("name", list(glc.DAMAGE))
def test_a_damaged_root_stops_where_the_contract_says(name):
    c, at, seq, states, p = glc.damaged(name)
    L = c.L
    q, st, healthy = seq[-1], states[-1], c.states[at]
    was = {f: np.array(v) for f, v in glc.before(c, at).items() if f != "errors"}
    tensor, flat_index, value = q["pokes"][0]
    was[tensor].reshape(-1)[flat_index] = value
    rows = slice(p * L, (p + 1) * L)
    data = name.startswith(("sim_visits", "choose_sim_visits", "pending"))  # a counter and pending are only ever compared or added: data
    assert bool(st["errors"] & glc.ERR_TREE) == (not data), name
    if name.startswith("absorb_"):
        assert not healthy["errors"] & glc.ERR_TREE
        for f in glc.TREE_FIELDS:  # ABSORB stopped before its first store
            assert pc.same_bits(st[f][p], was[f][p].astype(st[f].dtype)), f
    if name.startswith(("sim_index", "select_")):  # no descent: leaf 0 is the root itself, the others are none, no simulation is consumed
        assert st["selected"][rows].tolist() == [0] + [-1] * (L - 1) and st["path_len"][rows].tolist() == [0] + [-1] * (L - 1)
        assert (st["paths"][:, rows] == was["paths"][:, rows]).all()
        assert st["sim_index"][p] == was["sim_index"][p] and (st["sim_visits"][p] == was["sim_visits"][p]).all()
        assert st["pending"][p, 0] == 1 and not st["pending"][p, 1:].any()
    if name.startswith("pending"):  # whatever it holds, the stores stay where the healthy run's are and the counters stay counters
        assert (st["selected"][rows] >= -1).all() and (st["selected"][rows] < c.N).all()
        assert np.array_equal(st["sim_visits"][p].sum() - was["sim_visits"][p].sum(), st["sim_index"][p] - was["sim_index"][p])
    if name.startswith("choose_") and not data:
        assert st["move_slot"][p] == -1 and not st["move_action"][p].any() and not st["child_weights"][p].any() and not st["child_policy"][p].any() \
            and not st["child_actions"][p].any()
    others = [r for r in range(c.P) if r != p]
    other_rows = [r for r in range(c.P * L) if r // L != p]
    for f in glc.STATE_FIELDS + glc.OUT_FIELDS:  # the neighbours are the healthy run's
        take = (lambda a: a[:, other_rows]) if f == "paths" else (lambda a: a[other_rows]) if f in ("selected", "path_len") else (lambda a: a[others])
        assert pc.same_bits(take(st[f]), take(healthy[f])), f


# ---- a launch worked out by hand ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("L", [4, 8])
def test_a_launch_worked_out_by_hand(L):
    h = glc.HAND
    st = glc.run(glc.hand_state(L), h["k"], 1, h["n"], h["Mc"], L, h["rule"], [gc.call(glc.BEGIN | glc.SELECT, step_index=3)])[0]
    glc.check_hand(L, st)


# ---- whole searches ------------------------------------------------------------------------------------------------------
SEARCH = dict(P=9, levels=5, n=8, Mc=4, C=4, K=4, rule=(1.25, 50.0, 1.0), key=dict(seed=gc.SEED ^ 5, step_index=(1 << 33) + 3, first_root=4))


def record_search(s, L, evaluate, tree=None, capacity=None, launches=None):
    """gumbel_search(leaves=L) on the CPU -> (its result, the recorded evaluations as plc.record keeps them)."""
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
                       gumbel_step_index=s["key"]["step_index"], leaves=L, launches=launches)
    return gs, calls


def replay(s, L, gs, calls, start):
    seq = gc.search_calls(calls, s["key"])
    states = glc.run(start, s["C"], s["K"], s["n"], s["Mc"], L, s["rule"], seq, levels=s["levels"])
    R = s["P"] * L
    for m, st in enumerate(states[:len(calls)]):  # every selection is the recorded one
        want_paths, want_len = calls[m][0], calls[m][1]
        assert np.array_equal(st["path_len"], want_len), m
        for r in range(R):
            assert np.array_equal(st["paths"][:max(want_len[r], 0), r], want_paths[:max(want_len[r], 0), r])
        assert np.array_equal(st["sim_visits"].sum(axis=1), st["sim_index"])
    assert not states[len(calls)]["pending"].any()  # the last ABSORB has taken every leaf
    last = states[-1]
    pc.compare_with_search(dict(last, errors=max(st["errors"] for st in states)), gs.search)
    assert not last["pending"].any()
    assert np.array_equal(last["sim_index"], gs.sim_index.numpy()) and np.array_equal(last["sim_visits"], gs.sim_visits.numpy())
    for f in glc.OUT_FIELDS:
        want = getattr(gs, f).numpy()
        assert pc.same_bits(last[f], want if f in ("child_policy", "root_value") else want.astype(np.int64)), f
    return states


@pytest.mark.parametrize("L", [1, 2, 3, 4, 8])
def test_a_search_and_the_search_that_follows_it_in_the_kept_tree(L):
    s = SEARCH
    E = -(-s["n"] // L) + 1
    N = 1 + 2 * E * L * s["C"]
    ev = plc.leaves_evaluator(s["P"], s["levels"], s["K"], L, 23)
    gs, calls = record_search(s, L, ev, capacity=N)
    assert len(calls) == E
    states = replay(s, L, gs, calls, glc.with_leaves(gc.init_state(s["P"], N, s["C"], s["levels"]), s["P"], N, L, s["levels"]))
    expanded = states[1]["num_children"][:, 0] > 0
    assert expanded.any() and (~expanded).any() and (states[-1]["sim_index"][~expanded] == 0).all()
    assert (states[-1]["sim_index"] <= s["n"]).all() and (states[-1]["sim_index"][expanded & (states[-1]["terminal"][:, 0] == 0)] > 0).all()
    if L == 1:
        assert (states[-1]["sim_index"][expanded & (states[-1]["terminal"][:, 0] == 0)] == s["n"]).all()
    # the move's subtree, kept
    tree, _ = puct_reroot(search_tree(gs.search), gs.move_slot)
    s2 = dict(s, key=dict(s["key"], step_index=s["key"]["step_index"] + 1))
    gs2, calls2 = record_search(s2, L, plc.leaves_evaluator(s["P"], s["levels"], s["K"], L, 29), tree=tree)
    states2 = replay(s2, L, gs2, calls2, glc.with_leaves(gc.state_of(tree, s["P"], s["C"], s["levels"]), s["P"], N, L, s["levels"]))
    kept = (states2[0]["num_children"][:, 0] > 0) & (states2[0]["terminal"][:, 0] == 0)
    assert kept.any() and (states2[-1]["sim_index"][kept] > 0).all()


def test_too_few_launches_still_choose():
    s, L = SEARCH, 2
    gs, calls = record_search(s, L, plc.leaves_evaluator(s["P"], s["levels"], s["K"], L, 23), launches=3)
    assert len(calls) == 3
    N = 1 + 3 * L * s["C"]
    states = replay(s, L, gs, calls, glc.with_leaves(gc.init_state(s["P"], N, s["C"], s["levels"]), s["P"], N, L, s["levels"]))
    live = states[-1]["num_children"][:, 0] > 0
    assert live.any() and (states[-1]["sim_index"][live] <= 2 * L).all() and (states[-1]["sim_index"][live] < s["n"]).all()
    assert (states[-1]["move_slot"][live] >= 1).all()
