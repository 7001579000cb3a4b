"""The witnesses of tests/near_tie_node_cases.py on the CPU: on every witness the C++ models of the three later Gumbel kernels
(csrc/pcb_gumbel_leaves.h, csrc/pcb_gumbel_tree.h and csrc/pcb_gumbel_tree_leaves.h as sanitized programs of their own), the
Python reference and the torch specification go to the same child, and the witness's variant -- recomputed here, not trusted
from the generator -- goes to the other contender.  A header that forms S, Wv, Qv, vmix, Z or t another way fails here: kernel
and model share it.  Then the recorded real-valued searches of the three kernels."""
import shutil

import numpy as np
import pytest
import torch

import gumbel_cases as gc
import near_tie_cases as nt
import near_tie_node_cases as nn
from pcbenv.search import considered_visits, gumbel_choose, gumbel_select_node, gumbel_select_root

pytestmark = pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
WIDTHS = list(nn.WIDTHS)
TREE_KERNELS = ("gumbel_tree", "gumbel_tree_leaves")
FLOATS = gc.FLOATS + ("child_policy",)


def _healthy(states, may_fill_up=False):
    """may_fill_up: the tables of near_tie_cases have leaves that are not terminal and no slot to expand them into."""
    for st in states:
        assert st["errors"] in ((0, gc.ERR_FULL) if may_fill_up else (0,)) and not any(np.isnan(st[f]).any() for f in FLOATS)


def _leaves(kernel):
    return nn.L if nn.RUNS[kernel][1] else 1


def test_the_tables_are_what_they_are_there_for():
    tables = nn.check_cases()
    assert {name for name, G in tables} == {"node", "pending", "choose", "root"} and {G for name, G in tables} == set(WIDTHS)
    assert nn.tables()[1] < 4 * nn.MEASURED_SECONDS


# ---- the node rule ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("G", WIDTHS)
@pytest.mark.parametrize("name", ["node", "pending"])
def test_on_every_witness_the_variant_parts_from_the_reference(name, G):
    t = nn.tables()[0][(name, G)]
    for p, row in enumerate(t.rows):
        ref, sc = nn.reference_choice(t, p)
        var, sv = nn.reference_choice(t, p, row["variant"])
        assert ref == row["ref"] and var == row["var"] and ref != var, (p, row)
        fc = int(t.state["first_child"][p, row["node"]])
        for scores in (sc, sv):
            others = [s for c, s in enumerate(scores) if fc + c not in row["slots"]]
            assert not others or max(others) < min(scores[s - fc] for s in row["slots"]) - nn.MARGIN, (p, row)
            assert not any(np.isnan(s) for s in scores)


def _specification_children(t, pending):
    """gumbel_select_node at the witness node of every root -> the slots it goes to."""
    node = torch.tensor([row["node"] for row in t.rows])
    sel = gumbel_select_node(nt.tree_of(t), node, t.C, t.rule[1], t.rule[2], pending)
    assert int(sel["errors"]) == 0 and bool(sel["ok"].all())
    return [int(t.state["first_child"][p, row["node"]]) + int(sel["child"][p]) for p, row in enumerate(t.rows)]


@pytest.mark.parametrize("G", WIDTHS)
@pytest.mark.parametrize("kernel", TREE_KERNELS)
def test_the_tree_models_go_where_the_reference_and_the_specification_go(kernel, G):
    t = nn.node_table(G)
    case, seq, states = nn.node_calls(kernel, G)
    per, first = _leaves(kernel), states[1]
    spec = _specification_children(t, None if per == 1 else torch.zeros((t.P, t.N), dtype=torch.int64))
    for p, row in enumerate(t.rows):
        r = p * per
        assert first["selected"][r] == row["ref"] == spec[p] and first["path_len"][r] == row["level"] + 1, (p, row)
        assert first["paths"][row["level"], r, 2] == row["ref"] and (row["level"] == 0 or first["paths"][0, r, 2] == row["node"]), (p, row)
        assert first["sim_index"][p] == (nn.N_SIMS if row["level"] == 0 else per)  # level 0: the budget was spent; level 1: the schedule took the node
    _healthy(states)
    assert (states[2]["value_sum"][:, 0] != t.state["value_sum"][:, 0]).all()  # the ABSORB backed a real value up


@pytest.mark.parametrize("G", WIDTHS)
def test_the_tree_leaves_model_counts_pending_visits_as_the_reference_does(G):
    t = nn.pending_table(G)
    case, seq, states = nn.pending_calls(G)
    first = states[1]
    preset = torch.from_numpy(np.array(t.state["pending"])).to(torch.int64)
    after_a = preset.clone()  # a "launched" root after its first leaf
    for p, row in enumerate(t.rows):
        if row["kind"] == "launched":
            assert not preset[p].any()
            for s in (0, row["node"], row["slots"][0]):
                after_a[p, s] += 1
    spec, blind = _specification_children(t, after_a), _specification_children(t, None)
    for p, row in enumerate(t.rows):
        r = p * nn.L
        if row["kind"] == "launched":  # the launch itself makes the pending visit that decides its second leaf
            assert first["selected"][r] == blind[p] == row["slots"][0] and first["selected"][r + 1] == row["ref"] == spec[p] == row["slots"][1], (p, row)
            assert first["path_len"][r + 1] == 2 and first["paths"][0, r + 1, 2] == row["node"], (p, row)
        else:
            assert first["selected"][r] == row["ref"] == spec[p] and first["path_len"][r] == row["level"] + 1, (p, row)
    _healthy(states)
    assert {row["kind"] for row in t.rows} == set(nn.PENDING) - {"none"}


# ---- the root's scores in the leaf kernels -------------------------------------------------------------------------------------
@pytest.mark.parametrize("G", WIDTHS)
def test_on_every_root_score_witness_with_vmix_the_variant_parts_from_the_reference(G):
    t = nn.root_table(G)
    sims = torch.from_numpy(t.state["sim_index"]), torch.from_numpy(t.state["sim_visits"])
    sel = gumbel_select_root(nt.tree_of(t), sims[0], sims[1], considered_visits(t.Mc, t.n), t.C, t.rule[1], t.rule[2], **nn.KEY, full=True)
    for p, row in enumerate(t.rows):
        ref, sc = nn.root_choice(t, p)
        var, sv = nn.root_choice(t, p, row["variant"])
        assert ref == row["ref"] and var == row["var"] and ref != var, (p, row)
        assert bool(sel["scheduled"][p]) and 1 + int(sel["child"][p]) == ref, (p, row)
        assert t.state["visits"][p, row["slots"][0]] == 0  # a is completed with vmix
        for scores in (sc, sv):
            others = [s for c, s in enumerate(scores) if 1 + c not in row["slots"]]
            assert not others or max(others) < min(scores[s - 1] for s in row["slots"]) - nn.MARGIN, (p, row)
    for kernel in TREE_KERNELS:
        case, seq, states = nn.root_calls(kernel, G)
        per = _leaves(kernel)
        assert all(states[1]["selected"][p * per] == row["ref"] and states[0]["move_slot"][p] == row["ref"] for p, row in enumerate(t.rows)), kernel
        _healthy(states)


@pytest.mark.parametrize("G", WIDTHS)
@pytest.mark.parametrize("which", ["first", "second"])
@pytest.mark.parametrize("kernel", ["gumbel_leaves", "gumbel_tree_leaves"])
def test_the_leaf_models_take_the_root_score_witnesses_as_the_reference_does(kernel, which, G):
    """nt.table("gumbel", G)'s root-score witnesses at L = 2, deciding leaf 0 and -- behind a leaf that goes clearly to a third child
    -- leaf 1; tests/test_near_ties_model.py shows that each variant parts from the reference on them."""
    t, case, seq, states = nn.gumbel_rows_calls(kernel, G, which)
    first, checked = states[1], 0
    for p, row in enumerate(t.rows):
        if row["score"] != "gumbel":
            continue
        checked += 1
        if which == "first":
            assert first["selected"][p * nn.L] == row["ref"] and first["path_len"][p * nn.L] == 1, (p, row)
        else:
            assert first["selected"][p * nn.L] == t.third[p] and first["selected"][p * nn.L + 1] == row["ref"], (p, row)
            assert first["sim_index"][p] == 3 and first["sim_visits"][p, row["ref"] - 1] == 2, (p, row)
    assert checked == nt.FLOOR * len(nt.GUMBEL_VARIANTS)
    _healthy(states, may_fill_up=True)


@pytest.mark.parametrize("G", WIDTHS)
def test_the_gumbel_leaves_model_scores_pending_visits_below_a_scheduled_root_as_the_reference_does(G):
    """nt.table("leaves", G)'s witnesses at level 1: LEAVES_VARIANTS with pending visits, the root level taken by the schedule."""
    t, case, seq, states = nn.leaves_rows_calls(G)
    first, checked = states[1], 0
    for p, row in enumerate(t.rows):
        if row["level"] == 1:
            r = p * nn.L
            assert first["selected"][r] == row["ref"] and first["path_len"][r] == 2 and first["paths"][0, r, 2] == row["node"], (p, row)
            assert first["sim_index"][p] >= 1 and first["sim_visits"][p, row["node"] - 1] >= 1
            checked += 1
    assert checked == nt.FLOOR * len(nt.LEAVES_VARIANTS) and {row["kind"] for row in t.rows if row["level"] == 1} == set(nt.PENDING)
    _healthy(states, may_fill_up=True)


# ---- CHOOSE with v_mix ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("G", WIDTHS)
def test_the_tree_models_policy_target_is_the_reference_s_where_a_variant_s_is_not(G):
    t = nn.choose_table(G)
    cho = gumbel_choose(nt.tree_of(t), torch.from_numpy(t.state["sim_visits"]), t.C, t.rule[1], t.rule[2], **nn.KEY, full=True)
    assert int(cho["errors"]) == 0
    for kernel in TREE_KERNELS:
        case, seq, states = nn.choose_calls(kernel, G)
        got = states[0]
        assert got["errors"] == 0
        for p, row in enumerate(t.rows):
            w, pol = nn.choose_outputs(t, p)
            vw, vpol = nn.choose_outputs(t, p, row["variant"])
            assert got["child_weights"][p].tolist() == w and cho["child_weights"][p].tolist() == w, (p, row)
            assert nt.pc.same_bits(got["child_policy"][p], np.array(pol, np.float32)) and nt.pc.same_bits(cho["child_policy"][p].numpy(), np.array(pol, np.float32)), (p, row)
            assert (vw != w) if row["kind"] == "weights" else not nt.pc.same_bits(np.array(vpol, np.float32), np.array(pol, np.float32)), (p, row)
            assert abs(sum(w) - 2 ** 24) <= t.C // 2 + 1


@pytest.mark.parametrize("G", WIDTHS)
def test_the_tree_models_policy_target_on_the_choose_table_of_the_root_rule(G):
    """nt.choose_table(G) -- z_butterfly, reciprocal_z and fused on roots whose children all have a visit -- through tree_choose:
    nothing is completed with vmix, and the outputs are the reference's."""
    t = nt.choose_table(G)
    for kernel in TREE_KERNELS:
        case, seq, states = nn.root_rule_choose_calls(kernel, G)
        for p in range(t.P):
            w, pol = nt.choose_outputs(t, p)
            assert states[0]["child_weights"][p].tolist() == w and nt.pc.same_bits(states[0]["child_policy"][p], np.array(pol, np.float32)), (kernel, p)


# ---- recorded searches on real-valued evaluations ----------------------------------------------------------------------
REAL = [(kernel, name, leaves) for kernel, Ls in nn.REAL_LEAVES.items() for name in nn.REAL for leaves in Ls]


@pytest.mark.parametrize("kernel, name, leaves", REAL)
def test_the_model_replays_a_real_valued_search(kernel, name, leaves):
    case, seq, states, gs, calls = nn.real_search(kernel, name, leaves)
    for m, st in enumerate(states[:len(calls)]):  # every selection is the recorded one
        want_paths, want_len = calls[m][0], calls[m][1]
        assert np.array_equal(st["path_len"], want_len), m
        for r in range(case.P * leaves):
            assert np.array_equal(st["paths"][:max(want_len[r], 0), r], want_paths[:max(want_len[r], 0), r]), (m, r)
    last = states[-1]
    nt.pc.compare_with_search(dict(last, errors=max(st["errors"] for st in states)), gs.search)
    assert np.array_equal(last["sim_index"], gs.sim_index.numpy()) and np.array_equal(last["sim_visits"], gs.sim_visits.numpy())
    for f in gc.OUT_FIELDS:
        want = getattr(gs, f).numpy()
        assert nt.pc.same_bits(last[f], want if f in ("child_policy", "root_value") else want.astype(np.int64)), f
    assert not any(np.isnan(st[f]).any() for st in states for f in FLOATS) and (last["sim_index"] > 0).any()
    if leaves > 1:
        assert any((st["pending"] > 1).any() for st in states) and not last["pending"].any()
    if kernel != "gumbel_leaves":  # the node rule had its say: a root went three levels down, and a node below a root spread its visits
        assert int(last["depth"].max()) >= 3
        spread = False
        for p in range(case.P):
            for a in range(1, int(last["num_nodes"][p])):
                k, fc = int(last["num_children"][p, a]), int(last["first_child"][p, a])
                spread = spread or (k > 0 and int((last["visits"][p, fc:fc + k] > 0).sum()) >= 2)
        assert spread
