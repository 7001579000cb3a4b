"""The witnesses of tests/near_tie_cases.py on the CPU: on every witness root the C++ model (csrc/pcb_puct.h,
csrc/pcb_puct_leaves.h and csrc/pcb_gumbel.h as sanitized programs of their own), the Python reference and the torch
specification select the same node, and the witness's variant -- recomputed here, not trusted from the generator --
selects the other contender.  A header whose score is computed another way fails here: kernel and model share it."""
import shutil
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import gumbel_cases as gc
import near_tie_cases as nt
from pcbenv.search import Evaluation, considered_visits, gumbel_choose, gumbel_select_root, puct_search

pytestmark = pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
TABLES = [(kernel, G) for kernel in nt.KERNELS for G in nt.WIDTHS]
MARGIN = 1e-3  # the contenders stand this far above every other child: c_puct * 2^-20 * sqrt(2000) / 2 is below 3e-5, and a contender's q is above 0.15


def test_the_tables_are_what_they_are_there_for():
    tables = nt.check_cases()
    assert set(tables) == set(TABLES)
    assert nt.tables()[1] < 4 * nt.MEASURED_SECONDS


def specification_slots(t, L):
    """puct_search(tree=the table, iterations=1, leaves=L) with an evaluator that records the paths it is asked for -> the slot
    every row ends at (the tables give node s the action (s % 2, 0, s)), -1 for a row that is no leaf, and path_len."""
    seen = {}

    def evaluate(paths, path_len, step_index0):
        seen.update(paths=paths.clone().numpy(), path_len=path_len.clone().numpy())
        R = t.P * L
        return Evaluation(torch.zeros(R, dtype=torch.float64), torch.ones(R, dtype=torch.uint8), torch.zeros(R, dtype=torch.int32),
                          torch.zeros((R, 1, 3), dtype=torch.int32), torch.zeros((R, 1), dtype=torch.float32))
    puct_search(SimpleNamespace(num_envs=t.P, device="cpu", cfg=None), 1, 0, evaluate, c_puct=t.c_puct, max_children=t.C, max_steps=nt.T,
                tree=nt.tree_of(t), leaves=L)
    plen = seen["path_len"]
    return np.array([seen["paths"][plen[r] - 1, r, 2] if plen[r] > 0 else 0 if plen[r] == 0 else -1 for r in range(t.P * L)]), plen


@pytest.mark.parametrize("kernel, G", TABLES)
def test_on_every_witness_the_variant_parts_from_the_reference(kernel, G):
    t = nt.table(kernel, G)
    for p, row in enumerate(t.rows):
        ref, sc = nt.reference_choice(t, p)
        var, _ = nt.reference_choice(t, p, row["variant"])
        assert ref == row["ref"] and var == row["var"] and ref != var, (p, row)
        fc = int(t.state["first_child"][p, row["node"]])
        others = [s for c, s in enumerate(sc) if fc + c not in row["slots"]]
        assert not others or max(others) < min(sc[s - fc] for s in row["slots"]) - MARGIN, (p, row)
        assert not any(np.isnan(s) for s in sc)


@pytest.mark.parametrize("kernel, G", [(k, G) for k, G in TABLES if k != "gumbel"])
def test_the_model_selects_what_the_reference_and_the_specification_select(kernel, G):
    t, seq, states = nt.puct_calls(kernel, G)
    first = states[0]
    spec, spec_len = specification_slots(t, t.L)
    checked = 0
    for p, row in enumerate(t.rows):
        r = p * t.L
        assert first["selected"][r] == row["ref"] and first["path_len"][r] == row["level"] + 1, (p, row)
        assert first["paths"][row["level"], r, 2] == row["ref"], (p, row)
        if row["kind"] == "none":      # the specification starts from nothing pending
            assert spec[r] == row["ref"] and spec_len[r] == row["level"] + 1, (p, row)
            checked += 1
        elif row["kind"] == "natural":  # its first descent goes to a and leaves the witness's pending behind: the second decides
            assert spec[r] == row["slots"][0] and spec[r + 1] == row["ref"] and spec_len[r + 1] == row["level"] + 1, (p, row)
            checked += 1
    assert checked >= (t.P if kernel == "puct" else t.P // 3)
    for st in states:
        assert st["errors"] == 0 and not any(np.isnan(st[f]).any() for f in nt.lc.FLOATS)
    # the ABSORB backed a real value up: value_sum of a root is no longer what the table held
    assert (states[1]["value_sum"][:, 0] != t.state["value_sum"][:, 0]).all()


@pytest.mark.parametrize("G", list(nt.WIDTHS))
def test_the_gumbel_model_selects_what_the_reference_and_the_specification_select(G):
    t = nt.table("gumbel", G)
    case, seq, states = nt.gumbel_calls(G)
    chosen, selected = states[0], states[1]
    tree = nt.tree_of(t)
    table = considered_visits(t.Mc, t.n)
    sims = torch.from_numpy(t.state["sim_index"]), torch.from_numpy(t.state["sim_visits"])
    sel = gumbel_select_root(tree, sims[0], sims[1], table, t.C, t.rule[1], t.rule[2], **nt.GUMBEL_KEY)
    cho = gumbel_choose(tree, sims[1], t.C, t.rule[1], t.rule[2], **nt.GUMBEL_KEY)
    puct, puct_len = specification_slots(t, 1)  # PUCT at every level: the specification of the roots whose budget is spent
    assert int(sel["errors"]) == 0 and int(cho["errors"]) == 0
    for p, row in enumerate(t.rows):
        assert selected["selected"][p] == row["ref"] and selected["path_len"][p] == row["level"] + 1, (p, row)
        if row["score"] == "gumbel":
            assert bool(sel["scheduled"][p]) and 1 + int(sel["child"][p]) == row["ref"], (p, row)
            assert int(cho["move_slot"][p]) == row["ref"] and chosen["move_slot"][p] == row["ref"], (p, row)
            assert selected["sim_visits"][p, row["ref"] - 1] == 1 and selected["sim_index"][p] == 1
        else:
            assert puct[p] == row["ref"] and puct_len[p] == row["level"] + 1, (p, row)
            assert bool(sel["scheduled"][p]) == (row["level"] == 1)
            if row["level"] == 1:
                assert 1 + int(sel["child"][p]) == row["node"], (p, row)
    # CHOOSE's outputs are the specification's on every root, bit for bit
    assert np.array_equal(chosen["child_weights"], cho["child_weights"].numpy()) and gc.pc.same_bits(chosen["child_policy"], cho["child_policy"].numpy())
    assert np.array_equal(chosen["move_slot"], cho["move_slot"].numpy())
    for st in states:
        assert st["errors"] == 0 and not any(np.isnan(st[f]).any() for f in gc.FLOATS + ("child_policy",))


# ---- recorded searches on real-valued evaluations ----------------------------------------------------------------------
def _no_nan(states, floats):
    return not any(np.isnan(st[f]).any() for st in states for f in floats)


@pytest.mark.parametrize("name", list(nt.REAL_PUCT))
def test_the_model_replays_a_real_valued_search(name):
    """puct_cases.replay raises where a selection of the model differs from the recorded one; the end is the specification's bit for bit."""
    case = nt.real_puct(name)
    nt.pc.compare_with_search(case.states[-1], case.ps)
    assert _no_nan(case.states, nt.pc.FLOATS) and case.states[-1]["errors"] == 0
    last = case.states[-1]
    assert (last["reward_hi"][3::5] == last["reward_lo"][3::5]).all()  # the constant roots never had a range
    if case.P > 4:
        assert (np.abs(last["reward_hi"][4::5] - last["reward_lo"][4::5]) == np.spacing(nt.pc.ONE_ULP_APART[0])).any()  # a range of one ulp
    child = (np.arange(case.N)[None, :] < last["num_nodes"][:, None]) & (np.arange(case.N)[None, :] >= 1)
    assert (last["prior"][child] == 0.0).any() and ((last["prior"] > 0) & (last["prior"] < 2.0 ** -126)).any()  # a zero and a denormal prior in a tree
    assert (last["prior"][child] > 1.0).any() or case.P <= 5  # a row left unnormalised
    if name.startswith("deep"):
        assert int(last["visits"][:, 0].max()) >= nt.DEEP_VISITS and int(last["depth"].max()) >= 3 and not last["terminal"][:, 1:5].all()


@pytest.mark.parametrize("name", list(nt.REAL_LEAVES))
def test_the_leaves_model_replays_a_real_valued_search(name):
    case = nt.real_leaves(name)
    nt.lc.compare_with_search(case.states[-1], case.ps)
    assert _no_nan(case.states, nt.lc.FLOATS) and case.states[-1]["errors"] == 0
    assert any((st["pending"] > 1).any() for st in case.states) and nt.lc.repeat_share(case) < 0.5


@pytest.mark.parametrize("name", nt.REAL_GUMBEL)
def test_the_gumbel_model_replays_a_real_valued_search(name):
    case, seq, states, gs, calls = nt.real_gumbel(name)
    for m, st in enumerate(states[:len(calls)]):  # every selection is the recorded one
        want_paths, want_len = calls[m][0], calls[m][1]
        assert np.array_equal(st["path_len"], want_len)
        for p in range(case.P):
            assert np.array_equal(st["paths"][:want_len[p], p], want_paths[:want_len[p], p]), (m, p)
    last = states[-1]
    nt.pc.compare_with_search(dict(last, errors=max(st["errors"] for st in states)), gs.search)
    assert np.array_equal(last["sim_index"], gs.sim_index.numpy()) and np.array_equal(last["sim_visits"], gs.sim_visits.numpy())
    for f in gc.OUT_FIELDS:
        want = getattr(gs, f).numpy()
        assert nt.pc.same_bits(last[f], want if f in ("child_policy", "root_value") else want.astype(np.int64)), f
    assert _no_nan(states, gc.FLOATS + ("child_policy",)) and (last["sim_index"] == case.n).any()


# ---- CHOOSE's outputs --------------------------------------------------------------------------------------------------
def test_the_choose_tables_are_what_they_are_there_for():
    nt.check_choose_cases()


@pytest.mark.parametrize("G", list(nt.WIDTHS))
def test_the_model_s_policy_target_is_the_reference_s_where_a_variant_s_is_not(G):
    """On every root of the table some child_weights integer (kind "weights") or child_policy float32 (kind "policy") of the
    root's variant -- Z summed in butterfly order, e * (1 / Z), a fused improved logit -- differs from the reference's; the
    model's and the specification's are the reference's in every element."""
    t = nt.choose_table(G)
    case, seq, states = nt.choose_calls(G)
    got = states[0]
    cho = gumbel_choose(nt.tree_of(t), torch.from_numpy(t.state["sim_visits"]), t.C, t.rule[1], t.rule[2], **nt.GUMBEL_KEY)
    assert got["errors"] == 0 and int(cho["errors"]) == 0
    for p, row in enumerate(t.rows):
        w, pol = nt.choose_outputs(t, p)
        vw, vpol = nt.choose_outputs(t, p, row["variant"])
        assert got["child_weights"][p].tolist() == w and cho["child_weights"][p].tolist() == w, (p, row)
        assert nt.pc.same_bits(got["child_policy"][p], np.array(pol, np.float32)) and nt.pc.same_bits(cho["child_policy"][p].numpy(), np.array(pol, np.float32)), (p, row)
        assert (vw != w) if row["kind"] == "weights" else not nt.pc.same_bits(np.array(vpol, np.float32), np.array(pol, np.float32)), (p, row)
        assert abs(sum(w) - 2 ** 24) <= t.C // 2 + 1
