"""csrc/pcb_frontier.h -- the frontier step of pcbenv_frontier_advance as plain C++ -- against its specification,
pcbenv/search.py:frontier_advance, on the CPU: tools/frontier_check.cpp (AddressSanitizer + UBSan, a program of its own,
nothing preloaded) replays the call sequences of tests/frontier_cases.py, and the specification runs the same sequences from
the same sentinel-filled tensors.  The two agree after every call on every tensor, floats by their bits; what a call
leaves untouched is therefore compared too: it still holds the sentinel, or what an earlier call wrote.

The reach assertions say what the table of cases contains, so that tests/test_frontier_gpu.py, which holds the kernel to
the model on it, cannot be vacuous."""
import shutil

import numpy as np
import pytest

import frontier_cases as fc

pytestmark = pytest.mark.skipif(shutil.which("g++") is None, reason="no g++")


@pytest.mark.parametrize("name", list(fc.CASES))
def test_the_model_is_the_specification_after_every_call(name):
    c = fc.case(name)
    spec = fc.specify(c.P, c.W, c.K, c.T, c.prior_weight, c.seq)
    assert len(spec) == len(c.states) == len(c.seq)
    for i, (a, b) in enumerate(zip(c.states, spec)):
        for f in fc.STATE_FIELDS:
            assert fc.same_bits(a[f], b[f]), (name, i, f)
        assert a["errors"] == b["errors"], (name, i)


def test_the_table_reaches_every_arm_of_the_rule():
    fc.assert_reach(list(fc.CASES))
    searched = fc.reach([n for n in fc.CASES if fc.CASES[n][5] != "hand"])  # the searches alone, without the hand-made frontiers
    for arm in ("tie", "tie_at_the_cut", "nan_value", "inf_value", "fewer_than_W", "more_than_W", "zero_expandable", "first_evaluation_terminal", "row_at_T",
                "count_below_0", "count_above_K", "prior_zero", "prior_denormal", "prior_negative", "prior_inf", "prior_nan", "prior_above_1",
                "later_final_better", "later_final_equal"):
        assert searched.get(arm), arm
    hand = fc.reach(["hand_0", "hand_1"])
    assert not [a for a in fc.ARMS if a not in ("first_evaluation_terminal", "more_than_W", "weight_zero", "weight_non_zero") and not hand.get(a)]


def test_init_writes_the_out_set_and_nothing_else():
    c = fc.case("W3_K5")
    st = c.states[0]
    F = c.W * c.K
    assert c.seq[0]["phases"] == fc.INIT and c.seq[0]["swap"] == 1  # out = set 0
    want = np.full((c.P, F), -1)
    want[:, 0] = 0
    assert np.array_equal(st["path_len_0"].reshape(c.P, F), want) and (st["parent_row"] == -1).all() and (st["live"] == 1).all()
    cum = st["cum_logp_0"].reshape(c.P, F)
    assert (cum[:, 0] == 0.0).all() and not np.signbit(cum[:, 0]).any() and (cum[:, 1:] == fc.FILL_F).all()
    assert (st["best_len"] == -1).all() and np.isneginf(st["best_value"]).all()
    for f in ("paths_0", "paths_1", "path_len_1", "best_path"):
        assert (st[f] == fc.FILL).all(), f
    assert (st["cum_logp_1"] == fc.FILL_F).all()


def test_what_the_hand_made_calls_come_to():
    """The outcomes the header promises, on the model's dump under the sanitizers (call i of hand_made is state i + 1)."""
    c0, c1 = fc.case("hand_0"), fc.case("hand_1")
    F, K, T = c0.W * c0.K, c0.K, c0.T
    root1 = lambda st, f: st[f][F:2 * F]
    # -0.0 ties with +0.0: slot 1 (-0.0) goes before slot 4 (+0.0), both before slot 0 at -1
    st = c0.states[1]
    assert root1(st, "parent_row").tolist() == [1, 1, 1, 4, 4, 4] and st["live"][1] == 6
    # three rows at 0.5: the lower slots 2 (one child) and 3 (three children) are kept, slot 5 is not
    st = c0.states[2]
    assert root1(st, "parent_row").tolist() == [2, -1, -1, 3, 3, 3] and root1(st, "path_len_1").tolist() == [3, -1, -1, 2, 2, 2]
    # +inf first, then 0.0; NaN and -inf are not reached -- and alone they tie: the lower slot first
    assert root1(c0.states[3], "parent_row").tolist() == [2, 2, 2, 3, 3, 3]
    assert root1(c0.states[4], "parent_row").tolist() == [0, 0, -1, 1, 1, 1]
    # a NaN final is recorded as -inf, by the first of them
    st = c0.states[5]
    assert np.isneginf(st["best_value"][1]) and st["best_len"][1] == 2 and st["live"][1] == 0
    assert st["best_path"][:2, 1].tolist() == [[0, 0, F + 0], [0, 1, F + 0]] and (st["best_path"][2:, 1] == fc.FILL).all()
    # fewer than W; none at all
    assert c0.states[6]["live"][1] == 3 and root1(c0.states[6], "parent_row").tolist() == [3, 3, 3, -1, -1, -1]
    assert c0.states[7]["live"][1] == 0 and (root1(c0.states[7], "path_len_1") == -1).all() and c0.states[7]["best_len"][1] == 2
    # rows at T; the clamped counts: -3 gives no child, K + 5 gives K
    st = c0.states[8]
    assert st["best_len"][1] == T and root1(st, "parent_row").tolist() == [3, 3, 3, -1, -1, -1]
    # priors: the bad ones give -inf, 1.5 its logarithm
    st = c1.states[9]
    cum = root1(st, "cum_logp_1")
    assert root1(st, "parent_row").tolist() == [1, 1, 1, 0, 0, 0]  # -0.5 + 0.5 against -1.5 + 0.5
    assert np.isneginf(cum[[0, 1, 3, 5]]).all() and abs(cum[2] - (-0.5 + np.log(1.5))) < 1e-15
    assert np.isneginf(cum[4])  # a denormal prior is no prior
    # path_len out of range: bit 1, the rows are no rows, the healthy one is expanded
    st = c0.states[10]
    assert st["errors"] & fc.ERR_ROW and not c0.states[9]["errors"] and root1(st, "parent_row").tolist() == [2, 2, -1, -1, -1, -1]
    # later finals: 0.75 at slot 1 beats 0.25 and the equal 0.75 behind it; an equal and a worse one change nothing
    st = c0.states[11]
    assert st["best_value"][1] == 0.75 and st["best_len"][1] == 3
    st = c0.states[12]
    assert st["best_value"][1] == 0.25 and st["best_len"][1] == 4
    # the prior weight: without it slots 0 and 2 at 0.5; with it -inf sinks slot 0 and -2.0 slot 2 below slot 1
    assert root1(c0.states[13], "parent_row").tolist() == [0, -1, -1, 2, -1, -1]
    assert root1(c1.states[13], "parent_row").tolist() == [1, -1, -1, 2, -1, -1]
    # the neighbours: one ordinary row each, expanded in every call
    for st in c0.states[1:]:
        assert st["live"][0] == 2 and st["live"][2] == K
