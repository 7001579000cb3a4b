"""The cases of tests/rollout_cases.py, without a GPU: from the CPU plan alone, every case contains what
tests/test_rollout_edges_gpu.py is there to run -- terminals in the middle of a launch, environments that end two
episodes in one launch, "no legal cell" and routed terminals on the crowded grids, a launch that starts on a presampled
action, and enough steps whose slot survives their launch.  These are conditions on the reference, not measurements."""
import pytest

import rollout_cases as rc
from pcbenv.config import KIND_PIN, KIND_RECT, KIND_SPATIAL, KIND_SQUARE

# the rollout lengths every script must hold, in this order (further calls may stand between and behind them)
LENGTHS = {
    "spatial_7x100_t256": (5, 1, 7, 3), "spatial_7x100_compact": (5, 1, 7, 3), "pin_100x9": (6, 9, 4), "pin_40x48_k4_t256": (6, 9, 5),
    "rect_33x65": (9, 30, 12), "square_3x128": (30, 1, 20), "crowded_spatial_t256": (7, 7, 7),
    "crowded_pin_inplace": (2, 3, 1, 4, 2, 3, 1, 4), "rect_128_huge_inplace": (3, 2, 4, 1, 3), "rect_4x4_generator": (4, 4, 4, 3),
    "spatial_max_t64": (8,) * 9, "small_pin_incremental": (3, 5, 2, 4),
}


def test_the_table():
    assert set(rc.CASES) == set(LENGTHS)
    for name, case in rc.CASES.items():
        cfg = case.cfg()
        ops = [c[0] for c in case.script]
        rollouts = tuple(c[1] for c in case.script if c[0] == "rollout")
        assert rollouts[:len(LENGTHS[name])] == LENGTHS[name], name
        assert all(n <= case.S for n in rollouts[len(LENGTHS[name]):]), (name, "a rollout behind the table's is longer than S")
        assert case.B <= 16 and case.seed in (3, 2, 6), name
        pairs = list(zip(case.script, case.script[1:]))
        assert any(a == ("fused",) and b[0] == "rollout" for a, b in pairs), (name, "no fused call directly before a rollout")
        assert any(a == ("reset_mask", 0.5) and b[0] == "rollout" for a, b in pairs), (name, "no masked reset directly before a rollout")
        if cfg.kind in (KIND_PIN, KIND_SPATIAL):
            assert any(a[0] == "rollout" and b == ("step",) for a, b in pairs), (name, "no explicit step directly after a rollout")
        assert set(ops) <= {"rollout", "fused", "step", "reset_mask"}
        assert case.setup().auto_reset
    kinds = {c.cfg().kind for c in rc.CASES.values()}
    assert kinds == {KIND_SQUARE, KIND_RECT, KIND_PIN, KIND_SPATIAL}
    gen = rc.CASES["rect_4x4_generator"]
    assert gen.device_instances and gen.Q == 4 and max(LENGTHS["rect_4x4_generator"]) == gen.Q  # num_steps == queue_depth: the bound


@pytest.mark.parametrize("name", list(rc.CASES))
def test_the_plan_holds_what_the_case_is_there_for(name):
    case, plan = rc.CASES[name], rc.plan(name)
    assert rc.Plan(name).digest() == plan.digest(), "the plan is not a pure function of the case"
    mx = plan.mix()
    assert mx["transitions"] == case.B * sum(len(c["steps"]) for c in plan.calls)
    assert mx["terminals"] == mx["routed"] + mx["worst"] + mx["ends"]
    need = rc.conditions(case, mx)
    # what the conditions must be, name by name (rc.conditions is also what rc.pick_seed searched the seeds with)
    assert ("a mid-launch terminal" in need) == (name != "small_pin_incremental")
    assert ("an environment with two terminals in one launch" in need) == (name in (
        "spatial_7x100_t256", "pin_100x9", "rect_33x65", "crowded_spatial_t256", "rect_4x4_generator"))
    assert ("5 worst-case terminals mid-launch" in need) == ("5 routed terminals mid-launch" in need) == name.startswith("crowded_")
    assert ("a routed terminal" in need) == (case.cfg().kind in (KIND_PIN, KIND_SPATIAL) and not name.startswith("crowded_"))
    assert ("every environment terminal at every step" in need) == (name == "rect_4x4_generator")
    assert "a presample hit at t = 0" in need
    assert ("at most half of the transitions uncompared" in need) == ("a launch with n <= S" in need) == (case.S > 1)
    missed = [k for k, v in need.items() if not v]
    assert not missed, (name, missed, mx)
