"""The plans of tests/path_cases.py on the CPU oracle alone: the draw key depends on t and not on the path, so a path that
is a prefix of the path-less playout reproduces it; and every case's plan contains the ends the GPU test needs.  No GPU."""
import numpy as np
import pytest

import path_cases as pa

# (ended at path end, ended inside path, drew after path, differing continuation) with the seeds of playout_cases, after
# max_steps launches; a case not listed here is held to the conditions of path_cases.mix alone
FIGURES = {
    "small_pin": (24, 12, 12, 6),
    "c1": (16, 12, 20, 10),
    "c3_centroid": (16, 12, 20, 10),
    "spatial_7x100": (20, 12, 16, 8),
    "rect_4x4_full": (24, 8, 0, 0),
}
_PLANS = {}


def plan(name, parity=0):
    if (name, parity) not in _PLANS:
        _PLANS[name, parity] = pa.Plan(name, parity)
    return _PLANS[name, parity]


def _same(a, b, leaf=False):
    return (a["length"] == b["length"] and a["done"] == b["done"] and a["reward"].tobytes() == b["reward"].tobytes()
            and a["info"].tobytes() == b["info"].tobytes() and np.array_equal(a["actions"], b["actions"])
            and (not leaf or np.array_equal(a["leaf"], b["leaf"])))


@pytest.mark.parametrize("name", pa.GPU_CASES)
def test_a_prefix_of_the_pathless_playout_reproduces_it(name):
    p = plan(name)
    for i, (e, b) in enumerate(zip(p.expected, p.base)):
        if i % pa.K in (0, 1, 2):
            assert _same(e, b), (i, e, b)
        assert len(p.paths[i]) == p.path_len[i] <= p.path_steps <= p.limit
    # every depth d of one playout, not only the plan's three
    i = max(range(p.n), key=lambda i: p.base[i]["length"])
    r, b = p.root_of[i], p.base[i]
    for d in range(b["length"] + 1):
        e = pa.oracle_path_playout(p.cfg, p.roots.inst[r], p.roots.hist[r], p.roots.seed, i, pa.STEP0, p.limit, b["actions"][:d])
        assert _same(e, b), (i, d)


@pytest.mark.parametrize("name, parity", [(n, 0) for n in pa.GPU_CASES] + [(n, 1) for n in pa.BOTH_PARITIES])
def test_every_plan_has_every_end(name, parity):
    p = plan(name, parity)
    figures, missing = pa.mix(p)
    print(f"PATH-MIX {name} parity {parity}: {figures}")
    assert not missing, (missing, figures)
    assert figures["empty"] == p.P
    if name in FIGURES and parity == 0:
        assert (figures["at_end"], figures["inside"], figures["after"], figures["differing"]) == FIGURES[name]


@pytest.mark.parametrize("name", ["small_pin", "rect_4x4_full"])
def test_the_leaf_is_the_node_the_path_names(name):
    """leaf against a second statement of it: replay root and path with step_raw only, stop at the first done."""
    from oracle import oracle as orc
    p = plan(name)
    for i, e in enumerate(p.expected):
        r = p.root_of[i]
        ob = orc.OracleBatch(p.cfg, 1)
        ob.reset_packed(np.asarray(p.roots.inst[r])[None])
        env = ob.env(0)
        for a in p.roots.hist[r]:
            env.step_raw(a)
        for a in p.paths[i]:
            if env.step_raw(a)[1]:
                break
        assert np.array_equal(e["leaf"], pa.leaf_of(p.cfg, env)), i
        if i % pa.K == 0:  # an empty path: the root's own mask
            assert np.array_equal(e["leaf"], pa.leaf_of(p.cfg, p.roots.model.ob.env(r))), i
    j4 = [e for i, e in enumerate(p.expected) if i % pa.K == 4]
    assert all(e["length"] < 3 and e["done"] for e in j4)  # the repeated action ends the episode inside the path
