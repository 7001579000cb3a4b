"""The pin layouts of tests/routing_layouts.py, without a GPU: the committed table reaches every branch of the routing
reward the layouts were built for (coverage conditions on the tracer's events and on the CPU model of the pair sweep --
conditions, not measurements), and the oracle is pinned to the reference at exactly these layouts: reward and info bit for
bit against tests/golden/routing_layouts.npz, and the beam path of every net three ways -- fixture, tracer,
oracle.beam_search."""
import numpy as np
import pytest

import routing_layouts as rl
from oracle import oracle as orc


def _bits(*v):
    return tuple(int(b) for b in np.array(v, np.float64).view(np.uint64))


def test_the_table_is_the_recorded_one():
    z, rows = rl.fixture()
    lays = rl.layouts()
    assert [str(n) for n in z["names"]] == list(lays)
    assert z["num_nets"].tolist() == [len(lay) for lay in lays.values()]
    assert z["net_sizes"].tolist() == [len(net) for lay in lays.values() for net in lay]
    assert z["cells"].tolist() == [list(c) for lay in lays.values() for net in lay for c in net]
    per_layout = sum(2 * len(rl.BEAM_WIDTHS[kind]) + 1 for kind in rl.KINDS) + 1  # + the pin kind's centroid on 64 x 64
    assert len(rows) == per_layout * len(lays)
    for lay in lays.values():
        rl.check_layout(lay)


def test_coverage_conditions():
    ev = rl.event_counts()
    print("ROUTING-LAYOUT-EVENTS " + " ".join(f"{k}={ev[k]}" for k in sorted(ev)))
    missed = [k for k, holds in rl.conditions().items() if not holds]
    assert not missed, missed


def test_both_seeds_are_the_first_that_serve():
    assert rl.pick_both_seeds() == {1: rl.BOTH_SEEDS[0], -1: rl.BOTH_SEEDS[1], 0: rl.BOTH_SEEDS[2]}


def test_oracle_equals_reference_bits():
    _, rows = rl.fixture()
    lays = rl.layouts()
    cfgs = {}
    bad = []
    for (name, kind, rt, k, side), want in rows.items():
        cfg = cfgs.setdefault((kind, rt, k, side), rl.config(kind, rt, k, side))
        if _bits(*orc.find_reward(cfg, lays[name])) != want:
            bad.append((name, kind, rt, k, side))
    assert not bad, bad


def test_paths_three_ways():
    z, _ = rl.fixture()
    lays = rl.layouts()
    for k in (1, 2, 3, 4):
        rec, at = z[f"paths_k{k}"].tolist(), 0
        for name, lay in lays.items():
            for net, (path, _) in zip(lay, rl.trace(name, k)):
                want = rec[at:at + len(net)]
                at += len(net)
                assert sorted(want) == list(range(len(net))), (name, k)
                assert path == want, (name, k, "tracer", net)
                st = want[0]
                got = orc.beam_search(net[st], [p for i, p in enumerate(net) if i != st], k)
                assert [net.index(p) for p in got] == want, (name, k, "oracle", net)
                assert rl.pin_outlier(net) == st, (name, k, "pin_outlier", net)
        assert at == len(rec)


@pytest.mark.parametrize("kind,rt,k,shift,side", [("pin", "beam", 1, 0, 24), ("spatial", "both", 3, 1, 24), ("pin", "centroid", 2, 0, 64)])
def test_episodes_realise_the_layouts(kind, rt, k, shift, side):
    """layout_episode: the records pass pack_instances, the placements are legal, no episode ends before its last
    placement, and the terminal reward and info are the fixture's for the layout."""
    _, rows = rl.fixture()
    cfg = rl.config(kind, rt, k, side)
    names, packed, acts = rl.batch(kind, shift, side)
    B = len(names)
    ob = orc.OracleBatch(cfg, B)
    ob.reset_packed(packed)
    for t in range(rl.T):
        rr, dd, ii = ob.step(acts[t])
        assert dd.all() if t == rl.T - 1 else not dd.any(), t
    for i, name in enumerate(names):
        assert _bits(rr[i], ii[i, 0], ii[i, 1]) == rows[(name, kind, rt, k, side)], name
    assert (acts[:, :, 0] == 0).all()


def test_record_rules_for_both_pin_kinds():
    """What check_records (csrc/pcb_config.hip) asks of a record: net-major pins, spatial ids a permutation, pin-kind ids
    below max_num_pins_per_component and distinct inside a component, every pin inside its component."""
    for kind in rl.KINDS:
        cfg = rl.config(kind, "beam", 2)
        for name, lay in rl.layouts().items():
            inst, acts = rl.layout_episode(cfg, lay, rl.T)
            assert inst.num_components == rl.T == len(acts) and inst.num_pins == sum(map(len, lay))
            assert (np.diff(inst.pin_net) >= 0).all() and set(inst.pin_net.tolist()) == set(range(len(lay)))
            assert (inst.pin_rel_x < inst.comp_h[inst.pin_comp]).all() and (inst.pin_rel_y < inst.comp_w[inst.pin_comp]).all()
            if kind == "spatial":
                assert sorted(inst.pin_id.tolist()) == list(range(inst.num_pins))
            else:
                assert inst.pin_id.max() < cfg.max_num_pins_per_component
                assert len(set(zip(inst.pin_comp.tolist(), inst.pin_id.tolist()))) == inst.num_pins
            cells = [(a[1] + int(x), a[2] + int(y)) for a, x, y in zip((acts[c] for c in inst.pin_comp), inst.pin_rel_x, inst.pin_rel_y)]
            assert cells == [c for net in lay for c in net], name
            assert set(inst.comp_h[inst.pin_comp].tolist()) == set(inst.comp_w[inst.pin_comp].tolist()) == ({1} if inst.num_pins <= 64 else {2}), name


@pytest.mark.parametrize("method", ["beam", "centroid"])
def test_sweep_model_counts_the_oracles_intersections(method):
    """tools/pair_sweep_model.cpp, however the sweep steps are dealt to teams and wavefronts."""
    for name, lay in rl.layouts().items():
        for k in ((2, 4) if method == "beam" else (2,)):
            want = orc.find_num_intersection(orc.route(lay, method, k))
            for nwaves, nparts in ((1, 1), (4, 1), (1, 2), (4, 3)):
                assert rl.sweep_stats(lay, method, k, nwaves, nparts)["hits"] == want, (name, method, k, nwaves, nparts)
