"""pcbenv_playout on the GPU, through BatchedPlacementEnv.playout and direct calls of the C ABI, bit for bit against two
independent expectations: (a) the existing device path -- gather_ into a planner of n environments, then rollout_step
until the first done -- and (b) the CPU oracle (playout_cases.oracle_playout: reset_packed, a replay of the root's
actions, then draw / step_raw).  The roots are built with handle_model.Run following a plan made on the CPU
(playout_cases.Roots), so (b) and the mix of roots and ends a case must contain exist before any device call."""
from collections import Counter

import numpy as np
import pytest
import torch

from pcbenv import _lib, named_config
from pcbenv.batched_env import BatchedPlacementEnv
from pcbenv.config import KIND_SQUARE
from pcbenv.search import best_of_k, best_of_k_playouts, child_index

import playout_cases as pc
from handle_model import Run, _bytes_equal, _same_info

pytestmark = pytest.mark.gpu

_ROOTS = {}


def cpu_roots(name, parity):
    """The CPU plan of a case and the oracle's playouts from it, computed once."""
    key = (name, parity)
    if key not in _ROOTS:
        cfg = pc.case(name)[0]()
        roots = pc.Roots(name, pc.max_steps(cfg) + parity)
        _ROOTS[key] = (roots, pc.oracle_playouts(roots, [i // pc.K for i in range(roots.P * pc.K)]))
    return _ROOTS[key]


def device_roots(roots, **kw):
    """A Run brought to the plan's state (every step compared with the oracle on the way, as Run.step does)."""
    run = Run(roots.cfg, roots.P, run_seed=roots.seed, auto_reset=False, **dict(roots.kw, **kw))
    for t in range(roots.launches):
        run.step(t)
        if roots.plan[t] is not None:
            run.env.reset(torch.from_numpy(roots.plan[t]))
            run.oracle_reset(roots.plan[t])
    for i in range(roots.P):  # the device drew what the plan drew: the plan's expectations are this handle's
        assert np.array_equal(np.array(run.hist[i]).reshape(-1, 3), np.array(roots.hist[i]).reshape(-1, 3)), i
        assert roots.cfg.kind == KIND_SQUARE or np.array_equal(run.inst[i], roots.inst[i]), i
    return run


def check_against(po, expected, cfg, flat_first=None):
    """A Playout against a list of oracle playouts: reward and info by bit pattern, the rest exactly."""
    r, d, n = po.reward.cpu().numpy(), po.done.cpu().numpy(), po.length.cpu().numpy()
    acts = None if po.actions is None else po.actions.cpu().numpy()
    inf = None if po.info is None else po.info.cpu().numpy()
    assert (inf is not None) == pc.has_info(cfg)
    for i, e in enumerate(expected):
        assert n[i] == e["length"] and d[i] == e["done"], (i, n[i], d[i], e["length"], e["done"])
        assert np.float64(r[i]).tobytes() == e["reward"].tobytes(), (i, r[i], e["reward"])
        if inf is not None:
            assert _same_info(inf[i], e["info"]), (i, inf[i], e["info"])
        if acts is not None:
            m = min(e["length"], acts.shape[0])
            if acts.ndim == 3:
                assert np.array_equal(acts[:m, i], e["actions"][:m]), (i, acts[:m, i], e["actions"][:m])
            else:
                a = e["actions"][:m]
                want = a[:, 0] * cfg.height * cfg.width + a[:, 1] * cfg.width + a[:, 2]
                if flat_first is not None and m:
                    want[0] = flat_first[i]  # row 0: the forced action as given
                assert np.array_equal(acts[:m, i], want), (i, acts[:m, i], want)
            assert not acts[m:, i].any(), (i, "a row behind the playout's end was written")


def planner_playouts(root_env, cfg, n, index, seed, kw, limit, first=None):
    """Expectation (a): gather_ into a planner of n environments, rollout_step until the first done."""
    planner = BatchedPlacementEnv(cfg, n, queue_depth=1, run_seed=seed, **kw)
    planner.generate_instances()
    planner.reset()
    planner.gather_(index, source=root_env)
    dev = planner.device
    acts = torch.zeros((limit, n, 3), dtype=torch.int32, device=dev)
    final = torch.zeros(n, dtype=torch.float64, device=dev)
    info = torch.full((n, 2), float("nan"), dtype=torch.float64, device=dev)
    length = torch.zeros(n, dtype=torch.int32, device=dev)
    fin = torch.zeros(n, dtype=torch.bool, device=dev)
    for t in range(limit):
        if t == 0 and first is not None:
            _, r, d, _ = planner.step(first)
            acts[0] = first
        else:
            _, r, d, _, _ = planner.rollout_step(pc.STEP0 + t, out=acts[t])
        live = ~fin
        final = torch.where(live, r, final)
        info = torch.where(live[:, None], planner.info_raw, info)
        length = torch.where(live, torch.full_like(length, t + 1), length)
        acts[t] = torch.where(live[:, None], acts[t], torch.zeros_like(acts[t]))
        fin |= d.bool()
    out = dict(reward=final.cpu().numpy(), done=fin.cpu().numpy().astype(np.uint8), length=length.cpu().numpy(),
               info=info.cpu().numpy(), actions=acts.cpu().numpy())
    planner.close()
    return out


def check_same_as_planner(po, want, cfg):
    assert _bytes_equal(po.reward.cpu().numpy(), want["reward"])
    assert np.array_equal(po.done.cpu().numpy(), want["done"]) and np.array_equal(po.length.cpu().numpy(), want["length"])
    if po.info is not None:
        assert _same_info(po.info.cpu().numpy(), want["info"])
    assert np.array_equal(po.actions.cpu().numpy(), want["actions"])


@pytest.mark.parametrize("parity", [0, 1])
@pytest.mark.parametrize("name", list(pc.CASES))
def test_kinds_and_shapes(name, parity):
    """Case 1: every kind and team shape, roots at different depths, after an even and an odd number of step launches
    (the state blocks are double-buffered)."""
    roots, expected = cpu_roots(name, parity)
    cfg, P, K = roots.cfg, roots.P, pc.K
    status = Counter(roots.status())
    assert status["fresh"] >= 1 and status["mid"] >= 1 and status["finished"] >= 1, status
    assert cfg.kind == KIND_SQUARE or status["last"] >= 1, status
    ends = Counter("placed" if e["placed_all"] else "stuck" for e in expected)
    if cfg.kind == KIND_SQUARE:
        assert ends["stuck"] == len(expected)  # the square kind only ends with no legal cell left
    else:
        assert ends["placed"] >= 1
        assert name not in pc.SMALL_GRIDS or ends["stuck"] >= 1, ends
    assert len({e["length"] for e in expected}) >= 3 and all(e["done"] for e in expected)
    run = device_roots(roots)
    limit = pc.max_steps(cfg)
    po = run.env.playout(k=K, step_index=pc.STEP0)
    assert po.actions.shape == (limit, P * K, 3)
    check_against(po, expected, cfg)                                                     # (b) the CPU oracle
    want = planner_playouts(run.env, cfg, P * K, child_index(P, K, run.env.device), roots.seed, roots.kw, limit)
    check_same_as_planner(po, want, cfg)                                                 # (a) the existing device path
    run.compare_oracle("the roots after the playouts")
    run.close()


@pytest.mark.parametrize("parity", [0, 1])
@pytest.mark.parametrize("name", list(pc.EDGE_CASES))
def test_edge_shapes(name, parity):
    """Case 1 at the shapes where k_playout takes another path than at the named configurations (the table of
    playout_cases.EDGE_CASES): two mask words per row on one and on four wavefronts, more rows and pins than lanes,
    padding bits behind W, placements 64 or more bits wide and over both words, beam width 4, 1x1 components, a grid the
    first placement fills.  The mix each case must contain is playout_cases.edge_mix, computed before any device call.
    rect_4x4_full cannot have a root between fresh and finished (its first placement ends the episode), so there the
    mix asks for none instead."""
    roots, expected = cpu_roots(name, parity)
    cfg, P, K = roots.cfg, roots.P, pc.K
    mix, missing = pc.edge_mix(name, roots, expected)
    print(f"EDGE-MIX {name} parity {parity} seed {roots.seed}: {mix}")
    assert not missing, (missing, mix)
    run = device_roots(roots)
    limit = pc.max_steps(cfg)
    po = run.env.playout(k=K, step_index=pc.STEP0)
    assert po.actions.shape == (limit, P * K, 3)
    check_against(po, expected, cfg)                                                     # (b) the CPU oracle
    want = planner_playouts(run.env, cfg, P * K, child_index(P, K, run.env.device), roots.seed, roots.kw, limit)
    check_same_as_planner(po, want, cfg)                                                 # (a) the existing device path
    run.compare_oracle("the roots after the playouts")
    run.close()


def _tensors(e):
    d = {"traj/" + k: v.cpu().numpy() for k, v in e.traj.items()}
    d.update(reward=e.traj_reward.cpu().numpy(), done=e.traj_done.cpu().numpy(), info=e.traj_info.cpu().numpy(),
             mask_bits=e.mask_bits().cpu().numpy())
    return d


@pytest.mark.parametrize("kw", [dict(auto_reset=True), dict(auto_reset=True, num_slots=3)], ids=["auto_reset", "slots3"])
def test_root_is_untouched(kw):
    """Case 2: state blocks, every bound tensor and the queue cursors before and after; the next step against a twin."""
    cfg = named_config("c3")
    a, b = (BatchedPlacementEnv(cfg, 16, queue_depth=3, run_seed=4, **kw) for _ in range(2))
    for e in (a, b):
        e.generate_instances()
        e.reset()
    for t in range(cfg.max_num_components + 6):  # past the first episode ends: terminal-list marks, presampled actions, resets
        for e in (a, b):
            e.select_slot(t + 1)
            e.rollout_step(t)
        if t % 5 == 3 or t == cfg.max_num_components - 2:
            sd, before, cursors = a.state_dict(), _tensors(a), a.queue_cursors()
            po = a.playout(k=3, step_index=50 + t)
            assert int(po.length.min()) >= 1
            sd2, after = a.state_dict(), _tensors(a)
            assert a.queue_cursors() == cursors
            for k in before:
                assert _bytes_equal(before[k], after[k]), (t, k)
            for k in ("state", "generator"):
                assert _bytes_equal(np.asarray(sd[k]), np.asarray(sd2[k])), (t, k)
        ta, tb = _tensors(a), _tensors(b)
        for k in ta:
            assert _bytes_equal(ta[k], tb[k]), (t, k, "against the twin that never ran a playout")
    a.close(); b.close()


def _forced_cases(roots):
    """Per root a forced first action: legal, illegal (a cell the current component cannot take), out of range, legal, ..."""
    cfg = roots.cfg
    first = np.zeros((roots.P, 3), np.int32)
    kinds = []
    for i in range(roots.P):
        legal = pc.draw(cfg, roots.model.ob.env(i), 99, i, 7)
        kind = ("legal", "illegal", "range", "legal")[i % 4]
        if kind == "legal":
            first[i] = legal
        elif kind == "illegal":
            first[i] = (1, cfg.height - 1, cfg.width - 1)  # no component of two cells or more fits into the last cell
        else:
            first[i] = ((7, 0, 0), (0, -1, 3), (1, 2, cfg.width + 100))[(i // 4) % 3]
        kinds.append(kind)
    return first, kinds


@pytest.mark.parametrize("name,flat", [("c3_centroid", False), ("c3_centroid", True), ("spatial_7x100", True)],
                         ids=["tuple", "flat", "spatial_7x100-flat"])
def test_forced_first_actions(name, flat):
    """Case 3: legal, illegal and out-of-range first actions in both formats; a bad one is a terminal transition with the
    worst-case reward, as pcbenv_step makes it (the oracle's step_raw).  spatial_7x100: the flat decode by H * W = 700
    and W = 100, no power of two."""
    roots, _ = cpu_roots(name, 0)
    cfg, P = roots.cfg, roots.P
    first, kinds = _forced_cases(roots)
    H, W, A = cfg.height, cfg.width, cfg.num_orientations * cfg.height * cfg.width
    if flat:
        given = first[:, 0].astype(np.int64) * H * W + first[:, 1] * W + first[:, 2]
        for i, k in enumerate(kinds):
            if k == "range":
                given[i] = (-3, A, A + 12345)[(i // 4) % 3]
        given = given.astype(np.int32)
        decoded = np.stack([pc.decode_flat(cfg, int(a)) for a in given])
    else:
        given, decoded = first, first
    expected = pc.oracle_playouts(roots, list(range(P)), first_actions=decoded)
    status = roots.status()
    bad = [i for i in range(P) if kinds[i] != "legal" and status[i] != "finished"]
    assert len(bad) >= 4 and any(kinds[i] == "legal" and status[i] != "finished" for i in range(P))
    worst = min(e["reward"] for e in expected)
    for i in bad:
        assert expected[i]["length"] == 1 and expected[i]["done"] == 1 and expected[i]["reward"] == worst, i
    assert any(expected[i]["length"] > 1 for i in range(P))
    run = device_roots(roots)
    dev = run.env.device
    idx = torch.arange(P, dtype=torch.int32, device=dev)
    po = run.env.playout(index=idx, step_index=pc.STEP0, first_actions=torch.from_numpy(given).to(dev))
    check_against(po, expected, cfg, flat_first=given if flat else None)
    if not flat:
        want = planner_playouts(run.env, cfg, P, idx, roots.seed, roots.kw, pc.max_steps(cfg), first=torch.from_numpy(given).to(dev))
        check_same_as_planner(po, want, cfg)
    run.close()


def _direct(env, n, index, limit, actions_steps, actions, err):
    """pcbenv_playout called directly with the caller's own tensors."""
    dev = env.device
    out = dict(reward=torch.full((n,), -5.0, dtype=torch.float64, device=dev), done=torch.full((n,), 9, dtype=torch.uint8, device=dev),
               length=torch.full((n,), -9, dtype=torch.int32, device=dev), info=torch.full((n, 2), 5.0, dtype=torch.float64, device=dev))
    rc = env._L.pcbenv_playout(env._h, None if index is None else index.data_ptr(), n, None, _lib.ACTION_TUPLE, limit,
                               out["reward"].data_ptr(), out["done"].data_ptr(), out["length"].data_ptr(), out["info"].data_ptr(),
                               None if actions is None else actions.data_ptr(), actions_steps, None if err is None else err.data_ptr(),
                               env.run_seed, 0, pc.STEP0, env._stream())
    return rc, {k: v.cpu().numpy() for k, v in out.items()}


def test_root_index_with_repeats_and_errors():
    """Case 4: an explicit root_index with repeats and three out-of-range values."""
    roots, _ = cpu_roots("c3_centroid", 0)
    cfg, P = roots.cfg, roots.P
    index = np.array([0, 0, 3, P, 2, -1, 5, 5, 100000, 1, 11, 3], np.int32)
    ok = (index >= 0) & (index < P)
    assert (~ok).sum() == 3
    expected = pc.oracle_playouts(roots, [int(r) if g else 0 for r, g in zip(index, ok)])
    run = device_roots(roots)
    dev, n, limit = run.env.device, len(index), pc.max_steps(cfg)
    idx = torch.from_numpy(index).to(dev)
    err = torch.zeros(1, dtype=torch.int32, device=dev)
    acts = torch.full((limit, n, 3), -7, dtype=torch.int32, device=dev)
    rc, out = _direct(run.env, n, idx, limit, limit, acts, err)
    assert rc == _lib.PCBENV_OK and int(err.item()) == 1
    acts = acts.cpu().numpy()
    for i in range(n):
        if not ok[i]:  # the stated outputs of an out-of-range row; none of its action rows written
            assert out["length"][i] == 0 and out["done"][i] == 0 and out["reward"][i].tobytes() == np.float64(0.0).tobytes()
            assert np.isnan(out["info"][i]).all() and (acts[:, i] == -7).all()
            continue
        e = expected[i]
        assert out["length"][i] == e["length"] and out["done"][i] == e["done"] and out["reward"][i].tobytes() == e["reward"].tobytes(), i
        assert _same_info(out["info"][i], e["info"]) and np.array_equal(acts[:e["length"], i], e["actions"]) and (acts[e["length"]:, i] == -7).all()
    with pytest.raises(IndexError):
        run.env.playout(index=idx, step_index=pc.STEP0, check=True)
    good = run.env.playout(index=idx.clamp(0, P - 1), step_index=pc.STEP0, check=True)  # nothing out of range: no error
    assert np.array_equal(good.length.cpu().numpy()[ok], out["length"][ok])
    # without an error word the rows are the same
    rc, out2 = _direct(run.env, n, idx, limit, 0, None, None)
    assert rc == _lib.PCBENV_OK and all(_bytes_equal(out[k][ok], out2[k][ok]) for k in ("reward", "done", "length"))
    run.close()


@pytest.mark.parametrize("name", ["small_pin", "c3_centroid", "spatial_7x100"])
def test_truncation(name):
    """Case 5: max_steps = 2, actions_steps = 1: cut playouts report done = 0 and length = 2; action rows beyond
    actions_steps are not written.  Next to the cut playouts there are ones that end at their first transition and, in
    small_pin, ones that end exactly at max_steps (every c3 instance has 16 components and no root of the plan is two
    transitions from its end, so there the cut ones stand next to length 1 only).  spatial_7x100: two mask words per row
    with padding bits behind column 100."""
    roots, _ = cpu_roots(name, 1)
    cfg, P, K = roots.cfg, roots.P, 2
    root_of = [i // K for i in range(P * K)]
    expected = pc.oracle_playouts(roots, root_of, limit=2)
    cut = [i for i, e in enumerate(expected) if not e["done"]]
    assert len(cut) >= 4 and any(e["done"] and e["length"] == 1 for e in expected)
    assert name != "small_pin" or any(e["done"] and e["length"] == 2 for e in expected)
    run = device_roots(roots)
    dev, n = run.env.device, P * K
    acts = torch.full((2, n, 3), -7, dtype=torch.int32, device=dev)
    rc, out = _direct(run.env, n, None, 2, 1, acts, None)
    assert rc == _lib.PCBENV_OK
    acts = acts.cpu().numpy()
    assert (acts[1] == -7).all(), "a row beyond actions_steps was written"
    for i, e in enumerate(expected):
        assert out["length"][i] == e["length"] and out["done"][i] == e["done"] and out["reward"][i].tobytes() == e["reward"].tobytes(), i
        assert _same_info(out["info"][i], e["info"]) and np.array_equal(acts[0, i], e["actions"][0])
    for i in cut:
        assert out["length"][i] == 2 and out["done"][i] == 0 and out["reward"][i] == 0.0 and np.isnan(out["info"][i]).all()
    po = run.env.playout(k=K, step_index=pc.STEP0, max_steps=2, actions_steps=1)
    assert po.actions.shape == (1, n, 3) and np.array_equal(po.actions.cpu().numpy()[0], acts[0])
    assert run.env.playout(k=K, step_index=pc.STEP0, max_steps=2, actions_steps=0).actions is None
    with pytest.raises(ValueError):
        run.env.playout(k=K, max_steps=2, actions_steps=3)
    with pytest.raises(ValueError):
        run.env.playout(k=K, max_steps=0)
    run.close()


def test_state_errors():
    cfg = named_config("c2")
    env = BatchedPlacementEnv(cfg, 8, queue_depth=1, run_seed=1)
    with pytest.raises(_lib.PcbenvError) as ei:  # no episode yet
        env.playout(k=2)
    assert ei.value.code == _lib.PCBENV_ESTATE
    env.generate_instances()
    env.reset()
    assert int(env.playout(k=2).length.min()) >= 1
    rc, _ = _direct(env, 12, None, 3, 0, None, None)  # 12 playouts over 8 environments without an index
    assert rc == _lib.PCBENV_EINVAL
    env.close()


def test_best_of_k_playouts_equals_best_of_k():
    """Case 6: field by field on c3 with P = 8, k = 4."""
    cfg = named_config("c3")
    P, k = 8, 4
    root = BatchedPlacementEnv(cfg, P, queue_depth=1, run_seed=6)
    root.generate_instances()
    root.reset()
    for t in range(3):
        root.rollout_step(t)
    planner = BatchedPlacementEnv(cfg, P * k, queue_depth=1, run_seed=6)
    planner.generate_instances()
    planner.reset()
    want = best_of_k(root, planner, k, step_index=1000)
    got = best_of_k_playouts(root, k, step_index=1000)
    assert _bytes_equal(got.reward.cpu().numpy(), want.reward.cpu().numpy())
    assert _bytes_equal(got.child_rewards.cpu().numpy(), want.child_rewards.cpu().numpy())
    assert torch.equal(got.child, want.child) and torch.equal(got.length, want.length)
    assert got.length.dtype == want.length.dtype and got.actions.shape == want.actions.shape and got.actions.dtype == want.actions.dtype
    for p in range(P):
        n = int(want.length[p])
        assert torch.equal(got.actions[:n, p], want.actions[:n, p]), p
    planner.close(); root.close()
