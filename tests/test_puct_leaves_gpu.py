"""pcbenv_puct_advance_leaves on the GPU (tests/puct_leaves_cases.py has the cases and the CPU model).

1. The kernel alone: recorded leaf-parallel searches fed call by call through `BatchedPlacementEnv.puct_advance_leaves`,
   no evaluation launch; after EVERY call every tensor of the request -- pending among them -- equals the state of
   csrc/pcb_puct_leaves.h replayed on the CPU, floats by their bits.  Every group width (C in 1, 4, 5, 16, 32, 33, 64), L in
   1, 2, 3, 8, 64, P = 130 roots -- three blocks at G = 4 -- T = 5, N = 1 + 40 * C, which the searches of many leaves fill.
2. Every tensor is a view into a sentinel-filled buffer: the guards, the path rows behind path_len and behind a repeat and
   the inputs keep their bytes, and a phase that was not asked for writes nothing.
3. L = 1 against pcbenv_puct_advance on the same calls; one phase per call; trees the caller has damaged; a side stream.
4. On real roots: `puct_search_device(leaves=4)` next to `network_evaluator(leaves=4)` against `puct_search(leaves=4)`,
   and a game of `puct_selfplay(leaves=4)`.
What the cases reach is asserted on the CPU (tests/test_puct_leaves_model.py)."""
import time
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from pcbenv import _leaves_lib, _lib, named_config
from pcbenv.batched_env import BatchedPlacementEnv
from pcbenv.search import Evaluation, network_evaluator, puct_search, puct_search_device, puct_selfplay

import playout_cases as plc
import puct_cases as pc
import puct_leaves_cases as lc
from stream_cases import LAG_MS, lagged
from test_puct_advance_gpu import DTYPES, GUARD, Guarded, advance_and_compare as advance_one_leaf

pytestmark = pytest.mark.gpu


class GuardedLeaves(Guarded):
    """test_puct_advance_gpu.Guarded with pending and the leaf extent of the exchange tensors and the inputs."""

    def __init__(self, P, N, T, K, L, device):
        R = P * L
        shp = dict(lc.shapes(P, N, T, L), value=(R,), leaf_terminal=(R,), cand_count=(R,), cand_actions=(R, K, 3), cand_prior=(R, K), errors_dev=(1,))
        self.device, self.back, self.t, self.meta = device, {}, {}, {}
        for name, shape in shp.items():
            self.add(name, shape, DTYPES.get(name, torch.int32))
        self.t["errors_dev"].zero_()


@pytest.fixture(scope="module")
def handle():
    env = BatchedPlacementEnv(named_config("c3"), 2, queue_depth=1, run_seed=1)  # the handle gives the device only
    yield env
    env.close()


def advance_and_compare(handle, req, g, i, call, want, before):
    """Call i through puct_advance_leaves into the guarded tensors of g; want: the model's state after it; before: the snapshot
    after the call before.  -> the snapshot the call left."""
    inputs = {}
    for name, at, value in call.get("pokes", ()):  # the damage a caller does between two calls
        g.t[name].view(-1)[at] = value
    if call.get("pokes") and not call["phases"] & lc.ABSORB:
        before = g.snapshot()
    if call["phases"] & lc.ABSORB:
        for name, a in zip(pc.INPUTS, call["evaluation"]):
            g.t[name].copy_(torch.from_numpy(np.ascontiguousarray(a)))
            inputs[name] = g.t[name]
        before = g.snapshot()
    handle.puct_advance_leaves(req, call["phases"], **inputs)
    after = g.snapshot()
    for name in after:  # the guards, and what the call only reads
        assert np.array_equal(after[name][:GUARD], before[name][:GUARD]) and np.array_equal(after[name][-GUARD:], before[name][-GUARD:]), (i, name)
        if name in pc.INPUTS:
            assert np.array_equal(after[name], before[name]), (i, name)
    # every tensor against the model: that includes the path rows >= path_len and those behind a repeat, which hold what
    # they held before (the model's tensors start with the same fill)
    for f in lc.STATE_FIELDS:
        got = g.inside(after, f)
        if f in lc.FLOATS:
            assert lc.same_bits(got, want[f]), (i, f)
        else:
            assert np.array_equal(got.astype(np.int64), want[f]), (i, f)
    assert int(g.inside(after, "errors_dev")[0]) == want["errors"], i
    untouched = lc.TREE_FIELDS if call["phases"] == lc.SELECT else ("selected", "path_len", "paths") if call["phases"] in (lc.ABSORB, lc.INIT) else ()
    for f in untouched:  # a phase that was not asked for wrote nothing
        assert np.array_equal(after[f], before[f]), (i, f)
    return after


def assert_equals_the_model_after_every_call(handle, case):
    g = GuardedLeaves(case.P, case.N, case.T, case.K, case.L, handle.device)
    req = handle.puct_leaves_request(g.t, case.c_puct, case.C, case.L)
    assert req.num_leaves == case.L and req.max_children == case.C and req.capacity == case.N and req.max_steps == case.T and req.num_roots == case.P
    before = g.snapshot()
    for i, (call, want) in enumerate(zip(case.seq, case.states)):
        before = advance_and_compare(handle, req, g, i, call, want, before)
    return g


@pytest.mark.parametrize("name", list(lc.GPU_CASES))
def test_the_kernel_alone_equals_the_model_after_every_call(handle, name):
    case = lc.gpu_case(name)
    assert any((s["path_len"] > 0).any() for s in case.states)
    if case.L > 1:
        assert any((s["path_len"] == -1).any() for s in case.states) and any((s["pending"] > 1).any() for s in case.states)
    assert_equals_the_model_after_every_call(handle, case)


def test_one_leaf_is_puct_advance_on_the_same_calls(handle):
    """L = 1 against pcbenv_puct_advance: the same calls into two sets of guarded tensors leave every tree tensor, and the
    selection, identical after every call; pending is zero after every ABSORB."""
    for name in ("C4_L1",):
        case = lc.gpu_case(name)
        old = pc.synthetic(case.P, case.T, case.C, case.K, lc.GPU_CASES[name][3], capacity=case.N)
        a, b = GuardedLeaves(case.P, case.N, case.T, case.K, 1, handle.device), Guarded(case.P, case.N, case.T, case.K, handle.device)
        ra, rb = handle.puct_leaves_request(a.t, case.c_puct, case.C, 1), handle.puct_request(b.t, case.c_puct, case.C)
        sa, sb = a.snapshot(), b.snapshot()
        for i, (call, want, want_old) in enumerate(zip(case.seq, case.states, old.states)):
            sa = advance_and_compare(handle, ra, a, i, call, want, sa)
            _, sb = advance_one_leaf(handle, rb, b, i, call, want_old, sb)
            for f in pc.STATE_FIELDS + tuple(pc.INPUTS) + ("errors_dev",):
                assert np.array_equal(sa[f], sb[f]), (i, f)


@pytest.mark.parametrize("name", ["C5_L3", "C16_L8"])
def test_one_phase_per_call(handle, name):
    both, split = lc.gpu_case(name), lc.gpu_case(name, split=True)
    assert {c["phases"] for c in split.seq} == {lc.INIT, lc.ABSORB, lc.SELECT}
    g = assert_equals_the_model_after_every_call(handle, split)
    last = g.snapshot()
    for f in lc.STATE_FIELDS:  # and the combined calls' end
        got = g.inside(last, f)
        assert lc.same_bits(got, both.states[-1][f]) if f in lc.FLOATS else np.array_equal(got.astype(np.int64), both.states[-1][f]), f


@pytest.mark.parametrize("G, name", lc.DAMAGE_CASES)
def test_a_damaged_tree_is_handled_as_the_model_handles_it(handle, G, name):
    """Trees the caller has damaged (tests/puct_leaves_cases.py:damaged; tests/test_puct_leaves_model.py asserts on the model's
    dump what each scenario comes to): the kernel's lane-parallel checks give what the serial ones give, in every tensor
    after every call.  Only roots 0 < p < P - 1 are damaged: were a check missing, the stray access would fall into a
    neighbouring root's rows, which are compared."""
    sc = lc.damaged(G, name)
    assert 0 < sc.p < sc.P - 1
    N, C = sc.N, sc.C
    allowed = dict(selected=(-2, N), num_nodes=(0, N + 1), first_child=(0, N) + tuple(range(N - C + 1, N)), parent=(sc.node, N),
                   num_children=(-1, C + 5), pending=lc.GARBAGE)
    for f, at, value in sc.seq[sc.k].get("pokes", ()):
        assert value in allowed[f], (f, value)
    for s in sc.states:  # the comparison is by bits: no NaN may come of the damage, where lanes and a loop could differ
        assert not any(np.isnan(s[f]).any() for f in lc.FLOATS)
    assert_equals_the_model_after_every_call(handle, sc)


def test_no_roots_is_a_no_op(handle):
    R = _leaves_lib.PcbenvPuctLeavesRequest
    req = R(struct_size=240, phases=lc.ABSORB | lc.SELECT, num_roots=0, capacity=3, max_children=2, max_steps=2, num_candidates=2, c_puct=1.0, num_leaves=4)
    for n, _ in R._fields_[11:-2]:
        setattr(req, n, handle.reward.data_ptr())
    assert handle._L.pcbenv_puct_advance_leaves(handle._h, req) == _lib.PCBENV_OK
    torch.cuda.synchronize()


def test_side_stream(handle):
    """The whole search is enqueued on a non-blocking side stream behind a delay: it returns before the stream reaches it
    and grows the tree of the default-stream run.  The evaluations are the recorded ones, uploaded beforehand."""
    case = lc.gpu_case("C16_L8")
    P, T, C, L, iterations = case.P, case.T, case.C, case.L, lc.GPU_CASES["C16_L8"][3]
    dev = handle.device
    fixed = [Evaluation(*(torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in c["evaluation"])) for c in case.seq[1:]]
    search_root = SimpleNamespace(num_envs=P, device=dev, cfg=None, puct_leaves_request=handle.puct_leaves_request,
                                  puct_advance_leaves=handle.puct_advance_leaves)

    def search():
        it = iter(fixed)
        return puct_search_device(search_root, iterations, 100, lambda paths, path_len, s: next(it), c_puct=case.c_puct, max_children=C, max_steps=T,
                                  capacity=case.N, leaves=L)
    want = search()
    torch.cuda.synchronize()
    pc.compare_with_search(case.states[-1], SimpleNamespace(**{f: getattr(want, f).cpu() for f in pc.TREE_FIELDS + ("errors",)}))
    side = torch.cuda.Stream()
    with lagged(side) as before:
        search()  # once without a delay: the allocator has the search's buffers on this stream
        side.synchronize()
        before()
        reached = torch.cuda.Event()
        reached.record(side)
        t0 = time.perf_counter()
        got = search()
        dt = 1e3 * (time.perf_counter() - t0)
        ev = torch.cuda.Event()
        ev.record(side)
        assert not reached.query(), f"the search returned only after the stream had passed a {LAG_MS} ms delay ({dt:.2f} ms on the host)"
        assert not ev.query()
        side.synchronize()
    for f in want.__dataclass_fields__:
        a, b = getattr(got, f).cpu(), getattr(want, f).cpu()
        assert a.dtype == b.dtype and a.shape == b.shape and a.numpy().tobytes() == b.numpy().tobytes(), f


# ---- 4. real roots --------------------------------------------------------------------------------------------------
FIELDS = ("parent", "depth", "visits", "num_children", "first_child", "node_action", "prior", "value_sum", "value_max", "terminal",
          "reward_lo", "reward_hi", "num_nodes", "action", "child_visits", "child_actions", "child_priors", "root_value", "errors")
P_REAL, L_REAL, M_REAL, C_REAL = 8, 4, 6, 3


def _envs(cfg, seed):
    root = BatchedPlacementEnv(cfg, P_REAL, queue_depth=2, run_seed=seed, auto_reset=False)
    planner = BatchedPlacementEnv(cfg, P_REAL * L_REAL, queue_depth=2, run_seed=seed, auto_reset=False)
    for e in (root, planner):
        e.generate_instances()
        e.reset()
    return root, planner


def test_device_search_is_the_specification_on_real_roots():
    cfg = plc.case("small_pin")[0]()
    T = plc.max_steps(cfg)
    root, planner = _envs(cfg, 2)
    root.rollout_step(0)  # the roots a transition into their episodes
    dev = root.device
    zeros = torch.zeros((P_REAL * L_REAL, cfg.num_orientations * cfg.height * cfg.width), dtype=torch.float32, device=dev)
    evaluate = network_evaluator(root, planner, lambda obs: zeros, max_children=C_REAL, leaves=L_REAL)
    none = []

    def copied_over(paths, path_len, step_index0):
        ev = evaluate(paths.to(dev), path_len.to(dev), step_index0)
        none.append(int((path_len < 0).sum()))
        return Evaluation(*(getattr(ev, f).cpu() for f in ("value", "terminal", "cand_count", "cand_actions", "cand_prior")))
    want = puct_search(SimpleNamespace(num_envs=P_REAL, cfg=cfg, device="cpu"), M_REAL, 7000, copied_over, c_puct=1.25, max_children=C_REAL,
                       max_steps=T, leaves=L_REAL)
    got = puct_search_device(root, M_REAL, 7000, evaluate, c_puct=1.25, max_children=C_REAL, max_steps=T, leaves=L_REAL)
    torch.cuda.synchronize()
    assert int(want.errors) == 0 and int(want.num_nodes.max()) > 1 + C_REAL and int(want.depth.max()) >= 2
    # several leaves per launch below most roots (a root with nothing legal left has one), and rows that are none
    assert int((want.visits[:, 0] > M_REAL).sum()) >= P_REAL // 2 and 0 < sum(none) < M_REAL * P_REAL * L_REAL // 2
    for f in FIELDS:
        a, b = getattr(got, f).cpu(), getattr(want, f).cpu()
        assert a.dtype == b.dtype and a.shape == b.shape and a.numpy().tobytes() == b.numpy().tobytes(), f
    root.close()
    planner.close()


def test_selfplay_with_leaves_plays_a_game():
    cfg = plc.case("small_pin")[0]()
    root, planner = _envs(cfg, 3)
    dev = root.device
    zeros = torch.zeros((P_REAL * L_REAL, cfg.num_orientations * cfg.height * cfg.width), dtype=torch.float32, device=dev)
    evaluate = network_evaluator(root, planner, lambda obs: zeros, max_children=C_REAL, priors="device", leaves=L_REAL)
    moves = plc.max_steps(cfg)
    pending, visits = [], []

    def on_move(j, tree):
        pending.append(tree["pending"].ne(0).any())
        visits.append(tree["child_visits"].sum(dim=1).clone())
    got = puct_selfplay(root, evaluate, moves, M_REAL, step_index=500, c_puct=1.25, max_children=C_REAL, on_move=on_move, leaves=L_REAL)
    torch.cuda.synchronize()
    assert int(got.errors) == 0
    assert len(pending) == moves and not any(bool(x) for x in pending)  # pending is zero after every move's search
    assert int(visits[0].max()) > M_REAL - 1  # more than one leaf per launch went through the root's children
    assert bool(got.done.any()) and tuple(got.tree["pending"].shape) == (P_REAL, 1 + 2 * M_REAL * L_REAL * C_REAL)
    root.close()
    planner.close()


def test_the_alphazero_trainer_collects_and_updates_with_leaves():
    """AlphaZeroConfig(leaves=2): the planner has P * 2 environments, collect() plays searched moves whose launches carry two
    leaves per root, and update() trains on what it kept.  The 10 x 10 spatial configuration of tests/test_alphazero_gpu.py."""
    from pcbenv import EnvConfig
    from pcbenv.alphazero import AlphaZeroConfig, AlphaZeroTrainer
    from pcbenv.policy import SpatialPolicy
    torch.manual_seed(0)
    P, L, M, C = 16, 2, 4, 8
    cfg = EnvConfig.spatial(10, 10, 9, 9, 2, 2, 2, 2, 5, 5, 3, 3, 6, 6, "centroid", 2, 0.75)
    root = BatchedPlacementEnv(cfg, P, queue_depth=4, auto_reset=True)
    planner = BatchedPlacementEnv(cfg, P * L, queue_depth=1)
    for e in (root, planner):
        e.generate_instances()
        e.reset()
    trainer = AlphaZeroTrainer(root, planner, SpatialPolicy(cfg).to(root.device),
                               AlphaZeroConfig(moves=2, iterations=M, max_children=C, leaves=L, device_loss=True))
    batch = trainer.collect()
    torch.cuda.synchronize()
    assert int(batch["errors"]) == 0 and batch["child_visits"].shape == (2, P, C)
    visits = batch["child_visits"][0].sum(dim=1)
    assert int(visits.max()) > M - 1 and int(visits.max()) <= M * L  # more than one leaf per launch went below the root
    stats = trainer.update(batch)
    assert all(np.isfinite(stats[k]) for k in ("policy", "value", "entropy"))
    with pytest.raises(ValueError):  # a planner of P environments is not one for two leaves
        AlphaZeroTrainer(root, root, SpatialPolicy(cfg).to(root.device), AlphaZeroConfig(leaves=L))
    root.close()
    planner.close()
