"""pcbenv_gumbel_tree_advance on the GPU (tests/gumbel_tree_cases.py has the cases and the CPU model; the guarded views and
the comparisons are tests/test_gumbel_gpu.py's).

1. The kernel alone: every case through the C ABI into tensors that are views into sentinel-filled guarded buffers; after
   each call every tensor of the request, and every guard, equals the state of csrc/pcb_gumbel_tree.h run on the CPU, bit for
   bit; a call without ABSORB leaves the tree tensors byte-identical.  Damaged roots, and damaged nodes below the root, as the
   model handles them; once without an error word; no roots; a side stream.
2. `gumbel_search_device(full=True)` against `gumbel_search(full=True)`, field by field, floats by their bits: a fresh tree,
   then the kept, rerooted tree, with scripted evaluations.
3. `puct_selfplay(gumbel=, gumbel_full=True)` against the same game composed call by call from the specification.
4. `AlphaZeroTrainer` with gumbel_full: a collect and an update."""
import ctypes
import time
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from pcbenv import _gumbel_lib, _lib, _move_lib, named_config
from pcbenv.batched_env import BatchedPlacementEnv
from pcbenv.search import (gumbel_search, gumbel_search_device, network_evaluator, new_gumbel_tensors, new_move_tensors, new_puct_tree, puct_reroot,
                           puct_selfplay, search_tree)

import gumbel_tree_cases as gt
import puct_cases as pc
import puct_move_cases as mc
import test_gumbel_gpu as tg
from stream_cases import LAG_MS, lagged

pytestmark = pytest.mark.gpu

GUARD, INPUTS = tg.GUARD, tg.INPUTS


@pytest.fixture(scope="module")
def handle():
    env = BatchedPlacementEnv(named_config("c3"), 2, queue_depth=1, run_seed=1)  # the handle gives the device only
    yield env
    env.close()


def _abi_call(handle, req, call, inputs=None, K=0, stream=None):
    """One pcbenv_gumbel_tree_advance call through the C ABI: the request's scalars and ABSORB inputs are the call's."""
    req.phases, req.seed, req.step_index, req.first_root = call["phases"], call["seed"] & (2 ** 64 - 1), call["step_index"] & (2 ** 64 - 1), call["first_root"]
    req.num_candidates = K if inputs is not None else 0
    for name in INPUTS:
        setattr(req, name, inputs.t[name].data_ptr() if inputs is not None else None)
    req.stream = (stream if stream is not None else torch.cuda.current_stream(handle.device)).cuda_stream
    assert handle._L.pcbenv_gumbel_tree_advance(handle._h, ctypes.byref(req)) == _lib.PCBENV_OK, handle._L.pcbenv_last_error(handle._h)


def assert_equals_the_model_after_every_call(handle, c, seq, states, errors_dev=True):
    """c: a case of gumbel_tree_cases; seq, states: the calls and the model's states after them."""
    dev = handle.device
    arrays = dict(c.state, considered=c.table, **tg._outputs(c.P, c.C))
    if errors_dev:
        arrays["errors_dev"] = np.zeros(1, np.int32)
    g = tg.Guarded(arrays, dev)
    req = handle.gumbel_request(g.t, float("nan"), c.C, c.rule[1], c.rule[2])  # c_puct is never read
    assert (req.errors_dev is not None) == errors_dev and (req.num_roots, req.capacity, req.max_children, req.max_steps) == (c.P, c.N, c.C, gt.T)
    assert (req.num_simulations, req.max_considered) == (c.n, c.Mc)
    for i, (call, want) in enumerate(zip(seq, states)):
        if errors_dev:
            g.t["errors_dev"].zero_()  # the model reports the bits of each call
        for name, at, value in call["pokes"]:  # what the caller has done to its tree
            g.t[name].view(-1)[at] = value
        inputs = tg.Guarded(dict(zip(INPUTS, call["evaluation"])), dev) if call["phases"] & gt.ABSORB else None
        before, given = g.snapshot(), inputs.snapshot() if inputs else {}
        _abi_call(handle, req, call, inputs, c.K)
        after, left = g.snapshot(), inputs.snapshot() if inputs else {}
        for name in arrays:
            assert np.array_equal(after[name][:GUARD], before[name][:GUARD]) and np.array_equal(after[name][-GUARD:], before[name][-GUARD:]), (i, name)
        for name in given:  # what the call only reads
            assert np.array_equal(left[name], given[name]), (i, name)
        assert np.array_equal(after["considered"], before["considered"]), i
        if not call["phases"] & gt.ABSORB:  # SELECT and CHOOSE never store to the tree
            for name in gt.TREE_FIELDS:
                assert np.array_equal(after[name], before[name]), (i, name)
        if not call["phases"] & gt.CHOOSE:
            for name in gt.OUT_FIELDS:
                assert np.array_equal(after[name], before[name]), (i, name)
        for name in gt.STATE_FIELDS + gt.OUT_FIELDS:
            assert tg._same_as_model(g.inside(after, name), want[name], name), (i, name)
        if errors_dev:
            assert int(g.inside(after, "errors_dev")[0]) == want["errors"], i


# ---- 1. the kernel alone --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(gt.CASES))
def test_the_kernel_alone_equals_the_model_after_every_call(handle, name):
    gt.check_cases()
    c = gt.case(name)
    assert_equals_the_model_after_every_call(handle, c, c.seq, c.states)


@pytest.mark.parametrize("name", list(gt.DAMAGE))
def test_a_damaged_tree_is_handled_as_the_model_handles_it(handle, name):
    """Only a root 0 < p < P - 1 is damaged -- were a check missing, the stray access would fall into a neighbouring root's
    rows, or into the guards, which are compared -- and only by values the model has run under the sanitizers."""
    c, at, seq, states, p = gt.damaged(name)
    assert 0 < p < c.P - 1
    assert_equals_the_model_after_every_call(handle, c, seq, states)


def test_without_an_error_word(handle):
    c, at, seq, states, p = gt.damaged("below_first_child_0")
    assert states[-1]["errors"] == gt.ERR_TREE
    assert_equals_the_model_after_every_call(handle, c, seq, states, errors_dev=False)


def test_no_roots_is_a_no_op(handle):
    R = _gumbel_lib.PcbenvGumbelRequest
    req = R(struct_size=ctypes.sizeof(R), phases=gt.BEGIN | gt.ABSORB | gt.SELECT, num_roots=0, capacity=3, max_children=2, max_steps=2, num_candidates=1,
            num_simulations=4, max_considered=2, c_puct=1.0, c_visit=50.0, c_scale=1.0)
    for n in _gumbel_lib.PUCT_TREE_TENSORS + _gumbel_lib.PUCT_EXCHANGE + _gumbel_lib.PUCT_INPUTS + _gumbel_lib.GUMBEL_BUDGET + _gumbel_lib.GUMBEL_OUTPUTS:
        setattr(req, n, handle.reward.data_ptr())
    assert handle._L.pcbenv_gumbel_tree_advance(handle._h, ctypes.byref(req)) == _lib.PCBENV_OK
    tree = new_puct_tree(0, 3, 2, handle.device)
    tree.update(new_gumbel_tensors(0, 2, 2, 4, handle.device))
    handle.gumbel_tree_advance(handle.gumbel_request(tree, 1.0, 2), gt.BEGIN | gt.SELECT)  # and through the binding, whose empty tensors have no address
    torch.cuda.synchronize()


def test_side_stream(handle):
    """The launch enqueued on a non-blocking side stream behind a delay: the call returns before the stream reaches it and
    gives the model's result."""
    c = gt.case("G16_C16_P67")
    dev, i = handle.device, 1  # SELECT alone on the hand-built trees
    assert c.seq[i]["phases"] == gt.SELECT
    start = dict(c.states[0], considered=c.table)
    got = {f: torch.from_numpy(np.ascontiguousarray(v)).to(dev).to(tg._dtype(f)) for f, v in start.items() if f != "errors"}
    got["errors_dev"] = torch.zeros(1, dtype=torch.int32, device=dev)
    req = handle.gumbel_request(got, c.rule[0], c.C, c.rule[1], c.rule[2])
    side = torch.cuda.Stream()
    torch.cuda.synchronize()
    with lagged(side) as before:
        before()
        reached = torch.cuda.Event()
        reached.record(side)
        t0 = time.perf_counter()
        _abi_call(handle, req, c.seq[i], stream=side)
        dt = 1e3 * (time.perf_counter() - t0)
        ev = torch.cuda.Event()
        ev.record(side)
        assert not reached.query(), f"the call returned only after the stream had passed a {LAG_MS} ms delay ({dt:.2f} ms on the host)"
        assert not ev.query()
        side.synchronize()
    for f in gt.STATE_FIELDS:
        assert tg._same_as_model(got[f].cpu().numpy(), c.states[i][f], f), f
    assert int(got["errors_dev"][0]) == c.states[i]["errors"]


# ---- 2. the search against the specification ---------------------------------------------------------------------------
def test_the_device_search_is_the_specification_on_a_fresh_and_on_a_kept_tree(handle):
    """P = 5, n = 8 simulations over Mc = 4 candidates, C = 8, T = 5, scripted evaluations (a function of the path): the search
    of a fresh tree, pcbenv_puct_move(REROOT) on the move_slot CHOOSE wrote, and the search of the kept tree."""
    P, n, Mc, C, T, K = 5, 8, 4, 8, 5, 8
    root = BatchedPlacementEnv(named_config("c2"), P, queue_depth=1, run_seed=3, first_env_index=2)
    dev, N = root.device, 1 + 2 * (n + 1) * C
    cpu_root = SimpleNamespace(num_envs=P, cfg=None, device="cpu")
    kw = dict(max_considered=Mc, c_visit=50.0, c_scale=1.0, c_puct=1.25, max_children=C, max_steps=T, full=True)
    spec = dict(kw, seed=root.run_seed ^ 0x67756d62, first_root=2)
    first, second = pc.synthetic_evaluator(P, T, K, 31), pc.synthetic_evaluator(P, T, K, 37)
    got = gumbel_search_device(root, n, 100, tg._on_device(first, dev), capacity=N, **kw)  # a tree of its own
    want = gumbel_search(cpu_root, n, 100, first, capacity=N, **spec)
    tg._assert_same_search(got, want)
    assert bool((want.sim_index == n).any()) and bool((want.move_slot >= 1).any()) and int(want.search.errors) == 0
    assert int(want.search.depth.max()) >= 3  # the node rule ran below the root
    plain = gumbel_search(cpu_root, n, 100, first, capacity=N, **dict(spec, full=False))
    assert not tg._same(plain.search.visits, want.search.visits)  # and it is another search than the root rule's
    tree = new_puct_tree(P, N, T, dev)
    tree.update(new_move_tensors(P, N, C, dev))
    tree.update(new_gumbel_tensors(P, C, Mc, n, dev))
    root.puct_advance(root.puct_request(tree, 1.25, C), _lib.TREE_INIT)
    again = gumbel_search_device(root, n, 100, tg._on_device(first, dev), tree=tree, **kw)
    tg._assert_same_search(again, want)
    root.puct_move(root.puct_move_request(tree, C), _move_lib.MOVE_REROOT)  # reads move_slot as CHOOSE wrote it
    kept, remap = puct_reroot(search_tree(want.search), want.move_slot)
    assert tg._same(tree["remap"], remap) and bool((kept["num_children"][:, 0] > 0).any())
    got2 = gumbel_search_device(root, n, 200, tg._on_device(second, dev), tree=tree, gumbel_step_index=101, **kw)
    want2 = gumbel_search(cpu_root, n, 200, second, tree=kept, gumbel_step_index=101, **spec)
    tg._assert_same_search(got2, want2)
    root.close()


# ---- 3. self-play ----------------------------------------------------------------------------------------------------
def test_selfplay_with_the_full_rule_is_the_loop_of_the_specification():
    cfg, P, n, J, C, rule = named_config("c3"), 8, 8, 2, 16, (4, 50.0, 1.0)
    T = cfg.max_num_components
    root_a, plan_a, root_b, plan_b = envs = tg._envs(cfg, P, 4)
    dev = root_a.device
    zeros = torch.zeros((P, cfg.num_orientations * cfg.height * cfg.width), dtype=torch.float32, device=dev)
    trees = []
    keep = lambda j, tree: trees.append({f: tree[f].clone() for f in mc.TREE_FIELDS + ("remap", "move_slot")})
    got = puct_selfplay(root_a, network_evaluator(root_a, plan_a, lambda obs: zeros, max_children=C, priors="device"), J, n, step_index=500,
                        c_puct=1.25, max_children=C, on_move=keep, gumbel=rule, gumbel_full=True)
    torch.cuda.synchronize()
    ev_b = tg._copied_over(network_evaluator(root_b, plan_b, lambda obs: zeros, max_children=C, priors="device"), dev)
    cpu_root = SimpleNamespace(num_envs=P, cfg=cfg, device="cpu")
    N = 1 + 2 * (n + 1) * C
    tree = None
    for j in range(J):
        gs = gumbel_search(cpu_root, n, 500 + j * (n + 1) * T, ev_b, max_considered=rule[0], c_visit=rule[1], c_scale=rule[2], c_puct=1.25, max_children=C,
                           max_steps=T, capacity=N, tree=tree, seed=root_b.run_seed ^ 0x67756d62, first_root=0, gumbel_step_index=500 + j, full=True)
        _, reward, done, _ = root_b.step(gs.move_action.to(dev))
        tree, remap = puct_reroot(search_tree(gs.search), gs.move_slot, done.cpu())
        assert tg._same(got.actions[j], gs.move_action) and tg._same(got.child_visits[j], gs.child_weights), j
        assert tg._same(got.child_actions[j], gs.child_actions) and tg._same(got.root_value[j], gs.root_value), j
        assert tg._same(got.reward[j], reward) and tg._same(got.done[j], done) and tg._same(got.kept_visits[j], tree["visits"][:, 0]), j
        assert tg._same(trees[j]["move_slot"], gs.move_slot), j
        for f in mc.TREE_FIELDS:
            assert tg._same(trees[j][f], tree[f]), (j, f)
        assert tg._same(trees[j]["remap"], remap), j
    assert int(got.errors) == int(tree["errors_dev"][0]) == 0 and bool((tree["visits"][:, 0] > 0).any())
    for e in envs:
        e.close()


# ---- 4. the trainer --------------------------------------------------------------------------------------------------
def test_the_trainer_collects_and_updates_with_the_full_rule():
    from pcbenv import EnvConfig
    from pcbenv.alphazero import AlphaZeroConfig, AlphaZeroTrainer
    from pcbenv.policy import SpatialPolicy
    torch.manual_seed(0)
    P, MOVES, n, C = 32, 2, 4, 8
    cfg = EnvConfig.spatial(10, 10, 9, 9, 2, 2, 2, 2, 5, 5, 3, 3, 6, 6, "centroid", 2, 0.75)
    root = BatchedPlacementEnv(cfg, P, queue_depth=4, auto_reset=True)
    planner = BatchedPlacementEnv(cfg, P, queue_depth=1)
    for e in (root, planner):
        e.generate_instances()
        e.reset()
    trainer = AlphaZeroTrainer(root, planner, SpatialPolicy(cfg).to(root.device),
                               AlphaZeroConfig(moves=MOVES, iterations=n, max_children=C, device_loss=True, gumbel_considered=4, gumbel_full=True,
                                               entropy_coef=0.01))
    for t in range(3):
        root.step(root.sample_actions(t))
    batch = trainer.collect()
    assert int(batch["errors"]) == 0 and batch["child_visits"].shape == (MOVES, P, C) and batch["child_visits"].dtype == torch.int32
    total = batch["child_visits"].reshape(MOVES * P, C).to(torch.int64).sum(dim=1)
    assert bool(((total - 2 ** 24).abs() <= C // 2 + 1).all()) and bool((batch["child_visits"] >= 0).all())
    out = trainer.update(batch)
    assert set(out) == {"loss", "policy", "value", "entropy"} and all(np.isfinite(v) for v in out.values()), out
    for e in (root, planner):
        e.close()
