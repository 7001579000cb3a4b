"""pcbenv_gumbel_advance on the GPU (tests/gumbel_cases.py has the cases and the CPU model).

1. The kernel alone: every case through the C ABI into tensors that are views into sentinel-filled guarded buffers; after
   each call every tensor of the request, and every guard, equals the state of csrc/pcb_gumbel.h run on the CPU, bit for
   bit; a call without ABSORB leaves the tree tensors byte-identical.  Damaged roots as the model handles them; once
   without an error word; no roots; a side stream.
2. `gumbel_search_device` against `gumbel_search`, field by field, floats by their bits: a fresh tree, then the kept,
   rerooted tree, with scripted evaluations; and once with `network_evaluator(priors="device")` and constant logits.
3. `puct_selfplay(gumbel=)` against the same game composed call by call from the specification.
4. `AlphaZeroTrainer` with gumbel_considered: a collect, the device loss against the torch chain on the collected targets,
   an update."""
import ctypes
import time
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from pcbenv import _gumbel_lib, _lib, _move_lib, named_config
from pcbenv.batched_env import BatchedPlacementEnv
from pcbenv.search import (Evaluation, gumbel_search, gumbel_search_device, network_evaluator, new_gumbel_tensors, new_move_tensors, new_puct_tree,
                           puct_reroot, puct_selfplay, search_tree)

import gumbel_cases as gc
import playout_cases as plc
import puct_cases as pc
import puct_move_cases as mc
from stream_cases import LAG_MS, lagged

pytestmark = pytest.mark.gpu

GUARD, SENTINEL = 256, 0xA5
INPUTS = pc.INPUTS
F64, U8, F32 = ("prior", "value_sum", "value_max", "reward_lo", "reward_hi", "root_value", "value"), ("terminal", "leaf_terminal"), ("child_policy", "cand_prior")


def _dtype(name):
    return torch.float64 if name in F64 else torch.uint8 if name in U8 else torch.float32 if name in F32 else torch.int32


class Guarded:
    """Every tensor given as a view GUARD bytes into a sentinel-filled buffer of its own, GUARD bytes behind it."""

    def __init__(self, arrays, device):
        self.back, self.t, self.meta = {}, {}, {}
        for name, src in arrays.items():
            src, dtype = np.ascontiguousarray(src), _dtype(name)
            n = src.size * torch.empty((), dtype=dtype).element_size()
            buf = torch.full((GUARD + n + GUARD,), SENTINEL, dtype=torch.uint8, device=device)
            self.back[name] = buf
            self.t[name] = buf[GUARD:GUARD + n].view(dtype).view(src.shape)
            self.t[name].copy_(torch.from_numpy(src).to(dtype))
            self.meta[name] = (self.t[name].cpu().numpy().dtype, src.shape)

    def snapshot(self):
        return {name: buf.cpu().numpy().copy() for name, buf in self.back.items()}

    def inside(self, snap, name):
        dtype, shape = self.meta[name]
        return snap[name][GUARD:len(snap[name]) - GUARD].view(dtype).reshape(shape)


@pytest.fixture(scope="module")
def handle():
    env = BatchedPlacementEnv(named_config("c3"), 2, queue_depth=1, run_seed=1)  # the handle gives the device only
    yield env
    env.close()


def _outputs(P, C):
    shp = gc.shapes(P, 1, C)
    return {f: np.full(shp[f], gc.FILL, np.float64 if f == "root_value" else np.float32 if f == "child_policy" else np.int32) for f in gc.OUT_FIELDS}


def _abi_call(handle, req, call, inputs=None, K=0, stream=None):
    """One pcbenv_gumbel_advance call through the C ABI: the request's scalars and ABSORB inputs are the call's."""
    req.phases, req.seed, req.step_index, req.first_root = call["phases"], call["seed"] & (2 ** 64 - 1), call["step_index"] & (2 ** 64 - 1), call["first_root"]
    req.num_candidates = K if inputs is not None else 0
    for name in INPUTS:
        setattr(req, name, inputs.t[name].data_ptr() if inputs is not None else None)
    req.stream = (stream if stream is not None else torch.cuda.current_stream(handle.device)).cuda_stream
    assert handle._L.pcbenv_gumbel_advance(handle._h, ctypes.byref(req)) == _lib.PCBENV_OK, handle._L.pcbenv_last_error(handle._h)


def _same_as_model(got, want, name):
    if name in F64:
        return pc.same_bits(got, want)
    if name == "child_policy":
        return pc.same_bits(got, want)
    return np.array_equal(got.astype(np.int64), want)


def assert_equals_the_model_after_every_call(handle, c, seq, states, errors_dev=True):
    """c: a case of gumbel_cases; seq, states: the calls and the model's states after them."""
    dev = handle.device
    arrays = dict(c.state, considered=c.table, **_outputs(c.P, c.C))
    if errors_dev:
        arrays["errors_dev"] = np.zeros(1, np.int32)
    g = Guarded(arrays, dev)
    req = handle.gumbel_request(g.t, c.rule[0], c.C, c.rule[1], c.rule[2])
    assert (req.errors_dev is not None) == errors_dev and (req.num_roots, req.capacity, req.max_children, req.max_steps) == (c.P, c.N, c.C, gc.T)
    assert (req.num_simulations, req.max_considered) == (c.n, c.Mc)
    for i, (call, want) in enumerate(zip(seq, states)):
        if errors_dev:
            g.t["errors_dev"].zero_()  # the model reports the bits of each call
        for name, at, value in call["pokes"]:  # what the caller has done to its tree
            g.t[name].view(-1)[at] = value
        inputs = Guarded(dict(zip(INPUTS, call["evaluation"])), dev) if call["phases"] & gc.ABSORB else None
        before, given = g.snapshot(), inputs.snapshot() if inputs else {}
        _abi_call(handle, req, call, inputs, c.K)
        after, left = g.snapshot(), inputs.snapshot() if inputs else {}
        for name in arrays:
            assert np.array_equal(after[name][:GUARD], before[name][:GUARD]) and np.array_equal(after[name][-GUARD:], before[name][-GUARD:]), (i, name)
        for name in given:  # what the call only reads
            assert np.array_equal(left[name], given[name]), (i, name)
        assert np.array_equal(after["considered"], before["considered"]), i
        if not call["phases"] & gc.ABSORB:  # SELECT and CHOOSE never store to the tree
            for name in gc.TREE_FIELDS:
                assert np.array_equal(after[name], before[name]), (i, name)
        if not call["phases"] & gc.CHOOSE:
            for name in gc.OUT_FIELDS:
                assert np.array_equal(after[name], before[name]), (i, name)
        for name in gc.STATE_FIELDS + gc.OUT_FIELDS:
            assert _same_as_model(g.inside(after, name), want[name], name), (i, name)
        if errors_dev:
            assert int(g.inside(after, "errors_dev")[0]) == want["errors"], i


# ---- 1. the kernel alone --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(gc.CASES))
def test_the_kernel_alone_equals_the_model_after_every_call(handle, name):
    gc.check_cases()
    c = gc.case(name)
    assert_equals_the_model_after_every_call(handle, c, c.seq, c.states)


@pytest.mark.parametrize("name", list(gc.DAMAGE))
def test_a_damaged_root_is_handled_as_the_model_handles_it(handle, name):
    """Only a root 0 < p < P - 1 is damaged -- were a check missing, the stray access would fall into a neighbouring root's
    rows, or into the guards, which are compared -- and only by values the model has run under the sanitizers."""
    c, at, seq, states, p = gc.damaged(name)
    assert 0 < p < c.P - 1
    assert_equals_the_model_after_every_call(handle, c, seq, states)


def test_without_an_error_word(handle):
    c, at, seq, states, p = gc.damaged("select_first_child_0")
    assert states[-1]["errors"] == gc.ERR_TREE
    assert_equals_the_model_after_every_call(handle, c, seq, states, errors_dev=False)


def test_no_roots_is_a_no_op(handle):
    R = _gumbel_lib.PcbenvGumbelRequest
    req = R(struct_size=ctypes.sizeof(R), phases=gc.BEGIN | gc.ABSORB | gc.SELECT, num_roots=0, capacity=3, max_children=2, max_steps=2, num_candidates=1,
            num_simulations=4, max_considered=2, c_puct=1.0, c_visit=50.0, c_scale=1.0)
    for n in _gumbel_lib.PUCT_TREE_TENSORS + _gumbel_lib.PUCT_EXCHANGE + _gumbel_lib.PUCT_INPUTS + _gumbel_lib.GUMBEL_BUDGET + _gumbel_lib.GUMBEL_OUTPUTS:
        setattr(req, n, handle.reward.data_ptr())
    assert handle._L.pcbenv_gumbel_advance(handle._h, ctypes.byref(req)) == _lib.PCBENV_OK
    tree = new_puct_tree(0, 3, 2, handle.device)
    tree.update(new_gumbel_tensors(0, 2, 2, 4, handle.device))
    handle.gumbel_advance(handle.gumbel_request(tree, 1.0, 2), gc.BEGIN | gc.SELECT)  # and through the binding, whose empty tensors have no address
    torch.cuda.synchronize()


def test_side_stream(handle):
    """The launch enqueued on a non-blocking side stream behind a delay: the call returns before the stream reaches it and
    gives the model's result."""
    c = gc.case("G16_C16_P67")
    dev = handle.device
    got = {f: torch.from_numpy(np.ascontiguousarray(v)).to(dev).to(_dtype(f)) for f, v in dict(c.state, considered=c.table, **_outputs(c.P, c.C)).items()}
    got["errors_dev"] = torch.zeros(1, dtype=torch.int32, device=dev)
    req = handle.gumbel_request(got, c.rule[0], c.C, c.rule[1], c.rule[2])
    side = torch.cuda.Stream()
    torch.cuda.synchronize()
    with lagged(side) as before:
        before()
        reached = torch.cuda.Event()
        reached.record(side)
        t0 = time.perf_counter()
        _abi_call(handle, req, c.seq[0], stream=side)
        dt = 1e3 * (time.perf_counter() - t0)
        ev = torch.cuda.Event()
        ev.record(side)
        assert not reached.query(), f"the call returned only after the stream had passed a {LAG_MS} ms delay ({dt:.2f} ms on the host)"
        assert not ev.query()
        side.synchronize()
    for f in gc.STATE_FIELDS:
        assert _same_as_model(got[f].cpu().numpy(), c.states[0][f], f), f
    assert int(got["errors_dev"][0]) == c.states[0]["errors"]


# ---- 2. the search against the specification ---------------------------------------------------------------------------
def _same(a, b):
    a, b = a.cpu(), b.cpu()
    return a.shape == b.shape and a.to(torch.float64 if a.is_floating_point() else torch.int64).numpy().tobytes() == \
        b.to(torch.float64 if b.is_floating_point() else torch.int64).numpy().tobytes()


RESULT = ("action", "child_visits", "child_actions", "child_priors", "root_value", "errors") + mc.TREE_FIELDS
CHOICE = ("sim_index", "sim_visits", "move_slot", "move_action", "child_weights", "child_policy", "child_actions", "root_value")


def _assert_same_search(got, want):
    for f in RESULT:
        assert _same(getattr(got.search, f), getattr(want.search, f)), f
    for f in CHOICE:
        assert _same(getattr(got, f), getattr(want, f)), f
    assert got.child_policy.dtype == want.child_policy.dtype == torch.float32 and got.child_weights.dtype == want.child_weights.dtype == torch.int32


def _on_device(evaluate, dev):
    def on_device(paths, path_len, step_index0):
        ev = evaluate(paths.cpu(), path_len.cpu(), step_index0)
        return Evaluation(*(getattr(ev, f).to(dev).contiguous() for f in ("value", "terminal", "cand_count", "cand_actions", "cand_prior")))
    return on_device


def _copied_over(evaluate, dev):
    def copied_over(paths, path_len, step_index0):
        ev = evaluate(paths.to(dev), path_len.to(dev), step_index0)
        return Evaluation(*(getattr(ev, f).cpu() for f in ("value", "terminal", "cand_count", "cand_actions", "cand_prior")))
    return copied_over


def test_the_device_search_is_the_specification_on_a_fresh_and_on_a_kept_tree(handle):
    """P = 5, n = 8 simulations over Mc = 4 candidates, C = 8, scripted evaluations (a function of the path): the search of a
    fresh tree, pcbenv_puct_move(REROOT) on the move_slot CHOOSE wrote, and the search of the kept tree."""
    P, n, Mc, C, T, K = 5, 8, 4, 8, 5, 8
    root = BatchedPlacementEnv(named_config("c2"), P, queue_depth=1, run_seed=3, first_env_index=2)
    dev, N = root.device, 1 + 2 * (n + 1) * C
    cpu_root = SimpleNamespace(num_envs=P, cfg=None, device="cpu")
    kw = dict(max_considered=Mc, c_visit=50.0, c_scale=1.0, c_puct=1.25, max_children=C, max_steps=T)
    spec = dict(kw, seed=root.run_seed ^ 0x67756d62, first_root=2)
    first, second = pc.synthetic_evaluator(P, T, K, 31), pc.synthetic_evaluator(P, T, K, 37)
    got = gumbel_search_device(root, n, 100, _on_device(first, dev), capacity=N, **kw)  # a tree of its own
    want = gumbel_search(cpu_root, n, 100, first, capacity=N, **spec)
    _assert_same_search(got, want)
    assert bool((want.sim_index == n).any()) and bool((want.move_slot >= 1).any()) and int(want.search.errors) == 0
    # the same in a tree the caller keeps, then the move, then the next search in what is left
    tree = new_puct_tree(P, N, T, dev)
    tree.update(new_move_tensors(P, N, C, dev))
    tree.update(new_gumbel_tensors(P, C, Mc, n, dev))
    root.puct_advance(root.puct_request(tree, 1.25, C), _lib.TREE_INIT)
    again = gumbel_search_device(root, n, 100, _on_device(first, dev), tree=tree, **kw)
    _assert_same_search(again, want)
    root.puct_move(root.puct_move_request(tree, C), _move_lib.MOVE_REROOT)  # reads move_slot as CHOOSE wrote it
    kept, remap = puct_reroot(search_tree(want.search), want.move_slot)
    assert _same(tree["remap"], remap) and bool((kept["num_children"][:, 0] > 0).any())
    got2 = gumbel_search_device(root, n, 200, _on_device(second, dev), tree=tree, gumbel_step_index=101, **kw)
    want2 = gumbel_search(cpu_root, n, 200, second, tree=kept, gumbel_step_index=101, **spec)
    _assert_same_search(got2, want2)
    assert not _same(got2.child_policy, got.child_policy)
    root.close()


def test_the_device_search_with_a_network_evaluator():
    """A small pin configuration, P = 6, C = 4: `network_evaluator(priors="device")` with constant logits.  The evaluator is a
    function of the paths, so the device search and the specification (its evaluations copied over) share one."""
    cfg, P, C, n, Mc = plc.case("small_pin")[0](), 6, 4, 6, 4
    T = plc.max_steps(cfg)
    root = BatchedPlacementEnv(cfg, P, queue_depth=2, run_seed=2, auto_reset=False)
    planner = BatchedPlacementEnv(cfg, P, queue_depth=2, run_seed=2, auto_reset=False)
    for e in (root, planner):
        e.generate_instances()
        e.reset()
    root.rollout_step(0)  # the roots a transition into their episodes
    dev = root.device
    zeros = torch.zeros((P, cfg.num_orientations * cfg.height * cfg.width), dtype=torch.float32, device=dev)
    evaluate = network_evaluator(root, planner, lambda obs: zeros, max_children=C, priors="device")
    kw = dict(max_considered=Mc, c_visit=50.0, c_scale=1.0, c_puct=1.25, max_children=C, max_steps=T)
    got = gumbel_search_device(root, n, 300, evaluate, **kw)
    torch.cuda.synchronize()
    want = gumbel_search(SimpleNamespace(num_envs=P, cfg=cfg, device="cpu"), n, 300, _copied_over(evaluate, dev), seed=root.run_seed ^ 0x67756d62,
                         first_root=0, **kw)
    _assert_same_search(got, want)
    assert int(want.search.errors) == 0 and bool((want.sim_index == n).any())
    for e in (root, planner):
        e.close()


# ---- 3. self-play ----------------------------------------------------------------------------------------------------
def _envs(cfg, P, count, seed=11, **kw):
    def make():
        e = BatchedPlacementEnv(cfg, P, queue_depth=1, run_seed=seed, **kw)
        e.generate_instances()
        e.reset()
        return e
    return [make() for _ in range(count)]


def test_selfplay_with_gumbel_is_the_loop_of_the_specification():
    cfg, P, n, J, C, rule = named_config("c3"), 8, 8, 3, 16, (4, 50.0, 1.0)
    T = cfg.max_num_components
    root_a, plan_a, root_b, plan_b = envs = _envs(cfg, P, 4)
    dev = root_a.device
    zeros = torch.zeros((P, cfg.num_orientations * cfg.height * cfg.width), dtype=torch.float32, device=dev)
    trees = []
    keep = lambda j, tree: trees.append({f: tree[f].clone() for f in mc.TREE_FIELDS + ("remap", "move_slot")})
    got = puct_selfplay(root_a, network_evaluator(root_a, plan_a, lambda obs: zeros, max_children=C, priors="device"), J, n, step_index=500,
                        c_puct=1.25, max_children=C, on_move=keep, gumbel=rule)
    torch.cuda.synchronize()
    ev_b = _copied_over(network_evaluator(root_b, plan_b, lambda obs: zeros, max_children=C, priors="device"), dev)
    cpu_root = SimpleNamespace(num_envs=P, cfg=cfg, device="cpu")
    N = 1 + 2 * (n + 1) * C
    tree, kept_some = None, False
    for j in range(J):
        gs = gumbel_search(cpu_root, n, 500 + j * (n + 1) * T, ev_b, max_considered=rule[0], c_visit=rule[1], c_scale=rule[2], c_puct=1.25,
                           max_children=C, max_steps=T, capacity=N, tree=tree, seed=root_b.run_seed ^ 0x67756d62, first_root=0, gumbel_step_index=500 + j)
        _, reward, done, _ = root_b.step(gs.move_action.to(dev))
        tree, remap = puct_reroot(search_tree(gs.search), gs.move_slot, done.cpu())
        assert _same(got.actions[j], gs.move_action) and _same(got.child_visits[j], gs.child_weights), j
        assert _same(got.child_actions[j], gs.child_actions) and _same(got.root_value[j], gs.root_value), j
        assert _same(got.reward[j], reward) and _same(got.done[j], done) and _same(got.kept_visits[j], tree["visits"][:, 0]), j
        assert _same(trees[j]["move_slot"], gs.move_slot), j  # what pcbenv_puct_move(REROOT) read
        for f in mc.TREE_FIELDS:
            assert _same(trees[j][f], tree[f]), (j, f)
        assert _same(trees[j]["remap"], remap), j
        kept_some = kept_some or bool((tree["visits"][:, 0] > 0).any())
        weights = gs.child_weights.to(torch.int64)
        k = gs.search.num_children[:, 0]
        assert bool(((weights.sum(dim=1) - 2 ** 24).abs() <= k // 2 + 1)[k > 0].all()) and bool((weights.sum(dim=1)[k == 0] == 0).all())
    for f in mc.TREE_FIELDS:  # the final tree
        assert _same(got.tree[f], tree[f]), f
    assert kept_some and int(got.errors) == int(tree["errors_dev"][0]) == 0
    with pytest.raises(ValueError):
        puct_selfplay(root_a, ev_b, 1, n, gumbel=rule, root_noise=(0.3, 0.25))
    for e in envs:
        e.close()


# ---- 4. the trainer --------------------------------------------------------------------------------------------------
def test_the_trainer_collects_and_updates_on_the_gumbel_target():
    """One collect and one update with gumbel_considered = 4; pcbenv_evaluate_visits on the collected child_weights against
    cross_entropy_torch on the same rows, with the atol of 1e-4 tests/test_evaluate_visits_gpu.py holds the two to."""
    from pcbenv import EnvConfig
    from pcbenv.alphazero import AlphaZeroConfig, AlphaZeroTrainer
    from pcbenv.policy import SpatialPolicy
    from pcbenv.visit_targets import cross_entropy, cross_entropy_torch
    torch.manual_seed(0)
    P, MOVES, n, C = 32, 2, 4, 8
    cfg = EnvConfig.spatial(10, 10, 9, 9, 2, 2, 2, 2, 5, 5, 3, 3, 6, 6, "centroid", 2, 0.75)
    root = BatchedPlacementEnv(cfg, P, queue_depth=4, auto_reset=True)
    planner = BatchedPlacementEnv(cfg, P, queue_depth=1)
    for e in (root, planner):
        e.generate_instances()
        e.reset()
    dev = root.device
    trainer = AlphaZeroTrainer(root, planner, SpatialPolicy(cfg).to(dev),
                               AlphaZeroConfig(moves=MOVES, iterations=n, max_children=C, device_loss=True, gumbel_considered=4, entropy_coef=0.01))
    for t in range(3):
        root.step(root.sample_actions(t))
    batch = trainer.collect()
    N, A = MOVES * P, cfg.num_orientations * cfg.height * cfg.width
    assert int(batch["errors"]) == 0 and batch["child_visits"].shape == (MOVES, P, C) and batch["child_visits"].dtype == torch.int32
    weights, actions, bits = batch["child_visits"].reshape(N, C), batch["child_actions"].reshape(N, C, 3), batch["mask_bits"].reshape(N, 2, 10, 1)
    total = weights.to(torch.int64).sum(dim=1)
    assert bool(((total - 2 ** 24).abs() <= C // 2 + 1).all()) and bool((weights >= 0).all())
    share = (weights > 0).float().mean().item()
    print(f"GUMBEL-TARGET share of root entries with weight {share:.3f}")
    logits = torch.randn((N, A), device=dev)
    ce, ent = cross_entropy(root, logits, bits.contiguous(), weights.contiguous(), actions.contiguous())
    want_ce, want_ent = cross_entropy_torch(cfg, logits.cpu().double(), bits.cpu(), weights.cpu(), actions.cpu())  # the float64 chain
    assert bool(torch.isfinite(ce).all()) and float((ce.cpu().double() - want_ce).abs().max()) <= 1e-4 and float((ent.cpu().double() - want_ent).abs().max()) <= 1e-4
    out = trainer.update(batch)
    assert set(out) == {"loss", "policy", "value", "entropy"} and all(np.isfinite(v) for v in out.values()), out
    for e in (root, planner):
        e.close()
