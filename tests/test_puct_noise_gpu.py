"""pcbenv_puct_root_noise on the GPU (tests/puct_noise_cases.py has the cases and the CPU model).

1. The kernel alone: every case through the C ABI into tensors that are views into sentinel-filled guarded buffers; after
   each of the two calls every tensor of the request, and every guard, equals the state of csrc/pcb_puct_noise.h run on
   the CPU, bit for bit -- so nothing but the children's priors and `noised` is written, and the second call is a no-op.
   Damaged roots as the model handles them; once without an error word; no roots; a side stream.
2. `puct_search_device(root_noise=)` against `puct_search(root_noise=)`, field by field, floats by their bits: a fresh tree,
   a kept tree whose root is expanded, leaves = 2.
3. `puct_selfplay(root_noise=)` against the same game composed call by call from the specification; eps = 0 against the
   game without noise."""
import ctypes
import time
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from pcbenv import _lib, _noise_lib, named_config
from pcbenv.batched_env import BatchedPlacementEnv
from pcbenv.search import (MOVE_PROPORTIONAL, Evaluation, _puct_iterations, network_evaluator, new_puct_tree, puct_choose, puct_reroot, puct_search, puct_search_device,
                           puct_selfplay, search_tree)

import playout_cases as plc
import puct_cases as pc
import puct_move_cases as mc
import puct_noise_cases as nc
from stream_cases import LAG_MS, lagged

pytestmark = pytest.mark.gpu

GUARD, SENTINEL = 256, 0xA5
FIELDS = ("num_children", "first_child", "prior", "noised", "errors_dev")


class Guarded:
    """Every tensor of a request as a view GUARD bytes into a sentinel-filled buffer of its own, GUARD bytes behind it."""

    def __init__(self, tree, device):
        self.back, self.t, self.meta = {}, {}, {}
        for name in FIELDS:
            src = np.zeros(1, np.int32) if name == "errors_dev" else np.ascontiguousarray(tree[name])
            dtype = torch.float64 if name == "prior" else torch.int32
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


def _abi_call(handle, req, call, stream=None):
    """One pcbenv_puct_root_noise call through the C ABI: the request's scalars are the call's, first_root included."""
    req.alpha, req.eps, req.seed, req.step_index, req.first_root = call["alpha"], call["eps"], call["seed"], call["step_index"], call["first_root"]
    req.stream = (stream if stream is not None else torch.cuda.current_stream(handle.device)).cuda_stream
    assert handle._L.pcbenv_puct_root_noise(handle._h, ctypes.byref(req)) == _lib.PCBENV_OK


def assert_equals_the_model_after_every_call(handle, tree, C, seq, errors_dev=True):
    states = nc.run(tree, C, seq)
    g = Guarded(tree, handle.device)
    req = handle.puct_noise_request(g.t if errors_dev else {n: t for n, t in g.t.items() if n != "errors_dev"}, C)
    assert (req.errors_dev is not None) == errors_dev and req.max_children == C and (req.num_roots, req.capacity) == tree["prior"].shape
    for i, (call, want) in enumerate(zip(seq, states)):
        g.t["errors_dev"].zero_()  # the model reports the bits of each call
        before = g.snapshot()
        _abi_call(handle, req, call)
        after = g.snapshot()
        for name in FIELDS:
            assert np.array_equal(after[name][:GUARD], before[name][:GUARD]) and np.array_equal(after[name][-GUARD:], before[name][-GUARD:]), (i, name)
        for name in ("num_children", "first_child"):  # what the call only reads
            assert np.array_equal(after[name], before[name]), (i, name)
        assert pc.same_bits(g.inside(after, "prior"), want["prior"]), i
        assert np.array_equal(g.inside(after, "noised").astype(np.int64), want["noised"]), i
        assert int(g.inside(after, "errors_dev")[0]) == (want["errors"] if errors_dev else 0), i
    return states


# ---- 1. the kernel alone --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(nc.CASES))
def test_the_kernel_alone_equals_the_model_after_every_call(handle, name):
    nc.check_cases()
    c = nc.case(name)
    first, second = assert_equals_the_model_after_every_call(handle, c.tree, c.C, c.seq)
    assert pc.same_bits(first["prior"], second["prior"]) and np.array_equal(first["noised"], second["noised"])  # the second call is a no-op


@pytest.mark.parametrize("name", list(nc.DAMAGE))
def test_a_damaged_root_is_handled_as_the_model_handles_it(handle, name):
    """Only a root 0 < p < P - 1 is damaged -- were a check missing, the stray access would fall into a neighbouring root's
    rows, or into the guards, which are compared -- and only by values the model has run under the sanitizers."""
    c, tree, p = nc.damaged(name)
    st = assert_equals_the_model_after_every_call(handle, tree, c.C, c.seq)[0]
    assert st["errors"] == nc.ERR_TREE and st["noised"][p] == 0
    assert_equals_the_model_after_every_call(handle, tree, c.C, c.seq, errors_dev=False)


def test_no_roots_is_a_no_op(handle):
    R = _noise_lib.PcbenvPuctNoiseRequest
    req = R(struct_size=ctypes.sizeof(R), num_roots=0, capacity=3, max_children=2, alpha=0.3, eps=0.25)
    for n in _noise_lib.NOISE_TENSORS:
        setattr(req, n, handle.reward.data_ptr())
    assert handle._L.pcbenv_puct_root_noise(handle._h, ctypes.byref(req)) == _lib.PCBENV_OK
    tree = new_puct_tree(0, 3, 2, handle.device)
    handle.puct_root_noise(handle.puct_noise_request(tree, 2), 0.3, 0.25)  # and through the binding, whose empty tensors have no address
    torch.cuda.synchronize()


def test_side_stream(handle):
    """The launch enqueued on a non-blocking side stream behind a delay: the call returns before the stream reaches it and
    gives the model's result."""
    c = nc.case("G16_C16_P67")
    want = nc.run(c.tree, c.C, c.seq[:1])[0]
    dev = handle.device
    got = {f: torch.from_numpy(np.ascontiguousarray(v)).to(dev) for f, v in c.tree.items()}
    got["errors_dev"] = torch.zeros(1, dtype=torch.int32, device=dev)
    req = handle.puct_noise_request(got, c.C)
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
    assert pc.same_bits(got["prior"].cpu().numpy(), want["prior"]) and np.array_equal(got["noised"].cpu().numpy(), want["noised"])
    assert int(got["errors_dev"][0]) == 0


# ---- 2. the search against the specification ---------------------------------------------------------------------------
def _same(a, b):
    a, b = a.cpu(), b.cpu()
    return a.shape == b.shape and a.to(torch.float64 if a.is_floating_point() else torch.int64).numpy().tobytes() == \
        b.to(torch.float64 if b.is_floating_point() else torch.int64).numpy().tobytes()


RESULT = ("action", "child_visits", "child_actions", "child_priors", "root_value", "errors") + mc.TREE_FIELDS


def _envs(cfg, P, n, seed=11):
    def make():
        e = BatchedPlacementEnv(cfg, P, queue_depth=1, run_seed=seed)
        e.generate_instances()
        e.reset()
        return e
    return [make() for _ in range(n)]


def _copied_over(evaluate, dev):
    def copied_over(paths, path_len, step_index0):
        ev = evaluate(paths.to(dev), path_len.to(dev), step_index0)
        return Evaluation(*(getattr(ev, f).cpu() for f in ("value", "terminal", "cand_count", "cand_actions", "cand_prior")))
    return copied_over


@pytest.mark.parametrize("arm", ["fresh", "kept", "leaves"])
def test_the_device_search_is_the_specification(arm):
    """A small pin configuration, P = 6, C = 4, 6 iterations.  The evaluator is a function of the paths, so the device
    search and the specification (its evaluations copied over) share one."""
    cfg, P, C, M, noise = plc.case("small_pin")[0](), 6, 4, 6, (0.3, 0.25)
    T, L = plc.max_steps(cfg), 2 if arm == "leaves" else 1
    root = BatchedPlacementEnv(cfg, P, queue_depth=2, run_seed=2, auto_reset=False)
    planner = BatchedPlacementEnv(cfg, P * L, queue_depth=2, run_seed=2, auto_reset=False)
    for e in (root, planner):
        e.generate_instances()
        e.reset()
    root.rollout_step(0)  # the roots a transition into their episodes
    dev = root.device
    zeros = torch.zeros((P * L, cfg.num_orientations * cfg.height * cfg.width), dtype=torch.float32, device=dev)
    evaluate = network_evaluator(root, planner, lambda obs: zeros, max_children=C, priors="device", leaves=L)
    copied = _copied_over(evaluate, dev)
    cpu_root = SimpleNamespace(num_envs=P, cfg=cfg, device="cpu")
    spec_noise = dict(root_noise=noise, noise_seed=root.run_seed ^ 0x6e6f6973, noise_first_root=0)
    N = 1 + 2 * M * L * C
    tree, kept = None, None
    if arm == "kept":  # a search without noise first: the roots are expanded when the noise comes
        tree = new_puct_tree(P, N, T, dev)
        _puct_iterations(root, root.puct_request(tree, 1.25, C), tree, M, T, evaluate, 100, _lib.TREE_INIT | _lib.TREE_SELECT)
        kept = search_tree(puct_search(cpu_root, M, 100, copied, c_puct=1.25, max_children=C, max_steps=T, capacity=N))
        assert bool((kept["num_children"][:, 0] > 0).any())
    got = puct_search_device(root, M, 300, evaluate, c_puct=1.25, max_children=C, max_steps=T, capacity=N, tree=tree, leaves=L, root_noise=noise)
    torch.cuda.synchronize()
    want = puct_search(cpu_root, M, 300, copied, c_puct=1.25, max_children=C, max_steps=T, capacity=N, tree=kept, leaves=L, **spec_noise)
    for f in RESULT:
        assert _same(getattr(got, f), getattr(want, f)), f
    plain = puct_search(cpu_root, M, 300, copied, c_puct=1.25, max_children=C, max_steps=T, capacity=N, tree=kept, leaves=L)
    assert not _same(plain.child_priors, want.child_priors) and int(want.errors) == 0  # the noise is there
    root.close()
    planner.close()


# ---- 3. self-play ----------------------------------------------------------------------------------------------------
def test_selfplay_with_noise_is_the_loop_of_the_specification():
    cfg, P, M, J, C, noise = named_config("c3"), 8, 8, 3, 16, (0.3, 0.25)
    T = cfg.max_num_components
    root_a, plan_a, root_b, plan_b = envs = _envs(cfg, P, 4)
    dev = root_a.device
    zeros = torch.zeros((P, cfg.num_orientations * cfg.height * cfg.width), dtype=torch.float32, device=dev)
    trees = []
    keep = lambda j, tree: trees.append({f: tree[f].clone() for f in mc.TREE_FIELDS + ("remap",)})
    got = puct_selfplay(root_a, network_evaluator(root_a, plan_a, lambda obs: zeros, max_children=C, priors="device"), J, M, step_index=500,
                        c_puct=1.25, max_children=C, mode=MOVE_PROPORTIONAL, on_move=keep, root_noise=noise)
    torch.cuda.synchronize()
    ev_b = _copied_over(network_evaluator(root_b, plan_b, lambda obs: zeros, max_children=C, priors="device"), dev)
    cpu_root = SimpleNamespace(num_envs=P, cfg=cfg, device="cpu")
    N = 1 + 2 * M * C
    tree, kept_some = None, False
    for j in range(J):
        # the draws of move j have the key step_index + j, as CHOOSE's have
        noisy = puct_search(cpu_root, M, 500 + j * M * T, ev_b, c_puct=1.25, max_children=C, max_steps=T, capacity=N, tree=tree, root_noise=noise,
                            noise_seed=root_b.run_seed ^ 0x6e6f6973, noise_first_root=0, noise_step_index=500 + j)
        ch = puct_choose(search_tree(noisy), C, MOVE_PROPORTIONAL, root_b.run_seed ^ 0x6d6f7665, 500 + j, 0)
        _, reward, done, _ = root_b.step(ch["move_action"].to(dev))
        tree, remap = puct_reroot(search_tree(noisy), ch["move_slot"], done.cpu())
        assert _same(got.actions[j], ch["move_action"]) and _same(got.child_visits[j], ch["child_visits"]), j
        assert _same(got.child_actions[j], ch["child_actions"]) and _same(got.root_value[j], ch["root_value"]), j
        assert _same(got.reward[j], reward) and _same(got.done[j], done) and _same(got.kept_visits[j], tree["visits"][:, 0]), j
        for f in mc.TREE_FIELDS:
            assert _same(trees[j][f], tree[f]), (j, f)
        assert _same(trees[j]["remap"], remap), j
        kept_some = kept_some or bool((tree["visits"][:, 0] > 0).any())
    for f in mc.TREE_FIELDS:  # the final tree
        assert _same(got.tree[f], tree[f]), f
    assert kept_some and int(got.errors) == int(tree["errors_dev"][0])
    for e in envs:
        e.close()


def test_selfplay_with_eps_0_is_selfplay_without_noise():
    cfg, P, M, J, C = named_config("c3"), 8, 8, 3, 16
    root_a, plan_a, root_b, plan_b = envs = _envs(cfg, P, 4)
    zeros = torch.zeros((P, cfg.num_orientations * cfg.height * cfg.width), dtype=torch.float32, device=root_a.device)
    play = lambda root, plan, **kw: puct_selfplay(root, network_evaluator(root, plan, lambda obs: zeros, max_children=C, priors="device"), J, M,
                                                  step_index=500, c_puct=1.25, max_children=C, mode=MOVE_PROPORTIONAL, **kw)
    a, b = play(root_a, plan_a, root_noise=(0.3, 0.0)), play(root_b, plan_b)
    torch.cuda.synchronize()
    for f in ("actions", "child_visits", "child_actions", "root_value", "reward", "done", "kept_visits", "errors"):
        assert _same(getattr(a, f), getattr(b, f)), f
    for f in mc.TREE_FIELDS + ("remap", "move_slot"):
        assert _same(a.tree[f], b.tree[f]), f
    assert bool((a.tree["noised"] == 1).any()) and bool((b.tree["noised"] == 0).all())
    for e in envs:
        e.close()
