"""pcbenv_puct_move on the GPU (tests/puct_move_cases.py has the cases and the CPU model).

1. The kernel alone: every case three ways -- CHOOSE | REROOT in one launch, CHOOSE and REROOT in two, REROOT with a move the
   caller wrote -- through `BatchedPlacementEnv.puct_move` into tensors that are views into sentinel-filled guarded
   buffers; after EVERY launch every tensor of the request equals the state of csrc/pcb_puct_move.h run on the CPU, bit for
   bit, guards and inputs included, and a phase not asked for writes nothing.  Once without `reset`, once without an error word.
2. Trees the caller has damaged (puct_move_cases.damaged): the kernel does what the model does in every tensor.  Every one of
   them has run clean through the model under AddressSanitizer and UBSan (tests/test_puct_move_model.py).
3. The whole stack at c3: `puct_selfplay` against the same loop written with `puct_search(tree=)`, `puct_choose`,
   `puct_reroot` and `step`.
4. A launch on a side stream behind a delay returns before the stream reaches it and gives the default stream's result."""
import time
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from pcbenv import _lib, _move_lib, named_config
from pcbenv.batched_env import BatchedPlacementEnv
from pcbenv.search import (MOVE_GREEDY, MOVE_PROPORTIONAL, Evaluation, network_evaluator, puct_choose, puct_reroot, puct_search, puct_selfplay,
                           search_tree)

import puct_cases as pc
import puct_move_cases as mc
from stream_cases import LAG_MS, lagged

pytestmark = pytest.mark.gpu

GUARD, SENTINEL = 256, 0xA5
DTYPES = dict(prior=torch.float64, value_sum=torch.float64, value_max=torch.float64, reward_lo=torch.float64, reward_hi=torch.float64,
              terminal=torch.uint8, root_value=torch.float64, reset=torch.uint8)
INPUTS = ("reset",)


class Guarded:
    """Every tensor of a request as a view GUARD bytes into a sentinel-filled buffer of its own, GUARD bytes behind it.  The
    tree is the case's; the tensors the kernel writes start out as the model's do (FILL, root_value -7.0)."""

    def __init__(self, tree, C, device):
        P, N = tree["parent"].shape
        shp = dict(mc.shapes(P, N, C), reset=(P,), errors_dev=(1,))
        self.back, self.t, self.meta = {}, {}, {}
        for name, shape in shp.items():
            dtype = DTYPES.get(name, torch.int32)
            n = int(np.prod(shape)) * torch.empty((), dtype=dtype).element_size()
            buf = torch.full((GUARD + n + GUARD,), SENTINEL, dtype=torch.uint8, device=device)
            self.back[name] = buf
            self.t[name] = buf[GUARD:GUARD + n].view(dtype).view(shape)
            self.meta[name] = (self.t[name].cpu().numpy().dtype, tuple(shape))
            if name in tree:
                self.t[name].copy_(torch.from_numpy(np.ascontiguousarray(tree[name])).to(dtype))
            elif dtype == torch.int32:
                self.t[name].fill_(mc.FILL)
        self.t["root_value"].fill_(-7.0)
        self.t["errors_dev"].zero_()
        self.t["reset"].zero_()

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


def move_and_compare(handle, req, g, i, call, want, errors_dev=True, first_root=0):
    """Call i through puct_move into the guarded tensors of g; want: the model's state after it.  -> (the snapshot the call
    started from, the one it left)."""
    for name, at, value in call.get("pokes", ()):  # the damage a caller does before the call
        g.t[name].view(-1)[at] = value
    if call.get("move_slot") is not None:
        g.t["move_slot"].copy_(torch.from_numpy(call["move_slot"]))
    if call["reset"] is not None:
        g.t["reset"].copy_(torch.from_numpy(call["reset"]))
    g.t["errors_dev"].zero_()  # the model reports the bits of each call
    before = g.snapshot()
    handle.puct_move(req, call["phases"], mode=call["mode"], seed=call["seed"], step_index=call["step_index"],
                     reset=g.t["reset"] if call["reset"] is not None else None)
    assert req.first_root == handle.first_env_index == first_root
    after = g.snapshot()
    for name in after:  # the guards, and what the call only reads
        assert np.array_equal(after[name][:GUARD], before[name][:GUARD]) and np.array_equal(after[name][-GUARD:], before[name][-GUARD:]), (i, name)
        if name in INPUTS:
            assert np.array_equal(after[name], before[name]), (i, name)
    for f in mc.STATE_FIELDS:
        got = g.inside(after, f)
        if f in mc.FLOATS:
            assert pc.same_bits(got, want[f]), (i, f)
        else:
            assert np.array_equal(got.astype(np.int64), want[f]), (i, f)
    assert int(g.inside(after, "errors_dev")[0]) == (want["errors"] if errors_dev else 0), i
    untouched = ()
    if call["phases"] == mc.CHOOSE:
        untouched = mc.TREE_FIELDS + ("remap",)
    elif call["phases"] == mc.REROOT:
        untouched = ("move_slot", "move_action", "child_visits", "child_actions", "root_value")
    for f in untouched:  # a phase that was not asked for wrote nothing
        assert np.array_equal(after[f], before[f]), (i, f)
    return before, after


def assert_equals_the_model_after_every_call(handle, tree, C, seq, states, errors_dev=True):
    """seq call by call through puct_move into guarded tensors; states: the model's state after each call."""
    g = Guarded(tree, C, handle.device)
    req = handle.puct_move_request(g.t if errors_dev else {n: t for n, t in g.t.items() if n != "errors_dev"}, C)
    assert (req.errors_dev is not None) == errors_dev and req.max_children == C and req.capacity == tree["parent"].shape[1]
    for i, (call, want) in enumerate(zip(seq, states)):
        move_and_compare(handle, req, g, i, call, want, errors_dev)


def _first_root_0(seq):
    """The binding passes the handle's first_env_index (0 here) as first_root: the model's calls are given the same."""
    return [dict(c, first_root=0) for c in seq]


@pytest.mark.parametrize("way", mc.WAYS)
@pytest.mark.parametrize("name", mc.ALL_SHAPES)
def test_the_kernel_alone_equals_the_model_after_every_call(handle, name, way):
    mc.check_cases()
    if name in mc.CONSTRUCTED:  # with the checks, made on the CPU, that the shape reaches the spans and chunks it is there for
        mc.check_constructed()
    c = mc.case(name)
    seq = _first_root_0(mc.ways(c)[way])
    assert_equals_the_model_after_every_call(handle, c.tree, c.C, seq, mc.run(c.tree, c.C, seq))


@pytest.mark.parametrize("way", mc.WAYS)
def test_without_reset_and_without_an_error_word(handle, way):
    c = mc.case("G16_C16_P35")
    seq = _first_root_0(mc.ways(c, reset=False)[way])
    states = mc.run(c.tree, c.C, seq)
    asked = [p for p in range(c.P) if c.kinds[p] == "reset" and c.move_slot[p] > 0]
    assert asked and all(states[-1]["visits"][p, 0] > 0 for p in asked)  # without the tensor no root is reset
    assert_equals_the_model_after_every_call(handle, c.tree, c.C, seq, states)
    assert_equals_the_model_after_every_call(handle, c.tree, c.C, seq, states, errors_dev=False)


@pytest.mark.parametrize("name", mc.DAMAGE)
def test_a_damaged_tree_is_handled_as_the_model_handles_it(handle, name):
    """Bounds the kernel must honour: only a root 0 < p < P - 1 is damaged -- were a check missing, the stray access would
    fall into a neighbouring root's rows, or into the guards, which are compared -- and only by values next to the valid
    range.  The model has run every one of these under the sanitizers."""
    d = mc.damaged(name)
    c = d.case
    assert 0 < d.p < c.P - 1 and d.states[0]["errors"] == mc.ERR_TREE
    allowed = dict(num_nodes=(0, c.N + 1), parent=(d.n - 1, c.N), num_children=(-1, c.C + 5), first_child=(0, 1, d.n))
    for f, at, value in d.pokes:
        assert value in allowed[f], (f, value)
    assert int(d.move_slot[d.p]) in (d.m, c.N, -2)
    seq = _first_root_0(d.seq)
    assert_equals_the_model_after_every_call(handle, c.tree, c.C, seq, d.states)
    assert_equals_the_model_after_every_call(handle, c.tree, c.C, seq, d.states, errors_dev=False)


@pytest.mark.parametrize("shape, name", mc.DEEP_CASES)
def test_a_tree_damaged_in_its_third_span_is_handled_as_the_model_handles_it(handle, shape, name):
    """The same bounds, where the early exit follows two spans that have stored their ranks: a slot of the third span of a
    long chain and of a C = 64 tree, in a root between two others, damaged by values next to the valid range."""
    d = mc.damaged_deep(shape, name)
    c = d.case
    assert 0 < d.p < c.P - 1 and d.states[0]["errors"] == mc.ERR_TREE and (d.states[0]["remap"][d.p] == -1).all()
    allowed = dict(parent=(d.s, c.N), first_child=(mc.DEEP[shape][4], d.n))
    for f, at, value in d.pokes:
        assert value in allowed[f], (f, value)
    seq = _first_root_0(d.seq)
    assert_equals_the_model_after_every_call(handle, c.tree, c.C, seq, d.states)
    assert_equals_the_model_after_every_call(handle, c.tree, c.C, seq, d.states, errors_dev=False)


def test_no_roots_is_a_no_op(handle):
    R = _move_lib.PcbenvPuctMoveRequest
    req = R(struct_size=224, phases=3, num_roots=0, capacity=3, max_children=2)
    for n, _ in R._fields_[10:-3]:
        setattr(req, n, handle.reward.data_ptr())
    assert handle._L.pcbenv_puct_move(handle._h, req) == _lib.PCBENV_OK
    torch.cuda.synchronize()


# ---- 3. the whole stack ---------------------------------------------------------------------------------------------
def _same(a, b):
    a, b = a.cpu(), b.cpu()
    return a.shape == b.shape and a.to(torch.float64 if a.is_floating_point() else torch.int64).numpy().tobytes() == \
        b.to(torch.float64 if b.is_floating_point() else torch.int64).numpy().tobytes()


@pytest.mark.parametrize("mode", [MOVE_GREEDY, MOVE_PROPORTIONAL])
def test_selfplay_is_the_loop_of_the_specification(mode):
    cfg, P, M, J, C = named_config("c3"), 8, 8, 3, 16
    T = cfg.max_num_components

    def make():
        e = BatchedPlacementEnv(cfg, P, queue_depth=1, run_seed=11)
        e.generate_instances()
        e.reset()
        return e
    envs = [make() for _ in range(4)]
    (root_a, plan_a), (root_b, plan_b) = envs[:2], envs[2:]
    dev = root_a.device
    zeros = torch.zeros((P, cfg.num_orientations * cfg.height * cfg.width), dtype=torch.float32, device=dev)
    trees = []
    keep = lambda j, tree: trees.append({f: tree[f].clone() for f in mc.TREE_FIELDS + ("remap",)})
    got = puct_selfplay(root_a, network_evaluator(root_a, plan_a, lambda obs: zeros, max_children=C, priors="device"), J, M, step_index=500,
                        c_puct=1.25, max_children=C, mode=mode, on_move=keep)
    torch.cuda.synchronize()
    assert len(trees) == J
    # the same loop, the tree in tensor code on the CPU, the evaluations copied over
    evaluate_b = network_evaluator(root_b, plan_b, lambda obs: zeros, max_children=C, priors="device")

    def copied_over(paths, path_len, step_index0):
        ev = evaluate_b(paths.to(dev), path_len.to(dev), step_index0)
        return Evaluation(*(getattr(ev, f).cpu() for f in ("value", "terminal", "cand_count", "cand_actions", "cand_prior")))
    cpu_root = SimpleNamespace(num_envs=P, cfg=cfg, device="cpu")
    N = 1 + 2 * M * C
    tree, kept_some = None, False
    for j in range(J):
        ps = puct_search(cpu_root, M, 500 + j * M * T, copied_over, c_puct=1.25, max_children=C, max_steps=T, capacity=N, tree=tree)
        ch = puct_choose(search_tree(ps), C, mode, root_b.run_seed ^ 0x6d6f7665, 500 + j, 0)
        _, reward, done, _ = root_b.step(ch["move_action"].to(dev))
        tree, remap = puct_reroot(search_tree(ps), ch["move_slot"], done.cpu())
        assert _same(got.actions[j], ch["move_action"]) and _same(got.child_visits[j], ch["child_visits"]), j
        assert _same(got.child_actions[j], ch["child_actions"]) and _same(got.root_value[j], ch["root_value"]), j
        assert _same(got.reward[j], reward) and _same(got.done[j], done) and _same(got.kept_visits[j], tree["visits"][:, 0]), j
        for f in mc.TREE_FIELDS:
            assert _same(trees[j][f], tree[f]), (j, f)
        assert _same(trees[j]["remap"], remap), j
        kept_some = kept_some or bool((tree["visits"][:, 0] > 0).any())
    assert kept_some and int(got.errors) == int(tree["errors_dev"][0])
    assert int(got.child_visits[0].sum(dim=1).min()) == M - 1  # every iteration but the first went through a child of the root
    for e in envs:
        e.close()


# ---- 4. side stream -------------------------------------------------------------------------------------------------
def test_side_stream(handle):
    """CHOOSE | REROOT enqueued on a non-blocking side stream behind a delay: the call returns before the stream reaches it
    and gives the default stream's result."""
    c = mc.case("G4_C3_P130")
    dev = handle.device

    def fresh():
        t = {f: torch.from_numpy(np.ascontiguousarray(c.tree[f])).to(dev) for f in mc.TREE_FIELDS}
        for f in ("num_nodes", "parent", "depth", "visits", "num_children", "first_child"):
            t[f] = t[f].to(torch.int32)
        t["terminal"] = t["terminal"].to(torch.uint8)
        P, N = t["parent"].shape
        i32 = dict(dtype=torch.int32, device=dev)
        t.update(move_slot=torch.zeros(P, **i32), move_action=torch.zeros((P, 3), **i32), child_visits=torch.zeros((P, c.C), **i32),
                 child_actions=torch.zeros((P, c.C, 3), **i32), root_value=torch.zeros(P, dtype=torch.float64, device=dev),
                 remap=torch.zeros((P, N), **i32), errors_dev=torch.zeros(1, **i32))
        return t
    reset = torch.from_numpy(c.reset).to(dev)
    want = fresh()
    handle.puct_move(handle.puct_move_request(want, c.C), 3, mode=MOVE_PROPORTIONAL, seed=mc.SEED, step_index=mc.STEP, reset=reset)
    torch.cuda.synchronize()
    model = mc.run(c.tree, c.C, [mc.call(3, mc.PROPORTIONAL, reset=c.reset, first_root=0)])[0]
    assert np.array_equal(want["remap"].cpu().numpy().astype(np.int64), model["remap"]) and int(want["errors_dev"][0]) == 0
    side = torch.cuda.Stream()
    got = fresh()
    req = handle.puct_move_request(got, c.C)
    torch.cuda.synchronize()
    with lagged(side) as before:
        before()
        reached = torch.cuda.Event()
        reached.record(side)
        t0 = time.perf_counter()
        handle.puct_move(req, 3, mode=MOVE_PROPORTIONAL, seed=mc.SEED, step_index=mc.STEP, reset=reset)
        dt = 1e3 * (time.perf_counter() - t0)
        ev = torch.cuda.Event()
        ev.record(side)
        assert not reached.query(), f"the call returned only after the stream had passed a {LAG_MS} ms delay ({dt:.2f} ms on the host)"
        assert not ev.query()
        side.synchronize()
    for f in want:
        assert want[f].cpu().numpy().tobytes() == got[f].cpu().numpy().tobytes(), f
