"""pcbenv_gumbel_tree_advance_leaves on the GPU (tests/gumbel_tree_leaves_cases.py has the cases and the CPU model; the guarded
views and the comparisons are tests/test_gumbel_leaves_gpu.py's).

1. The kernel alone: every case through the C ABI into tensors that are views into sentinel-filled guarded buffers; after
   each call every tensor of the request, and every guard, equals the state of csrc/pcb_gumbel_tree_leaves.h run on the CPU, bit
   for bit -- the exchange tensors start from a sentinel, so the path rows >= path_len and the rows behind a -1 are seen to be
   untouched; a call without ABSORB leaves the tree tensors byte-identical.  The launch worked out by hand.  Damaged roots, nodes
   and counts as the model handles them; once without an error word; no roots; a side stream; and with one leaf,
   pcbenv_gumbel_tree_advance itself on the same trees (I1).
2. `gumbel_search_device(node_rule="gumbel", leaves=4)` against `gumbel_search(node_rule="gumbel", leaves=4)`, field by field,
   floats by their bits: a fresh tree, then the kept, rerooted tree.
3. `puct_selfplay(gumbel=, gumbel_node_rule="gumbel", leaves=4)` against the same game composed call by call from the
   specification; nothing is pending when a move is made.
4. `AlphaZeroTrainer` with gumbel_node_rule="gumbel" and leaves: a collect and an update."""
import ctypes
import time
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from pcbenv import _gumbel_leaves_lib, _lib, _move_lib, named_config
from pcbenv.batched_env import BatchedPlacementEnv
from pcbenv.search import (considered_visits, gumbel_search, gumbel_search_device, network_evaluator, new_gumbel_tensors, new_move_tensors, new_puct_tree,
                           puct_reroot, puct_selfplay, search_tree)

import gumbel_cases as gc
import gumbel_tree_cases as gtc
import gumbel_tree_leaves_cases as gtl
import puct_leaves_cases as plc
import puct_move_cases as mc
import test_gumbel_leaves_gpu as tl
from stream_cases import LAG_MS, lagged

pytestmark = pytest.mark.gpu

GUARD, INPUTS = tl.GUARD, tl.INPUTS
ENTRY = "pcbenv_gumbel_tree_advance_leaves"


@pytest.fixture(scope="module")
def handle():
    env = BatchedPlacementEnv(named_config("c3"), 2, queue_depth=1, run_seed=1)  # the handle gives the device only
    yield env
    env.close()


def _abi_call(handle, req, call, inputs=None, K=0, stream=None, entry=ENTRY):
    tl._abi_call(handle, req, call, inputs, K, stream, entry)


def assert_equals_the_model_after_every_call(handle, c, seq, states, errors_dev=True, state=None, table=None, levels=gtl.T):
    """c: a case of gumbel_tree_leaves_cases (P, N, C, K, L, n, Mc, rule); seq, states: the calls and the model's states after them."""
    dev = handle.device
    arrays = dict(c.state if state is None else state, considered=c.table if table is None else table, **tl._outputs(c.P, c.C))
    if errors_dev:
        arrays["errors_dev"] = np.zeros(1, np.int32)
    g = tl.Guarded(arrays, dev)
    req = handle.gumbel_leaves_request(g.t, float("nan"), c.C, c.rule[1], c.rule[2], c.L)  # c_puct is never read
    assert (req.errors_dev is not None) == errors_dev and (req.num_roots, req.capacity, req.max_children, req.max_steps) == (c.P, c.N, c.C, levels)
    assert (req.num_simulations, req.max_considered, req.num_leaves) == (c.n, c.Mc, c.L)
    for i, (call, want) in enumerate(zip(seq, states)):
        if errors_dev:
            g.t["errors_dev"].zero_()  # the model reports the bits of each call
        for name, at, value in call["pokes"]:  # what the caller has done to its tree
            g.t[name].view(-1)[at] = value
        inputs = tl.Guarded(dict(zip(INPUTS, call["evaluation"])), dev) if call["phases"] & gc.ABSORB else None
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
        if not call["phases"] & gc.SELECT and not call["phases"] & gc.ABSORB:  # BEGIN does not touch pending, CHOOSE stores nothing else
            assert np.array_equal(after["pending"], before["pending"]), i
        if not call["phases"] & gc.CHOOSE:
            for name in gc.OUT_FIELDS:
                assert np.array_equal(after[name], before[name]), (i, name)
        for name in gtl.STATE_FIELDS + gc.OUT_FIELDS:
            assert tl._same_as_model(g.inside(after, name), want[name], name), (i, name)
        if errors_dev:
            assert int(g.inside(after, "errors_dev")[0]) == want["errors"], i


def _on_device_tensors(arrays, dev):
    got = {f: torch.from_numpy(np.array(v)).to(dev).to(tl._dtype(f)) for f, v in arrays.items()}  # a copy: a model state is not writable
    got["errors_dev"] = torch.zeros(1, dtype=torch.int32, device=dev)
    return got


# ---- 1. the kernel alone --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,L", gtl.CASES)
def test_the_kernel_alone_equals_the_model_after_every_call(handle, name, L):
    c = gtl.case(name, L)
    assert_equals_the_model_after_every_call(handle, c, c.seq, c.states)


def test_a_launch_worked_out_by_hand(handle):
    h = gtl.HAND
    L, k = h["L"], len(h["priors"])
    st = gtl.one_node_state(h["priors"], L)
    P, N = st["parent"].shape
    c = SimpleNamespace(P=P, N=N, C=k, K=1, L=L, n=h["n"], Mc=h["Mc"], rule=h["rule"])
    table = considered_visits(h["Mc"], h["n"]).numpy()
    seq = [gc.call(gc.BEGIN | gc.SELECT, step_index=3)]
    states = gtl.run(st, k, 1, h["n"], h["Mc"], L, h["rule"], seq)
    assert_equals_the_model_after_every_call(handle, c, seq, states, state=st, table=table)
    # and the kernel's own tensors against the hand-derived facts, not through the model
    got = _on_device_tensors(dict(st, considered=table, **tl._outputs(P, k)), handle.device)
    req = handle.gumbel_leaves_request(got, h["rule"][0], k, h["rule"][1], h["rule"][2], L)
    _abi_call(handle, req, seq[0])
    torch.cuda.synchronize()
    gtl.check_hand(dict({f: got[f].cpu().numpy() for f in gtl.STATE_FIELDS}, errors=int(got["errors_dev"][0])))


@pytest.mark.parametrize("name", list(gtl.DAMAGE))
def test_a_damaged_tree_is_handled_as_the_model_handles_it(handle, name):
    """Only a root 0 < p < P - 1 is damaged -- were a check missing, the stray access would fall into a neighbouring root's
    rows, or into the guards, which are compared -- and only by values the model has run under the sanitizers.  pending is
    data: whatever it holds, Msum == -1 included, it addresses nothing."""
    c, at, seq, states, p, healthy = gtl.damaged(name)
    assert 0 < p < c.P - 1
    assert_equals_the_model_after_every_call(handle, c, seq, states)


def test_without_an_error_word(handle):
    c, at, seq, states, p, healthy = gtl.damaged("below_first_child_0")
    assert states[-1]["errors"] & gc.ERR_TREE
    assert_equals_the_model_after_every_call(handle, c, seq, states, errors_dev=False)


def test_no_roots_is_a_no_op(handle):
    R = _gumbel_leaves_lib.PcbenvGumbelLeavesRequest
    req = R(struct_size=ctypes.sizeof(R), phases=gc.BEGIN | gc.ABSORB | gc.SELECT, num_roots=0, capacity=3, max_children=2, max_steps=2, num_candidates=1,
            num_simulations=4, max_considered=2, c_puct=1.0, c_visit=50.0, c_scale=1.0, num_leaves=4)
    for n, _ in R._fields_:
        if getattr(R, n).offset >= R.num_nodes.offset and n not in ("errors_dev", "stream"):
            setattr(req, n, handle.reward.data_ptr())
    assert getattr(handle._L, ENTRY)(handle._h, ctypes.byref(req)) == _lib.PCBENV_OK
    tree = new_puct_tree(0, 3, 2, handle.device, 4)
    tree.update(new_gumbel_tensors(0, 2, 2, 4, handle.device))
    handle.gumbel_tree_advance_leaves(handle.gumbel_leaves_request(tree, 1.0, 2, leaves=4), gc.BEGIN | gc.SELECT)  # the binding's empty tensors have no address
    torch.cuda.synchronize()


def test_side_stream(handle):
    """The launch enqueued on a non-blocking side stream behind a delay: the call returns before the stream reaches it and
    gives the model's result."""
    c = gtl.case("G16_C16_P67", 4)
    i = 1  # SELECT alone on the hand-built trees
    assert c.seq[i]["phases"] == gc.SELECT
    got = _on_device_tensors(dict({f: v for f, v in c.states[0].items() if f != "errors"}, considered=c.table), handle.device)
    req = handle.gumbel_leaves_request(got, c.rule[0], c.C, c.rule[1], c.rule[2], c.L)
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
    for f in gtl.STATE_FIELDS:
        assert tl._same_as_model(got[f].cpu().numpy(), c.states[i][f], f), f
    assert int(got["errors_dev"][0]) == c.states[i]["errors"]


@pytest.mark.parametrize("name", list(gtc.CASES))
def test_I1_one_leaf_is_pcbenv_gumbel_tree_advance_on_the_same_trees(handle, name):
    """L = 1, pending zero: after every call every tensor pcbenv_gumbel_tree_advance writes has the same bits in both kernels' runs."""
    c = gtl.case(name, 1)
    dev = handle.device
    start = dict(c.state, considered=c.table, **tl._outputs(c.P, c.C))
    one, old = _on_device_tensors(start, dev), _on_device_tensors(start, dev)
    req_one = handle.gumbel_leaves_request(one, c.rule[0], c.C, c.rule[1], c.rule[2], 1)
    req_old = handle.gumbel_request(old, c.rule[0], c.C, c.rule[1], c.rule[2])
    for i, call in enumerate(c.seq):
        inputs = tl.Guarded(dict(zip(INPUTS, call["evaluation"])), dev) if call["phases"] & gc.ABSORB else None
        _abi_call(handle, req_one, call, inputs, c.K)
        _abi_call(handle, req_old, call, inputs, c.K, entry="pcbenv_gumbel_tree_advance")
        for f in gc.STATE_FIELDS + gc.OUT_FIELDS + ("errors_dev",):
            assert one[f].cpu().numpy().tobytes() == old[f].cpu().numpy().tobytes(), (i, f)
        if not call["phases"] & gc.SELECT:
            assert not bool(one["pending"].any()), i


# ---- 2. the search against the specification ---------------------------------------------------------------------------
def test_the_device_search_is_the_specification_on_a_fresh_and_on_a_kept_tree():
    """One handle of the c3 configuration, 64 roots, C = 16, n = 8 simulations over Mc = 4 candidates, L = 4, scripted
    evaluations (a function of root and path): the search of a fresh tree, pcbenv_puct_move(REROOT) on the move_slot CHOOSE
    wrote, and the search of the kept tree."""
    P, n, Mc, C, T, K, L = 64, 8, 4, 16, 5, 16, 4
    root = BatchedPlacementEnv(named_config("c3"), P, queue_depth=1, run_seed=3, first_env_index=2)
    E = -(-n // L) + 1
    dev, N = root.device, 1 + 2 * E * L * C
    cpu_root = SimpleNamespace(num_envs=P, cfg=None, device="cpu")
    kw = dict(max_considered=Mc, c_visit=50.0, c_scale=1.0, c_puct=1.25, max_children=C, max_steps=T, leaves=L, node_rule="gumbel")
    spec = dict(kw, seed=root.run_seed ^ 0x67756d62, first_root=2)
    first, second = plc.leaves_evaluator(P, T, K, L, 31), plc.leaves_evaluator(P, T, K, L, 37)
    got = gumbel_search_device(root, n, 100, tl._on_device(first, dev), capacity=N, **kw)  # a tree of its own
    want = gumbel_search(cpu_root, n, 100, first, capacity=N, **spec)
    tl._assert_same_search(got, want)
    assert bool((want.sim_index == n).any()) and bool((want.move_slot >= 1).any()) and int(want.search.errors) == 0
    plain = gumbel_search(cpu_root, n, 100, first, capacity=N, **dict(spec, node_rule="puct"))
    assert not tl._same(plain.search.visits, want.search.visits)  # and it is another search than the root rule's with leaves
    # the same in a tree the caller keeps, then the move, then the next search in what is left
    tree = new_puct_tree(P, N, T, dev, L)
    tree.update(new_move_tensors(P, N, C, dev))
    tree.update(new_gumbel_tensors(P, C, Mc, n, dev))
    root.puct_advance_leaves(root.puct_leaves_request(tree, 1.25, C, L), _lib.TREE_INIT)
    again = gumbel_search_device(root, n, 100, tl._on_device(first, dev), tree=tree, **kw)
    tl._assert_same_search(again, want)
    assert not bool(tree["pending"].any())  # I2
    root.puct_move(root.puct_move_request(tree, C), _move_lib.MOVE_REROOT)  # reads move_slot as CHOOSE wrote it
    kept, remap = puct_reroot(search_tree(want.search), want.move_slot)
    assert tl._same(tree["remap"], remap) and bool((kept["num_children"][:, 0] > 0).any())
    got2 = gumbel_search_device(root, n, 200, tl._on_device(second, dev), tree=tree, gumbel_step_index=101, **kw)
    want2 = gumbel_search(cpu_root, n, 200, second, tree=kept, gumbel_step_index=101, **spec)
    tl._assert_same_search(got2, want2)
    assert not tl._same(got2.child_policy, got.child_policy) and not bool(tree["pending"].any())
    assert int(want2.search.depth.max()) >= 3  # the node rule ran below the root
    root.close()


# ---- 3. self-play ----------------------------------------------------------------------------------------------------
def test_selfplay_with_the_full_rule_and_leaves_is_the_loop_of_the_specification():
    cfg, P, n, J, C, L, rule = named_config("c3"), 8, 8, 3, 16, 4, (4, 50.0, 1.0)
    T = cfg.max_num_components
    root_a, plan_a, root_b, plan_b = envs = tl._envs(cfg, (P, P * L, P, P * L))
    dev = root_a.device
    zeros = torch.zeros((P * L, cfg.num_orientations * cfg.height * cfg.width), dtype=torch.float32, device=dev)
    trees, pending = [], []

    def keep(j, tree):  # behind REROOT, which neither reads nor writes pending: what it found
        trees.append({f: tree[f].clone() for f in mc.TREE_FIELDS + ("remap", "move_slot")})
        pending.append(tree["pending"].ne(0).any())
    got = puct_selfplay(root_a, network_evaluator(root_a, plan_a, lambda obs: zeros, max_children=C, priors="device", leaves=L), J, n, step_index=500,
                        c_puct=1.25, max_children=C, on_move=keep, gumbel=rule, leaves=L, gumbel_node_rule="gumbel")
    torch.cuda.synchronize()
    assert len(pending) == J and not any(bool(x) for x in pending)  # pending all zero before every REROOT
    ev_b = tl._copied_over(network_evaluator(root_b, plan_b, lambda obs: zeros, max_children=C, priors="device", leaves=L), dev)
    cpu_root = SimpleNamespace(num_envs=P, cfg=cfg, device="cpu")
    E = -(-n // L) + 1
    N = 1 + 2 * E * L * C
    assert tuple(got.tree["pending"].shape) == (P, N)
    tree, kept_some = None, False
    for j in range(J):
        gs = gumbel_search(cpu_root, n, 500 + j * E * T, ev_b, max_considered=rule[0], c_visit=rule[1], c_scale=rule[2], c_puct=1.25, max_children=C,
                           max_steps=T, capacity=N, tree=tree, seed=root_b.run_seed ^ 0x67756d62, first_root=0, gumbel_step_index=500 + j, leaves=L,
                           node_rule="gumbel")
        _, reward, done, _ = root_b.step(gs.move_action.to(dev))
        tree, remap = puct_reroot(search_tree(gs.search), gs.move_slot, done.cpu())
        assert tl._same(got.actions[j], gs.move_action) and tl._same(got.child_visits[j], gs.child_weights), j
        assert tl._same(got.child_actions[j], gs.child_actions) and tl._same(got.root_value[j], gs.root_value), j
        assert tl._same(got.reward[j], reward) and tl._same(got.done[j], done) and tl._same(got.kept_visits[j], tree["visits"][:, 0]), j
        assert tl._same(trees[j]["move_slot"], gs.move_slot), j  # what pcbenv_puct_move(REROOT) read
        for f in mc.TREE_FIELDS:
            assert tl._same(trees[j][f], tree[f]), (j, f)
        assert tl._same(trees[j]["remap"], remap), j
        kept_some = kept_some or bool((tree["visits"][:, 0] > 0).any())
        assert bool((gs.sim_index > 0).any()) and bool((gs.search.visits[:, 0] > E).any())  # more than one leaf per launch below the root
    for f in mc.TREE_FIELDS:  # the final tree
        assert tl._same(got.tree[f], tree[f]), f
    assert kept_some and int(got.errors) == int(tree["errors_dev"][0]) == 0
    for e in envs:
        e.close()


# ---- 4. the trainer --------------------------------------------------------------------------------------------------
def test_the_trainer_collects_and_updates_with_the_full_rule_and_leaves():
    """One collect and one update with gumbel_considered = 4, gumbel_node_rule = "gumbel" and leaves = 2, on the 10 x 10 spatial
    configuration of tests/test_gumbel_gpu.py."""
    from pcbenv import EnvConfig
    from pcbenv.alphazero import AlphaZeroConfig, AlphaZeroTrainer
    from pcbenv.batched_env import default_max_steps
    from pcbenv.policy import SpatialPolicy
    torch.manual_seed(0)
    P, MOVES, n, C, L = 16, 2, 4, 8, 2
    cfg = EnvConfig.spatial(10, 10, 9, 9, 2, 2, 2, 2, 5, 5, 3, 3, 6, 6, "centroid", 2, 0.75)
    root = BatchedPlacementEnv(cfg, P, queue_depth=4, auto_reset=True)
    planner = BatchedPlacementEnv(cfg, P * L, queue_depth=1)
    for e in (root, planner):
        e.generate_instances()
        e.reset()
    trainer = AlphaZeroTrainer(root, planner, SpatialPolicy(cfg).to(root.device),
                               AlphaZeroConfig(moves=MOVES, iterations=n, max_children=C, leaves=L, device_loss=True, gumbel_considered=4,
                                               gumbel_node_rule="gumbel", entropy_coef=0.01))
    for t in range(3):
        root.step(root.sample_actions(t))
    first = trainer.step_index
    batch = trainer.collect()
    torch.cuda.synchronize()
    assert trainer.step_index - first == MOVES * (-(-n // L) + 1) * default_max_steps(cfg)  # ceil(n / L) + 1 evaluations per move
    assert int(batch["errors"]) == 0 and batch["child_visits"].shape == (MOVES, P, C) and batch["child_visits"].dtype == torch.int32
    weights = batch["child_visits"].reshape(MOVES * P, C)
    total = weights.to(torch.int64).sum(dim=1)
    assert bool(((total - 2 ** 24).abs() <= C // 2 + 1).all()) and bool((weights >= 0).all())
    out = trainer.update(batch)
    assert set(out) == {"loss", "policy", "value", "entropy"} and all(np.isfinite(v) for v in out.values()), out
    for e in (root, planner):
        e.close()
