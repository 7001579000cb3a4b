"""pcbenv_frontier_sample on the GPU (tests/frontier_sample_cases.py has the cases and the CPU model).

1. The kernel alone: the call sequences of the table fed call by call through `BatchedPlacementEnv.frontier_sample`, no
   evaluation launch; after EVERY call every tensor of the request equals the state of csrc/pcb_frontier_sample.h replayed
   on the CPU, floats by their bits.  The shapes are those at which the mapping -- one wavefront per root, row j * 64 + lane
   in register j, set slot j in lane j, a parent's K children in consecutive lanes -- can go wrong: F = 1; F = 15, ragged,
   children straddling nothing but unaligned; F = 64 with the set in four lanes; F = 65; K = 40, whose parents straddle
   two register rounds; F = 1024 as 64 x 16, every lane a rank and a set slot, and as 16 x 64, a parent a full wave; 1 x 64;
   T = 1; P = 1, 2, 5, 6 and 23 roots, whose last workgroup is partly empty; the ties, NaNs, infinities and damaged
   lengths of the hand-made calls.
2. Every tensor is a view into a sentinel-filled buffer: the guards, the path rows behind a length, the slots that are no
   row or no entry and the inputs keep their bytes.
3. Without an error word; no roots; a side stream; one launch worked out by hand.
4. The whole stack on real roots: `frontier_sample_search_device` next to `network_evaluator(priors="device", leaves=W * K)`
   against `frontier_sample_search`, and every set entry's path replayed with `step`.
What the cases reach is asserted on the CPU (tests/test_frontier_sample_model.py)."""
import time
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from pcbenv import _frontier_sample_lib, _lib
from pcbenv.batched_env import BatchedPlacementEnv
from pcbenv import named_config
from pcbenv.search import Evaluation, frontier_sample_search, frontier_sample_search_device, network_evaluator

import frontier_sample_cases as sc
import playout_cases as plc
import puct_cases as pc
from stream_cases import LAG_MS, lagged
from test_puct_advance_gpu import DTYPES, GUARD, Guarded

pytestmark = pytest.mark.gpu


class GuardedSample(Guarded):
    """test_puct_advance_gpu.Guarded with the tensors of a frontier sample request: the int32 ones start out as the model's
    do (frontier_sample_cases.FILL), the float64 ones of the state as FILL_F."""

    def __init__(self, P, W, K, T, device, errors=True):
        R = P * W * K
        shp = dict(sc.shapes(P, W, K, T), value=(R,), leaf_terminal=(R,), cand_count=(R,), cand_actions=(R, K, 3), cand_prior=(R, K), errors_dev=(1,))
        self.device, self.back, self.t, self.meta = device, {}, {}, {}
        for name, shape in shp.items():
            self.add(name, shape, torch.float64 if name in sc.FLOATS else DTYPES.get(name, torch.int32))
            if name in sc.FLOATS:
                self.t[name].fill_(sc.FILL_F)
        self.t["errors_dev"].zero_()
        if not errors:
            self.word = self.t.pop("errors_dev")


@pytest.fixture(scope="module")
def handle():
    env = BatchedPlacementEnv(named_config("c3"), 2, queue_depth=1, run_seed=1)  # the handle gives the device only
    yield env
    env.close()


def advance_and_compare(handle, req, g, i, call, want, errors=True):
    """Call i through frontier_sample into the guarded tensors of g; want: the model's state after it."""
    ev = None
    if call["load"] is not None:  # a state of the caller's making
        sc.apply_load(g.t, call["load"], call["swap"])
    if call["evaluation"] is not None:
        for name, a in zip(pc.INPUTS, call["evaluation"]):
            g.t[name].copy_(torch.from_numpy(np.ascontiguousarray(a)))
        ev = Evaluation(g.t["value"], g.t["leaf_terminal"], g.t["cand_count"], g.t["cand_actions"], g.t["cand_prior"])
    before = g.snapshot()
    handle.frontier_sample(req, call["phases"], call["step_index"], ev, swap=bool(call["swap"]))
    after = g.snapshot()
    s = 1 if call["swap"] else 0
    for name in after:  # the guards, and what the call only reads: the inputs and the in set
        assert np.array_equal(after[name][:GUARD], before[name][:GUARD]) and np.array_equal(after[name][-GUARD:], before[name][-GUARD:]), (i, name)
        if name in pc.INPUTS or name in tuple(f"{n}_{s}" for n in sc.ROW_SET):
            assert np.array_equal(after[name], before[name]), (i, name)
    for f in sc.STATE_FIELDS:  # every tensor against the model, what the call leaves alone included
        got = g.inside(after, f)
        if f in sc.FLOATS:
            assert sc.same_bits(got, want[f]), (i, f)
        else:
            assert np.array_equal(got.astype(np.int64), want[f]), (i, f)
    if errors:
        assert int(g.inside(after, "errors_dev")[0]) == want["errors"], i
    if call["phases"] == sc.INIT:  # INIT writes no path and of the set its lengths alone
        for f in ("paths_0", "paths_1", "best_path", "set_path", "set_gumbel", "set_logp", "set_value"):
            assert np.array_equal(after[f], before[f]), (i, f)


def assert_equals_the_model_after_every_call(handle, case, errors=True):
    g = GuardedSample(case.P, case.W, case.K, case.T, handle.device, errors)
    req = handle.frontier_sample_request(g.t, case.W, case.K, case.seed, case.first_root)
    assert (req.num_roots, req.width, req.num_candidates, req.max_steps, req.seed, req.first_root) == (case.P, case.W, case.K, case.T, case.seed, case.first_root)
    assert bool(req.errors_dev) == errors
    for i, (call, want) in enumerate(zip(case.seq, case.states)):
        advance_and_compare(handle, req, g, i, call, want, errors)
    return g


@pytest.mark.parametrize("name", list(sc.CASES))
def test_the_kernel_alone_equals_the_model_after_every_call(handle, name):
    case = sc.case(name)
    assert any((s["live"] > 0).any() for s in case.states[1:]) and any((s["set_len"] >= 0).any() for s in case.states)
    assert_equals_the_model_after_every_call(handle, case)


def test_without_an_error_word(handle):
    """errors_dev null: the same states, the damaged lengths included, and the word that is not the request's stays zero."""
    case = sc.case("hand")
    assert case.states[-1]["errors"] == sc.ERR_ROW | sc.ERR_SET
    g = assert_equals_the_model_after_every_call(handle, case, errors=False)
    assert int(g.word[0]) == 0


def test_no_roots_is_a_no_op(handle):
    R = _frontier_sample_lib.PcbenvFrontierSampleRequest
    req = R(struct_size=248, phases=sc.ADVANCE, num_roots=0, width=3, num_candidates=2, max_steps=2, seed=1)
    for n, _ in R._fields_[10:-2]:
        setattr(req, n, handle.reward.data_ptr())
    assert handle._L.pcbenv_frontier_sample(handle._h, req) == _lib.PCBENV_OK
    torch.cuda.synchronize()
    ft = sc.search.new_frontier_sample_tensors(0, 3, 2, 2, handle.device)
    handle.frontier_sample(handle.frontier_sample_request(ft, 3, 2, 1), sc.INIT, 0)
    torch.cuda.synchronize()


def test_side_stream(handle):
    """The whole search is enqueued on a non-blocking side stream behind a delay: it returns before the stream reaches it
    and gives the result of the default-stream run.  The evaluations are the recorded ones, uploaded beforehand."""
    case = sc.case("W4_K16")
    dev = handle.device
    fixed = [Evaluation(*(torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in c["evaluation"])) for c in case.seq[1:]]
    root = SimpleNamespace(num_envs=case.P, device=dev, cfg=None, frontier_sample_request=handle.frontier_sample_request, frontier_sample=handle.frontier_sample)

    def search():
        it = iter(fixed)
        return frontier_sample_search_device(root, lambda paths, path_len, s: next(it), case.W, case.K, sc.STEP_INDEX, case.seed, case.first_root, max_steps=case.T)
    want = search()
    torch.cuda.synchronize()
    last = case.states[-1]
    assert sc.same_bits(want.set_gumbel.cpu().numpy(), last["set_gumbel"]) and np.array_equal(want.set_len.cpu().numpy(), last["set_len"])
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


def test_one_launch_worked_out_by_hand(handle):
    """P = 1, W = 2, K = 2 (F = 4), T = 3.  The state read:
      set slot 0  free                       set slot 1  a placement of 2 steps, G -1.5
      row 0  path (0,1,1)  G -0.25  2 candidates (0,2,0) (0,2,1), priors 0.5 and 0.0, cum_logp -1.0
      row 1  path (0,1,2)  G -1.0   final, value 0.75, cum_logp -2.0
      row 2  path (0,1,3)  G -1.25  1 candidate
      row 3  path (0,3,3)  G -3.0   final, value 0.9
    By value row 3 is the best final: best_value 0.9.  By G the two winners are row 0 and row 1: the entry of slot 1 is
    dropped (its length becomes -1, the rest stays), row 1 enters slot 0, the lowest slot without a survivor, with its G, its
    cum_logp, its value and its path, and row 0 is the one parent.  Its child 0 is the only one with a logarithm, so it has
    the largest G_c and takes the parent's G, -0.25, exactly; child 1 has cum_logp -inf and G -inf."""
    P, W, K, T = 1, 2, 2, 3
    dev = handle.device
    ft = sc.new_state(P, W, K, T, dev)
    req = handle.frontier_sample_request(ft, W, K, seed=3)
    handle.frontier_sample(req, sc.INIT, 0)  # into set 1; set 0 is filled in by hand below
    torch.cuda.synchronize()
    assert ft["set_len"].tolist() == [-1, -1] and ft["gumbel_1"].tolist() == [0.0, sc.FILL_F, sc.FILL_F, sc.FILL_F]
    i32 = lambda x: torch.tensor(x, dtype=torch.int32, device=dev)
    f64 = lambda x: torch.tensor(x, dtype=torch.float64, device=dev)
    ft["path_len_0"].copy_(i32([1, 1, 1, 1]))
    ft["cum_logp_0"].copy_(f64([-1.0, -2.0, -0.5, 0.0]))
    ft["gumbel_0"].copy_(f64([-0.25, -1.0, -1.25, -3.0]))
    ft["paths_0"][0].copy_(i32([[0, 1, 1], [0, 1, 2], [0, 1, 3], [0, 3, 3]]))
    ft["set_len"].copy_(i32([-1, 2]))
    ft["set_gumbel"].copy_(f64([7.0, -1.5]))
    ev = Evaluation(f64([0.5, 0.75, 0.5, 0.9]), torch.tensor([0, 1, 0, 1], dtype=torch.uint8, device=dev), i32([2, 0, 1, 0]),
                    i32([[[0, 2, 0], [0, 2, 1]], [[7, 7, 7], [7, 7, 7]], [[1, 9, 9], [8, 8, 8]], [[6, 6, 6], [6, 6, 6]]]),
                    torch.tensor([[0.5, 0.0], [0.5, 0.5], [0.5, 0.5], [0.5, 0.5]], dtype=torch.float32, device=dev))
    handle.frontier_sample(req, sc.ADVANCE, 5, ev)  # reads set 0, writes set 1
    torch.cuda.synchronize()
    hi, lo = 6.93147180369123816490e-01, 1.90821492927058770002e-10
    assert ft["best_value"].tolist() == [0.9] and ft["best_len"].tolist() == [1] and ft["best_path"][0, 0].tolist() == [0, 3, 3]
    assert ft["set_len"].tolist() == [1, -1] and ft["set_gumbel"].tolist() == [-1.0, -1.5] and ft["set_logp"].tolist() == [-2.0, sc.FILL_F]
    assert ft["set_value"].tolist() == [0.75, sc.FILL_F] and ft["set_path"][0].tolist() == [[0, 1, 2], [sc.FILL] * 3] and (ft["set_path"][1:] == sc.FILL).all()
    assert ft["parent_row"].tolist() == [0, 0, -1, -1] and ft["path_len_1"].tolist() == [2, 2, -1, -1] and ft["live"].tolist() == [2]
    assert ft["paths_1"][:2, :2].tolist() == [[[0, 1, 1], [0, 1, 1]], [[0, 2, 0], [0, 2, 1]]]
    assert ft["cum_logp_1"][:2].tolist() == [-1.0 + (-1.0 * hi + (-1.0 * lo + 0.0)), float("-inf")]
    assert ft["gumbel_1"].tolist() == [-0.25, float("-inf"), sc.FILL_F, sc.FILL_F] and int(ft["errors_dev"][0]) == 0


# ---- 4. real roots --------------------------------------------------------------------------------------------------
P_REAL, W_REAL, K_REAL, SEED_REAL = 8, 3, 3, 6
FIELDS = ("best_path", "best_len", "best_value", "action", "live", "errors", "set_len", "set_gumbel", "set_logp", "set_value", "set_path")


def test_the_whole_stack_on_real_roots_and_every_entry_replayed():
    cfg = plc.case("small_pin")[0]()
    T = plc.max_steps(cfg)
    F = W_REAL * K_REAL
    root = BatchedPlacementEnv(cfg, P_REAL, queue_depth=2, run_seed=SEED_REAL, auto_reset=False)
    planner = BatchedPlacementEnv(cfg, P_REAL * F, queue_depth=2, run_seed=SEED_REAL, auto_reset=False)
    replay = BatchedPlacementEnv(cfg, P_REAL * W_REAL, queue_depth=2, run_seed=SEED_REAL, auto_reset=False)
    for e in (root, planner, replay):
        e.generate_instances()
        e.reset()
    root.rollout_step(0)  # the roots a transition into their episodes
    dev = root.device
    zeros = torch.zeros((P_REAL * F, cfg.num_orientations * cfg.height * cfg.width), dtype=torch.float32, device=dev)
    evaluate = network_evaluator(root, planner, lambda obs: zeros, max_children=K_REAL, priors="device", leaves=F)
    rows = []

    def copied_over(paths, path_len, step_index0):
        ev = evaluate(paths.to(dev), path_len.to(dev), step_index0)
        rows.append(int((path_len >= 0).sum()))
        return Evaluation(*(getattr(ev, f).cpu() for f in ("value", "terminal", "cand_count", "cand_actions", "cand_prior")))
    want = frontier_sample_search(SimpleNamespace(num_envs=P_REAL, cfg=cfg, device="cpu"), copied_over, W_REAL, K_REAL, 7000, seed=17, max_steps=T)
    got = frontier_sample_search_device(root, evaluate, W_REAL, K_REAL, 7000, seed=17, max_steps=T)
    torch.cuda.synchronize()
    assert int(want.errors) == 0 and rows[0] == P_REAL and max(rows) > P_REAL * W_REAL and len(rows) == T + 1
    for f in FIELDS:
        a, b = getattr(got, f).cpu(), getattr(want, f).cpu()
        assert a.dtype == b.dtype and a.shape == b.shape and a.numpy().tobytes() == b.numpy().tobytes(), f
    S = P_REAL * W_REAL
    set_len = got.set_len
    assert int(got.live.sum()) == 0 and int((set_len >= 1).sum()) >= P_REAL // 2 and bool((set_len <= T).all()), set_len.tolist()
    # the paths of a root's entries are pairwise different
    path, n = got.set_path.cpu().numpy().reshape(T, P_REAL, W_REAL, 3), set_len.cpu().numpy().reshape(P_REAL, W_REAL)
    assert (n >= 0).sum(axis=1).max() >= 2  # some root has more than one plan to tell apart
    for p in range(P_REAL):
        plans = [path[:n[p, j], p, j].tobytes() for j in range(W_REAL) if n[p, j] >= 0]
        assert len(set(plans)) == len(plans), p
    # every entry's path replayed with `step` on a fork of its root ends at exactly set_len with reward == set_value
    replay.gather_(torch.arange(P_REAL, dtype=torch.int32, device=dev).repeat_interleave(W_REAL), source=root)
    no_action = torch.full((S, 3), -1, dtype=torch.int32, device=dev)
    ended = torch.zeros(S, dtype=torch.bool, device=dev)
    for t in range(T):
        held = set_len <= t  # past its plan or no entry: an action that is no action leaves the episode as it is
        _, r, d, _ = replay.step(torch.where(held[:, None], no_action, got.set_path[t]))
        last = set_len == t + 1
        assert not bool((d.bool() & ~held & ~last).any()), t  # not done before the plan's last step
        assert bool(d.bool()[last].all()), t
        assert r[last].cpu().numpy().tobytes() == got.set_value[last].cpu().numpy().tobytes(), t  # the value the search reported, bit for bit
        ended |= last
    assert bool((ended == (set_len >= 1)).all())
    # the best plan is the entry with the largest value, where the set kept it: best_value is at least every set_value
    assert bool((got.best_value.repeat_interleave(W_REAL)[set_len >= 0] >= got.set_value[set_len >= 0]).all())
    for e in (root, planner, replay):
        e.close()
