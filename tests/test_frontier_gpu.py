"""pcbenv_frontier_advance on the GPU (tests/frontier_cases.py has the cases and the CPU model).

1. The kernel alone: the call sequences of the table fed call by call through `BatchedPlacementEnv.frontier_advance`, no
   evaluation launch; after EVERY call every tensor of the request equals the state of csrc/pcb_frontier.h replayed on
   the CPU, floats by their bits.  The shapes are those at which the mapping -- one wavefront per root, row j * 64 + lane in
   register j, four roots per workgroup -- can go wrong: F = 1; F = 15, ragged against any power of two; F = 64 exactly; F =
   65, the first row beyond a wavefront; F = 1024 as 16 x 64 and as 64 x 16, all sixteen registers and W = 64 rounds; T = 1
   and T = 5; P = 1, and P = 6, which fills one workgroup, starts a second and leaves two of its four wavefronts without a
   root; both arms of the prior weight; the ties, NaNs and damaged rows of the hand-made calls.
2. Every tensor is a view into a sentinel-filled buffer: the guards, the path rows behind a row's length, the slots that are
   no row and the inputs keep their bytes.
3. Without an error word; no roots; a side stream; one launch worked out by hand.
4. The whole stack on real roots: `frontier_search_device` next to `network_evaluator(priors="device", leaves=W * K)`
   against `frontier_search`, and every root's best_path replayed with `step`.
What the cases reach is asserted on the CPU (tests/test_frontier_model.py)."""
import time
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from pcbenv import _frontier_lib, _lib
from pcbenv.batched_env import BatchedPlacementEnv
from pcbenv import named_config
from pcbenv.search import Evaluation, frontier_search, frontier_search_device, network_evaluator

import frontier_cases as fc
import playout_cases as plc
import puct_cases as pc
from stream_cases import LAG_MS, lagged
from test_puct_advance_gpu import DTYPES, GUARD, Guarded

pytestmark = pytest.mark.gpu

F64 = ("cum_logp_0", "cum_logp_1", "best_value")


class GuardedFrontier(Guarded):
    """test_puct_advance_gpu.Guarded with the tensors of a frontier request: the int32 ones start out as the model's do
    (frontier_cases.FILL), the float64 ones of the state as FILL_F."""

    def __init__(self, P, W, K, T, device, errors=True):
        R = P * W * K
        shp = dict(fc.shapes(P, W, K, T), value=(R,), leaf_terminal=(R,), cand_count=(R,), cand_actions=(R, K, 3), cand_prior=(R, K), errors_dev=(1,))
        self.device, self.back, self.t, self.meta = device, {}, {}, {}
        for name, shape in shp.items():
            self.add(name, shape, torch.float64 if name in F64 else DTYPES.get(name, torch.int32))
            if name in F64:
                self.t[name].fill_(fc.FILL_F)
        self.t["errors_dev"].zero_()
        if not errors:
            self.word = self.t.pop("errors_dev")


@pytest.fixture(scope="module")
def handle():
    env = BatchedPlacementEnv(named_config("c3"), 2, queue_depth=1, run_seed=1)  # the handle gives the device only
    yield env
    env.close()


def advance_and_compare(handle, req, g, i, call, want, errors=True):
    """Call i through frontier_advance into the guarded tensors of g; want: the model's state after it."""
    ev = None
    if call["load"] is not None:  # a frontier of the caller's making
        fc.apply_load(g.t, call["load"], call["swap"])
    if call["evaluation"] is not None:
        for name, a in zip(pc.INPUTS, call["evaluation"]):
            g.t[name].copy_(torch.from_numpy(np.ascontiguousarray(a)))
        ev = Evaluation(g.t["value"], g.t["leaf_terminal"], g.t["cand_count"], g.t["cand_actions"], g.t["cand_prior"])
    before = g.snapshot()
    handle.frontier_advance(req, call["phases"], ev, swap=bool(call["swap"]))
    after = g.snapshot()
    s = 1 if call["swap"] else 0
    for name in after:  # the guards, and what the call only reads: the inputs and the in set
        assert np.array_equal(after[name][:GUARD], before[name][:GUARD]) and np.array_equal(after[name][-GUARD:], before[name][-GUARD:]), (i, name)
        if name in pc.INPUTS or name in (f"paths_{s}", f"path_len_{s}", f"cum_logp_{s}"):
            assert np.array_equal(after[name], before[name]), (i, name)
    # every tensor against the model: that includes the path rows behind a row's length, the slots that are no row and their
    # cum_logp, which hold what they held before (the model's tensors start with the same fill)
    for f in fc.STATE_FIELDS:
        got = g.inside(after, f)
        if f in fc.FLOATS:
            assert fc.same_bits(got, want[f]), (i, f)
        else:
            assert np.array_equal(got.astype(np.int64), want[f]), (i, f)
    if errors:
        assert int(g.inside(after, "errors_dev")[0]) == want["errors"], i
    if call["phases"] == fc.INIT:  # INIT writes neither paths nor best_path
        for f in ("paths_0", "paths_1", "best_path"):
            assert np.array_equal(after[f], before[f]), (i, f)


def assert_equals_the_model_after_every_call(handle, case, errors=True):
    g = GuardedFrontier(case.P, case.W, case.K, case.T, handle.device, errors)
    req = handle.frontier_request(g.t, case.W, case.K, case.prior_weight)
    assert (req.num_roots, req.width, req.num_candidates, req.max_steps, req.prior_weight) == (case.P, case.W, case.K, case.T, case.prior_weight)
    assert bool(req.errors_dev) == errors
    for i, (call, want) in enumerate(zip(case.seq, case.states)):
        advance_and_compare(handle, req, g, i, call, want, errors)
    return g


def test_the_table_has_the_shapes_the_mapping_can_go_wrong_at():
    shapes = {(fc.CASES[n][1], fc.CASES[n][2]) for n in fc.CASES}
    assert {(1, 1), (3, 5), (4, 16), (5, 13), (16, 64), (64, 16)} <= shapes and 4 * 16 == 64 and 5 * 13 == 65 and 16 * 64 == 64 * 16 == fc.search.MAX_FRONTIER_ROWS
    assert {fc.CASES[n][3] for n in fc.CASES} >= {1, 5} and {fc.CASES[n][4] == 0.0 for n in fc.CASES} == {True, False}
    per_block = fc.ROOTS_PER_BLOCK
    roots = {fc.CASES[n][0] for n in fc.CASES}
    assert 1 in roots and 6 in roots and -(-6 // per_block) == 2 and 0 < 6 % per_block < per_block  # one workgroup full, a second begun, its tail partly filled
    assert 23 in roots and -(-23 // per_block) == 6 and 23 % per_block == 3
    for n in ("W16_K64", "W64_K16"):  # the widest cases do fill up: a launch reads more than W expandable rows (all W rounds) and writes rows of the last register
        c = fc.case(n)
        assert fc.facts(c).get("more_than_W") and max(int(s["live"].max()) for s in c.states) > 900
        assert any((s[f"path_len_{i}"].reshape(c.P, 1024)[:, 15 * 64:] >= 0).any() for s in c.states for i in (0, 1))
    c = fc.case("W5_K13")
    assert fc.facts(c).get("more_than_W") and any((s[f"path_len_{i}"].reshape(c.P, 65)[:, 64] >= 0).any() for s in c.states for i in (0, 1))  # row 64 in use


@pytest.mark.parametrize("name", list(fc.CASES))
def test_the_kernel_alone_equals_the_model_after_every_call(handle, name):
    case = fc.case(name)
    assert any((s["live"] > 0).any() for s in case.states[1:]) and any((s["best_len"] >= 0).any() for s in case.states)
    assert_equals_the_model_after_every_call(handle, case)


def test_without_an_error_word(handle):
    """errors_dev null: the same states, the damaged rows included, and the word that is not the request's stays zero."""
    case = fc.case("hand_0")
    assert case.states[-1]["errors"] & fc.ERR_ROW
    g = assert_equals_the_model_after_every_call(handle, case, errors=False)
    assert int(g.word[0]) == 0


def test_no_roots_is_a_no_op(handle):
    R = _frontier_lib.PcbenvFrontierRequest
    req = R(struct_size=184, phases=fc.ADVANCE, num_roots=0, width=3, num_candidates=2, max_steps=2, prior_weight=1.0)
    for n, _ in R._fields_[9:-2]:
        setattr(req, n, handle.reward.data_ptr())
    assert handle._L.pcbenv_frontier_advance(handle._h, req) == _lib.PCBENV_OK
    torch.cuda.synchronize()
    ft = fc.search.new_frontier_tensors(0, 3, 2, 2, handle.device)
    handle.frontier_advance(handle.frontier_request(ft, 3, 2), fc.INIT)
    torch.cuda.synchronize()


def test_side_stream(handle):
    """The whole search is enqueued on a non-blocking side stream behind a delay: it returns before the stream reaches it
    and gives the result of the default-stream run.  The evaluations are the recorded ones, uploaded beforehand."""
    case = fc.case("W4_K16")
    dev = handle.device
    fixed = [Evaluation(*(torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in c["evaluation"])) for c in case.seq[1:]]
    root = SimpleNamespace(num_envs=case.P, device=dev, cfg=None, frontier_request=handle.frontier_request, frontier_advance=handle.frontier_advance)

    def search():
        it = iter(fixed)
        return frontier_search_device(root, lambda paths, path_len, s: next(it), case.W, case.K, 100, prior_weight=case.prior_weight, max_steps=case.T)
    want = search()
    torch.cuda.synchronize()
    last = case.states[-1]
    assert fc.same_bits(want.best_value.cpu().numpy(), last["best_value"]) and np.array_equal(want.best_len.cpu().numpy(), last["best_len"])
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
    """P = 1, W = 2, K = 2 (F = 4), T = 3, prior_weight = 0.  The frontier read:
      slot 0  path (0,1,1)          value 0.5    2 candidates (0,2,0) (0,2,1), priors 0.5 0.25, cum_logp -1.0
      slot 1  path (0,1,2)          value 0.75   final
      slot 2  path (1,0,0) (1,0,1)  value 0.5    1 candidate  (1,9,9), prior 0.5, cum_logp -0.5
      slot 3  path (0,3,3)          value 0.625  a count of 5, clamped to 2: (0,4,0) (0,4,1), priors 1.0 and 0.0, cum_logp 0.0
    Slot 1 is the best final so far: best_value 0.75, best_len 1, best_path (0,1,2).  The others are expandable; by value
    slot 3 goes first, and slots 0 and 2 tie at 0.5: the lower slot is kept, slot 2 is cut.  The children: slot 3's in slots 0
    and 1 -- ln 1 = 0, and the prior 0 has no logarithm: -inf -- slot 0's in slots 2 and 3 with -1 + ln 0.5 and -1 + ln 0.25,
    which ieee_ln gives as -(LN2_HI + LN2_LO) and -(2 LN2_HI + 2 LN2_LO) grouped as below."""
    P, W, K, T = 1, 2, 2, 3
    dev = handle.device
    ft = fc.new_state(P, W, K, T, dev)
    req = handle.frontier_request(ft, W, K, 0.0)
    handle.frontier_advance(req, fc.INIT)  # into set 1; set 0 is filled in by hand below
    i32 = lambda x: torch.tensor(x, dtype=torch.int32, device=dev)
    ft["path_len_0"].copy_(i32([1, 1, 2, 1]))
    ft["cum_logp_0"].copy_(torch.tensor([-1.0, -9.0, -0.5, 0.0], dtype=torch.float64, device=dev))
    ft["paths_0"][0].copy_(i32([[0, 1, 1], [0, 1, 2], [1, 0, 0], [0, 3, 3]]))
    ft["paths_0"][1, 2].copy_(i32([1, 0, 1]))
    ev = Evaluation(torch.tensor([0.5, 0.75, 0.5, 0.625], dtype=torch.float64, device=dev), torch.tensor([0, 1, 0, 0], dtype=torch.uint8, device=dev), i32([2, 0, 1, 5]),
                    i32([[[0, 2, 0], [0, 2, 1]], [[7, 7, 7], [7, 7, 7]], [[1, 9, 9], [8, 8, 8]], [[0, 4, 0], [0, 4, 1]]]),
                    torch.tensor([[0.5, 0.25], [0.5, 0.5], [0.5, 0.5], [1.0, 0.0]], dtype=torch.float32, device=dev))
    handle.frontier_advance(req, fc.ADVANCE, ev)  # reads set 0, writes set 1
    torch.cuda.synchronize()
    hi, lo = 6.93147180369123816490e-01, 1.90821492927058770002e-10
    assert ft["best_value"].tolist() == [0.75] and ft["best_len"].tolist() == [1] and ft["best_path"][0, 0].tolist() == [0, 1, 2]
    assert (ft["best_path"][1:] == fc.FILL).all()
    assert ft["parent_row"].tolist() == [3, 3, 0, 0] and ft["path_len_1"].tolist() == [2, 2, 2, 2] and ft["live"].tolist() == [4]
    assert ft["paths_1"][:2].tolist() == [[[0, 3, 3], [0, 3, 3], [0, 1, 1], [0, 1, 1]], [[0, 4, 0], [0, 4, 1], [0, 2, 0], [0, 2, 1]]]
    assert (ft["paths_1"][2] == fc.FILL).all()
    assert ft["cum_logp_1"].tolist() == [0.0, float("-inf"), -1.0 + (-1.0 * hi + (-1.0 * lo + 0.0)), -1.0 + (-2.0 * hi + (-2.0 * lo + 0.0))]
    assert abs(ft["cum_logp_1"][2].item() - (-1.0 + np.log(0.5))) < 1e-15 and int(ft["errors_dev"][0]) == 0


# ---- 4. real roots --------------------------------------------------------------------------------------------------
P_REAL, W_REAL, K_REAL, SEED_REAL = 8, 2, 3, 6
FIELDS = ("best_path", "best_len", "best_value", "action", "live", "errors", "paths", "path_len", "cum_logp", "parent_row")


def test_the_whole_stack_on_real_roots_and_the_plan_replayed():
    cfg = plc.case("small_pin")[0]()
    T = plc.max_steps(cfg)
    F = W_REAL * K_REAL
    # run seed 6: every one of its eight roots has a placement that finishes within the frontier (on this 10 x 10 grid a row
    # can run out of legal cells, which is no final: with seeds 2 to 5 some root ends with best_len -1; the test asserts its condition)
    root = BatchedPlacementEnv(cfg, P_REAL, queue_depth=2, run_seed=SEED_REAL, auto_reset=False)
    planner = BatchedPlacementEnv(cfg, P_REAL * F, queue_depth=2, run_seed=SEED_REAL, auto_reset=False)
    replay = BatchedPlacementEnv(cfg, P_REAL, queue_depth=2, run_seed=SEED_REAL, auto_reset=False)
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
    want = frontier_search(SimpleNamespace(num_envs=P_REAL, cfg=cfg, device="cpu"), copied_over, W_REAL, K_REAL, 7000, max_steps=T)
    got = frontier_search_device(root, evaluate, W_REAL, K_REAL, 7000, max_steps=T)
    torch.cuda.synchronize()
    assert int(want.errors) == 0 and rows[0] == P_REAL and max(rows) > P_REAL * W_REAL and len(rows) == T + 1
    for f in FIELDS:
        a, b = getattr(got, f).cpu(), getattr(want, f).cpu()
        assert a.dtype == b.dtype and a.shape == b.shape and a.numpy().tobytes() == b.numpy().tobytes(), f
    # the condition of this test: every root has a finished placement of at least one step
    best_len = got.best_len.cpu()
    assert (best_len >= 1).all() and (best_len <= T).all(), best_len.tolist()
    # the plan: best_path replayed with `step` on a fork of the roots ends at exactly best_len with reward == best_value
    replay.gather_(torch.arange(P_REAL, dtype=torch.int32, device=dev), source=root)
    no_action = torch.full((P_REAL, 3), -1, dtype=torch.int32, device=dev)
    ended = torch.zeros(P_REAL, dtype=torch.bool, device=dev)
    for t in range(T):
        held = got.best_len <= t  # past its plan: an action that is no action leaves the episode as it is
        _, r, d, _ = replay.step(torch.where(held[:, None], no_action, got.best_path[t]))
        last = got.best_len == t + 1
        assert not bool((d.bool() & ~held & ~last).any()), t  # not done before the plan's last step
        assert bool(d.bool()[last].all()), t
        assert r[last].cpu().numpy().tobytes() == got.best_value[last].cpu().numpy().tobytes(), t  # the reward the search reported, bit for bit
        ended |= last
    assert bool(ended.all()) and got.action.tolist() == got.best_path[0].tolist()
    for e in (root, planner, replay):
        e.close()
