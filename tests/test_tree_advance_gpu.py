"""pcbenv_tree_advance on the GPU (tests/tree_cases.py has the cases and the CPU model).

1. `tree_search_device` -- two launches per iteration, the tree on the device -- grows the tree `tree_search` grows on the CPU
   with the CPU oracle's playouts, in every field, floats by their bits, on the roots of tests/test_tree_search_gpu.py and on
   a ragged grid; the roots are untouched.
2. The kernel alone: recorded searches fed call by call through `BatchedPlacementEnv.tree_advance`, no playout launch; after
   EVERY call every tensor of the request equals the state of csrc/pcb_tree.h replayed on the CPU.
3. Every tensor is a view into a sentinel-filled buffer: the guards, the rows nothing was due in and the inputs keep their
   bytes, and a phase that was not asked for writes nothing.
4. A search on a side stream behind a delay returns before the stream reaches it and gives the default stream's tree."""
import time
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from pcbenv import _lib, named_config
from pcbenv.batched_env import BatchedPlacementEnv
from pcbenv.search import ln_table, tree_search_device

import tree_cases as tc
from stream_cases import LAG_MS, lagged
from test_playout_gpu import device_roots

pytestmark = pytest.mark.gpu

GUARD, SENTINEL = 256, 0xA5
DTYPES = dict(value_sum=torch.float64, value_max=torch.float64, reward_lo=torch.float64, reward_hi=torch.float64, best_reward=torch.float64,
              terminal=torch.uint8, ln_dev=torch.float64, reward=torch.float64)
RESULT_FIELDS = ("num_nodes", "parent", "depth", "node_action", "visits", "terminal", "children", "child_visits", "child_actions", "action", "best_length")


def _bits(t):
    return t.cpu().numpy().view(np.uint64)


def assert_same_search(got, want):
    for f in RESULT_FIELDS:
        assert torch.equal(getattr(got, f).cpu(), getattr(want, f)), f
    for f in ("value_sum", "value_max", "best_reward"):
        assert np.array_equal(_bits(getattr(got, f)), _bits(getattr(want, f))), f
    L = want.best_length
    for p in range(L.shape[0]):
        assert torch.equal(got.best_actions[:int(L[p]), p].cpu(), want.best_actions[:int(L[p]), p]), p
    assert int(got.errors) == 0


# ---- 1. identical trees ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name, iterations", tc.ORACLE_CASES)
def test_device_search_grows_the_tree_of_tree_search(name, iterations):
    case = tc.oracle_case(name, iterations)  # tree_search on the CPU, the playouts by the CPU oracle (shared, computed once)
    assert case.P == 12 or name not in ("small_pin", "c3_centroid")
    assert int(case.ts.num_nodes.max()) > 4
    run = device_roots(case.roots)
    got = tree_search_device(run.env, iterations, tc.STEP_INDEX, c_uct=tc.C_UCT, max_children=tc.MAX_CHILDREN)
    assert_same_search(got, case.ts)
    run.compare_oracle("the roots after the search")
    run.close()


# ---- 2. and 3. the kernel alone, in guarded tensors -----------------------------------------------------------------
class Guarded:
    """Every tensor of a request as a view GUARD bytes into a sentinel-filled buffer of its own, GUARD bytes behind it.
    The int32 tensors start out as the model's do (tree_cases.FILL), the others as the sentinel."""

    def __init__(self, P, N, C, T, device):
        shp = dict(tc.shapes(P, N, C, T), ln_dev=(N + 1,), reward=(P,), length=(P,), actions=(T, P, 3), errors_dev=(1,))
        self.back, self.t, self.meta = {}, {}, {}
        for name, shape in shp.items():
            dtype = DTYPES.get(name, torch.int32)
            n = int(np.prod(shape)) * torch.empty((), dtype=dtype).element_size()
            buf = torch.full((GUARD + n + GUARD,), SENTINEL, dtype=torch.uint8, device=device)
            self.back[name] = buf
            self.t[name] = buf[GUARD:GUARD + n].view(dtype).view(shape)
            self.meta[name] = (self.t[name].cpu().numpy().dtype, tuple(shape))
            if dtype == torch.int32:
                self.t[name].fill_(tc.FILL)
        self.t["errors_dev"].zero_()
        self.t["ln_dev"].copy_(ln_table(N))

    def snapshot(self):
        return {name: buf.cpu().numpy().copy() for name, buf in self.back.items()}

    def inside(self, snap, name):
        dtype, shape = self.meta[name]
        return snap[name][GUARD:len(snap[name]) - GUARD].view(dtype).reshape(shape)


REPLAYS = {  # P, T, C, iterations, capacity, split, cells of the game (x 2 orientations = its actions)
    "chain_C1": (7, 5, 1, 40, None, False, 3),
    "C3": (7, 5, 3, 40, None, False, 3),
    "C5_P67": (67, 5, 5, 40, None, False, 3),
    "C64_P1": (1, 5, 64, 110, None, False, 100),  # 200 actions: the root has its 64 children after some 75 playouts
    "T1": (7, 1, 3, 12, None, False, 3),
    "capacity4": (7, 5, 3, 40, 4, False, 3),
    "one_phase_per_call": (7, 5, 3, 16, None, True, 3),
}


@pytest.fixture(scope="module")
def handle():
    env = BatchedPlacementEnv(named_config("c3"), 2, queue_depth=1, run_seed=1)  # the handle gives the device only
    yield env
    env.close()


@pytest.mark.parametrize("what", list(REPLAYS))
def test_the_kernel_alone_equals_the_model_after_every_call(handle, what):
    P, T, C, iterations, capacity, split, cells = REPLAYS[what]
    case = tc.synthetic(P, T, C, iterations, capacity=capacity, split=split, cells=cells)
    if what == "C64_P1":
        assert any(s["path_len"].max() > 0 for s in case.states), "no descent over 64 children"
    if what == "capacity4":
        assert case.states[-1]["errors"] & 1
    g = Guarded(P, case.N, C, T, handle.device)
    req = handle.tree_request(g.t, case.c_uct)
    before = g.snapshot()
    for i, (call, want) in enumerate(zip(case.seq, case.states)):
        playout = {}
        if call["phases"] & tc.ABSORB:
            for name, a in zip(("reward", "length", "actions"), call["playout"]):
                g.t[name].copy_(torch.from_numpy(np.ascontiguousarray(a)))
                playout[name] = g.t[name]
            before = g.snapshot()
        handle.tree_advance(req, call["phases"], **playout)
        after = g.snapshot()
        for name in after:  # the guards, and what the call only reads
            assert np.array_equal(after[name][:GUARD], before[name][:GUARD]) and np.array_equal(after[name][-GUARD:], before[name][-GUARD:]), (i, name)
            if name in ("ln_dev", "reward", "length", "actions"):
                assert np.array_equal(after[name], before[name]), (i, name)
        # every tensor against the model: that includes the paths rows >= path_len and the best_actions rows >= best_length,
        # which hold what they held before (the model's tensors start with the same fill)
        for f in tc.STATE_FIELDS:
            model = want[f]
            got = g.inside(after, f)
            if f in tc.FLOATS:
                assert tc.same_bits(got, model), (i, f)
            else:
                assert np.array_equal(got.astype(np.int64), model), (i, f)
        assert int(g.inside(after, "errors_dev")[0]) == want["errors"], i
        untouched = ()
        if call["phases"] == tc.SELECT:
            untouched = tc.TREE_FIELDS
        elif call["phases"] == tc.ABSORB:
            untouched = ("selected", "path_len", "paths")
        elif call["phases"] == tc.INIT:
            untouched = ("selected", "path_len", "paths", "best_actions")
        for f in untouched:  # a phase that was not asked for wrote nothing
            assert np.array_equal(after[f], before[f]), (i, f)
        before = after


def test_no_roots_is_a_no_op(handle):
    """num_roots == 0 succeeds without a launch: the addresses (valid ones, of a tensor of the handle's) are not looked at."""
    R = _lib.PcbenvTreeRequest
    req = R(struct_size=224, phases=tc.ABSORB | tc.SELECT, num_roots=0, capacity=3, max_children=2, max_steps=2, c_uct=1.0)
    for n, _ in R._fields_[7:-2]:
        setattr(req, n, handle.reward.data_ptr())
    assert handle._L.pcbenv_tree_advance(handle._h, req) == _lib.PCBENV_OK
    torch.cuda.synchronize()


# ---- 4. side stream -------------------------------------------------------------------------------------------------
def test_side_stream():
    """The whole search is enqueued on a non-blocking side stream behind a delay: it returns before the stream reaches
    it -- no call of it waits for the device -- and grows the tree of the default-stream run."""
    name, iterations = "small_pin", 8
    case = tc.oracle_case(name, tc.ITERATIONS)
    run = device_roots(case.roots)
    search = lambda: tree_search_device(run.env, iterations, tc.STEP_INDEX, c_uct=tc.C_UCT, max_children=tc.MAX_CHILDREN)
    want = search()
    torch.cuda.synchronize()
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
    want_cpu = SimpleNamespace(**{f: getattr(want, f).cpu() for f in RESULT_FIELDS + ("value_sum", "value_max", "best_reward", "best_actions")})
    assert_same_search(got, want_cpu)
    run.compare_oracle("the roots after the searches")
    run.close()
