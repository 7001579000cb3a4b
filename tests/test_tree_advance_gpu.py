"""pcbenv_tree_advance on the GPU (tests/tree_cases.py has the cases and the CPU model).

1. `tree_search_device` -- two launches per iteration, the tree on the device -- grows the tree `tree_search` grows on the CPU
   with the CPU oracle's playouts, in every field, floats by their bits, on the roots of tests/test_tree_search_gpu.py and on
   a ragged grid; the roots are untouched.
2. The kernel alone: recorded searches fed call by call through `BatchedPlacementEnv.tree_advance`, no playout launch; after
   EVERY call every tensor of the request equals the state of csrc/pcb_tree.h replayed on the CPU.
3. Every tensor is a view into a sentinel-filled buffer: the guards, the rows nothing was due in and the inputs keep their
   bytes, and a phase that was not asked for writes nothing.
4. A search on a side stream behind a delay returns before the stream reaches it and gives the default stream's tree.
5. 2. and 3. at every group width G (k_tree_advance<4> ... <64>) with C == G and with C == G / 2 + 1, over three blocks whose last
   one, and from G = 16 on its last wavefront, is partly filled (tree_cases.WIDTHS); and once with no error word in the request.
6. Trees the caller has damaged between two calls (tree_cases.damaged): the kernel does what the model does, in every tensor."""
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
# every k_tree_advance<G> with C == G and with C == G / 2 + 1, three blocks each, the last one and its last wavefront partly filled
REPLAYS.update({name: (P, tc.WIDTH_T, C, iterations, None, False, cells) for name, (P, C, iterations, cells, _, _) in tc.WIDTHS.items()})


@pytest.fixture(scope="module")
def handle():
    env = BatchedPlacementEnv(named_config("c3"), 2, queue_depth=1, run_seed=1)  # the handle gives the device only
    yield env
    env.close()


def assert_equals_the_model_after_every_call(handle, case, errors_dev=True):
    """case.seq call by call through tree_advance into guarded tensors; case.states: the model's state after each call.
    errors_dev=False: the request names no error word (the guarded one must keep its zero)."""
    P, C, T = case.P, case.C, case.T
    g = Guarded(P, case.N, C, T, handle.device)
    req = handle.tree_request(g.t if errors_dev else {n: t for n, t in g.t.items() if n != "errors_dev"}, case.c_uct)
    assert (req.errors_dev is not None) == errors_dev
    before = g.snapshot()
    for i, (call, want) in enumerate(zip(case.seq, case.states)):
        playout = {}
        for name, at, value in call.get("pokes", ()):  # the damage a caller does between two calls
            g.t[name].view(-1)[at] = value
        if call.get("pokes") and not call["phases"] & tc.ABSORB:
            before = g.snapshot()
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
        assert int(g.inside(after, "errors_dev")[0]) == (want["errors"] if errors_dev else 0), i
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


@pytest.mark.parametrize("what", list(REPLAYS))
def test_the_kernel_alone_equals_the_model_after_every_call(handle, what):
    P, T, C, iterations, capacity, split, cells = REPLAYS[what]
    if what in tc.WIDTHS:  # with the checks, made on the CPU, that the row reaches what it is there for
        case = tc.width_case(what)
    else:
        case = tc.synthetic(P, T, C, iterations, capacity=capacity, split=split, cells=cells)
    if what == "C64_P1":
        assert any(s["path_len"].max() > 0 for s in case.states), "no descent over 64 children"
    if what == "capacity4":
        assert case.states[-1]["errors"] & 1
    assert_equals_the_model_after_every_call(handle, case)


def test_without_an_error_word(handle):
    """errors_dev is optional: the search of a tree of four slots, which is full (ERR_FULL) in most of its calls, with no
    error word in the request grows the model's tree all the same."""
    P, T, C, iterations, capacity, split, cells = REPLAYS["capacity4"]
    case = tc.synthetic(P, T, C, iterations, capacity=capacity, split=split, cells=cells)
    assert sum(bool(s["errors"] & tc.ERR_FULL) for s in case.states) > 10
    assert_equals_the_model_after_every_call(handle, case, errors_dev=False)


@pytest.mark.parametrize("G, name", tc.DAMAGE_CASES)
def test_a_damaged_tree_is_handled_as_the_model_handles_it(handle, G, name):
    """Trees the caller has damaged (tests/tree_cases.py:damaged; tests/test_tree_model.py asserts on the model's dump that
    each scenario reaches the path it is named after): the kernel's lane-parallel checks give what the serial ones give,
    in every tensor after every call.  Only roots 0 < p < P - 1 are damaged and only by values within two slots of the valid
    range: were a check missing, the stray access would fall into a neighbouring root's rows, which are compared."""
    sc = tc.damaged(G, name)
    assert 0 < sc.p < sc.P - 1
    N, C, T = sc.N, sc.C, sc.T
    allowed = dict(selected=(-1, 0, sc.child[0], N), num_nodes=(0, N + 1), children=(0, N), parent=(sc.child[0], N), depth=(-1, T, T + 3),
                   num_children=(-1, C, C + 5))
    for f, at, value in sc.seq[sc.k]["pokes"]:
        assert value in allowed[f], (f, value)
    assert_equals_the_model_after_every_call(handle, sc)


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
