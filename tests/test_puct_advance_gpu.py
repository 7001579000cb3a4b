"""pcbenv_puct_advance on the GPU (tests/puct_cases.py has the cases and the CPU model).

1. The kernel alone: recorded searches fed call by call through `BatchedPlacementEnv.puct_advance`, no evaluation launch;
   after EVERY call every tensor of the request equals the state of csrc/pcb_puct.h replayed on the CPU.
2. Every tensor is a view into a sentinel-filled buffer: the guards, the rows nothing was due in and the inputs keep their
   bytes, and a phase that was not asked for writes nothing.  Once with one phase per call, once with no error word.
3. 1. and 2. at every group width G (k_puct_advance<4> ... <64>) with C == G and with C == G / 2 + 1, over three blocks whose
   last one, and from G = 16 on its last wavefront, is partly filled (puct_cases.WIDTHS), K below, equal to and above C.
4. A tree too small for the search, and trees the caller has damaged between two calls (puct_cases.damaged), at G = 4, 16
   and 64: the kernel does what the model does, in every tensor, the neighbouring roots' rows included.
5. A search on a side stream behind a delay returns before the stream reaches it and gives the default stream's tree."""
import time
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from pcbenv import _lib, _search_lib, named_config
from pcbenv.batched_env import BatchedPlacementEnv
from pcbenv.search import Evaluation, puct_search_device

import puct_cases as pc
from stream_cases import LAG_MS, lagged

pytestmark = pytest.mark.gpu

GUARD, SENTINEL = 256, 0xA5
DTYPES = dict(prior=torch.float64, value_sum=torch.float64, value_max=torch.float64, reward_lo=torch.float64, reward_hi=torch.float64,
              terminal=torch.uint8, value=torch.float64, leaf_terminal=torch.uint8, cand_prior=torch.float32)


class Guarded:
    """Every tensor of a request as a view GUARD bytes into a sentinel-filled buffer of its own, GUARD bytes behind it.
    The int32 tensors start out as the model's do (puct_cases.FILL), the others as the sentinel."""

    def __init__(self, P, N, T, K, device):
        shp = dict(pc.shapes(P, N, T), value=(P,), leaf_terminal=(P,), cand_count=(P,), cand_actions=(P, K, 3), cand_prior=(P, K), errors_dev=(1,))
        self.device, self.back, self.t, self.meta = device, {}, {}, {}
        for name, shape in shp.items():
            self.add(name, shape, DTYPES.get(name, torch.int32))
        self.t["errors_dev"].zero_()

    def add(self, name, shape, dtype):
        n = int(np.prod(shape)) * torch.empty((), dtype=dtype).element_size()
        buf = torch.full((GUARD + n + GUARD,), SENTINEL, dtype=torch.uint8, device=self.device)
        self.back[name] = buf
        self.t[name] = buf[GUARD:GUARD + n].view(dtype).view(shape)
        self.meta[name] = (self.t[name].cpu().numpy().dtype, tuple(shape))
        if dtype == torch.int32:
            self.t[name].fill_(pc.FILL)

    def snapshot(self):
        return {name: buf.cpu().numpy().copy() for name, buf in self.back.items()}

    def inside(self, snap, name):
        dtype, shape = self.meta[name]
        return snap[name][GUARD:len(snap[name]) - GUARD].view(dtype).reshape(shape)


REPLAYS = {  # P, T, C, K, iterations, capacity, split
    "chain_C1": (7, 5, 1, 3, 40, None, False),
    "C3": (7, 5, 3, 3, 40, None, False),
    "C5_K3": (7, 5, 5, 3, 40, None, False),
    "C3_K6_P14": (14, 5, 3, 6, 40, None, False),
    "T1": (7, 1, 3, 3, 12, None, False),
    "capacity6": (7, 5, 3, 3, 40, 6, False),
    "one_phase_per_call": (7, 5, 3, 3, 16, None, True),
}
# every k_puct_advance<G> with C == G and with C == G / 2 + 1, three blocks each, the last one and its last wavefront partly filled
REPLAYS.update({name: (P, pc.WIDTH_T, C, K, iterations, None, False) for name, (P, C, K, iterations, _, _) in pc.WIDTHS.items()})


@pytest.fixture(scope="module")
def handle():
    env = BatchedPlacementEnv(named_config("c3"), 2, queue_depth=1, run_seed=1)  # the handle gives the device only
    yield env
    env.close()


def advance_and_compare(handle, req, g, i, call, want, before, errors_dev=True):
    """Call i through puct_advance into the guarded tensors of g; want: the model's state after it; before: the snapshot after
    the call before.  -> (the snapshot the call started from, the one it left)."""
    inputs = {}
    for name, at, value in call.get("pokes", ()):  # the damage a caller does between two calls
        g.t[name].view(-1)[at] = value
    if call.get("pokes") and not call["phases"] & pc.ABSORB:
        before = g.snapshot()
    if call["phases"] & pc.ABSORB:
        for name, a in zip(pc.INPUTS, call["evaluation"]):
            g.t[name].copy_(torch.from_numpy(np.ascontiguousarray(a)))
            inputs[name] = g.t[name]
        before = g.snapshot()
    handle.puct_advance(req, call["phases"], **inputs)
    after = g.snapshot()
    for name in after:  # the guards, and what the call only reads
        assert np.array_equal(after[name][:GUARD], before[name][:GUARD]) and np.array_equal(after[name][-GUARD:], before[name][-GUARD:]), (i, name)
        if name in pc.INPUTS:
            assert np.array_equal(after[name], before[name]), (i, name)
    # every tensor against the model: that includes the paths rows >= path_len, which hold what they held before (the
    # model's tensors start with the same fill)
    for f in pc.STATE_FIELDS:
        model = want[f]
        got = g.inside(after, f)
        if f in pc.FLOATS:
            assert pc.same_bits(got, model), (i, f)
        else:
            assert np.array_equal(got.astype(np.int64), model), (i, f)
    assert int(g.inside(after, "errors_dev")[0]) == (want["errors"] if errors_dev else 0), i
    untouched = ()
    if call["phases"] == pc.SELECT:
        untouched = pc.TREE_FIELDS
    elif call["phases"] in (pc.ABSORB, pc.INIT):
        untouched = ("selected", "path_len", "paths")
    for f in untouched:  # a phase that was not asked for wrote nothing
        assert np.array_equal(after[f], before[f]), (i, f)
    return before, after


def assert_equals_the_model_after_every_call(handle, case, errors_dev=True):
    """case.seq call by call through puct_advance into guarded tensors; case.states: the model's state after each call.
    errors_dev=False: the request names no error word (the guarded one must keep its zero)."""
    P, C, T, K = case.P, case.C, case.T, case.K
    g = Guarded(P, case.N, T, K, handle.device)
    req = handle.puct_request(g.t if errors_dev else {n: t for n, t in g.t.items() if n != "errors_dev"}, case.c_puct, C)
    assert (req.errors_dev is not None) == errors_dev and req.max_children == C and req.capacity == case.N and req.max_steps == T
    before = g.snapshot()
    for i, (call, want) in enumerate(zip(case.seq, case.states)):
        _, before = advance_and_compare(handle, req, g, i, call, want, before, errors_dev)


@pytest.mark.parametrize("what", list(REPLAYS))
def test_the_kernel_alone_equals_the_model_after_every_call(handle, what):
    P, T, C, K, iterations, capacity, split = REPLAYS[what]
    if what in pc.WIDTHS:  # with the checks, made on the CPU, that the row reaches what it is there for
        case = pc.width_case(what)
    else:
        case = pc.synthetic(P, T, C, K, iterations, capacity=capacity, split=split)
    if what == "G64_C64_P1":
        assert any(s["path_len"].max() > 0 for s in case.states) and int(case.states[-1]["num_children"].max()) == 64, "no descent over 64 children"
    if what == "capacity6":
        assert case.states[-1]["errors"] & pc.ERR_FULL
    if what == "one_phase_per_call":
        assert {c["phases"] for c in case.seq} == {pc.INIT, pc.ABSORB, pc.SELECT}
    assert_equals_the_model_after_every_call(handle, case)


def test_without_an_error_word(handle):
    """errors_dev is optional: the search of a tree of six slots, which is full (ERR_FULL) in most of its calls, with no
    error word in the request grows the model's tree all the same."""
    P, T, C, K, iterations, capacity, split = REPLAYS["capacity6"]
    case = pc.synthetic(P, T, C, K, iterations, capacity=capacity, split=split)
    assert sum(bool(s["errors"] & pc.ERR_FULL) for s in case.states) > 10
    assert_equals_the_model_after_every_call(handle, case, errors_dev=False)


@pytest.mark.parametrize("G", sorted(pc.DAMAGE_GAMES))
def test_a_full_tree_at_every_damage_width(handle, G):
    P, T, C, K, iterations, _ = pc.DAMAGE_GAMES[G]
    case = pc.synthetic(P, T, C, K, iterations, capacity=1 + 2 * C)
    assert case.states[-1]["errors"] == pc.ERR_FULL and pc.group_lanes(C) == G
    assert_equals_the_model_after_every_call(handle, case)


@pytest.mark.parametrize("G, name", pc.DAMAGE_CASES)
def test_a_damaged_tree_is_handled_as_the_model_handles_it(handle, G, name):
    """Trees the caller has damaged (tests/puct_cases.py:damaged; tests/test_puct_model.py asserts on the model's dump that
    each scenario reaches the path it is named after): the kernel's lane-parallel checks give what the serial ones give,
    in every tensor after every call.  Only roots 0 < p < P - 1 are damaged and only by values within a node's children of
    the valid range: were a check missing, the stray access would fall into a neighbouring root's rows, which are compared."""
    sc = pc.damaged(G, name)
    assert 0 < sc.p < sc.P - 1
    N, C = sc.N, sc.C
    allowed = dict(selected=(-1, N), num_nodes=(0, N + 1), first_child=(0, N) + tuple(range(N - C + 1, N)), parent=(sc.node, N),
                   num_children=(-1, C + 5))
    for f, at, value in sc.seq[sc.k].get("pokes", ()):
        assert value in allowed[f], (f, value)
    assert_equals_the_model_after_every_call(handle, sc)


def test_no_roots_is_a_no_op(handle):
    """num_roots == 0 succeeds without a launch: the addresses (valid ones, of a tensor of the handle's) are not looked at."""
    R = _search_lib.PcbenvPuctRequest
    req = R(struct_size=224, phases=pc.ABSORB | pc.SELECT, num_roots=0, capacity=3, max_children=2, max_steps=2, num_candidates=2, c_puct=1.0)
    for n, _ in R._fields_[9:-2]:
        setattr(req, n, handle.reward.data_ptr())
    assert handle._L.pcbenv_puct_advance(handle._h, req) == _lib.PCBENV_OK
    torch.cuda.synchronize()


# ---- 5. side stream -------------------------------------------------------------------------------------------------
def test_side_stream(handle):
    """The whole search is enqueued on a non-blocking side stream behind a delay: it returns before the stream reaches
    it -- no call of it waits for the device -- and grows the tree of the default-stream run.  The evaluations are the
    recorded ones of a synthetic search, uploaded beforehand: the tree step is all that is enqueued."""
    P, T, C, K, iterations = 70, 5, 8, 8, 10
    case = pc.width_case("G8_C8_P70")
    dev = handle.device
    fixed = [Evaluation(*(torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in c["evaluation"])) for c in case.seq[1:]]
    # the handle gives the device and the stream only: the P roots of the search are the recording's
    search_root = SimpleNamespace(num_envs=P, device=dev, cfg=None, puct_request=handle.puct_request, puct_advance=handle.puct_advance)

    def search():
        it = iter(fixed)
        return puct_search_device(search_root, iterations, 100, lambda paths, path_len, s: next(it), c_puct=case.c_puct, max_children=C, max_steps=T)
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
