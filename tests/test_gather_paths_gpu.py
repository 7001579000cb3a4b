"""pcbenv_gather_paths on the GPU, through BatchedPlacementEnv.gather_(paths=...) and direct calls of the C ABI, bit for
bit against the CPU oracle (gather_path_cases: the node a path names) on plans made before any device call
(path_cases.Plan; tests/test_gather_path_cases.py checks on the CPU that every plan holds every kind of end), against the
identity of include/pcbenv.h executed literally with existing calls, and against pcbenv_gather where no path is given.
The roots are brought to the plan with test_playout_gpu.device_roots; a destination is a handle_model.Run of its own, so
that every bound tensor of every row is compared with the oracle.  60 nodes per launch (40 where a case has 8 roots)."""
import ctypes as C
import time

import numpy as np
import pytest
import torch

from pcbenv import _lib
from pcbenv.batched_env import BatchedPlacementEnv
from pcbenv.search import policy_backend, tree_search, tree_search_device

import emission_cases as ec
import gather_path_cases as gp
import path_cases as pa
import playout_cases as pc
from handle_model import Run, _bytes_equal, _same_info
from stream_cases import LAG_MS, lagged
from test_playout_gpu import device_roots
from test_playout_paths_gpu import defined_bits

pytestmark = pytest.mark.gpu

K, STEP0 = gp.K, gp.STEP0
_PLANS = {}


def plan_of(name, parity=0):
    if (name, parity) not in _PLANS:
        p = pa.Plan(name, parity)
        _PLANS[name, parity] = (p, gp.nodes_of(p))
    return _PLANS[name, parity]


def destination(plan, n=None, seed_offset=1, **kw):
    """A handle of the plan's definition with episodes of its own (another run seed than the roots'), next to its model."""
    kw = dict(plan.roots.kw, **kw)
    return Run(plan.cfg, plan.n if n is None else n, run_seed=plan.roots.seed + seed_offset, auto_reset=False, **kw)


def on(dev, a, dtype=torch.int32):
    return torch.from_numpy(np.ascontiguousarray(a)).to(device=dev, dtype=dtype)


def tensors(env):
    """Everything a handle shows in its selected slot, on the host."""
    out = {k: v.cpu().numpy() for k, v in env.obs.items()}
    out.update({"marginal_" + k: v.cpu().numpy() for k, v in env.mask_marginals.items()})
    out.update(reward=env.reward.cpu().numpy(), done=env.done.cpu().numpy(), mask_bits=env.mask_bits().cpu().numpy())
    return out


def same_tensors(a, b, tag):
    ta, tb = tensors(a), tensors(b)
    assert set(ta) == set(tb)
    for k in ta:
        assert _bytes_equal(ta[k], tb[k]), (tag, k, np.flatnonzero([not _bytes_equal(x, y) for x, y in zip(ta[k], tb[k])])[:5].tolist())
    assert _same_info(a.info_raw.cpu().numpy(), b.info_raw.cpu().numpy()), (tag, "info")


def state_blob(env):
    return np.asarray(env.state_dict()["state"])


def check_outputs(dst, length, got, tag):
    """reward / done / info of the destination's selected slot and the applied lengths `got` against its model."""
    e, m = dst.env, dst.model
    s = m.slot
    assert _bytes_equal(e.reward.cpu().numpy(), m.R[s]), (tag, "reward", np.flatnonzero(e.reward.cpu().numpy().view(np.uint64) != m.R[s].view(np.uint64))[:5].tolist())
    assert np.array_equal(e.done.cpu().numpy(), m.D[s]), (tag, "done")
    assert _same_info(e.info_raw.cpu().numpy(), m.I[s]), (tag, "info")
    assert got.dtype == np.int32 and np.array_equal(got, length), (tag, "length", got.tolist(), length.tolist())


def gather_paths(dst, idx, src, paths, path_len, tag, flat=None, **kw):
    """gather_(paths=...) on the device, the same on the model, and the comparison of every tensor with the oracle.
    paths: numpy [D, B, 3] (what the model applies); flat: the flat twin handed to the device instead."""
    dev = dst.env.device
    given = on(dev, paths if flat is None else flat)
    dst.env.gather_(on(dev, idx), source=None if src is dst else src.env, paths=given,
                    path_len=None if path_len is None else on(dev, path_len), **kw)
    length = on_the_model(dst, idx, src, paths, path_len)
    dst.compare_oracle(tag)
    check_outputs(dst, length, dst.env.gather_length.cpu().numpy(), tag)
    return length


def on_the_model(dst, idx, src, paths, path_len):
    """The call on the destination's model: a row with a path_len outside [0, path_steps] keeps its episode like a row with
    index -1.  Returns the transitions applied per row."""
    plen = np.full(dst.B, paths.shape[0], np.int32) if path_len is None else np.asarray(path_len, np.int32)
    ok = (plen >= 0) & (plen <= paths.shape[0])
    taken = dst.model.gather(np.where(ok, idx, -1), None if src is dst else src.model)
    return gp.apply_paths(dst.model, taken, paths, np.where(ok, plen, 0))


# ---- 1. against the oracle ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name, parity", [(n, 0) for n in gp.GPU_CASES] + [(n, 1) for n in gp.BOTH_PARITIES])
def test_nodes_against_the_oracle(name, parity):
    """Every kind and team shape (one and four wavefronts, one and two mask words with padding bits, more rows than lanes, a
    grid the first placement fills), a routed terminal on the path; c3_centroid and spatial_7x100 after an even and an odd
    number of step launches (the state sets are double-buffered).  Path rows behind a path's end hold an action that is no
    action: they are never read."""
    plan, nodes = plan_of(name, parity)
    cfg, n = plan.cfg, plan.n
    figures, missing = gp.mix(plan, nodes)
    print(f"GATHER-PATH-MIX {name} parity {parity}: {figures}")
    assert not missing, (missing, figures)
    root = device_roots(plan.roots)
    dst = destination(plan)
    dev = dst.env.device
    paths = plan.path_tensor(fill=gp.NO_ACTION)
    idx = np.array(plan.root_of, np.int64)
    length = gather_paths(dst, idx, root, paths, plan.path_len, (name, parity), check=True)
    # ... and against the nodes stated on a fresh oracle each: every bound tensor, the outputs, the length
    got = dst.host_obs(f64=True)
    for k in nodes[0]["obs"]:
        want = np.stack([nd["obs"][k] for nd in nodes]).reshape(got[k].shape)
        assert _bytes_equal(got[k].astype(np.float64), want), (k, np.flatnonzero([not np.array_equal(a, b) for a, b in zip(got[k].astype(np.float64), want)])[:5].tolist())
    r, d, inf = dst.env.reward.cpu().numpy(), dst.env.done.cpu().numpy(), dst.env.info_raw.cpu().numpy()
    rr, rd, ri = root.env.reward.cpu().numpy(), root.env.done.cpu().numpy(), root.env.info_raw.cpu().numpy()
    for i, nd in enumerate(nodes):
        assert length[i] == nd["length"], i
        j = plan.root_of[i]
        if nd["length"] == 0:  # no transition applied: the source row's, as pcbenv_gather copies them
            assert r[i].tobytes() == rr[j].tobytes() and d[i] == rd[j] and _same_info(inf[i], ri[j]), i
        else:
            assert r[i].tobytes() == nd["reward"].tobytes() and d[i] == nd["done"], (i, r[i], nd["reward"])
            assert not pc.has_info(cfg) or _same_info(inf[i], nd["info"]), (i, inf[i], nd["info"])
    # the legal mask of the node: what pcbenv_playout_paths reports as the leaf of the same paths, on the defined bits
    po = root.env.playout(k=K, step_index=STEP0, paths=on(dev, paths), path_len=on(dev, plan.path_len), leaf_mask=True, max_steps=plan.limit)
    keep = defined_bits(cfg)
    bits, leaf = dst.env.mask_bits().cpu().numpy().view(np.uint64), po.leaf_mask.cpu().numpy().view(np.uint64)
    assert np.array_equal(bits & keep, leaf & keep)
    for i, nd in enumerate(nodes):
        assert np.array_equal(bits[i] & keep, nd["leaf"] & keep), (i, "mask bits")
    root.compare_oracle("the roots after the gather")
    root.close(); dst.close()


# ---- 2. the identity, executed literally ---------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["small_spatial", "c3_both_t256"])
def test_the_identity_with_existing_calls(name):
    """Twin A follows the header's sentence with existing calls only: gather_, then for every ply t a step of ALL rows,
    after which the rows that had stopped before t (path_len <= t, or done at an earlier ply) are put back from holder S.
    Then every tensor of A equals the destination's, and two further fused launches on both stay equal: the state block,
    the presampled action, the feature cache and the list marks behave as after those calls."""
    plan, _ = plan_of(name)
    n = plan.n
    root = device_roots(plan.roots)
    kw = dict(plan.roots.kw)
    mk = lambda: BatchedPlacementEnv(plan.cfg, n, queue_depth=2, run_seed=plan.roots.seed + 1, auto_reset=False, **kw)
    A, S, D = mk(), mk(), mk()
    for e in (A, S, D):
        e.generate_instances()
        e.reset()
    dev = D.device
    idx = on(dev, plan.root_of)
    paths = on(dev, plan.path_tensor(fill=gp.NO_ACTION))
    plen = on(dev, plan.path_len)
    everyone = torch.arange(n, dtype=torch.int32, device=dev)
    D.gather_(idx, source=root.env, paths=paths, path_len=plen)
    A.gather_(idx, source=root.env)
    ended = torch.zeros(n, dtype=torch.bool, device=dev)
    applied = torch.zeros(n, dtype=torch.int32, device=dev)
    for t in range(plan.path_steps):
        S.gather_(everyone, source=A)
        A.step(paths[t])
        stopped = (plen <= t) | ended
        ended = ended | (~stopped & A.done.bool())
        applied = torch.where(stopped, applied, torch.full_like(applied, t + 1))
        A.gather_(torch.where(stopped, everyone, torch.full_like(everyone, -1)), source=S)
    same_tensors(A, D, "after the path")
    assert torch.equal(applied, D.gather_length)
    assert int(ended.sum()) >= 1 and int((applied < plen).sum()) >= 1 and int((applied == 0).sum()) >= 1
    for t in (100, 101):
        a = A.rollout_step(t)[-1]
        d = D.rollout_step(t)[-1]
        assert torch.equal(a, d), ("actions", t)
        same_tensors(A, D, ("after launch", t))
    for e in (A, S, D):
        e.close()
    root.close()


# ---- 3. no path ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["c3_centroid", "small_spatial"])
def test_no_path_is_gather(name):
    """path_steps == 0 (an empty paths tensor; no paths tensor and path_len = 0), every path_len = 0 under path_steps > 0,
    and gather_ without the keywords: four twins, bit for bit the same tensors and state blocks."""
    plan, _ = plan_of(name)
    n = plan.n
    root = device_roots(plan.roots)
    mk = lambda: BatchedPlacementEnv(plan.cfg, n, queue_depth=2, run_seed=plan.roots.seed + 1, auto_reset=False, **plan.roots.kw)
    envs = [mk() for _ in range(4)]
    for e in envs:
        e.generate_instances()
        e.reset()
        e.rollout_step(0)  # an episode of its own in progress, a presampled action in the header
    dev = envs[0].device
    idx = np.array(plan.root_of, np.int64)
    idx[5], idx[11] = -1, plan.P + 3
    idx = on(dev, idx)
    zeros = torch.zeros(n, dtype=torch.int32, device=dev)
    envs[0].gather_(idx, source=root.env)
    envs[1].gather_(idx, source=root.env, paths=torch.zeros((0, n, 3), dtype=torch.int32, device=dev))
    envs[2].gather_(idx, source=root.env, path_len=zeros)
    envs[3].gather_(idx, source=root.env, paths=on(dev, plan.path_tensor(fill=gp.NO_ACTION)), path_len=zeros)
    want = state_blob(envs[0])
    for i, e in enumerate(envs[1:], 1):
        same_tensors(envs[0], e, ("twin", i))
        assert _bytes_equal(state_blob(e), want), ("state blocks", i)
        assert not e.gather_length.any()
    assert not hasattr(envs[0], "gather_length")
    with pytest.raises(IndexError):
        envs[1].gather_(idx, source=root.env, path_len=zeros, check=True)
    for e in envs:
        e.close()
    root.close()


# ---- 4. one handle ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["c3_centroid", "spatial_7x100_t256"])
def test_one_handle_with_a_permutation_with_repeats(name):
    """source=None: rows read rows other teams of the same launch overwrite.  The call reads nothing the launch writes:
    the result is that of the same call between two handles."""
    plan, _ = plan_of(name)
    P = plan.P
    root = device_roots(plan.roots)
    one, two = destination(plan, n=P), destination(plan, n=P)
    everyone = np.arange(P, dtype=np.int64)
    for d in (one, two):
        d.gather(everyone, root)
    perm = np.array(([3, 3, 0, 7, 1, -1, 2, 2, 5, 11, 0, 4] if P == 12 else [3, 3, 0, 7, 1, -1, 2, 2])[:P], np.int64)
    paths = [plan.paths[int(r) * K + i % K] if r >= 0 else plan.paths[0] for i, r in enumerate(perm)]
    plen = np.array([len(p) for p in paths], np.int32)
    assert len(set(plen.tolist())) >= 3
    pt = plan.path_tensor(paths, fill=gp.NO_ACTION)
    gather_paths(one, perm, one, pt, plen, (name, "one handle"), check=True)
    gather_paths(two, perm, root, pt, plen, (name, "two handles"), check=True)
    same_tensors(one.env, two.env, name)
    assert torch.equal(one.env.gather_length, two.env.gather_length)
    assert _bytes_equal(state_blob(one.env), state_blob(two.env))
    for r in (one, two, root):
        r.close()


# ---- 5. layouts ---------------------------------------------------------------------------------------------------------
def test_a_trajectory_slot_with_compact_features():
    """num_slots = 3, compact features, slot 2 selected: the slot is written whole, the other slots keep every byte."""
    plan, _ = plan_of("small_spatial")
    root = device_roots(plan.roots)
    dst = destination(plan, num_slots=3, compact_features=True, mask_marginals=True)
    e = dst.env
    dst.step(0)  # slot 1 holds a step of the destination's own
    e.select_slot(2)
    dst.model.select(2)
    whole = lambda: dict({k: v.cpu().numpy() for k, v in e.traj.items()}, reward=e.traj_reward.cpu().numpy(), done=e.traj_done.cpu().numpy(),
                         info=e.traj_info.cpu().numpy(), **{"m_" + k: v.cpu().numpy() for k, v in e.traj_marginals.items()})
    before = whole()
    gather_paths(dst, np.array(plan.root_of, np.int64), root, plan.path_tensor(fill=gp.NO_ACTION), plan.path_len, "slot 2")
    after = whole()
    for k in before:
        for s in (0, 1):
            assert (_same_info if k == "info" else _bytes_equal)(after[k][s], before[k][s]), (k, "slot", s)
    assert any(not _bytes_equal(after[k][2], before[k][2]) for k in e.traj)
    dst.step(1)  # the next slot, from the gathered state: the feature cache was refilled under the destination's tag
    root.close(); dst.close()


def test_an_incremental_destination_stepped_afterwards():
    plan, _ = plan_of("small_spatial")
    root = device_roots(plan.roots)
    dst = destination(plan, incremental_obs=True)
    gather_paths(dst, np.array(plan.root_of, np.int64), root, plan.path_tensor(fill=gp.NO_ACTION), plan.path_len, "incremental")
    for t in (7, 8):
        dst.step(t, fused=(t == 7))
    root.close(); dst.close()


@pytest.mark.parametrize("name, threads", [("c3_both_t256", 64), ("spatial_7x100", 256)])
def test_a_destination_with_another_team_size(name, threads):
    plan, _ = plan_of(name)
    root = device_roots(plan.roots)
    dst = destination(plan, threads_per_env=threads)
    assert dst.env._ccfg.threads_per_env != root.env._ccfg.threads_per_env
    gather_paths(dst, np.array(plan.root_of, np.int64), root, plan.path_tensor(fill=gp.NO_ACTION), plan.path_len, (name, threads), check=True)
    dst.step(3)
    root.close(); dst.close()


# ---- 6. refused and kept rows ------------------------------------------------------------------------------------------
def direct(dst, src, idx, paths, path_len, path_steps, fmt=_lib.ACTION_TUPLE, errors=True, stream=None):
    """pcbenv_gather_paths called directly -> (rc, error word, lengths), the lengths in a guarded buffer of their own."""
    e, dev = dst.env if isinstance(dst, Run) else dst, (dst.env if isinstance(dst, Run) else dst).device
    n = e.num_envs
    back = torch.full((ec.GUARD + 4 * n + ec.GUARD,), ec.SENTINEL, dtype=torch.uint8, device=dev)
    length = back[ec.GUARD:ec.GUARD + 4 * n].view(torch.int32)
    length.fill_(-7)
    err = torch.zeros(1, dtype=torch.int32, device=dev)
    ptr = lambda t: None if t is None else t.data_ptr()
    R = _lib.PcbenvGatherPathsRequest
    req = R(struct_size=C.sizeof(R), action_format=fmt, src=None if src is None else src._h, src_index_dev=ptr(idx), path_actions_dev=ptr(paths),
            path_len_dev=ptr(path_len), path_steps=path_steps, length_dev=ptr(length), errors_dev=ptr(err) if errors else None,
            stream=(e._stream() if stream is None else stream).value)
    rc = e._L.pcbenv_gather_paths(e._h, C.byref(req))
    h = back.cpu().numpy()
    assert (h[:ec.GUARD] == ec.SENTINEL).all() and (h[ec.GUARD + 4 * n:] == ec.SENTINEL).all(), "a guard byte of length_dev was written"
    return rc, int(err.item()), length.cpu().numpy()


@pytest.mark.parametrize("name", ["c3_centroid", "spatial_7x100_t256", "rect_11x10"])
def test_refused_and_kept_rows_keep_every_byte(name):
    """The destination's tensors are views into sentinel-filled, guarded buffers (emission_cases.PlacedAllocator).  Rows
    with -1, an out-of-range index, path_len = -1 and path_len = path_steps + 1 keep every byte, the guards are intact, the
    error word has exactly bits 0 | 1, length = 0 on those rows; everyone else is the oracle's node."""
    plan, nodes = plan_of(name)
    cfg, n = plan.cfg, plan.n
    root = device_roots(plan.roots)
    alloc = ec.PlacedAllocator()
    dst = destination(plan, allocator=alloc)
    dst.step(0)
    dev = dst.env.device
    kept, bad_index, len_lo, len_hi = 4, 7, 21, 33
    idx = np.array(plan.root_of, np.int64)
    idx[kept], idx[bad_index] = -1, plan.P
    plen = plan.path_len.copy()
    plen[len_lo], plen[len_hi] = -1, plan.path_steps + 1
    refused = np.zeros(n, bool)
    refused[[kept, bad_index, len_lo, len_hi]] = True
    paths = plan.path_tensor(fill=gp.NO_ACTION)
    before = alloc.snapshot()
    rdi = (dst.env.reward.cpu().numpy(), dst.env.done.cpu().numpy(), dst.env.info_raw.cpu().numpy())
    rc, err, length = direct(dst, root.env, on(dev, idx), on(dev, paths), on(dev, plen), plan.path_steps)
    assert rc == _lib.PCBENV_OK and err == 3, (rc, err)
    want = on_the_model(dst, idx, root, paths, plen)
    assert not want[refused].any() and not length[refused].any()
    after = alloc.snapshot()
    for k, (front, inner, back) in after.items():
        assert (front == ec.SENTINEL).all() and (back == ec.SENTINEL).all(), (k, "a guard byte was written")
        a, b = alloc.typed(k, inner)[0], alloc.typed(k, before[k][1])[0]
        assert _bytes_equal(a[refused], b[refused]), (k, "a refused or kept row was written")
    r, d, inf = dst.env.reward.cpu().numpy(), dst.env.done.cpu().numpy(), dst.env.info_raw.cpu().numpy()
    assert _bytes_equal(r[refused], rdi[0][refused]) and _bytes_equal(d[refused], rdi[1][refused]) and _same_info(inf[refused], rdi[2][refused])
    # everyone else is the node its path names, and the kept rows still show their own episodes
    dst.compare_oracle("the taken rows are nodes, the others their own episodes")
    check_outputs(dst, want, length, name)
    for i in np.flatnonzero(~refused):
        assert length[i] == nodes[i]["length"], i
    # one bit each, and no error word at all
    plen2 = plan.path_len.copy()
    rc, err, _ = direct(dst, root.env, on(dev, idx), on(dev, paths), on(dev, plen2), plan.path_steps)
    assert rc == _lib.PCBENV_OK and err == 1
    idx2 = np.array(plan.root_of, np.int64)
    rc, err, _ = direct(dst, root.env, on(dev, idx2), on(dev, paths), on(dev, plen), plan.path_steps)
    assert rc == _lib.PCBENV_OK and err == 2
    rc, err, length = direct(dst, root.env, on(dev, idx), on(dev, paths), on(dev, plen), plan.path_steps, errors=False)
    assert rc == _lib.PCBENV_OK and err == 0 and not length[refused].any()
    with pytest.raises(IndexError):
        dst.env.gather_(on(dev, idx2), source=root.env, paths=on(dev, paths), path_len=on(dev, plen), check=True)
    root.close(); dst.close()


def test_state_and_argument_errors():
    """What the CPU test cannot reach: two handles of different definitions, a handle without buffers, a captured stream."""
    plan, _ = plan_of("small_spatial")
    other, _ = plan_of("small_pin")
    a = BatchedPlacementEnv(plan.cfg, 8, queue_depth=1, run_seed=1)
    b = BatchedPlacementEnv(other.cfg, 8, queue_depth=1, run_seed=1)
    for e in (a, b):
        e.generate_instances()
        e.reset()
    dev = a.device
    idx = torch.arange(8, dtype=torch.int32, device=dev)
    rc, _, _ = direct(a, b, idx, None, None, 0)
    assert rc == _lib.PCBENV_EINVAL and "different environment definitions" in a._L.pcbenv_last_error(a._h).decode()
    ccfg = _lib.make_config(plan.cfg, 8)
    h = C.c_void_p()
    _lib.check(a._L.pcbenv_create(C.byref(ccfg), torch.cuda.current_device(), C.byref(h)))
    R = _lib.PcbenvGatherPathsRequest
    req = R(struct_size=C.sizeof(R), src=a._h, src_index_dev=idx.data_ptr(), stream=a._stream().value)
    assert a._L.pcbenv_gather_paths(h, C.byref(req)) == _lib.PCBENV_ESTATE and "pcbenv_bind_buffers" in a._L.pcbenv_last_error(h).decode()
    a._L.pcbenv_destroy(h)
    with pytest.raises(ValueError):
        a.gather_(idx, paths=torch.zeros((2, 7, 3), dtype=torch.int32, device=dev))
    with pytest.raises(ValueError):
        a.gather_(idx, path_len=torch.zeros(7, dtype=torch.int32, device=dev))
    paths = torch.zeros((1, 8, 3), dtype=torch.int32, device=dev)
    a.gather_(idx, paths=paths)
    torch.cuda.synchronize()
    scratch = torch.zeros(4, device=dev)
    scratch.add_(1.0)  # loaded before the capture
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        scratch.add_(1.0)
        req = R(struct_size=C.sizeof(R), src_index_dev=idx.data_ptr(), path_actions_dev=paths.data_ptr(), path_steps=1, stream=a._stream().value)
        rc = a._L.pcbenv_gather_paths(a._h, C.byref(req))
        msg = a._L.pcbenv_last_error(a._h).decode()
    assert rc == _lib.PCBENV_ESTATE and "pcbenv_gather_paths cannot be captured" in msg
    a.gather_(idx, paths=paths)  # the handle works on
    assert int(a.gather_length.max()) == 1
    a.close(); b.close()


# ---- 7. the flat format -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["c3_centroid", "spatial_7x100"])
def test_the_flat_format_equals_the_tuple_format(name):
    """... including flat values out of range (negative, O*H*W, far beyond): no such action, a terminal transition."""
    plan, _ = plan_of(name)
    cfg, n = plan.cfg, plan.n
    A = cfg.num_orientations * cfg.height * cfg.width
    flat = plan.flat(plan.path_tensor())
    out = [i for i in range(n) if i % K == 4]                      # their second action is illegal anyway: now it is no action
    first = [i for i in range(n) if i % K == 3 and i % 2]          # and some paths start with one
    for c, i in enumerate(out):
        flat[1, i] = (-3, A, A + 12345)[c % 3]
    for c, i in enumerate(first):
        flat[0, i] = (A, -1, 2 ** 31 - 1)[c % 3]
    tuples = gp.decode_flat_paths(cfg, flat)
    root = device_roots(plan.roots)
    d1, d2 = destination(plan), destination(plan)
    idx = np.array(plan.root_of, np.int64)
    l1 = gather_paths(d1, idx, root, tuples, plan.path_len, (name, "tuple"))
    l2 = gather_paths(d2, idx, root, tuples, plan.path_len, (name, "flat"), flat=flat)
    assert np.array_equal(l1, l2) and all(l1[i] == 1 for i in first) and all(1 <= l1[i] <= 2 for i in out) and any(l1[i] == 2 for i in out)
    same_tensors(d1.env, d2.env, name)
    assert _bytes_equal(state_blob(d1.env), state_blob(d2.env))
    for r in (root, d1, d2):
        r.close()


# ---- 8. the stream ------------------------------------------------------------------------------------------------------
def test_side_stream():
    """One call on a non-blocking side stream behind a delay: it returns before the stream reaches it, runs on that stream
    (its inputs are wrong until the stream has passed the delay), and the result is the default-stream result."""
    plan, _ = plan_of("c3_centroid")
    n = plan.n
    root = device_roots(plan.roots)
    want, got = destination(plan), destination(plan)
    dev = got.env.device
    idx = np.array(plan.root_of, np.int64)
    paths = plan.path_tensor(fill=gp.NO_ACTION)
    gather_paths(want, idx, root, paths, plan.path_len, "default stream")
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    good = (on(dev, idx), on(dev, paths), on(dev, plan.path_len))
    with lagged(side) as before:
        live = tuple(torch.full_like(t, -1) for t in good)  # kept rows, no action, a refused length: wrong until the copies below run
        got.env.gather_(live[0], source=root.env, paths=live[1], path_len=torch.zeros_like(live[2]))  # once without a delay: the wrapper's buffers exist on this stream
        side.synchronize()
        before()
        reached = torch.cuda.Event()
        reached.record(side)
        for t, g in zip(live, good):
            t.copy_(g, non_blocking=True)  # on the side stream, behind the delay: a launch on any other stream reads -1
        t0 = time.perf_counter()
        got.env.gather_(live[0], source=root.env, paths=live[1], path_len=live[2])
        dt = 1e3 * (time.perf_counter() - t0)
        ev = torch.cuda.Event()
        ev.record(side)
        assert not reached.query(), f"pcbenv_gather_paths returned only after the stream had passed a {LAG_MS} ms delay ({dt:.2f} ms on the host)"
        assert not ev.query()
        side.synchronize()
    same_tensors(want.env, got.env, "side stream")
    assert torch.equal(want.env.gather_length, got.env.gather_length) and int(got.env.gather_length.max()) >= 2
    for r in (root, want, got):
        r.close()


# ---- 9. the whole stack -------------------------------------------------------------------------------------------------
def test_tree_search_with_a_constant_policy_is_the_uniform_search():
    """Constant logits draw bit for bit what pcbenv_sample_actions draws under the same (seed, environment, step) keys:
    tree_search and tree_search_device with policy_backend(zeros) are tree_search with the uniform playouts, field by field."""
    cfg = pc.case("small_pin")[0]()
    P, M, S0 = 8, 12, 500
    root = BatchedPlacementEnv(cfg, P, queue_depth=2, run_seed=5)
    planner = BatchedPlacementEnv(cfg, P, queue_depth=1, run_seed=5, auto_reset=False)
    for e in (root, planner):
        e.generate_instances()
        e.reset()
    root.rollout_step(0)
    zeros = torch.zeros((P, cfg.num_orientations * cfg.height * cfg.width), dtype=torch.float32, device=root.device)
    calls = [0]

    def logits_fn(obs):
        assert set(obs) == set(planner.obs)
        calls[0] += 1
        return zeros
    backend = policy_backend(root, planner, logits_fn)
    before = tensors(root)
    want = tree_search(root, M, S0)
    got = tree_search(root, M, S0, backend=backend)
    T = cfg.max_num_components
    assert calls[0] == M * T
    dev_got = tree_search_device(root, M, S0, backend=backend)
    for f in want.__dataclass_fields__:
        a, b, c = getattr(want, f), getattr(got, f), getattr(dev_got, f)
        assert a.dtype == b.dtype and torch.equal(a, b), f
        assert torch.equal(a.to(c.dtype), c), ("tree_search_device", f)
    # some tree grew a node per iteration: with four children per node at most it is deeper than two plies, so paths of
    # two steps and more were materialised (a root whose episode ends with its first transition keeps a tree of two nodes)
    assert int(dev_got.errors) == 0 and int(want.num_nodes.max()) == M + 1 and int(want.depth.max()) >= 2
    after = tensors(root)
    assert all(_bytes_equal(before[k], after[k]) for k in before)
    root.close(); planner.close()
