"""pcbenv_sample_axis on the GPU: one stage of a factorised policy against the float64 restatement of its contract
(tests/factor_contract.py) -- the uniform pick for constant logits, the inverse CDF, log-probability, entropy and the
greedy pick for random ones -- chains of stages ending on legal actions, whole policy loops against the CPU oracle, the
error cases that are data, and: it writes nothing the library owns."""
import ctypes as C

import numpy as np
import pytest
import torch

import factor_contract as fc
import logits_cases as lc
from axis_cases import CASES, CONFIGS, SEED, GridEncoder, as_read, dense_of, episode_steps, host_dist, legal_sets, make_env, sizes
from pcbenv import EnvConfig, _lib, named_config
from pcbenv.factorised import ORDERS, FactorisedPolicy
from pcbenv.rollout import collect, masked_logits

pytestmark = pytest.mark.gpu

SENTINEL = -77
DTYPES = (torch.float32, torch.bfloat16)


def _fresh_actions(env):
    return torch.full((env.num_envs, 3), SENTINEL, dtype=torch.int32, device=env.device)


def _untouched(before, after, axis):
    keep = [c for c in range(3) if c != axis]
    return torch.equal(before[:, keep], after[:, keep])


def _composed_legal(dense, actions):
    a = actions.cpu().numpy()
    has = dense.reshape(len(dense), -1).any(1)
    rows = np.flatnonzero(has)
    return dense[rows, a[rows, 0], a[rows, 1], a[rows, 2]].all() and (a[~has] == 0).all()


@pytest.mark.parametrize("name, B", CASES)
def test_constant_logits_draw_the_uniform_pick(name, B):
    cfg = CONFIGS[name]()
    env = make_env(cfg, B, first_env_index=5)
    for t in range(episode_steps(cfg)):
        dense = dense_of(env)
        for k, order in enumerate(fc.ALL_ORDERS):
            for dtype in DTYPES:
                actions = _fresh_actions(env)
                for axis, given in fc.stages_of(order):
                    logits = torch.full((B, sizes(cfg)[axis]), (0.0, 3.25)[(t + k) & 1], dtype=dtype, device=env.device)
                    before = actions.clone()
                    lp, ent = env.sample_axis(axis, logits, t, actions, given, check=True)
                    assert _untouched(before, actions, axis), (name, t, order, axis)
                    L, ok = legal_sets(dense, axis, given, before.cpu().numpy())
                    assert ok.all()
                    want = [fc.uniform_pick(L[e], fc.hi32_axis(SEED, 5 + e, t, axis)) for e in range(B)]
                    assert actions[:, axis].cpu().tolist() == want, (name, t, order, axis, dtype)
                    n = L.sum(1)
                    has = n > 0
                    lp, ent = lp.cpu().numpy().astype(np.float64), ent.cpu().numpy().astype(np.float64)
                    np.testing.assert_allclose(lp[has], -np.log(n[has]), rtol=1e-6)
                    np.testing.assert_allclose(ent[has], np.log(n[has]), rtol=1e-6)
                    assert not lp[~has].any() and not ent[~has].any()
                assert _composed_legal(dense, actions), (name, t, order)
        env.step(actions)
        env.reset_done()
    env.close()


@pytest.mark.parametrize("name, B", CASES)
def test_random_logits_on_the_inverse_cdf_and_greedy(name, B):
    cfg = CONFIGS[name]()
    env = make_env(cfg, B, first_env_index=11)
    rng = np.random.RandomState(3)
    rows = np.arange(B)
    reference_orders = [tuple(axis for axis, _ in stages) for stages in ORDERS.values()]
    for t in range(episode_steps(cfg)):
        dense = dense_of(env)
        # both reference orders every step (the last one's action is stepped), the other four in turn
        orders = [fc.ALL_ORDERS[t % 6]] + reference_orders[::-1 if t & 1 else 1]
        for k, order in enumerate(orders):
            dtype = DTYPES[(t + k) & 1] if k == 0 else None
            for dt in ((dtype,) if dtype is not None else DTYPES):
                actions = _fresh_actions(env)
                for axis, given in fc.stages_of(order):
                    before = actions.clone()
                    L, ok = legal_sets(dense, axis, given, before.cpu().numpy())
                    has = L.any(1)
                    dev, l = as_read(lc.tame(rng, L), dt, env.device)      # logits are drawn after L is known
                    lp, ent = env.sample_axis(axis, dev, t, actions, given, check=True)
                    assert _untouched(before, actions, axis)
                    v = actions[:, axis].cpu().numpy()
                    assert L[has, v[has]].all() and (v[~has] == 0).all(), (name, t, order, axis, dt)
                    M, Z, Cp, H = host_dist(l, L)
                    for e in np.flatnonzero(has):
                        u = fc.u_axis(SEED, 11 + e, t, axis)
                        lo = Cp[e, v[e] - 1] if v[e] > 0 else 0.0
                        assert lo - 3e-5 <= u <= Cp[e, v[e]] + 3e-5, (name, t, order, axis, dt, e, lo, u, Cp[e, v[e]])
                        assert l[e, v[e]] > -np.inf  # never a value of weight 0
                    np.testing.assert_allclose(lp.cpu().numpy()[has], (l[rows, v] - M - np.log(Z))[has], atol=1e-4, rtol=0)
                    np.testing.assert_allclose(ent.cpu().numpy()[has], H[has], atol=1e-4, rtol=0)
                    assert not lp.cpu().numpy()[~has].any() and not ent.cpu().numpy()[~has].any()
                    # greedy: the lowest masked argmax; four-valued logits tie everywhere
                    qdev, q = as_read(rng.randint(0, 4, size=L.shape).astype(np.float32), dt, env.device)
                    greedy_actions = before.clone()
                    glp, gent = env.sample_axis(axis, qdev, t, greedy_actions, given, greedy=True, check=True)
                    gv = greedy_actions[:, axis].cpu().numpy()
                    want = np.argmax(np.where(L, q, -np.inf), axis=1)
                    assert np.array_equal(gv[has], want[has]) and (gv[~has] == 0).all(), (name, t, order, axis, dt)
                    for e in np.flatnonzero(has)[:3]:
                        assert gv[e] == fc.greedy(q[e], L[e])
                    _, gZ, _, gH = host_dist(q, L)
                    np.testing.assert_allclose(glp.cpu().numpy()[has], -np.log(gZ[has]), atol=1e-4, rtol=0)
                    np.testing.assert_allclose(gent.cpu().numpy()[has], gH[has], atol=1e-4, rtol=0)
                # chain legality: the composed action is set in action_mask
                assert _composed_legal(dense, actions), (name, t, order)
        env.step(actions)
        env.reset_done()
    env.close()


@pytest.mark.parametrize("name", ["rect_6x6", "square_5x5", "c3", "spatial_7x100", "c5"])
def test_raw_masked_and_nan_logits_agree(name):
    cfg = CONFIGS[name]()
    B = 32
    env = make_env(cfg, B)
    rng = np.random.RandomState(5)
    for t in range(4):
        dense = dense_of(env)
        for order in ORDERS.values():
            for dtype in DTYPES:
                actions = _fresh_actions(env)
                for axis, given in order:
                    L, _ = legal_sets(dense, axis, given, actions.cpu().numpy())
                    Lt = torch.from_numpy(L).to(env.device)
                    raw = torch.from_numpy((rng.randn(B, sizes(cfg)[axis]) * 2).astype(np.float32)).to(env.device).to(dtype)
                    nan = raw.clone()
                    nan[~Lt] = float("nan")
                    for greedy in (False, True):
                        ref_a = actions.clone()
                        ref = env.sample_axis(axis, raw, t, ref_a, given, greedy=greedy, check=True)
                        for other in (masked_logits(raw, Lt).contiguous(), nan):
                            got_a = actions.clone()
                            got = env.sample_axis(axis, other, t, got_a, given, greedy=greedy, check=True)  # no error bit
                            assert torch.equal(ref_a, got_a), (name, t, axis, dtype, greedy)
                            for x, y in zip(ref, got):
                                assert torch.equal(x, y), (name, t, axis, dtype, greedy)
                    env.sample_axis(axis, raw, t, actions, given)
        env.step(actions)
        env.reset_done()
    env.close()


def _raw_sample(env, axis, given, logits, t, actions, greedy=False, first_env=0):
    """Straight through the C ABI -> (log_prob, entropy, error bits)."""
    B = env.num_envs
    lp = torch.empty(B, dtype=torch.float32, device=env.device)
    ent = torch.empty(B, dtype=torch.float32, device=env.device)
    err = torch.zeros(1, dtype=torch.int32, device=env.device)
    _lib.check(env._L.pcbenv_sample_axis(env._h, axis, fc.given_bits(given), logits.data_ptr(), _lib.LOGITS_F32,
                                         _lib.DRAW_GREEDY if greedy else _lib.DRAW_SAMPLE, actions.data_ptr(), lp.data_ptr(),
                                         ent.data_ptr(), err.data_ptr(), SEED, first_env, t, env._stream()), env._h)
    return lp, ent, int(err.item())


@pytest.mark.parametrize("bad, bit", [(-np.inf, 2), (np.nan, 1), (np.inf, 1), ("given", 8)])
def test_error_cases_are_data(bad, bit):
    cfg = named_config("c3")
    B, k, t = 8, 3, 4
    env = make_env(cfg, B, first_env_index=2)
    env.step(env.sample_actions(0))
    dense = dense_of(env)
    rng = np.random.RandomState(9)
    for stages in ORDERS.values():
        # a legal triple per environment feeds the given columns of every stage
        base_actions = torch.from_numpy(np.stack([np.argwhere(dense[e])[rng.randint(dense[e].sum())] for e in range(B)]).astype(np.int32)).to(env.device)
        for axis, given in stages:
            if bad == "given" and not given:
                continue
            hurt_actions = base_actions.clone()
            if bad == "given":
                hurt_actions[k, given[-1]] = sizes(cfg)[given[-1]] if axis != 1 else -1
            L, ok = legal_sets(dense, axis, given, hurt_actions.cpu().numpy())
            base = lc.tame(rng, L)
            hurt = base.copy()
            n = int(L[k].sum())
            if bad == -np.inf:
                hurt[k, L[k]] = -np.inf
            elif bad != "given":
                hurt[k, np.flatnonzero(L[k])[-1]] = bad
            others = [i for i in range(B) if i != k]
            for greedy in (False, True):
                ok_a = base_actions.clone()
                ok_lp, ok_ent = env.sample_axis(axis, torch.from_numpy(base).to(env.device), t, ok_a, given, greedy=greedy, check=True)
                a = hurt_actions.clone()
                logits = torch.from_numpy(hurt).to(env.device)
                lp, ent, err = _raw_sample(env, axis, given, logits, t, a, greedy, first_env=2)
                assert err == bit, (axis, given, greedy)
                if bad == "given":
                    assert not ok[k] and a[k, axis].item() == 0 and lp[k].item() == 0 and ent[k].item() == 0
                else:
                    assert a[k, axis].item() == fc.uniform_pick(L[k], fc.hi32_axis(SEED, 2 + k, t, axis))  # in both modes
                    assert lp[k].item() == pytest.approx(-np.log(n), rel=1e-6) and ent[k].item() == pytest.approx(np.log(n), rel=1e-6)
                assert torch.equal(a[others], ok_a[others]) and torch.equal(lp[others], ok_lp[others]) and torch.equal(ent[others], ok_ent[others])
                with pytest.raises(FloatingPointError):
                    env.sample_axis(axis, logits, t, hurt_actions.clone(), given, greedy=greedy, check=True)
    env.close()


def test_empty_legal_set():
    """A crowded grid whose episodes end because the next component has no legal cell: without a reset the mask stays
    empty.  Value 0, log_prob = entropy = 0, no error bit; the other environments are drawn as usual.  Also a given
    combination without a legal completion."""
    cfg = EnvConfig.spatial(12, 12, 5, 5, 2, 5, 2, 5, 8, 8, 3, 5, 7, 2, "centroid", 2, 0.5)
    B = 64
    env = make_env(cfg, B)
    for t in range(12):
        dense = dense_of(env)
        if (~dense.reshape(B, -1).any(1)).any():
            break
        env.step(env.sample_actions(t))
    empty = ~dense.reshape(B, -1).any(1)
    assert empty.any() and (~empty).any()
    rng = np.random.RandomState(8)
    for stages in ORDERS.values():
        for greedy in (False, True):
            actions = _fresh_actions(env)
            for axis, given in stages:
                L, _ = legal_sets(dense, axis, given, actions.cpu().numpy())
                assert not L[empty].any()
                lp, ent = env.sample_axis(axis, torch.from_numpy(lc.tame(rng, L)).to(env.device), 3, actions, given, greedy=greedy, check=True)
                assert not actions.cpu().numpy()[empty, axis].any() and not lp.cpu().numpy()[empty].any() and not ent.cpu().numpy()[empty].any()
            assert _composed_legal(dense, actions)
    # no legal completion: y given an x whose row is closed in every plane
    live = np.flatnonzero(~empty)
    closed = [(e, x) for e in live for x in range(cfg.height) if not dense[e, :, x].any()]
    assert closed
    actions = torch.zeros((B, 3), dtype=torch.int32, device=env.device)
    for e, x in closed:
        actions[e, 1] = int(x)
    L, ok = legal_sets(dense, 2, (1,), actions.cpu().numpy())
    lp, ent = env.sample_axis(2, torch.from_numpy(lc.tame(rng, L)).to(env.device), 3, actions, (1,), check=True)
    rows = sorted({int(e) for e, _ in closed})
    assert ok.all() and not L[rows].any()
    assert not actions.cpu().numpy()[rows, 2].any() and not lp.cpu().numpy()[rows].any() and not ent.cpu().numpy()[rows].any()
    env.close()


def _obs_equal(a, b):
    for k in a.obs:
        assert torch.equal(a.obs[k], b.obs[k]), k
    assert torch.equal(a.reward, b.reward) and torch.equal(a.done, b.done)
    assert torch.equal(a.info_raw.nan_to_num(7.0), b.info_raw.nan_to_num(7.0))


@pytest.mark.parametrize("name", ["c3", "c4"])
def test_writes_nothing_the_library_owns(name):
    """Interleave step, chains of sample_axis, gather_ (a permutation), reset(mask) and set_state: every chain ends on a
    legal action, and every step (the fused sampler's included) is bit-identical to a twin that never called
    sample_axis."""
    cfg = named_config(name)
    B = 32
    envs = [make_env(cfg, B, queue_depth=3, auto_reset=False) for _ in range(2)]
    me, twin = envs
    rng = np.random.RandomState(10)
    gen = torch.Generator(device=me.device).manual_seed(1)
    orders = list(ORDERS.values())

    def draw(t):
        dense = dense_of(me)
        for greedy in (False, True):
            actions = _fresh_actions(me)
            for axis, given in orders[(t + greedy) & 1]:
                logits = torch.randn((B, sizes(cfg)[axis]), generator=gen, device=me.device) * 2
                me.sample_axis(axis, logits, t, actions, given, greedy=greedy, check=True)
            assert _composed_legal(dense, actions)
        return actions
    snap = None
    for t in range(24):
        a = draw(t)
        if t % 3 == 0:
            for e in envs:
                e.step(a)
        else:  # the fused sampler: its presampled action must survive the call
            outs = [e.rollout_step(t)[4] for e in envs]
            assert torch.equal(outs[0], outs[1])
        _obs_equal(me, twin)
        draw(t + 1000)
        if t == 5:
            idx = torch.from_numpy(rng.permutation(B).astype(np.int32))
            for e in envs:
                e.gather_(idx)
        if t == 9:
            snap = [e.state_dict() for e in envs]
        if t == 14:
            for e, s in zip(envs, snap):
                e.load_state_dict(s)
        m = torch.from_numpy((rng.rand(B) < 0.2).astype(np.uint8))
        for e in envs:
            e.reset_done()
            e.reset(m)
        draw(t + 2000)
        _obs_equal(me, twin)
    for e in envs:
        e.close()


@pytest.mark.parametrize("name, B, order", [("c3", 256, "orientation"), ("c4", 128, "coordinates")])
def test_policy_loop_against_the_oracle(name, B, order):
    """rollout.collect(factorised_policy=...) on the trajectory layout with auto_reset for two episodes; the recorded
    actions replayed on the CPU oracle: every tensor of every step bit-equal."""
    from test_gather_gpu import Run, _bytes_equal
    cfg = named_config(name)
    r = Run(cfg, B, run_seed=SEED, queue_depth=3, num_slots=2, auto_reset=True)
    env = r.env
    torch.manual_seed(2)
    policy = FactorisedPolicy(GridEncoder(cfg), cfg, order).to(env.device)
    with torch.no_grad():
        for h in policy.heads.heads:
            h.weight.mul_(20.0)  # logits a few units apart
    for t in range(2 * cfg.max_num_components + 1):
        dense = dense_of(env)
        env.select_slot(t + 1)
        tr = collect(env, 1, factorised_policy=policy, t0=t)
        assert _composed_legal(dense, tr.actions[0])
        assert tr.log_prob.shape == tr.entropy.shape == (1, B)
        assert torch.isfinite(tr.log_prob).all() and (tr.log_prob <= 0).all() and (tr.entropy >= 0).all()
        a = tr.actions[0].cpu().numpy()
        rr, dd, ii = r.ob.step(a)
        r.last_done = dd.copy()
        r.oracle_reset(dd)
        assert np.array_equal(tr.dones[0].cpu().numpy(), dd), t
        assert _bytes_equal(tr.rewards[0].cpu().numpy(), rr), t
        inf = tr.info[0].cpu().numpy()
        has_info = ~np.isnan(inf[:, 0])
        assert _bytes_equal(inf[has_info], ii[has_info]), t
        r.compare_oracle(("step", t))
    assert r.cursor.min() >= 3  # two episodes done everywhere
    r.close()


def test_refused_without_bound_buffers_and_under_capture():
    cfg = named_config("c3")
    B = 16
    L = _lib.load()
    logits = torch.zeros((B, cfg.num_orientations), dtype=torch.float32, device="cuda")
    actions = torch.zeros((B, 3), dtype=torch.int32, device="cuda")

    def call(handle, stream):
        return L.pcbenv_sample_axis(handle, 0, 0, logits.data_ptr(), _lib.LOGITS_F32, _lib.DRAW_SAMPLE, actions.data_ptr(),
                                    None, None, None, SEED, 0, 0, stream)
    ccfg = _lib.make_config(cfg, B)
    h = C.c_void_p()
    _lib.check(L.pcbenv_create(C.byref(ccfg), torch.cuda.current_device(), C.byref(h)))
    assert call(h, None) == _lib.PCBENV_ESTATE
    assert "pcbenv_bind_buffers" in L.pcbenv_last_error(h).decode()
    L.pcbenv_destroy(h)
    env = make_env(cfg, B)
    assert call(env._h, env._stream()) == _lib.PCBENV_OK
    torch.cuda.synchronize()
    scratch = torch.zeros(4, device="cuda")
    scratch.add_(1.0)  # loaded before the capture
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        scratch.add_(1.0)
        rc = call(env._h, env._stream())
        msg = L.pcbenv_last_error(env._h).decode()
    assert rc == _lib.PCBENV_ESTATE and "captured" in msg
    env.step(env.sample_actions(0))  # the handle works on
    env.close()


def test_a_handle_named_without_an_index_lives_on_the_current_device():
    """`device="cuda"` is resolved once, at creation: `env.device` carries the index, and tensors made with `env.device`
    or with "cuda" are accepted and give what a handle made with the explicit index gives, bit for bit."""
    cfg, B = CONFIGS["rect_6x6"](), 2
    O, H, W = sizes(cfg)
    here = torch.device("cuda", torch.cuda.current_device())
    rng = np.random.RandomState(3)
    flat, row = rng.randn(B, O * H * W).astype(np.float32), rng.randn(B, O).astype(np.float32)

    def run(env, device):
        on = lambda a: torch.from_numpy(a).to(device)
        bits = env.mask_bits(out=torch.empty((B, 2, H, (W + 63) // 64), dtype=torch.int64, device=device))
        actions, lp, ent = env.sample_logits(on(flat), 0)
        staged = torch.zeros((B, 3), dtype=torch.int32, device=device)
        out = [bits, actions, lp, ent, *env.sample_axis(0, on(row), 0, staged), staged]
        out += env.evaluate_logits(on(flat), bits, actions)
        out += env.evaluate_axis_forward(0, (), on(row), bits, staged)
        return [t.cpu() for t in out]
    want = None
    for name in ("cuda", str(here)):
        env = make_env(cfg, B, device=name)
        assert env.device == here
        for device in (env.device, "cuda"):
            got = run(env, device)
            want = want or got
            assert len(got) == len(want) == 11 and all(torch.equal(a, b) for a, b in zip(got, want)), (name, device)
        env.close()
