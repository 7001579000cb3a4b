"""pcbenv_sample_logits on the GPU: the masked categorical draw from policy logits against the float64 restatement of
its contract (tests/sampling_contract.py), against the uniform sampler it reduces to for constant logits, against
torch's masked argmax, and against the CPU oracle for whole policy loops.  Also: it writes nothing the library owns."""
import numpy as np
import pytest
import torch

import sampling_contract as sc
from logits_cases import RAGGED, SAMPLER_RAGGED
from pcbenv import EnvConfig, _lib, named_config
from pcbenv.batched_env import BatchedPlacementEnv
from pcbenv.config import KIND_SQUARE
from pcbenv.rollout import collect, masked_logits

pytestmark = pytest.mark.gpu

CONFIGS = {"c1": lambda: named_config("c1"), "c2": lambda: named_config("c2"), "c3": lambda: named_config("c3"),
           "c4": lambda: named_config("c4"), "c5": lambda: named_config("c5"),
           "rect_6x6": lambda: EnvConfig.rect(6, 6, 2, 4, 2, 4, 4, 2), "square_5x5": lambda: EnvConfig.square(5, 5, 2)}
# ragged grids (H != W, a partial second mask word, one load per logit with one and with four wavefronts): whole episodes
CONFIGS.update({name: RAGGED[name] for name in SAMPLER_RAGGED})
SEED = 7


def _env(cfg, B, **kw):
    env = BatchedPlacementEnv(cfg, B, queue_depth=kw.pop("queue_depth", 2), run_seed=SEED, **kw)
    env.generate_instances()
    env.reset()
    return env


def _A(cfg):
    return cfg.num_orientations * cfg.height * cfg.width


def _legal(env):
    """bool [B, A] from the bit rows, checked against the action_mask tensor."""
    cfg, B = env.cfg, env.num_envs
    bits = env.mask_bits().cpu().numpy().view(np.uint64)
    legal = np.stack([sc.legal_flat(bits[e], cfg.num_orientations, cfg.height, cfg.width) for e in range(B)])
    assert np.array_equal(legal, env.action_mask.reshape(B, -1).cpu().numpy().astype(bool))
    return legal


def _flat(env, a):
    a = a.cpu().numpy().astype(np.int64)
    if a.ndim == 1:
        return a
    H, W = env.cfg.height, env.cfg.width
    return a[:, 0] * H * W + a[:, 1] * W + a[:, 2]


def _host_dist(l, legal):
    """Vectorised float64 restatement: (M, Z, prefix C / Z [B, A], entropy [B])."""
    with np.errstate(all="ignore"):  # rows without a legal action are not compared
        lm = np.where(legal, l, -np.inf)
        M = lm.max(1, keepdims=True)
        live = legal & (lm > -np.inf)
        w = np.where(live, np.exp(np.where(live, lm - M, 0.0)), 0.0)
        Z = w.sum(1, keepdims=True)
        ent = np.log(Z[:, 0]) - np.where(live, w / Z * np.where(live, lm - M, 0.0), 0.0).sum(1)
        return M[:, 0], Z[:, 0], np.cumsum(w, 1) / Z, ent


def _episode(env, steps, body):
    for t in range(steps):
        a = body(t)
        env.step(a)
        env.reset_done()


@pytest.mark.parametrize("name", list(CONFIGS))
def test_constant_logits_equal_the_uniform_sampler(name):
    cfg = CONFIGS[name]()
    B = 32 if name == "c5" else 64
    env = _env(cfg, B, first_env_index=5)
    A = _A(cfg)
    steps = (cfg.max_num_components if cfg.kind != KIND_SQUARE else 6) + 3

    def body(t):
        flat = bool(t & 1)
        want = env.sample_actions(t, flat=flat)
        n = _legal(env).sum(1)
        for dtype in (torch.float32, torch.bfloat16):
            for value in (0.0, 3.25):
                logits = torch.full((B, A), value, dtype=dtype, device=env.device)
                a, lp, ent = env.sample_logits(logits, t, flat=flat, check=True)
                assert torch.equal(a, want), (name, t, dtype, value)
                has = n > 0
                lp, ent = lp.cpu().numpy().astype(np.float64), ent.cpu().numpy().astype(np.float64)
                np.testing.assert_allclose(lp[has], -np.log(n[has]), rtol=1e-6)
                np.testing.assert_allclose(ent[has], np.log(n[has]), rtol=1e-6)
                assert not lp[~has].any() and not ent[~has].any()
        return want
    _episode(env, steps, body)
    env.close()


def _random_logits(rng, legal, scale=3.0, p_neg_inf=0.05):
    B, A = legal.shape
    l = (rng.randn(B, A) * scale).astype(np.float32)
    l[rng.rand(B, A) < p_neg_inf] = -np.inf
    for e in range(B):  # keep one finite legal logit: every legal logit -inf is the error case, tested below
        idx = np.flatnonzero(legal[e])
        if idx.size and not np.isfinite(l[e, idx]).any():
            l[e, idx[0]] = 0.0
    return l


@pytest.mark.parametrize("name", list(CONFIGS))
def test_legal_and_on_the_inverse_cdf(name):
    cfg = CONFIGS[name]()
    B = 32 if name == "c5" else 64
    env = _env(cfg, B, first_env_index=11)
    rng = np.random.RandomState(3)
    steps = (cfg.max_num_components if cfg.kind != KIND_SQUARE else 6) + 3

    def body(t):
        legal = _legal(env)
        l32 = _random_logits(rng, legal)
        out = None
        for k, dtype in enumerate((torch.float32, torch.bfloat16)):
            dev = torch.from_numpy(l32).to(env.device).to(dtype)
            flat = bool((t + k) & 1)
            a, lp, ent = env.sample_logits(dev, t, flat=flat, check=True)
            fa = _flat(env, a)
            l = dev.float().cpu().numpy().astype(np.float64)  # what the kernel read
            has = legal.any(1)
            assert legal[has, fa[has]].all() and (fa[~has] == 0).all(), (name, t, dtype)
            M, Z, C, H = _host_dist(l, legal)
            for e in np.flatnonzero(has):
                u = sc.u_of(SEED, 11 + e, t)
                lo = C[e, fa[e] - 1] if fa[e] > 0 else 0.0
                assert lo - 3e-5 <= u <= C[e, fa[e]] + 3e-5, (name, t, dtype, e, lo, u, C[e, fa[e]])
            want_lp = l[np.arange(B), fa] - M - np.log(Z)
            np.testing.assert_allclose(lp.cpu().numpy()[has], want_lp[has], atol=1e-4, rtol=0)
            np.testing.assert_allclose(ent.cpu().numpy()[has], H[has], atol=1e-4, rtol=0)
            out = a if not flat else None
        return out if out is not None else env.sample_actions(t)
    _episode(env, steps, body)
    env.close()


@pytest.mark.parametrize("name", list(CONFIGS))
def test_greedy_equals_the_masked_argmax(name):
    cfg = CONFIGS[name]()
    B = 32 if name == "c5" else 64
    env = _env(cfg, B)
    rng = np.random.RandomState(4)
    steps = (cfg.max_num_components if cfg.kind != KIND_SQUARE else 6) + 3

    def body(t):
        legal = _legal(env)
        q = rng.randint(0, 4, size=legal.shape).astype(np.float32)  # four values: ties everywhere
        for dtype in (torch.float32, torch.bfloat16):
            for raw in (q, (rng.randn(*legal.shape) * 3).astype(np.float32)):
                dev = torch.from_numpy(raw).to(env.device).to(dtype)
                a, lp, ent = env.sample_logits(dev, t, greedy=True, flat=True, check=True)
                has = legal.any(1)
                want = torch.argmax(masked_logits(dev, env.action_mask), dim=1).cpu().numpy()
                got = a.cpu().numpy()
                assert np.array_equal(got[has], want[has]), (name, t, dtype)
                l = dev.float().cpu().numpy().astype(np.float64)
                for e in np.flatnonzero(has)[:4]:
                    assert got[e] == sc.greedy(l[e], legal[e])
                M, Z, _, H = _host_dist(l, legal)
                np.testing.assert_allclose(lp.cpu().numpy()[has], -np.log(Z[has]), atol=1e-4, rtol=0)
                np.testing.assert_allclose(ent.cpu().numpy()[has], H[has], atol=1e-4, rtol=0)
        return env.sample_actions(t)
    _episode(env, steps, body)
    env.close()


@pytest.mark.parametrize("name", ["c2", "c3", "c5", "square_5x5", "rect_6x6"])
def test_masked_and_unmasked_logits_agree(name):
    cfg = CONFIGS[name]()
    B = 32
    env = _env(cfg, B)
    rng = np.random.RandomState(5)
    for t in range(4):
        legal = _legal(env)
        for dtype in (torch.float32, torch.bfloat16):
            raw = torch.from_numpy((rng.randn(B, _A(cfg)) * 2).astype(np.float32)).to(env.device).to(dtype)
            nan = raw.clone()
            nan[~torch.from_numpy(legal).to(env.device)] = float("nan")
            for greedy in (False, True):
                ref = env.sample_logits(raw, t, greedy=greedy, check=True)
                for other in (masked_logits(raw, env.action_mask).contiguous(), nan):
                    got = env.sample_logits(other, t, greedy=greedy, check=True)  # NaN on illegal entries: no error bit
                    for x, y in zip(ref, got):
                        assert torch.equal(x, y), (name, t, dtype, greedy)
        env.step(env.sample_actions(t))
        env.reset_done()
    env.close()


def _chi2_sf(stat, df):
    return float(torch.special.gammaincc(torch.tensor(df / 2.0, dtype=torch.float64), torch.tensor(stat / 2.0, dtype=torch.float64)))


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_distribution_chi_square(dtype):
    cfg = named_config("c1")
    B = 4096
    env = _env(cfg, B)
    legal = _legal(env)
    assert (legal == legal[0]).all()  # right after reset every environment shows the same mask
    rng = np.random.RandomState(6)
    row = (rng.randn(_A(cfg)) * 1.5).astype(np.float32)
    logits = torch.from_numpy(row).to(env.device).to(dtype).expand(B, -1).contiguous()
    counts = np.zeros(_A(cfg), np.int64)
    for step in range(16):
        a, _, _ = env.sample_logits(logits, step, flat=True, check=True)
        counts += np.bincount(a.cpu().numpy(), minlength=_A(cfg))
    assert counts[~legal[0]].sum() == 0
    l = logits[0].float().cpu().numpy().astype(np.float64)
    p = np.where(legal[0], np.exp(l - l[legal[0]].max()), 0.0)
    p /= p.sum()
    exp = p[legal[0]] * counts.sum()
    obs = counts[legal[0]].astype(np.float64)
    order = np.argsort(exp)  # merge the bins whose expectation is below 5 (smallest first) into one
    small = exp[order] < 5
    e_bins = list(exp[order][~small]) + ([exp[order][small].sum()] if small.any() else [])
    o_bins = list(obs[order][~small]) + ([obs[order][small].sum()] if small.any() else [])
    e_bins, o_bins = np.array(e_bins), np.array(o_bins)
    stat = float(((o_bins - e_bins) ** 2 / e_bins).sum())
    pval = _chi2_sf(stat, len(e_bins) - 1)
    assert pval > 1e-6, (stat, len(e_bins), pval)
    env.close()


def test_no_legal_action():
    """A crowded grid whose episodes end because the next component has no legal cell: without a reset the mask stays
    empty.  Action 0, log_prob = entropy = 0, no error bit; the other environments are drawn as usual."""
    cfg = EnvConfig.spatial(12, 12, 5, 5, 2, 5, 2, 5, 8, 8, 3, 5, 7, 2, "centroid", 2, 0.5)
    B = 64
    env = _env(cfg, B)
    for t in range(12):
        legal = _legal(env)
        if (~legal.any(1)).any():
            break
        env.step(env.sample_actions(t))
    empty = ~legal.any(1)
    assert empty.any() and (~empty).any()
    rng = np.random.RandomState(8)
    logits = torch.from_numpy(_random_logits(rng, legal)).to(env.device)
    for greedy in (False, True):
        a, lp, ent = env.sample_logits(logits, 3, greedy=greedy, check=True)
        a, lp, ent = a.cpu().numpy(), lp.cpu().numpy(), ent.cpu().numpy()
        assert (a[empty] == 0).all() and (lp[empty] == 0).all() and (ent[empty] == 0).all()
        fa = a[:, 0] * 144 + a[:, 1] * 12 + a[:, 2]
        assert legal[~empty, fa[~empty]].all()
    env.close()


@pytest.mark.parametrize("bad, bit", [(-np.inf, 2), (np.nan, 1), (np.inf, 1)])
def test_error_cases_take_the_uniform_draw(bad, bit):
    cfg = named_config("c3")
    B = 8
    env = _env(cfg, B, first_env_index=2)
    env.step(env.sample_actions(0))
    legal = _legal(env)
    rng = np.random.RandomState(9)
    base = _random_logits(rng, legal)
    k = 3
    n = int(legal[k].sum())  # legal flat actions (the mirrored orientations included)
    hurt = base.copy()
    if bad == -np.inf:
        hurt[k, legal[k]] = -np.inf
    else:
        hurt[k, np.flatnonzero(legal[k])[5]] = bad
    for greedy in (False, True):
        ok = env.sample_logits(torch.from_numpy(base).to(env.device), 4, greedy=greedy, check=True)
        err = torch.zeros(1, dtype=torch.int32, device=env.device)
        a = torch.empty((B, 3), dtype=torch.int32, device=env.device)
        lp = torch.empty(B, dtype=torch.float32, device=env.device)
        ent = torch.empty(B, dtype=torch.float32, device=env.device)
        logits = torch.from_numpy(hurt).to(env.device)
        _lib.check(env._L.pcbenv_sample_logits(env._h, logits.data_ptr(), _lib.LOGITS_F32,
                                               _lib.DRAW_GREEDY if greedy else _lib.DRAW_SAMPLE, a.data_ptr(),
                                               _lib.ACTION_TUPLE, lp.data_ptr(), ent.data_ptr(), err.data_ptr(), SEED, 2, 4,
                                               env._stream()), env._h)
        assert int(err.item()) == bit
        uni = env.sample_actions(4)
        assert torch.equal(a[k], uni[k])
        assert lp[k].item() == pytest.approx(-np.log(n), rel=1e-6) and ent[k].item() == pytest.approx(np.log(n), rel=1e-6)
        others = [i for i in range(B) if i != k]
        for x, y in zip((a, lp, ent), ok):
            assert torch.equal(x[others], y[others])
        with pytest.raises(FloatingPointError):
            env.sample_logits(logits, 4, greedy=greedy, check=True)
    env.close()


def _obs_equal(a, b):
    for k in a.obs:
        assert torch.equal(a.obs[k], b.obs[k]), k
    assert torch.equal(a.reward, b.reward) and torch.equal(a.done, b.done)
    assert torch.equal(a.info_raw.nan_to_num(7.0), b.info_raw.nan_to_num(7.0))


@pytest.mark.parametrize("name", ["c3", "c4"])
def test_writes_nothing_the_library_owns(name):
    """Interleave step, sample_logits, gather_ (a permutation), reset(mask) and set_state: every draw is legal, and
    every step (the fused sampler's included) is bit-identical to a twin that never called sample_logits."""
    cfg = named_config(name)
    B = 32
    envs = [_env(cfg, B, queue_depth=3, auto_reset=False) for _ in range(2)]
    me, twin = envs
    rng = np.random.RandomState(10)
    gen = torch.Generator(device=me.device).manual_seed(1)

    def draw(t):
        legal = _legal(me)
        logits = torch.randn((B, _A(cfg)), generator=gen, device=me.device) * 2
        for greedy in (False, True):
            a, _, _ = me.sample_logits(logits, t, greedy=greedy, check=True)
            fa = _flat(me, a)
            has = legal.any(1)
            assert legal[has, fa[has]].all()
        return a
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


@pytest.mark.parametrize("name, B", [("c3", 4096), ("c4", 1024)])
def test_policy_loop_against_the_oracle(name, B):
    """rollout.collect(logits_policy=...) on the trajectory layout with auto_reset for two episodes; the recorded
    actions replayed on the CPU oracle: every tensor of every step bit-equal."""
    from test_gather_gpu import Run, _bytes_equal
    cfg = named_config(name)
    r = Run(cfg, B, run_seed=SEED, queue_depth=3, num_slots=2, auto_reset=True)
    env = r.env
    gen = torch.Generator(device=env.device).manual_seed(2)
    A = _A(cfg)

    def policy(obs):
        return torch.randn((B, A), generator=gen, device=env.device) * 3
    steps = 2 * cfg.max_num_components + 1
    for t in range(steps):
        legal = _legal(env)
        env.select_slot(t + 1)
        tr = collect(env, 1, logits_policy=policy, t0=t)
        a = tr.actions[0].cpu().numpy()
        fa = a[:, 0] * cfg.height * cfg.width + a[:, 1] * cfg.width + a[:, 2]
        has = legal.any(1)
        assert legal[has, fa[has]].all()
        assert tr.log_prob.shape == (1, B) and torch.isfinite(tr.log_prob).all() and (tr.log_prob <= 0).all()
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


def test_ppo_device_sampler():
    from pcbenv.policy import SpatialPolicy
    from pcbenv.ppo import PPOConfig, PPOTrainer
    torch.manual_seed(0)
    cfg = EnvConfig.spatial(10, 10, 9, 9, 2, 2, 2, 2, 5, 5, 3, 3, 6, 6, "centroid", 2, 0.75)
    env = BatchedPlacementEnv(cfg, 64, queue_depth=4, auto_reset=True)
    env.generate_instances()
    env.reset()
    policy = SpatialPolicy(cfg).to(env.device)
    tr = PPOTrainer(env, policy, PPOConfig(rollout_steps=10, epochs=1, minibatches=2, device_sampler=True))
    batch = tr.collect()
    assert tr.draws == 10
    policy.eval()
    with torch.no_grad():
        for t in range(10):
            logits, _ = policy({k: v[t] for k, v in batch["obs"].items()})
            want = torch.distributions.Categorical(logits=logits).log_prob(batch["act"][t])
            assert torch.allclose(batch["logp"][t], want, atol=1e-4, rtol=0), t
    stats = tr.update(batch)
    assert all(np.isfinite(v) for v in stats.values())
    tr.update(tr.collect())
    assert tr.draws == 20
    assert len(tr.returns) == 2 and all(-11.0 < r < 0.0 for r in tr.returns)
    env.close()
