"""pcbenv_evaluate_logits / pcbenv_evaluate_logits_backward on the GPU: log-probability, entropy and their gradient
against the float64 restatement of the contract (tests/evaluate_contract.py), against torch autograd through the
reference's masked chain, and inside PPO.  Configurations, masks and the logits distribution are those of
tests/test_sample_logits_gpu.py.

Gradient tolerance: not a fixed number.  For every case the error of torch's float32 chain (masked_logits + Categorical,
autograd, on the CPU, same inputs) against the float64 contract gradient is measured, and the kernel is allowed 4x that
error plus 1e-7 absolute (4x: reordered float32 sums and exp2-based weights; 1e-7: keeps the bound off 0).  bf16: the same
after rounding the contract gradient to bf16, plus one bf16 ulp."""
import copy

import numpy as np
import pytest
import torch

import evaluate_contract as ec
from pcbenv import EnvConfig, _lib, named_config
from pcbenv.batched_env import BatchedPlacementEnv
from pcbenv.config import KIND_SQUARE
from pcbenv.masked_categorical import evaluate, unpack_mask_bits
from pcbenv.rollout import collect, masked_logits
from test_sample_logits_gpu import CONFIGS, _A, _env, _legal, _random_logits

pytestmark = pytest.mark.gpu


def _points(cfg):
    n = cfg.max_num_components if cfg.kind != KIND_SQUARE else 6
    return {"reset": 0, "midway": n // 2, "last": n - 1}


def _advance(env, done_steps, upto):
    while done_steps < upto:
        env.step(env.sample_actions(done_steps))
        env.reset_done()
        done_steps += 1
    return done_steps


def _random_legal_actions(rng, legal):
    a = np.zeros(legal.shape[0], np.int64)
    for r in range(legal.shape[0]):
        idx = np.flatnonzero(legal[r])
        if idx.size:
            a[r] = idx[rng.randint(idx.size)]
    return a


def _as_actions(a, cfg, fmt, device):
    t = torch.from_numpy(a.astype(np.int32))
    if fmt == "tuple":
        HW, W = cfg.height * cfg.width, cfg.width
        t = torch.stack([t // HW, (t % HW) // W, t % W], 1).to(torch.int32)
    return t.contiguous().to(device)


def _bf16_round(x):
    return torch.from_numpy(np.asarray(x, np.float64)).to(torch.bfloat16).double().numpy()


def _bf16_ulp(x):
    ax = np.abs(x)
    with np.errstate(divide="ignore"):
        return np.where(ax > 0, 2.0 ** (np.floor(np.log2(np.where(ax > 0, ax, 1.0))) - 7), 0.0)


def _cpu_float32_chain_grad(l, legal, a, g_lp, g_h):
    """The reference error's source: torch's float32 chain on the CPU, gradient as float64."""
    x = torch.tensor(np.where(legal, l, 0.0), dtype=torch.float32, requires_grad=True)
    d = torch.distributions.Categorical(logits=masked_logits(x, torch.from_numpy(legal)), validate_args=False)
    loss = (d.log_prob(torch.from_numpy(a)) * torch.from_numpy(g_lp).float() + d.entropy() * torch.from_numpy(g_h).float()).sum()
    loss.backward()
    return x.grad.double().numpy()


def _close_with_inf(got, want, atol):
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    inf = np.isinf(want)
    assert np.array_equal(got[inf], want[inf])
    np.testing.assert_allclose(got[~inf], want[~inf], atol=atol, rtol=0)


def _backward(env, x, bits, acts, g_lp, g_h):
    """Forward with stats + one backward launch into a NaN-filled buffer."""
    N = x.shape[0]
    stats = torch.empty((N, 4), dtype=torch.float32, device=x.device)
    err = torch.zeros(1, dtype=torch.int32, device=x.device)
    lp, ent = env.evaluate_logits_forward(x, bits, acts, stats, err)
    out = torch.full_like(x, float("nan"))
    glp = None if g_lp is None else torch.from_numpy(g_lp).float().to(x.device)
    gh = None if g_h is None else torch.from_numpy(g_h).float().to(x.device)
    env.evaluate_logits_backward(x, bits, acts, stats, glp, gh, out=out)
    return lp, ent, out, int(err.item()), stats


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("name", list(CONFIGS))
def test_forward_and_backward_against_the_contract(name, dtype):
    cfg = CONFIGS[name]()
    B = 32 if name == "c5" else 64
    env = _env(cfg, B, first_env_index=3)
    O, H, W, A = cfg.num_orientations, cfg.height, cfg.width, _A(cfg)
    rng = np.random.RandomState(17)
    done_steps = 0
    for pname, at in _points(cfg).items():
        done_steps = _advance(env, done_steps, at)
        legal = _legal(env)
        bits = env.mask_bits()
        assert np.array_equal(ec.legal_rows(bits.cpu().numpy(), O, H, W), legal)
        has = legal.any(1)
        dev = torch.from_numpy(_random_logits(rng, legal)).to(env.device).to(dtype)
        l = dev.float().cpu().numpy().astype(np.float64)  # what the kernels read
        a_s, lp_s, ent_s = env.sample_logits(dev, done_steps, flat=True, check=True)
        sets = {"sampled": a_s.cpu().numpy().astype(np.int64), "random": _random_legal_actions(rng, legal)}
        for k, (sname, a) in enumerate(sets.items()):
            fmt = ("flat", "tuple")[(k + done_steps) & 1]
            acts = _as_actions(a, cfg, fmt, env.device)
            g_lp, g_h = rng.randn(B), 0.01 * rng.randn(B)
            want_lp, want_ent, want_bits, want_status = ec.evaluate(l, legal, a)
            want_g = ec.gradient(l, legal, a, g_lp, g_h)
            assert want_bits == 0

            lp, ent, g, err, stats = _backward(env, dev, bits, acts, g_lp, g_h)
            assert err == 0
            assert np.array_equal(stats[:, 3].cpu().numpy(), want_status.astype(np.float32))
            _close_with_inf(lp.cpu().numpy(), want_lp, 1e-4)
            np.testing.assert_allclose(ent.cpu().numpy(), want_ent, atol=1e-4, rtol=0)
            if sname == "sampled":
                d_lp = float((lp - lp_s)[torch.from_numpy(has).to(env.device)].abs().max()) if has.any() else 0.0
                d_ent = float((ent - ent_s).abs().max())
                print(f"EVAL-VS-SAMPLER {name} {pname} {dtype} max|dlog_prob| {d_lp:.3e} max|dentropy| {d_ent:.3e}")

            # structural, exact
            gk = g.float().cpu().numpy().astype(np.float64)
            assert np.isfinite(gk).all()
            assert not gk[~legal].any()
            assert not gk[~has].any()

            # the bound: 4 x the CPU float32 chain's own error + 1e-7 (rows with a legal action; a row with none is 0 by
            # contract and uniform over all A for the chain)
            ref = _cpu_float32_chain_grad(l, legal, a, g_lp, g_h)
            e_ref = float(np.abs(ref - want_g)[has].max()) if has.any() else 0.0
            bound = 4.0 * e_ref + 1e-7
            if dtype == torch.float32:
                want, allow = want_g, bound
            else:
                want = _bf16_round(want_g)
                allow = bound + _bf16_ulp(want)
            e_k = float(np.abs(gk - want).max())
            print(f"EVAL-GRAD {name} {pname} {sname} {dtype} |g|max {np.abs(want_g).max():.3f} ref_f32_chain_err {e_ref:.3e} "
                  f"kernel_err {e_k:.3e} bound {bound:.3e}")
            assert (np.abs(gk - want) <= allow).all(), (name, pname, sname, dtype, e_k, bound)

            # torch autograd on the device through the masked chain, the same bound
            xd = dev.float().clone().requires_grad_(True)
            d = torch.distributions.Categorical(logits=masked_logits(xd, env.action_mask), validate_args=False)
            fa = torch.from_numpy(a).to(env.device)
            (d.log_prob(fa) * torch.from_numpy(g_lp).float().to(env.device)
             + d.entropy() * torch.from_numpy(g_h).float().to(env.device))[torch.from_numpy(has).to(env.device)].sum().backward()
            gt = xd.grad.double().cpu().numpy()
            if dtype == torch.bfloat16:
                gt = _bf16_round(gt)
            e_t = float(np.abs(gk - gt)[has].max()) if has.any() else 0.0
            print(f"EVAL-GRAD-VS-DEVICE-TORCH {name} {pname} {sname} {dtype} diff {e_t:.3e} bound {bound:.3e}")
            assert (np.abs(gk - gt) <= allow)[has].all(), (name, pname, sname, e_t, bound)

            # the autograd wrapper: the same bits as the direct calls
            x = dev.clone().requires_grad_(True)
            lp2, ent2 = evaluate(env, x, bits, acts)
            (lp2 * torch.from_numpy(g_lp).float().to(env.device) + ent2 * torch.from_numpy(g_h).float().to(env.device)).sum().backward()
            assert x.grad.dtype == dtype
            assert torch.equal(lp2.detach(), lp) and torch.equal(ent2.detach(), ent)
            assert torch.equal(x.grad, g)
    env.close()


@pytest.mark.parametrize("name", ["c2", "c3", "c5", "square_5x5", "rect_6x6"])
def test_illegal_logits_are_never_read(name):
    """NaN or garbage at illegal positions changes no output bit; masked and unmasked logits give identical bits."""
    cfg = CONFIGS[name]()
    B = 32 if name == "c5" else 64
    env = _env(cfg, B)
    rng = np.random.RandomState(5)
    _advance(env, 0, 2)
    legal = _legal(env)
    bits = env.mask_bits()
    tl = torch.from_numpy(legal).to(env.device)
    a = _as_actions(_random_legal_actions(rng, legal), cfg, "flat", env.device)
    g_lp, g_h = rng.randn(B), 0.01 * rng.randn(B)
    for dtype in (torch.float32, torch.bfloat16):
        raw = torch.from_numpy(_random_logits(rng, legal)).to(env.device).to(dtype)
        base = _backward(env, raw, bits, a, g_lp, g_h)
        variants = {"nan": torch.where(tl, raw, torch.full_like(raw, float("nan"))),
                    "garbage": torch.where(tl, raw, torch.full_like(raw, 3.0e38)),
                    "masked": masked_logits(raw.float(), env.action_mask).to(dtype)}
        assert torch.equal(variants["masked"][tl].view(-1), raw[tl].view(-1))  # adding log(1) = 0 changes no legal logit
        for vname, x in variants.items():
            got = _backward(env, x.contiguous(), bits, a, g_lp, g_h)
            for u, v in zip(got[:3], base[:3]):
                assert torch.equal(u.view(torch.uint8), v.view(torch.uint8)), (name, dtype, vname)
            assert got[3] == base[3] == 0
    env.close()


def test_num_rows_is_arbitrary_and_rows_may_be_permuted():
    """A [T, B] trajectory evaluated as one call of T*B = 10 240 rows, permuted, equals the per-step calls; 0 and 1 row."""
    cfg = named_config("c3")
    T, B = 10, 1024
    env = _env(cfg, B, queue_depth=2)
    A = _A(cfg)
    gen = torch.Generator(device=env.device).manual_seed(4)
    state = {}

    def logits_policy(obs):
        state["l"] = torch.randn((B, A), generator=gen, device=env.device) * 3
        state.setdefault("all", []).append(state["l"])
        return state["l"]
    traj = collect(env, T, logits_policy=logits_policy, store_mask_bits=True)
    assert traj.mask_bits.shape == (T, B, 2, cfg.height, 1) and traj.mask_bits.dtype == torch.int64
    logits = torch.stack(state["all"])                     # [T, B, A]
    acts = traj.actions                                    # [T, B, 3] int32
    N = T * B
    perm = torch.randperm(N, generator=gen, device=env.device)
    x = logits.reshape(N, A)[perm].contiguous()
    mb = traj.mask_bits.reshape(N, 2, cfg.height, 1)[perm].contiguous()
    ac = acts.reshape(N, 3)[perm].contiguous()
    err = torch.zeros(1, dtype=torch.int32, device=env.device)
    lp, ent = env.evaluate_logits(x, mb, ac, errors=err)
    assert int(err.item()) == 0
    # the draw's own log-probability and entropy, row for row: each kernel is held to 1e-4 of the contract
    assert float((lp - traj.log_prob.reshape(N)[perm]).abs().max()) <= 2e-4
    assert float((ent - traj.entropy.reshape(N)[perm]).abs().max()) <= 2e-4
    g_lp = torch.randn(N, generator=gen, device=env.device)
    xg = x.clone().requires_grad_(True)
    lp2, ent2 = evaluate(env, xg, mb, ac)
    (lp2 * g_lp).sum().backward()
    for t in (0, T - 1):                                   # per-step calls of B rows give the same bits
        rows = torch.nonzero((perm >= t * B) & (perm < (t + 1) * B)).squeeze(1)
        order = rows[torch.argsort(perm[rows])]
        xs = logits[t].clone().requires_grad_(True)
        lps, ents = evaluate(env, xs, traj.mask_bits[t], acts[t])
        (lps * g_lp[order]).sum().backward()
        assert torch.equal(lps.detach(), lp[order]) and torch.equal(ents.detach(), ent[order])
        assert torch.equal(xs.grad, xg.grad[order])
    for n in (0, 1):
        l1, e1 = env.evaluate_logits(x[:n].contiguous(), mb[:n].contiguous(), ac[:n].contiguous())
        assert l1.shape == (n,) and torch.equal(l1, lp[:n]) and torch.equal(e1, ent[:n])
        xn = x[:n].clone().requires_grad_(True)
        ln, en = evaluate(env, xn, mb[:n].contiguous(), ac[:n].contiguous())
        (ln.sum() + en.sum()).backward()
        assert xn.grad.shape == (n, A) and bool(torch.isfinite(xn.grad).all())
    # num_rows == 0 at the ABI: success, nothing written
    out = torch.full((4,), 7.0, device=env.device)
    _lib.check(env._L.pcbenv_evaluate_logits(env._h, x.data_ptr(), _lib.LOGITS_F32, mb.data_ptr(), ac.data_ptr(), _lib.ACTION_TUPLE,
                                             0, out.data_ptr(), out.data_ptr(), None, None, env._stream()), env._h)
    _lib.check(env._L.pcbenv_evaluate_logits_backward(env._h, x.data_ptr(), _lib.LOGITS_F32, mb.data_ptr(), ac.data_ptr(),
                                                      _lib.ACTION_TUPLE, 0, out.data_ptr(), None, None, out.data_ptr(),
                                                      env._stream()), env._h)
    assert bool((out == 7.0).all())
    env.close()


SCALAR = {5: lambda: EnvConfig.square(5, 5, 2), 6: lambda: EnvConfig.rect(6, 6, 2, 4, 2, 4, 4, 2),
          10: lambda: EnvConfig.spatial(10, 10, 9, 9, 2, 2, 2, 2, 5, 5, 3, 3, 6, 6, "centroid", 2, 0.75)}


@pytest.mark.parametrize("W", [5, 6, 10])
def test_scalar_path_widths(W):
    """W % 4 != 0: one load and one store per element; every element of a NaN-filled buffer is written."""
    cfg = SCALAR[W]()
    assert cfg.width == W
    B = 64
    env = _env(cfg, B)
    rng = np.random.RandomState(W)
    _advance(env, 0, 1)
    legal = _legal(env)
    bits = env.mask_bits()
    a = _random_legal_actions(rng, legal)
    g_lp, g_h = rng.randn(B), 0.01 * rng.randn(B)
    for dtype in (torch.float32, torch.bfloat16):
        dev = torch.from_numpy(_random_logits(rng, legal)).to(env.device).to(dtype)
        l = dev.float().cpu().numpy().astype(np.float64)
        lp, ent, g, err, _ = _backward(env, dev, bits, _as_actions(a, cfg, "tuple", env.device), g_lp, g_h)
        want_lp, want_ent, _, _ = ec.evaluate(l, legal, a)
        want_g = ec.gradient(l, legal, a, g_lp, g_h)
        _close_with_inf(lp.cpu().numpy(), want_lp, 1e-4)
        np.testing.assert_allclose(ent.cpu().numpy(), want_ent, atol=1e-4, rtol=0)
        gk = g.float().cpu().numpy().astype(np.float64)
        assert np.isfinite(gk).all() and not gk[~legal].any() and err == 0
        has = legal.any(1)
        e_ref = float(np.abs(_cpu_float32_chain_grad(l, legal, a, g_lp, g_h) - want_g)[has].max())
        bound = 4.0 * e_ref + 1e-7
        want = want_g if dtype == torch.float32 else _bf16_round(want_g)
        allow = bound if dtype == torch.float32 else bound + _bf16_ulp(want)
        assert (np.abs(gk - want) <= allow).all(), (W, dtype, float(np.abs(gk - want).max()), bound)
    env.close()


def test_edge_cases_are_data():
    """No legal action; a legal NaN / +inf (bit 0); every legal logit -inf (bit 1); a stored action out of range or not
    legal (bit 2): the stated outputs, the stated zero gradient rows, the stated bits."""
    cfg = EnvConfig.spatial(12, 12, 5, 5, 2, 5, 2, 5, 8, 8, 3, 5, 7, 2, "centroid", 2, 0.5)
    B = 64
    env = _env(cfg, B)
    for t in range(12):  # a crowded grid: some episodes end with no legal cell; without a reset the mask stays empty
        legal = _legal(env)
        if (~legal.any(1)).any():
            break
        env.step(env.sample_actions(t))
    empty = ~legal.any(1)
    assert empty.any() and (~empty).sum() >= 8
    O, H, W, A = cfg.num_orientations, cfg.height, cfg.width, _A(cfg)
    bits = env.mask_bits()
    rng = np.random.RandomState(12)
    base = _random_logits(rng, legal)
    live = np.flatnonzero(~empty)
    r_nan, r_inf, r_neg, r_illegal, r_range, r_tuple = live[:6]
    a = _random_legal_actions(rng, legal)
    g_lp, g_h = rng.randn(B), rng.randn(B)

    def run(l32, a, fmt="flat", acts=None, dtype=torch.float32):
        dev = torch.from_numpy(l32).to(env.device).to(dtype)
        acts = _as_actions(a, cfg, fmt, env.device) if acts is None else acts
        lp, ent, g, err, stats = _backward(env, dev, bits, acts, g_lp, g_h)
        return lp.cpu().numpy(), ent.cpu().numpy(), g.float().cpu().numpy(), err, stats[:, 3].cpu().numpy()

    n = legal.sum(1)
    for dtype in (torch.float32, torch.bfloat16):
        lp, ent, g, err, status = run(base, a, dtype=dtype)
        assert err == 0
        assert not lp[empty].any() and not ent[empty].any() and not g[empty].any()
        assert (status[empty] == ec.ROW_ZERO).all() and (status[~empty] == ec.ROW_OK).all()
        assert np.isfinite(g).all()

        for row, value, bit in ((r_nan, np.nan, ec.ERR_NONFINITE), (r_inf, np.inf, ec.ERR_NONFINITE), (r_neg, -np.inf, ec.ERR_ALL_NEG_INF)):
            hurt = base.copy()
            if value == -np.inf:
                hurt[row, legal[row]] = -np.inf
            else:
                hurt[row, np.flatnonzero(legal[row])[-1]] = value
            lp2, ent2, g2, err2, status2 = run(hurt, a, dtype=dtype)
            assert err2 == bit
            assert lp2[row] == pytest.approx(-np.log(n[row]), rel=1e-6) and ent2[row] == pytest.approx(np.log(n[row]), rel=1e-6)
            assert not g2[row].any() and status2[row] == ec.ROW_ZERO and np.isfinite(g2).all()
            others = np.arange(B) != row
            assert np.array_equal(lp2[others], lp[others]) and np.array_equal(ent2[others], ent[others])
            assert np.array_equal(g2[others], g[others])

        # a stored action that is not legal / out of range (flat) / out of range (tuple)
        b = a.copy()
        b[r_illegal] = np.flatnonzero(~legal[r_illegal])[0]
        b[r_range] = A + 5
        lp3, ent3, g3, err3, status3 = run(base, b, dtype=dtype)
        tup = _as_actions(a, cfg, "tuple", env.device)
        tup[r_tuple] = torch.tensor([0, H, 0], dtype=torch.int32)
        tup[r_range] = torch.tensor([-1, 0, 0], dtype=torch.int32)
        lp4, ent4, g4, err4, status4 = run(base, a, acts=tup, dtype=dtype)
        for lpx, entx, gx, errx, statusx, rows in ((lp3, ent3, g3, err3, status3, (r_illegal, r_range)),
                                                   (lp4, ent4, g4, err4, status4, (r_tuple, r_range))):
            assert errx == ec.ERR_ACTION
            ulp = 2.0 ** -23 if dtype == torch.float32 else 2.0 ** -8
            for row in rows:
                assert lpx[row] == 0 and entx[row] == ent[row] and statusx[row] == ec.ROW_NO_ONE_HOT
                # the one-hot term is dropped: the row of the valid action everywhere but at that action, where it
                # is g_lp less (two roundings to the output dtype and the float32 operations between: 4 ulp)
                at = np.arange(A) == a[row]
                assert np.array_equal(gx[row][~at], g[row][~at])
                drop = float(g[row][a[row]]) - float(gx[row][a[row]])
                scale = max(abs(g_lp[row]), abs(float(g[row][a[row]])), abs(float(gx[row][a[row]])))
                assert abs(drop - g_lp[row]) <= 4 * ulp * scale, (row, drop, g_lp[row])
                assert not gx[row][~legal[row]].any()
            others = np.ones(B, bool)
            others[list(rows)] = False
            assert np.array_equal(lpx[others], lp[others]) and np.array_equal(gx[others], g[others])

    # null gradients mean zero; errors may be NULL
    dev = torch.from_numpy(base).to(env.device)
    acts = _as_actions(a, cfg, "flat", env.device)
    _, _, g_none, _, _ = _backward(env, dev, bits, acts, None, None)
    assert not g_none.any()
    _, _, g_only_lp, _, _ = _backward(env, dev, bits, acts, g_lp, None)
    _, _, g_zero_h, _, _ = _backward(env, dev, bits, acts, g_lp, np.zeros(B))
    assert torch.equal(g_only_lp, g_zero_h)
    lp5, ent5 = env.evaluate_logits(dev, bits, acts)
    assert lp5.shape == (B,) and ent5.shape == (B,)
    env.close()


def _ppo_setup(seed=0, B=64):
    cfg = EnvConfig.spatial(10, 10, 9, 9, 2, 2, 2, 2, 5, 5, 3, 3, 6, 6, "centroid", 2, 0.75)
    env = BatchedPlacementEnv(cfg, B, queue_depth=4, auto_reset=True)
    env.generate_instances()
    env.reset()
    return cfg, env


def test_ppo_update_matches_the_torch_branch():
    """From identical weights and one identical batch, one update with device_evaluator off and one with it on."""
    from pcbenv.policy import SpatialPolicy
    from pcbenv.ppo import PPOConfig, PPOTrainer
    torch.manual_seed(0)
    cfg, env = _ppo_setup()
    policy = SpatialPolicy(cfg).to(env.device)
    kw = dict(rollout_steps=10, epochs=1, minibatches=1)
    collector = PPOTrainer(env, copy.deepcopy(policy), PPOConfig(device_evaluator=True, **kw))
    batch = collector.collect()
    assert batch["mask_bits"].shape == (10, 64, 2, 10, 1)
    # every row has a legal action: a row with none is where the two paths differ by definition
    assert bool(batch["obs"]["action_mask"].reshape(10 * 64, -1).any(1).all())
    assert torch.equal(unpack_mask_bits(cfg, batch["mask_bits"].reshape(640, 2, 10, 1)),
                       batch["obs"]["action_mask"].reshape(640, -1).bool())  # the stored bits are the stored masks
    stats = {}
    for on in (False, True):
        tr = PPOTrainer(env, copy.deepcopy(policy), PPOConfig(device_evaluator=on, **kw))
        b = dict(batch)
        if not on:
            del b["mask_bits"]  # what collect() returns with the option off
        torch.manual_seed(123)  # the same permutation and BatchNorm refresh rows
        stats[on] = tr.update(b)
    print("PPO-UPDATE-AB", stats)
    for k in ("pg", "vf", "entropy"):
        assert abs(stats[False][k] - stats[True][k]) <= 1e-4, (k, stats)
    env.close()


def test_ppo_runs_without_action_mask():
    """Both device options on, obs_keys without "action_mask": nothing on that path reads it."""
    from pcbenv.policy import SpatialPolicy
    from pcbenv.ppo import PPOConfig, PPOTrainer
    torch.manual_seed(0)
    cfg, env = _ppo_setup()
    policy = SpatialPolicy(cfg).to(env.device)
    tr = PPOTrainer(env, policy, PPOConfig(rollout_steps=10, epochs=1, minibatches=2, device_sampler=True, device_evaluator=True),
                    obs_keys=("grid", "pin_grid", "component_grid", "placement_mask"))
    for _ in range(2):
        batch = tr.collect()
        assert "action_mask" not in batch["obs"] and "mask_bits" in batch
        stats = tr.update(batch)
        assert all(np.isfinite(v) for v in stats.values())
    assert tr.draws == 20
    assert len(tr.returns) == 2 and all(-11.0 < r < 0.0 for r in tr.returns)
    env.close()


def test_ppo_option_off_keeps_the_torch_branch():
    from pcbenv.policy import SpatialPolicy
    from pcbenv.ppo import PPOConfig, PPOTrainer
    from pcbenv import masked_categorical
    torch.manual_seed(0)
    cfg, env = _ppo_setup()
    tr = PPOTrainer(env, SpatialPolicy(cfg).to(env.device), PPOConfig(rollout_steps=10, epochs=1, minibatches=2))
    assert tr.cfg.device_evaluator is False
    batch = tr.collect()
    assert "mask_bits" not in batch
    calls = []
    orig = masked_categorical.evaluate
    masked_categorical.evaluate = lambda *a, **k: calls.append(1) or orig(*a, **k)
    try:
        stats = tr.update(batch)
    finally:
        masked_categorical.evaluate = orig
    assert not calls and all(np.isfinite(v) for v in stats.values())
    env.close()
