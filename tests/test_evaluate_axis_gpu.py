"""pcbenv_evaluate_axis / pcbenv_evaluate_axis_backward on the GPU: log-probability, entropy and their gradient for one
stage of a factorised policy against the float64 restatement of the contract (tests/factor_contract.py), for every stage
of both reference orders, on synthetic bit rows and their dirty twins; the error cases that are data; and
FactorisedPolicy's act -> evaluate round trip.

Tolerances are those of tests/test_evaluate_logits_gpu.py: atol 1e-4 on log_prob and entropy; the gradient within
4 x e_ref + 1e-7 of the contract, e_ref being the error of torch's float32 chain on the CPU (logits_cases.chain32 on the
stage's rows, same inputs) against the contract; bf16: the same after rounding the contract gradient to bf16, plus one
bf16 ulp."""
import numpy as np
import pytest
import torch

import factor_contract as fc
import logits_cases as lc
from axis_cases import CONFIGS, SEED, GridEncoder, as_read, dense_of_bits, legal_sets, make_env, sizes
from pcbenv import EnvConfig, named_config
from pcbenv.factorised import ORDERS, FactorisedPolicy, evaluate_axis
from pcbenv.rollout import collect

pytestmark = pytest.mark.gpu

STAGES = [(order, i) for order in ORDERS for i in range(3)]
NUM_ROWS = (0, 1, 3, 257)
GRADS = ("log_prob", "entropy", "both", "null")


def _bf16_round(x):
    return torch.from_numpy(np.asarray(x, np.float64)).to(torch.bfloat16).double().numpy()


def _bf16_ulp(x):
    ax = np.abs(x)
    with np.errstate(divide="ignore"):
        return np.where(ax > 0, 2.0 ** (np.floor(np.log2(np.where(ax > 0, ax, 1.0))) - 7), 0.0)


def _rows(cfg, N, rng):
    """N synthetic rows -> (clean int64 [N, 2, H, WW], dirty twin, dense bool [N, O, H, W], actions int32 [N, 3]): every
    mask class, a legal triple stored in three rows of four, anything in range in the fourth."""
    O, H, W = sizes(cfg)
    classes = lc.bits(cfg.kind, O, H, W, rng)
    clean = classes[rng.randint(len(classes), size=N)] if N > 3 else classes[:N]  # the first three: densities 0.02 and 0.5
    dirty = lc.dirty_twin(clean, cfg.kind, W, rng)
    dense = dense_of_bits(clean, cfg)
    actions = np.stack([rng.randint(0, s, size=N) for s in (O, H, W)], axis=1).astype(np.int32)
    for r in range(N):
        hit = np.argwhere(dense[r])
        if len(hit) and r % 4 != 3:
            actions[r] = hit[rng.randint(len(hit))]
    return clean, dirty, dense, actions


def _call(env, axis, given, dev, bits, acts, g_lp, g_h):
    """Forward + one backward launch into a NaN-filled buffer -> (log_prob, entropy, gradient, error bits)."""
    err = torch.zeros(1, dtype=torch.int32, device=dev.device)
    lp, ent = env.evaluate_axis_forward(axis, given, dev, bits, acts, err)
    out = torch.full_like(dev, float("nan"))
    glp = None if g_lp is None else torch.from_numpy(g_lp).float().to(dev.device)
    gh = None if g_h is None else torch.from_numpy(g_h).float().to(dev.device)
    env.evaluate_axis_backward(axis, given, dev, bits, acts, glp, gh, out=out)
    return lp, ent, out, int(err.item())


def _contract(l, L, ok, a, g_lp, g_h):
    N = len(l)
    rows = [fc.evaluate(l[r], L[r], ok[r], a[r]) for r in range(N)]
    bits = 0
    for _, _, b in rows:
        bits |= b
    g = [fc.gradient(l[r], L[r], a[r], 0.0 if g_lp is None else g_lp[r], 0.0 if g_h is None else g_h[r]) for r in range(N)]
    return (np.array([x[0] for x in rows]), np.array([x[1] for x in rows]), bits,
            np.stack(g) if N else np.zeros((0, L.shape[1])))


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("name", list(CONFIGS))
def test_forward_and_backward_against_the_contract(name, dtype):
    cfg = CONFIGS[name]()
    env = make_env(cfg, 4)  # the handle gives the geometry and the device; the rows are the caller's
    rng = np.random.RandomState(17)
    for s, (order, i) in enumerate(STAGES):
        axis, given = ORDERS[order][i]
        n = sizes(cfg)[axis]
        for j, N in enumerate(NUM_ROWS):
            clean, dirty, dense, actions = _rows(cfg, N, rng)
            L, ok = legal_sets(dense, axis, given, actions) if N else (np.zeros((0, n), bool), np.zeros(0, bool))
            assert ok.all()
            a = actions[:, axis]
            acts = torch.from_numpy(actions).to(env.device)
            has = L.any(1)
            a_in = has & L[np.arange(N), a] if N else has
            l32 = lc.tame(rng, L) if N else np.zeros((0, n), np.float32)  # drawn after L is known
            for r in np.flatnonzero(a_in):
                if l32[r, a[r]] == -np.inf:  # a stored value has a weight: it was drawn
                    l32[r, a[r]] = 0.0
            dev, l = as_read(l32, dtype, env.device)
            for mode in (GRADS if N == 257 else (GRADS[(s + j) % 4],)):
                g_lp = rng.randn(N) if mode in ("log_prob", "both") else None
                g_h = 0.01 * rng.randn(N) if mode in ("entropy", "both") else None
                want_lp, want_ent, want_bits, want_g = _contract(l, L, ok, a, g_lp, g_h)
                assert want_bits in (0, fc.ERR_VALUE)
                out = [_call(env, axis, given, dev, torch.from_numpy(b).to(env.device), acts, g_lp, g_h) for b in (clean, dirty)]
                for x, y in zip(*out):  # the dirty twin: identical bytes
                    assert torch.equal(x, y) if isinstance(x, torch.Tensor) else x == y, (name, order, i, N, mode)
                lp, ent, g, err = out[0]
                assert err == want_bits and tuple(g.shape) == (N, n)
                if N == 0:  # the wrappers return early; the entry points themselves: a no-op success
                    ptr, code = acts.new_zeros(4).data_ptr(), 0 if dtype == torch.float32 else 1
                    assert env._L.pcbenv_evaluate_axis(env._h, axis, fc.given_bits(given), ptr, code, ptr, ptr, 0, None, None, None, env._stream()) == 0
                    assert env._L.pcbenv_evaluate_axis_backward(env._h, axis, fc.given_bits(given), ptr, code, ptr, ptr, 0, None, None, ptr, env._stream()) == 0
                    continue
                np.testing.assert_allclose(lp.cpu().numpy(), want_lp, atol=1e-4, rtol=0)
                np.testing.assert_allclose(ent.cpu().numpy(), want_ent, atol=1e-4, rtol=0)
                gk = g.float().cpu().numpy().astype(np.float64)
                assert np.isfinite(gk).all()          # the NaN-filled buffer comes back fully written
                assert not gk[~L].any()
                if mode == "null":
                    assert not gk.any()
                # e_ref: torch's float32 chain on the CPU against the contract, on the rows where both state the same thing
                z = np.zeros(N)
                _, _, ref, fin = lc.chain32(l, L, np.where(a_in, a, 0), z if g_lp is None else g_lp, z if g_h is None else g_h)
                use = a_in & fin
                e_ref = float(np.abs(ref - want_g)[use].max()) if use.any() else 0.0
                bound = 4.0 * e_ref + 1e-7
                want, allow = (want_g, bound) if dtype == torch.float32 else (_bf16_round(want_g), bound + _bf16_ulp(_bf16_round(want_g)))
                e_k = float(np.abs(gk - want).max())
                print(f"AXIS-EVAL-GRAD {name} {order}[{i}] rows {N} {mode} {dtype} |g|max {np.abs(want_g).max():.3f} "
                      f"ref_f32_chain_err {e_ref:.3e} kernel_err {e_k:.3e} bound {bound:.3e}")
                assert (np.abs(gk - want) <= allow).all(), (name, order, i, N, mode, dtype, e_k, bound)
                # the autograd wrapper: the same bits as the direct calls
                x = dev.clone().requires_grad_(True)
                lp2, ent2 = evaluate_axis(env, axis, given, x, torch.from_numpy(clean).to(env.device), acts)
                assert torch.equal(lp2, lp) and torch.equal(ent2, ent)
                if mode == "both":
                    (lp2 * torch.from_numpy(g_lp).float().to(env.device) + ent2 * torch.from_numpy(g_h).float().to(env.device)).sum().backward()
                    assert torch.equal(x.grad, g)
    env.close()


def test_error_cases_are_data():
    cfg = named_config("c3")
    env = make_env(cfg, 4)
    rng = np.random.RandomState(19)
    N, k = 9, 4
    for order in ORDERS:
        for axis, given in ORDERS[order]:
            while True:
                clean, _, dense, actions = _rows(cfg, N, rng)
                actions[k] = np.argwhere(dense[k])[0] if dense[k].any() else actions[k]
                L, ok = legal_sets(dense, axis, given, actions)
                if L[k].sum() >= 2:
                    break
            bits = torch.from_numpy(clean).to(env.device)
            base = lc.tame(rng, L, p_neg_inf=0.0)
            g_lp, g_h = rng.randn(N), 0.01 * rng.randn(N)
            others = [r for r in range(N) if r != k]
            ref = _call(env, axis, given, torch.from_numpy(base).to(env.device), bits, torch.from_numpy(actions).to(env.device), g_lp, g_h)
            assert ref[3] in (0, fc.ERR_VALUE)
            n = int(L[k].sum())
            cases = {"nan": 1, "inf": 1, "neg_inf": 2, "not_in_L": 4, "out_of_range": 4}
            if L[k].all():
                del cases["not_in_L"]
            if given:
                cases["given"] = 8
            for case, bit in cases.items():
                l, acts = base.copy(), actions.copy()
                if case == "nan":
                    l[k, np.flatnonzero(L[k])[-1]] = np.nan
                elif case == "inf":
                    l[k, np.flatnonzero(L[k])[0]] = np.inf
                elif case == "neg_inf":
                    l[k, L[k]] = -np.inf
                elif case == "not_in_L":
                    acts[k, axis] = np.flatnonzero(~L[k])[0]
                elif case == "out_of_range":
                    acts[k, axis] = (-1, sizes(cfg)[axis])[axis & 1]
                else:
                    acts[k, given[0]] = (-1, sizes(cfg)[given[0]])[axis & 1]
                lp, ent, g, err = _call(env, axis, given, torch.from_numpy(l).to(env.device), bits, torch.from_numpy(acts).to(env.device), g_lp, g_h)
                assert err == (bit | ref[3]), (order, axis, case)
                gk = g[k].cpu().numpy().astype(np.float64)
                if bit in (1, 2):
                    assert lp[k].item() == pytest.approx(-np.log(n), rel=1e-6) and ent[k].item() == pytest.approx(np.log(n), rel=1e-6)
                    assert not gk.any()
                elif bit == 4:
                    want_lp, want_ent, want_bits = fc.evaluate(l[k], L[k], True, acts[k, axis])
                    assert want_bits == 4 and lp[k].item() == 0.0 and ent[k].item() == pytest.approx(want_ent, abs=1e-4)
                    assert ent[k].item() == ref[1][k].item()
                    # the one-hot term is dropped: the row of the valid stored value everywhere but at that value, where it
                    # is g_lp less (two roundings to float32 and the float32 operations between: 4 ulp, the rule of
                    # tests/test_evaluate_logits_gpu.py for its rows of this kind)
                    g_ref = ref[2][k].cpu().numpy().astype(np.float64)
                    at = np.arange(len(gk)) == actions[k, axis]
                    assert np.array_equal(gk[~at], g_ref[~at])
                    drop = float(g_ref[at][0]) - float(gk[at][0])
                    scale = max(abs(g_lp[k]), abs(float(g_ref[at][0])), abs(float(gk[at][0])))
                    assert abs(drop - g_lp[k]) <= 4 * 2.0 ** -23 * scale, (order, axis, case, drop, g_lp[k])
                    assert not gk[~L[k]].any()
                else:
                    assert lp[k].item() == 0.0 and ent[k].item() == 0.0 and not gk.any()
                for x, y in zip((lp, ent, g), ref[:3]):
                    assert torch.equal(x[others], y[others]), (order, axis, case)
    env.close()


@pytest.mark.parametrize("encoder, order", [("grid", "orientation"), ("grid", "coordinates"), ("spatial", "orientation")])
def test_policy_act_then_evaluate(encoder, order):
    """act for a few steps, then evaluate on the stored mask_bits and actions: the rollout's summed log_prob comes back
    (three float32 stages: 3 x 1e-4), and a backward pass reaches every head and the encoder with finite gradients."""
    torch.manual_seed(3)
    if encoder == "grid":
        cfg = named_config("c3")
        enc = GridEncoder(cfg)
    else:
        from pcbenv.policy import SpatialPolicy
        cfg = EnvConfig.spatial(10, 10, 9, 9, 2, 2, 2, 2, 5, 5, 3, 3, 6, 6, "centroid", 2, 0.75)
        enc = SpatialPolicy(cfg)
    B, T = 64, 6
    env = make_env(cfg, B, queue_depth=4, auto_reset=True)
    policy = FactorisedPolicy(enc, cfg, order).to(env.device)
    policy.eval()  # the encoder's batch norm: the same statistics in act and evaluate
    with torch.no_grad():
        for h in policy.heads.heads:
            h.weight.mul_(10.0)
    keys = ("grid",) if encoder == "grid" else ("grid", "pin_grid", "component_grid", "placement_mask")
    tr = collect(env, T, factorised_policy=policy, store_obs=keys, store_mask_bits=True)
    obs = {k: v.flatten(0, 1) for k, v in tr.obs.items()}
    lp, ent, value = policy.evaluate(env, obs, tr.mask_bits.flatten(0, 1), tr.actions.flatten(0, 1))
    assert lp.shape == ent.shape == value.shape == (T * B,)
    d_lp = float((lp.detach() - tr.log_prob.flatten()).abs().max())
    d_ent = float((ent.detach() - tr.entropy.flatten()).abs().max())
    print(f"AXIS-ACT-VS-EVALUATE {encoder} {order} max|dlog_prob| {d_lp:.3e} max|dentropy| {d_ent:.3e}")
    assert d_lp <= 3e-4 and d_ent <= 3e-4
    (lp.mean() + 0.01 * ent.mean() + value.mean()).backward()
    unused = ("encoder.logits.", "encoder.value.")  # SpatialPolicy's flat head and its own value: not part of this policy
    for pname, p in policy.named_parameters():
        if pname.startswith(unused):
            assert p.grad is None, pname
            continue
        assert p.grad is not None and torch.isfinite(p.grad).all(), pname
    for h in policy.heads.heads:
        assert h.weight.grad.abs().sum() > 0
    assert policy.encoder.net.weight.grad.abs().sum() > 0 if encoder == "grid" else policy.encoder.grid_net.net[0].weight.grad.abs().sum() > 0
    env.close()
