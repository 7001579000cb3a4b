"""pcbenv/factorised.py and the axis wrappers of BatchedPlacementEnv without a device: the layer shapes and closed-form parameter counts of the reference's three
heads for both orders, `evaluate_axis_torch` (the reference's chain on the unpacked mask) against the float64 contract
in value and autograd gradient, `FactorisedPolicy.evaluate` on CPU tensors, `collect`'s argument exclusivity, and every ValueError of the wrappers'
argument checks (they come before any library call)."""
import types

import numpy as np
import pytest
import torch

import factor_contract as fc
import logits_cases as lc
from pcbenv import EnvConfig
from pcbenv.batched_env import BatchedPlacementEnv
from pcbenv.factorised import ORDERS, FactorisedHeads, FactorisedPolicy, evaluate_axis, evaluate_axis_torch
from pcbenv.rollout import collect

CONFIGS = {"rect_6x6": lambda: EnvConfig.rect(6, 6, 2, 4, 2, 4, 4, 2), "square_5x5": lambda: EnvConfig.square(5, 5, 2),
           "spatial_7x100": lc.RAGGED["spatial_7x100"], "pin_100x9": lc.RAGGED["pin_100x9"]}


def test_orders_are_the_references():
    assert ORDERS == fc.ORDERS
    assert ORDERS["orientation"] == ((0, ()), (1, (0,)), (2, (0, 1)))   # p(o) p(x|o) p(y|o,x)
    assert ORDERS["coordinates"] == ((1, ()), (2, (1,)), (0, (1, 2)))   # p(x) p(y|x) p(o|x,y)


@pytest.mark.parametrize("name", list(CONFIGS))
def test_head_shapes_and_parameter_counts(name):
    cfg = CONFIGS[name]()
    O, H, W, E = cfg.num_orientations, cfg.height, cfg.width, 37
    # rectangle_pin_factorized_model.py:166-303, one Dense per model: inputs -> outputs
    want = {"orientation": [(E, O), (E + O, H), (E + O + 1, W)], "coordinates": [(E, H), (E + 1, W), (E + 2, O)]}
    count = {"orientation": (E + 1) * O + (E + O + 1) * H + (E + O + 2) * W, "coordinates": (E + 1) * H + (E + 2) * W + (E + 3) * O}
    for order in ORDERS:
        heads = FactorisedHeads(E, cfg, order)
        assert [(h.in_features, h.out_features) for h in heads.heads] == want[order]
        assert sum(p.numel() for p in heads.parameters()) == count[order]
        enc = torch.randn(3, E)
        actions = torch.tensor([[0, 1, 2], [O - 1, H - 1, W - 1], [0, 0, 0]], dtype=torch.int32)
        for i, (axis, given) in enumerate(ORDERS[order]):
            x = heads.head_input(i, enc, actions)
            assert x.shape == (3, want[order][i][0]) and x.dtype == torch.float32
            assert torch.equal(x[:, :E], enc)
            assert heads.logits(i, enc, actions).shape == (3, (O, H, W)[axis])
    heads = FactorisedHeads(E, cfg, "orientation")
    x = heads.head_input(2, torch.zeros(2, E), torch.tensor([[O - 1, H - 1, 5], [0, 1, 5]], dtype=torch.int32))
    assert x[0, E:E + O].tolist() == [0.0] * (O - 1) + [1.0]          # the one-hot orientation as float
    assert x[0, E + O].item() == np.float32((H - 1) / H) and x[1, E + O].item() == np.float32(1 / H)  # x / H as float32
    y = FactorisedHeads(E, cfg, "coordinates").head_input(2, torch.zeros(1, E), torch.tensor([[0, 2, W - 1]], dtype=torch.int32))
    assert y[0, E:].tolist() == [np.float32(2 / H), np.float32((W - 1) / W)]
    with pytest.raises(ValueError):
        FactorisedHeads(E, cfg, "rows")


def _stage_rows(cfg, axis, given, rng):
    """Synthetic rows: every mask class, given values valid, stored values mostly in L; finite float32 logits drawn
    after L is known (torch's chain has no gradient at a -inf logit inside the mask: 0 * -inf)."""
    O, H, W = cfg.num_orientations, cfg.height, cfg.width
    sizes = (O, H, W)
    bits = lc.bits(cfg.kind, O, H, W, rng)
    N = bits.shape[0]
    actions = np.stack([rng.randint(0, s, size=N) for s in sizes], axis=1).astype(np.int32)
    Ls, oks = [], []
    for r in range(N):
        dense = fc.dense_legal(bits[r], O, H, W)
        hit = np.argwhere(dense)
        if hit.size and r % 4:           # a legal triple: every stage's L holds the stored value
            actions[r] = hit[rng.randint(len(hit))]
        L, ok = fc.legal_axis(dense, axis, {a: actions[r, a] for a in given})
        Ls.append(L)
        oks.append(ok)
    L = np.stack(Ls)
    return bits, actions, L, np.array(oks), lc.tame(rng, L, p_neg_inf=0.0)


@pytest.mark.parametrize("order", list(ORDERS))
@pytest.mark.parametrize("name", list(CONFIGS))
def test_evaluate_axis_torch_matches_the_contract(name, order):
    cfg = CONFIGS[name]()
    rng = np.random.RandomState(17)
    for axis, given in ORDERS[order]:
        bits, actions, L, ok, l = _stage_rows(cfg, axis, given, rng)
        N = len(l)
        # |g_H| <= 1: the chain's entropy multiplies the masked logit (finfo.min) by it, and beyond 1 that overflows to NaN
        g_lp, g_h = rng.randn(N), rng.uniform(-1.0, 1.0, size=N)
        x = torch.tensor(l, dtype=torch.float64, requires_grad=True)
        lp, ent = evaluate_axis_torch(cfg, axis, given, x, torch.from_numpy(bits), torch.from_numpy(actions))
        (lp * torch.from_numpy(g_lp) + ent * torch.from_numpy(g_h)).sum().backward()
        for r in range(N):
            want_lp, want_ent, _ = fc.evaluate(l[r], L[r], ok[r], actions[r, axis])
            assert lp[r].item() == pytest.approx(want_lp, abs=1e-9), (axis, r)
            assert ent[r].item() == pytest.approx(want_ent, abs=1e-9), (axis, r)
            want_g = fc.gradient(l[r], L[r], actions[r, axis], g_lp[r], g_h[r])
            assert np.allclose(x.grad[r].numpy(), want_g, atol=1e-9, rtol=0), (axis, r)
    # a given value outside its axis leaves the row empty; a stored value outside L gives log_prob 0
    axis, given = ORDERS[order][2]
    bits, actions, L, ok, l = _stage_rows(cfg, axis, given, rng)
    actions[0, given[0]] = -1
    actions[1, given[1]] = (cfg.num_orientations, cfg.height, cfg.width)[given[1]]
    actions[2, axis] = 1 << 20
    lp, ent = evaluate_axis_torch(cfg, axis, given, torch.from_numpy(l), torch.from_numpy(bits), torch.from_numpy(actions))
    assert lp[:3].tolist() == [0.0, 0.0, 0.0] and ent[:2].tolist() == [0.0, 0.0]
    assert ent[2].item() == pytest.approx(fc.evaluate(l[2], L[2], ok[2], 1 << 20)[1], abs=1e-5)


class _TinyEncoder(torch.nn.Module):
    enc_dim = 12

    def __init__(self, cfg):
        super().__init__()
        self.net = torch.nn.Linear(cfg.height * cfg.width, self.enc_dim)

    def encode(self, obs):
        return torch.tanh(self.net(obs["grid"].float().flatten(1)))


@pytest.mark.parametrize("order", list(ORDERS))
def test_policy_evaluate_on_cpu_tensors(order):
    cfg = CONFIGS["rect_6x6"]()
    rng = np.random.RandomState(23)
    torch.manual_seed(0)
    policy = FactorisedPolicy(_TinyEncoder(cfg), cfg, order)
    bits, actions, _, _, _ = _stage_rows(cfg, 2, (0, 1), rng)
    N = len(bits)
    obs = {"grid": torch.from_numpy(rng.randint(0, 2, size=(N, cfg.height, cfg.width)).astype(np.uint8))}
    env = types.SimpleNamespace(cfg=cfg)  # CPU tensors take evaluate_axis_torch: only the configuration is read
    mb, act = torch.from_numpy(bits), torch.from_numpy(actions)
    lp, ent, value = policy.evaluate(env, obs, mb, act)
    assert lp.shape == ent.shape == value.shape == (N,)
    enc = policy.encoding(obs)
    want_lp = want_ent = 0
    for i, (axis, given) in enumerate(ORDERS[order]):
        a, b = evaluate_axis(env, axis, given, policy.heads.logits(i, enc, act), mb, act)
        want_lp, want_ent = want_lp + a, want_ent + b
    assert torch.equal(lp, want_lp) and torch.equal(ent, want_ent)
    assert (lp <= 0).all() and (ent >= 0).all() and torch.isfinite(lp).all()
    (lp.sum() + 0.1 * ent.sum() + value.sum()).backward()
    for name, p in policy.named_parameters():
        assert p.grad is not None and torch.isfinite(p.grad).all(), name
    for h in policy.heads.heads:
        assert h.weight.grad.abs().sum() > 0


def test_collect_argument_exclusivity():
    def f(*a, **k):
        raise AssertionError("not called")
    with pytest.raises(ValueError, match="factorised_policy"):
        collect(None, 1, policy=f, factorised_policy=f)
    with pytest.raises(ValueError, match="factorised_policy"):
        collect(None, 1, logits_policy=f, factorised_policy=f)
    with pytest.raises(ValueError, match="either policy or logits_policy"):
        collect(None, 1, policy=f, logits_policy=f)


class _Shell(BatchedPlacementEnv):
    """The wrappers' argument checks without a handle: they raise before anything reaches the library."""

    def __init__(self, cfg, num_envs, device):
        self.cfg, self.num_envs, self.device, self._h = cfg, num_envs, torch.device(device), None


def test_wrapper_argument_errors():
    cfg = CONFIGS["spatial_7x100"]()
    O, H, W, B = cfg.num_orientations, cfg.height, cfg.width, 4
    env = _Shell(cfg, B, "cpu")
    assert env._axis_stage(2, (0, 1)) == (2, 3, W) and env._axis_stage(0, 6) == (0, 6, O) and env._axis_stage(1, ()) == (1, 0, H)
    for axis, given in ((3, ()), (-1, ()), (1, (1,)), (0, (0, 2)), (2, 4), (2, 8), (0, (3,))):
        with pytest.raises(ValueError):
            env._axis_stage(axis, given)
    ok = dict(logits=torch.zeros((B, H)), actions=torch.zeros((B, 3), dtype=torch.int32), bits=torch.zeros((B, 2, H, 2), dtype=torch.int64))
    assert env._check_rows(H, ok["logits"], ok["actions"], ok["bits"]) == (B, 0)
    assert env._check_rows(H, ok["logits"].bfloat16(), ok["actions"])[1] == 1
    bad = [
        dict(logits=torch.zeros((B, H), dtype=torch.float64)), dict(logits=torch.zeros((B, H), dtype=torch.float16)),
        dict(logits=torch.zeros((B, H + 1))), dict(logits=torch.zeros(B * H)), dict(logits=torch.zeros((B, 2 * H))[:, ::2]),
        dict(actions=torch.zeros((B, 3), dtype=torch.int64)), dict(actions=torch.zeros(B, dtype=torch.int32)),
        dict(actions=torch.zeros((B + 1, 3), dtype=torch.int32)), dict(actions=torch.zeros((B, 6), dtype=torch.int32)[:, ::2]),
        dict(bits=torch.zeros((B, 2, H, 2), dtype=torch.int32)), dict(bits=torch.zeros((B, 2, H, 1), dtype=torch.int64)),
        dict(bits=torch.zeros((B, 2, H, 4), dtype=torch.int64)[..., ::2]),
    ]
    for change in bad:
        args = dict(ok, **change)
        with pytest.raises(ValueError):
            env._check_rows(H, args["logits"], args["actions"], args["bits"])
        with pytest.raises(ValueError):
            env.evaluate_axis_forward(1, (0,), args["logits"], args["bits"], args["actions"])
        with pytest.raises(ValueError):
            env.evaluate_axis_backward(1, (0,), args["logits"], args["bits"], args["actions"], None, None)
        if "bits" not in change:
            with pytest.raises(ValueError):
                env.sample_axis(1, args["logits"], 0, args["actions"], (0,))
    with pytest.raises(ValueError, match="must have shape"):   # the sampler's rows are the handle's environments
        env.sample_axis(1, torch.zeros((B + 1, H)), 0, torch.zeros((B + 1, 3), dtype=torch.int32), (0,))
    with pytest.raises(ValueError, match="given"):
        env.sample_axis(1, ok["logits"], 0, ok["actions"], (1,))
    for name, t in (("grad_log_prob", torch.zeros(B + 1)), ("grad_entropy", torch.zeros(B, dtype=torch.float64))):
        with pytest.raises(ValueError, match=name):
            env.evaluate_axis_backward(1, (0,), ok["logits"], ok["bits"], ok["actions"], t if name == "grad_log_prob" else None,
                                       t if name == "grad_entropy" else None)
    with pytest.raises(ValueError, match="out must match"):
        env.evaluate_axis_backward(1, (0,), ok["logits"], ok["bits"], ok["actions"], None, None, out=torch.zeros((B, H), dtype=torch.bfloat16))
    with pytest.raises(ValueError, match="must be on"):  # a handle on a GPU refuses host tensors before any device call
        _Shell(cfg, B, "cuda:0")._check_rows(H, ok["logits"], ok["actions"])
