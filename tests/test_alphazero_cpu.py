"""pcbenv/alphazero.py without a device: the value-target scan on hand-written reward / done arrays, the loss, and
`visit_targets.cross_entropy` taking the torch branch for CPU tensors."""
from types import SimpleNamespace

import numpy as np
import torch

import visits_cases as vc
from logits_cases import _pack
from pcbenv import visit_targets
from pcbenv.alphazero import AlphaZeroConfig, alphazero_loss, value_targets


def _scan(reward, done):
    z, w = value_targets(torch.tensor(reward, dtype=torch.float32).T.contiguous(), torch.tensor(done, dtype=torch.uint8).T.contiguous())
    return z.T.tolist(), w.T.tolist()


def test_value_targets_scan():
    # one line per root, one column per move
    reward = [[-1.0, -2.0, -3.0, -4.0],    # an episode ending at the last move
              [-1.0, -2.0, -3.0, -4.0],    # an episode ending at move 1, the next one spans the batch end
              [-1.0, -2.0, -3.0, -4.0],    # two episodes of one root, both inside the batch
              [-1.0, -2.0, -3.0, -4.0],    # no episode ends
              [-5.0, -6.0, -7.0, -8.0]]    # every move ends an episode
    done = [[0, 0, 0, 1],
            [0, 1, 0, 0],
            [0, 1, 0, 1],
            [0, 0, 0, 0],
            [1, 1, 1, 1]]
    z, w = _scan(reward, done)
    assert z == [[-4.0, -4.0, -4.0, -4.0], [-2.0, -2.0, 0.0, 0.0], [-2.0, -2.0, -4.0, -4.0], [0.0, 0.0, 0.0, 0.0], [-5.0, -6.0, -7.0, -8.0]]
    assert w == [[1.0, 1.0, 1.0, 1.0], [1.0, 1.0, 0.0, 0.0], [1.0, 1.0, 1.0, 1.0], [0.0, 0.0, 0.0, 0.0], [1.0, 1.0, 1.0, 1.0]]
    # the reward of a move that ends nothing is not a target, whatever it holds
    reward[0][1] = 99.0
    assert _scan(reward, done)[0][0] == [-4.0, -4.0, -4.0, -4.0]
    # float64 rewards and a uint8 done, as SelfPlay holds them
    z64, w64 = value_targets(torch.tensor([[-1.5], [-2.5]], dtype=torch.float64), torch.tensor([[0], [1]], dtype=torch.uint8))
    assert z64.dtype == torch.float64 and z64.tolist() == [[-2.5], [-2.5]] and w64.tolist() == [[1.0], [1.0]]


def test_loss_terms():
    cfg = AlphaZeroConfig(policy_coef=2.0, value_coef=0.5, entropy_coef=0.1)
    ce, ent = torch.tensor([1.0, 3.0]), torch.tensor([0.5, 1.5])
    value, z, w = torch.tensor([1.0, 5.0]), torch.tensor([0.0, 0.0]), torch.tensor([1.0, 0.0])
    loss, policy, vf, e = alphazero_loss(ce, ent, value, z, w, cfg)
    assert (float(policy), float(vf), float(e)) == (2.0, 1.0, 1.0)  # the weighted mse counts the weighted move alone
    assert abs(float(loss) - (2.0 * 2.0 + 0.5 * 1.0 - 0.1 * 1.0)) < 1e-6
    assert float(alphazero_loss(ce, ent, value, z, torch.zeros(2), cfg)[2]) == 0.0  # no episode ended: no value loss, no 0 / 0
    assert AlphaZeroConfig().device_loss is False


def test_cross_entropy_on_cpu_tensors_takes_the_torch_branch(monkeypatch):
    O, H, W = 2, 4, 6
    cfg = SimpleNamespace(num_orientations=O, height=H, width=W)

    class NoKernels:  # a handle whose kernels must not be reached
        def __init__(self):
            self.cfg = cfg

        def __getattr__(self, name):
            raise AssertionError(f"the torch branch must not touch env.{name}")
    rng = np.random.RandomState(0)
    cells, legal = vc.planes_legal(rng, O, H, W, 6)
    visits, idx = vc.draw_targets(rng, legal, 8)
    bits = torch.from_numpy(_pack(cells).view(np.int64))
    tv, ta = torch.from_numpy(visits), torch.from_numpy(vc.as_actions(idx, H, W, "tuple"))
    calls = []
    orig = visit_targets.cross_entropy_torch
    monkeypatch.setattr(visit_targets, "cross_entropy_torch", lambda *a: calls.append(a[0]) or orig(*a))
    x = torch.randn(6, O * H * W, requires_grad=True)
    ce, ent = visit_targets.cross_entropy(NoKernels(), x, bits, tv, ta)
    assert calls == [cfg]
    want_ce, want_ent = orig(cfg, x, bits, tv, ta)
    assert torch.equal(ce, want_ce) and torch.equal(ent, want_ent)
    (ce.sum() + 0.1 * ent.sum()).backward()
    assert x.grad is not None and bool(torch.isfinite(x.grad).all()) and not x.grad[~torch.from_numpy(legal)].any()
