"""`puct_search(root_noise=)` on the toy evaluator of tests/test_puct_search.py, on the CPU: eps = 0 is the search without
noise, bit for bit; with eps = 1 the root's priors are exactly `puct_root_noise` of the evaluator's; no prior below depth 1
differs from the evaluator's; a kept tree is noised before its first descent, once."""
from types import SimpleNamespace

import pytest
import torch

import puct_cases as pc
import test_puct_search as toy
from pcbenv.search import PUCT_TREE_TENSORS, puct_root_noise, puct_search, search_tree

P, C, K, SEED = 4, 2, 2, 0x1234ABCD5678


def _search(iterations, **kw):
    root = SimpleNamespace(num_envs=P, device="cpu")
    return puct_search(root, iterations, 7, toy.evaluator_for(P, K), c_puct=1.0, max_children=C, max_steps=toy.T, **kw)


def _same_tree(a, b):
    for f in PUCT_TREE_TENSORS + ("child_priors", "child_visits", "child_actions", "action", "root_value", "errors"):
        assert pc.same_bits(getattr(a, f).numpy(), getattr(b, f).numpy()), f


@pytest.mark.parametrize("iterations", [1, 5, 24])
@pytest.mark.parametrize("alpha", [0.3, 2.5])
def test_eps_0_is_the_search_without_noise(iterations, alpha):
    _same_tree(_search(iterations, root_noise=(alpha, 0.0), noise_seed=SEED), _search(iterations))


@pytest.mark.parametrize("iterations", [1, 2, 24])
@pytest.mark.parametrize("alpha, eps", [(0.3, 1.0), (2.5, 0.25)])
def test_the_roots_priors_are_the_noise_of_the_evaluators(iterations, alpha, eps):
    plain, noisy = _search(iterations), _search(iterations, root_noise=(alpha, eps), noise_seed=SEED, noise_first_root=5)
    first = _search(1)  # the tree after the first expansion: what the noise is applied to
    want, noised = puct_root_noise(search_tree(first), torch.zeros(P, dtype=torch.int32), C, alpha, eps, SEED, 7, 5)
    has = first.num_children[:, 0] > 0
    assert noised.tolist() == has.to(torch.int32).tolist() and has.any() and not has.all()  # root 3 is terminal: no children, no noise
    kids = slice(1, 1 + C)  # the root's children are the first nodes made
    assert (first.first_child[:, 0][has] == 1).all()
    assert pc.same_bits(noisy.prior[:, kids].contiguous().numpy(), want[:, kids].contiguous().numpy())
    assert pc.same_bits(noisy.child_priors[has].numpy(), want[:, kids][has].contiguous().numpy())
    assert not pc.same_bits(noisy.prior[:, kids].contiguous().numpy(), plain.prior[:, kids].contiguous().numpy())
    if eps == 1.0:
        assert (noisy.child_priors[has].sum(dim=1) - 1.0).abs().max() < 2.0 ** -22
    # no prior below depth 1 differs from the evaluator's: every such prior is one of the table's
    table = {float(torch.tensor(v, dtype=torch.float32)) for row in toy.PRIOR.values() if row for v in row} | {0.0}
    deep = noisy.depth >= 2
    assert set(noisy.prior[deep].tolist()) <= table and (iterations < 24 or deep.any())
    assert int(noisy.errors) == 0


def test_a_kept_tree_is_noised_once_before_its_first_descent():
    alpha, eps = 0.3, 0.5
    kept = search_tree(_search(6))
    before = {f: kept[f].clone() for f in kept}
    noisy = _search(1, tree=kept, root_noise=(alpha, eps), noise_seed=SEED)
    for f in kept:
        assert pc.same_bits(kept[f].numpy(), before[f].numpy()), f  # the tree given is not modified
    want, noised = puct_root_noise(kept, torch.zeros(P, dtype=torch.int32), C, alpha, eps, SEED, 7, 0)
    has = kept["num_children"][:, 0] > 0
    assert noised.tolist() == has.to(torch.int32).tolist()
    assert pc.same_bits(noisy.prior[:, 1:1 + C].contiguous().numpy(), want[:, 1:1 + C].contiguous().numpy())  # once: not mixed a second time
    again = _search(1, tree=kept, root_noise=(alpha, eps), noise_seed=SEED)
    _same_tree(noisy, again)  # and reproducible
    other = _search(1, tree=kept, root_noise=(alpha, eps), noise_seed=SEED + 1)
    assert not pc.same_bits(noisy.prior.numpy(), other.prior.numpy())


def test_arguments():
    with pytest.raises(ValueError):
        _search(2, root_noise=(0.3, 0.25))  # a root without run_seed needs noise_seed
    for bad in ((0.001, 0.25), (0.3, 1.5), (float("nan"), 0.1), (200.0, 0.0), (0.3, -0.1)):
        with pytest.raises(ValueError):
            _search(2, root_noise=bad, noise_seed=1)
    root = SimpleNamespace(num_envs=P, device="cpu", run_seed=9, first_env_index=2)
    a = puct_search(root, 3, 7, toy.evaluator_for(P, K), max_children=C, max_steps=toy.T, root_noise=(0.3, 0.5))
    b = _search(3, root_noise=(0.3, 0.5), noise_seed=9 ^ 0x6e6f6973, noise_first_root=2)
    _same_tree(a, b)
