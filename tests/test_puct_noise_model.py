"""csrc/pcb_puct_noise.h -- Dirichlet noise on a root's priors as plain C++ -- against its specification,
pcbenv/search.py:puct_root_noise, on the CPU: tools/puct_noise_check.cpp (AddressSanitizer + UBSan, a program of its own,
nothing preloaded) runs the cases of tests/puct_noise_cases.py and returns prior, noised and the error word after every
call, which must be the specification's bit for bit.  Then the three elementary functions of csrc/pcb_ieee_math.h against
numpy over the arguments the sampler produces, the independence of a root's noise from its batch, and the distribution."""
import shutil

import numpy as np
import pytest
import torch

import puct_cases as pc
import puct_noise_cases as nc
from pcbenv.search import (ieee_exp, ieee_ln, ieee_sqrt, new_puct_tree, noise_base, noise_gammas, noise_uniform, puct_noise_errors,
                           puct_root_noise)

pytestmark = pytest.mark.skipif(shutil.which("g++") is None, reason="no g++")

REL_ERR = 5e-16  # csrc/pcb_ieee_math.h:REL_ERR


def _spec(tree, C, c):
    t = nc.torch_tree(tree)
    prior, noised = puct_root_noise(t, t["noised"], C, c["alpha"], c["eps"], c["seed"], c["step_index"], c["first_root"])
    return prior.numpy(), noised.numpy(), int(puct_noise_errors(t, t["noised"], C))


def test_the_cases_are_what_they_are_there_for():
    nc.check_cases()
    assert new_puct_tree(3, 4, 2, "cpu")["noised"].tolist() == [0, 0, 0] and new_puct_tree(3, 4, 2, "cpu")["noised"].dtype == torch.int32


@pytest.mark.parametrize("name", list(nc.CASES))
def test_the_model_is_the_specification(name):
    c = nc.case(name)
    first, second = nc.run(c.tree, c.C, c.seq)
    before = {f: np.array(v) for f, v in c.tree.items()}
    prior, noised, errors = _spec(c.tree, c.C, c.seq[0])
    for f in c.tree:  # the specification does not modify what it is given
        assert pc.same_bits(c.tree[f], before[f]), f
    assert first["errors"] == errors == 0
    assert pc.same_bits(first["prior"], prior) and np.array_equal(first["noised"], noised) and noised.dtype == np.int32
    # the second call is a no-op, in the model and in the specification
    assert second["errors"] == 0 and pc.same_bits(second["prior"], first["prior"]) and np.array_equal(second["noised"], first["noised"])
    again = dict(c.tree, prior=prior, noised=noised)
    prior2, noised2, errors2 = _spec(again, c.C, c.seq[1])
    assert pc.same_bits(prior2, prior) and np.array_equal(noised2, noised) and errors2 == 0
    # what the kinds mean, on the result
    changed = 0
    for p, kind in enumerate(c.kinds):
        k, fc = int(c.k[p]), int(c.tree["first_child"][p, 0])
        mine = np.zeros(c.N, bool)
        if kind in ("full", "one", "part"):
            mine[fc:fc + k] = True
        assert pc.same_bits(first["prior"][p, ~mine], c.tree["prior"][p, ~mine]), (p, kind)  # nothing but the children
        assert first["noised"][p] == (0 if kind == "none" else 1)
        new, old = first["prior"][p, mine], c.tree["prior"][p, mine]
        assert pc.same_bits(new, new.astype(np.float32).astype(np.float64))  # a prior is a float32 value
        if kind == "one" and c.eps == 1.0:
            assert new.tolist() == [1.0]
        if c.eps == 0.0:
            assert pc.same_bits(new, old)
        if c.eps == 1.0 and k > 1 and mine.any():
            assert abs(new.sum() - 1.0) < k * 2.0 ** -24 and (new >= 0).all()
        changed += int((new != old).sum())
    assert (changed > 0) == (c.eps > 0.0)


@pytest.mark.parametrize("name", list(nc.DAMAGE))
def test_a_damaged_root_is_left_alone(name):
    c, tree, p = nc.damaged(name)
    healthy = nc.run(c.tree, c.C, c.seq[:1])[0]
    st = nc.run(tree, c.C, c.seq[:1])[0]
    prior, noised, errors = _spec(tree, c.C, c.seq[0])
    assert st["errors"] == errors == nc.ERR_TREE and healthy["errors"] == 0
    assert pc.same_bits(st["prior"], prior) and np.array_equal(st["noised"], noised)
    assert pc.same_bits(st["prior"][p], tree["prior"][p]) and st["noised"][p] == 0 and healthy["noised"][p] == 1  # untouched, and a later call finds it
    others = [q for q in range(c.P) if q != p]
    assert pc.same_bits(st["prior"][others], healthy["prior"][others]) and np.array_equal(st["noised"][others], healthy["noised"][others])


# ---- the elementary functions -----------------------------------------------------------------------------------------
def _sampler_arguments():
    """Arguments of the kinds the sampler produces, from its own uniform stream: u and s in (0, 1) down to 2^-103, v around
    1 and far from it, (-2 ln s) / s from 1e-16 to 1e33, ln(u) / alpha down to -708 and below, d."""
    base = noise_base(nc.SEED, torch.arange(2048, dtype=torch.int64), 5)[:, None]
    c = torch.arange(8, dtype=torch.int64)[None, :]
    u = torch.cat([noise_uniform(base, c, t).reshape(-1) for t in range(3)]).numpy()
    tiny = 2.0 ** -np.arange(1, 104, dtype=np.float64)
    near_one = 1.0 - 2.0 ** -np.arange(1, 54, dtype=np.float64)
    s = np.concatenate([u, tiny, near_one, u[:len(tiny)] * tiny])
    v = np.concatenate([(1.0 + 0.6 * (2.0 * u - 1.0)) ** 3, np.exp(100.0 * (u - 0.5)), 1.0 + (2.0 * u[:512] - 1.0) * 2.0 ** -30])
    ln_args = np.concatenate([s, v])
    root_args = np.concatenate([-2.0 * np.log(s) / s, [a - 1.0 / 3.0 for a in (1.01, 1.03, 1.3, 1.0, 2.5, 100.0, 1.99)]])
    exp_args = np.concatenate([np.log(u) / 0.03, np.log(u) / 0.3, np.log(u) / 0.99, -708.0 * u, [0.0, -708.0, -2.0 ** -60, -0.34657, -0.34658]])
    return ln_args, exp_args[exp_args >= -708.0], root_args


def test_the_elementary_functions_are_within_their_bound_and_the_same_in_the_model_and_the_specification():
    ln_args, exp_args, root_args = _sampler_arguments()
    assert ln_args.min() > 0 and ln_args.min() < 1e-30 and ln_args.max() > 1e20 and root_args.max() > 1e30 and root_args.min() < 1e-15
    for name, fn, ref, x in (("ieee_ln", ieee_ln, np.log, ln_args), ("ieee_exp", ieee_exp, np.exp, exp_args), ("ieee_sqrt", ieee_sqrt, np.sqrt, root_args)):
        got = nc.model_function(name, x)
        assert pc.same_bits(got, fn(torch.from_numpy(x)).numpy()), name  # the same operations on either side
        want = ref(x.astype(np.longdouble))
        err = np.abs((got.astype(np.longdouble) - want) / want).max()
        print(f"{name}: {len(x)} arguments, largest relative error {float(err):.3e}")
        assert err < REL_ERR, (name, float(err))
    below = np.array([-708.0000001, -709.0, -745.0, -1e4, -1e300])
    assert (nc.model_function("ieee_exp", below) == 0.0).all() and (ieee_exp(torch.from_numpy(below)) == 0.0).all()
    assert nc.model_function("ieee_exp", [-708.0])[0] > 2.0 ** -1022  # a normal number down to the cut
    assert nc.model_function("ieee_ln", [1.0])[0] == 0.0 and nc.model_function("ieee_sqrt", [4.0, 1.0, 0.25])[0:3].tolist() == [2.0, 1.0, 0.5]


# ---- a root's noise is its own ---------------------------------------------------------------------------------------------
def _flat_tree(P, C, k, value=0.0):
    N = C + 1
    nchild, fchild = np.zeros((P, N), np.int32), np.full((P, N), -1, np.int32)
    nchild[:, 0], fchild[:, 0] = k, 1
    return dict(num_children=nchild, first_child=fchild, prior=np.full((P, N), value, np.float64), noised=np.zeros(P, np.int32))


def test_a_slice_of_a_batch_has_the_bits_of_the_batch():
    c = nc.case("G16_C16_P67")
    whole = nc.run(c.tree, c.C, c.seq[:1])[0]
    for a, b in ((0, 1), (5, 23), (64, 67), (66, 67)):
        part = {f: v[a:b] for f, v in c.tree.items()}
        call = dict(c.seq[0], first_root=c.first_root + a)
        st = nc.run(part, c.C, [call])[0]
        assert pc.same_bits(st["prior"], whole["prior"][a:b]) and np.array_equal(st["noised"], whole["noised"][a:b])
        prior, noised, _ = _spec(part, c.C, call)
        assert pc.same_bits(prior, whole["prior"][a:b])
    # and of the width: the first 3 children of a root drawn alone are the first 3 of 16, before the mix
    base = noise_base(nc.SEED, torch.arange(4, dtype=torch.int64), 9)[:, None]
    g16, _ = noise_gammas(base, torch.arange(16, dtype=torch.int64)[None, :], 0.3)
    g3, _ = noise_gammas(base, torch.arange(3, dtype=torch.int64)[None, :], 0.3)
    assert pc.same_bits(g16[:, :3].contiguous().numpy(), g3.numpy())


def test_another_key_gives_other_values():
    tree = _flat_tree(4, 8, 8)
    base = nc.call(0.3, 1.0, nc.SEED, 77, 0)
    eta = lambda c: nc.run(tree, 8, [c])[0]["prior"][:, 1:]
    e0 = eta(base)
    for other in (dict(base, step_index=78), dict(base, seed=nc.SEED ^ 1), dict(base, first_root=1), dict(base, step_index=77 + (1 << 32))):
        assert (eta(other) != e0).all()
    assert all(len(set(row)) == 8 for row in e0.tolist())  # and another child
    assert pc.same_bits(eta(dict(base, first_root=1))[:3], e0[1:])  # root p + 1 of one batch is root p of the next


# ---- the distribution --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("alpha, k", [(0.03, 16), (0.3, 16), (1.0, 8), (2.5, 4)])
def test_eta_is_dirichlet(alpha, k):
    """P = 4 096 roots, eps = 1, priors 0: the prior left is float32(eta).  Every child's mean within 5 standard errors of
    1 / k; the pooled variance relative to (k - 1) / (k^2 (k alpha + 1)) inside the range 32 numpy batches of the same
    shape show, widened by half its width on either side."""
    P = 4096
    st = nc.run(_flat_tree(P, k, k), k, [nc.call(alpha, 1.0, nc.SEED, 3, 0)])[0]
    eta = st["prior"][:, 1:]
    assert st["errors"] == 0 and (st["noised"] == 1).all() and (eta >= 0).all() and np.abs(eta.sum(axis=1) - 1.0).max() < k * 2.0 ** -24
    var = (k - 1) / (k * k * (k * alpha + 1))
    z = (eta.mean(axis=0) - 1.0 / k) / np.sqrt(var / P)
    print(f"alpha {alpha} k {k}: largest |z| of a child's mean {np.abs(z).max():.2f}")
    assert np.abs(z).max() < 5.0

    def ratio(e):
        return ((e - 1.0 / k) ** 2).mean() / var
    ref = [ratio(np.random.default_rng(i).dirichlet([alpha] * k, P)) for i in range(32)]
    lo, hi = min(ref), max(ref)
    got = ratio(eta)
    print(f"alpha {alpha} k {k}: pooled variance ratio {got:.4f}, numpy's 32 batches {lo:.4f} .. {hi:.4f}")
    assert lo - 0.5 * (hi - lo) <= got <= hi + 0.5 * (hi - lo)
