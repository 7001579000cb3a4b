"""tests/top_priors_cases.py on the CPU: every regime reaches what it is in the table for, the bit rows have the legal
counts they claim, and the float64 contract agrees with pcbenv/search.py:top_priors (torch, CPU) where the two must agree
-- the counts everywhere, the actions in the regimes whose float32 probabilities do not collapse (there torch, which orders
probabilities, falls back to index order while the contract keeps logit order)."""
import numpy as np
import pytest
import torch

import logits_cases as lc
import top_priors_cases as tc
from pcbenv.search import top_priors


def _case(name, regime, bf16=False):
    cfg, O, H, W = tc.geometry(name)
    legal, bits, names = tc.synthetic(name)
    return cfg, O, H, W, legal, tc.logits(name, regime, legal, bf16), names


def test_the_table_covers_every_launch_path_and_mask_class():
    assert {lc.EXPECTED[n][3:] for n in tc.GEOMETRIES} == {(True, 1), (False, 1), (True, 4), (False, 4)}
    assert set(lc.REGIMES) < set(tc.REGIMES) and len(tc.REGIMES) == len(lc.REGIMES) + len(tc.OWN)
    for name in tc.GEOMETRIES:
        legal, bits, names = tc.synthetic(name)
        assert 9 <= len(names) <= 15 and {"none", "last_bit", "full"} <= set(names)
        W = tc.geometry(name)[3]
        assert ("col63" in names) == (W > 63) and ("col64" in names) == ("word1_only" in names) == (W > 64)
        assert legal[names.index("none")].sum() == 0
    assert "plane1_only" in tc.synthetic("rect_33x65")[2] and "plane1_only" not in tc.synthetic("square_3x128")[2]


@pytest.mark.parametrize("name", tc.GEOMETRIES)
def test_constant_logits_are_one_tie_class(name):
    cfg, O, H, W, legal, l, _ = _case(name, "constant")
    assert np.unique(l).size == 1
    count, actions, prior, errors = tc.contract(l, legal, 16, H, W)
    for r in range(legal.shape[0]):
        idx, n = np.flatnonzero(legal[r]), int(legal[r].sum())
        assert tc.flat_of(actions[r], H, W)[:count[r]].tolist() == idx[:16].tolist()
        assert n == 0 or (prior[r, :count[r]] == 1.0 / n).all()  # Z = n exactly
    assert errors == 0


def _wavefront_of(segs, nw):
    """The wavefront that reads segment j in a round of pass 1: 16 lanes per segment, so 4 segments per wavefront."""
    return (segs % (4 * nw)) // 4


@pytest.mark.parametrize("name", tc.GEOMETRIES)
@pytest.mark.parametrize("bf16", [False, True])
def test_four_values_put_the_boundary_inside_a_tie_class_across_segments_and_wavefronts(name, bf16):
    cfg, O, H, W, legal, l, _ = _case(name, "four_values", bf16)
    assert np.unique(l).size == 4
    nw = tc.wavefronts(name)

    def spread(a):
        segs = tc.segment_of(a, O, H, W)
        return np.unique(segs).size > 1 and (nw == 1 or np.unique(_wavefront_of(segs, nw)).size > 1)
    for K in tc.KS:
        cut = [(ties, kept) for ties, kept in tc.threshold_ties(l, legal, K) if 0 < kept < ties.size]  # the class is cut
        assert sum(1 for ties, _ in cut if spread(ties)) >= 2, K
        if K == 64:  # and so are the ones kept: their places cannot come from one wavefront's ballot
            assert sum(1 for ties, kept in cut if spread(ties[:kept])) >= 2


@pytest.mark.parametrize("name", tc.GEOMETRIES)
def test_signed_zeros_tie_by_index(name):
    cfg, O, H, W, legal, l, _ = _case(name, "signed_zeros")
    count, actions, prior, _ = tc.contract(l, legal, 64, H, W)
    mixed = 0
    for r in range(legal.shape[0]):
        flat = tc.flat_of(actions[r], H, W)[:count[r]]
        v = l[r, flat]
        if count[r] == 64 and (v == 0).all():
            assert (np.diff(flat) > 0).all()  # one class: -0.0 and +0.0 interleave in index order
            mixed += int(np.signbit(v).any() and not np.signbit(v).all())
    assert mixed >= 2


@pytest.mark.parametrize("name", tc.GEOMETRIES)
@pytest.mark.parametrize("regime", ["denormals_negative", "denormals_mixed"])
@pytest.mark.parametrize("bf16", [False, True])
def test_denormals_are_kept_and_ordered(name, regime, bf16):
    cfg, O, H, W, legal, l, _ = _case(name, regime, bf16)
    assert set(np.unique(np.abs(l))) >= set(tc.DENORMALS.tolist())  # bfloat16 keeps them
    count, actions, _, _ = tc.contract(l, legal, 64, H, W)
    seen_pos = seen_neg = 0
    for r in range(legal.shape[0]):
        v = l[r, tc.flat_of(actions[r], H, W)[:count[r]]].astype(np.float64)
        assert (np.diff(v) <= 0).all()
        sub = (np.abs(v) > 0) & (np.abs(v) < tc.TINY)
        seen_pos += int((sub & (v > 0)).any())
        seen_neg += int((sub & (v < 0)).any())
    assert seen_neg >= 2 if regime == "denormals_negative" else seen_pos >= 2
    assert (l <= 0).all() if regime == "denormals_negative" else ((l < 0).any() and (l > 0).any())


@pytest.mark.parametrize("name", tc.GEOMETRIES)
def test_few_finite_rows_end_in_neg_inf_entries_in_index_order(name):
    cfg, O, H, W, legal, l, _ = _case(name, "few_finite")
    count, actions, prior, errors = tc.contract(l, legal, 16, H, W)
    tails = 0
    for r in range(legal.shape[0]):
        flat = tc.flat_of(actions[r], H, W)[:count[r]]
        v = l[r, flat]
        finite = int(np.isfinite(v).sum())
        assert finite <= 2 and np.isfinite(v[:finite]).all() and (v[finite:] == -np.inf).all()
        if count[r] > finite:
            tails += 1
            assert (np.diff(flat[finite:]) > 0).all() and not prior[r, finite:].any()
            assert flat[finite:].tolist() == [a for a in np.flatnonzero(legal[r]) if l[r, a] == -np.inf][:count[r] - finite]
    assert tails >= 5 and errors == 0


@pytest.mark.parametrize("name", tc.GEOMETRIES)
def test_bad_rows_take_the_uniform_fallback(name):
    cfg, O, H, W, legal, l, _ = _case(name, "bad_rows")
    count, actions, prior, errors = tc.contract(l, legal, 16, H, W)
    assert errors == tc.ERR_BAD | tc.ERR_ALL_NEG_INF
    kinds = set()
    for r in range(legal.shape[0]):
        idx = np.flatnonzero(legal[r])
        if idx.size:
            kinds.add(r % 3)
            assert tc.flat_of(actions[r], H, W)[:count[r]].tolist() == idx[:16].tolist()
            assert (prior[r, :count[r]] == np.float64(np.float32(1.0 / idx.size))).all()
    assert kinds == {0, 1, 2}


def test_counted_rows_reach_every_count_around_K():
    exact = {K: set() for K in tc.KS}
    for name in tc.GEOMETRIES:
        for K in tc.KS:
            legal, bits, targets = tc.counted(name, K)
            exact[K] |= set(targets)
            count = tc.contract(lc.tame(tc.rng_for("counted", name), legal), legal, K, *tc.geometry(name)[2:])[0]
            assert count.tolist() == [min(K, n) for n in targets]
    for K in tc.KS:
        assert {0, 1, K - 1, K, K + 1} <= exact[K]


def test_bfloat16_inputs_tie_at_the_boundary():
    """8 bits of significand: equal legal logits are frequent, and the K-th boundary falls among them."""
    cut = {name: 0 for name in tc.GEOMETRIES}
    for name in tc.GEOMETRIES:
        cfg, O, H, W, legal, l, _ = _case(name, "tame", bf16=True)
        cut[name] = sum(1 for K in (16, 64) for ties, kept in tc.threshold_ties(l, legal, K) if 0 < kept < ties.size)
    assert sum(cut.values()) >= 20 and all(cut[n] >= 2 for n in tc.GEOMETRIES if tc.wavefronts(n) == 4), cut


def _probabilities_of_top_priors(x, legal):
    """The float32 probabilities pcbenv/search.py:top_priors sorts, as its docstring states them: exp(l - max) / sum."""
    top = torch.where(legal, x, torch.full_like(x, float("-inf"))).max(dim=1, keepdim=True).values
    e = torch.where(legal, torch.exp(x - torch.where(legal.any(dim=1, keepdim=True), top, torch.zeros_like(top))), torch.zeros_like(x))
    return (e / e.sum(dim=1, keepdim=True).clamp(min=torch.finfo(torch.float32).tiny)).numpy()


def _must_agree(l, p32, legal, K):
    """Rows on which a stable sort by float32 probability gives the contract's list: wherever the logit falls along the
    contract's order, up to the end of the class the K-th candidate is in, the probability falls too (equal logits have
    equal probabilities and go by index on both sides; float32 exp and division are monotone, so the next lower logit
    speaks for all below it)."""
    out = np.zeros(legal.shape[0], bool)
    for r in range(legal.shape[0]):
        idx = np.flatnonzero(legal[r])
        order = np.lexsort((idx, -l[r, idx].astype(np.float64)))
        v, p, m = l[r, idx][order], p32[r, idx][order], min(K, idx.size)
        falls = np.flatnonzero(v[:-1] > v[1:])
        upto = np.concatenate([falls[falls < m - 1], falls[falls >= m - 1][:1]])
        out[r] = bool((p[upto] > p[upto + 1]).all())
    return out


@pytest.mark.parametrize("name", tc.GEOMETRIES)
@pytest.mark.parametrize("regime", list(tc.REGIMES))
def test_contract_against_the_torch_chain(name, regime):
    """Counts everywhere.  Actions on every row whose float32 probabilities keep the listed logits apart: where float32
    `exp` makes unequal logits equally probable, or zero, the torch chain falls back to index order and the contract keeps
    logit order.  In the regimes of tc.TORCH_AGREES, up to their K, that is nearly every row (the mismatches counted on
    these rows are of that kind: 1 - 4 of 13 - 15 rows for scale30 at K = 64, one row for near_uniform at K = 64 on two
    geometries); with constant logits the two are bit-identical, priors included."""
    cfg, O, H, W, legal, l, _ = _case(name, regime)
    mask = torch.from_numpy(legal.reshape(-1, O, H, W).astype(np.uint8))
    x = torch.from_numpy(np.where(legal, l, 0.0).astype(np.float32))
    for K in tc.KS:
        count, actions, prior, _ = tc.contract(l, legal, K, H, W)
        t_count, t_actions, t_prior = top_priors(x, mask, K)
        assert t_count.numpy().tolist() == count.tolist()
        assert not actions[np.arange(K)[None, :] >= count[:, None]].any()
        if regime == "constant":
            assert np.array_equal(t_actions.numpy(), actions) and np.array_equal(t_prior.numpy(), prior.astype(np.float32))  # float32(1 / n) on both sides
        if regime == "bad_rows":  # the contract's own ground: the torch chain has no fallback
            continue
        p32 = _probabilities_of_top_priors(x, torch.from_numpy(legal))
        rows = _must_agree(l, p32, legal, K)
        assert np.array_equal(t_actions.numpy()[rows], actions[rows]), (name, regime, K)
        if K <= tc.TORCH_AGREES.get(regime, 0):
            assert rows.sum() > 0.5 * len(rows) and (t_actions.numpy() != actions).any(axis=(1, 2)).sum() <= (1 if K == 64 else 0), (name, regime, K)


def test_nested_lists():
    """The list at K is the head of the list at 64."""
    for name in ("rect_33x65", "pin_40x48"):
        for regime in ("tame", "four_values", "few_finite"):
            cfg, O, H, W, legal, l, _ = _case(name, regime)
            c64, a64, p64, _ = tc.contract(l, legal, 64, H, W)
            for K in (1, 3, 16):
                c, a, p, _ = tc.contract(l, legal, K, H, W)
                assert np.array_equal(c, np.minimum(c64, K)) and np.array_equal(a, a64[:, :K]) and np.array_equal(p, p64[:, :K])
