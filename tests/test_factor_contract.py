"""The float64 restatement of the axis contract (tests/factor_contract.py) against the reference's own formulation and
against itself: the per-axis legal set equals the reduce_max / gather chain on the unpacked mask for every stage of both
orders, chains of draws end on legal actions, the stage probabilities multiply to a distribution over the legal triples,
and constant logits give the uniform pick.  No device, no library call."""
import numpy as np
import pytest

import factor_contract as fc
import logits_cases as lc
from pcbenv.config import KIND_PIN, KIND_RECT, KIND_SQUARE

GEOMETRIES = [(1, 8, 8), (2, 6, 6), (4, 10, 10), (4, 16, 64), (4, 5, 128), (2, 33, 65), (4, 100, 9), (2, 128, 36), (1, 3, 128)]
KIND_OF = {1: KIND_SQUARE, 2: KIND_RECT, 4: KIND_PIN}


def _rows(O, H, W):
    """(clean uint64 [N, 2, H, WW], dirty twin) of every mask class."""
    rng = np.random.RandomState(O * 100000 + H * 1000 + W)
    clean = np.concatenate([b for _, b, _ in lc.mask_classes(KIND_OF[O], O, H, W, rng)])
    return clean, lc.dirty_twin(clean, KIND_OF[O], W, rng).view(np.uint64)


def _action_mask(bits, O, H, W):
    """The uint8 action_mask [O, H, W] the reference's distributions read, unpacked column by column."""
    m = np.zeros((O, H, W), np.uint8)
    for o in range(O):
        for x in range(H):
            for w in range((W + 63) // 64):
                word = int(bits[o & 1, x, w])
                for y in range(64 * w, min(W, 64 * w + 64)):
                    m[o, x, y] = (word >> (y - 64 * w)) & 1
    return m


def _reference_mask(am, axis, given):
    """factorized_action_distributions.py on action_mask [O, H, W]: :358 reduce_max over (H, W); :398-401 gather o then
    reduce_max over W; :445-448 gather o, x; :717 reduce_max over (o, W); :757-758 gather x then max over o; :803-808
    gather x, y."""
    if axis == 0 and not given:
        return am.max(axis=(1, 2))
    if axis == 1 and set(given) == {0}:
        return am[given[0]].max(axis=1)
    if axis == 2 and set(given) == {0, 1}:
        return am[given[0]][given[1]]
    if axis == 1 and not given:
        return am.max(axis=(0, 2))
    if axis == 2 and set(given) == {1}:
        return am[:, given[1]].max(axis=0)
    if axis == 0 and set(given) == {1, 2}:
        return am[:, given[1], given[2]]
    raise AssertionError("not a stage of the reference")


@pytest.mark.parametrize("O, H, W", GEOMETRIES)
def test_legal_set_is_the_references_mask(O, H, W):
    clean, dirty = _rows(O, H, W)
    rng = np.random.RandomState(3)
    for c, d in zip(clean, dirty):
        am = _action_mask(c, O, H, W)
        dense = fc.dense_legal(c, O, H, W)
        assert np.array_equal(dense, am.astype(bool))
        assert np.array_equal(fc.dense_legal(d, O, H, W), dense)  # columns >= W and the square kind's plane 1 never count
        for stages in fc.ORDERS.values():
            for axis, given_axes in stages:
                for _ in range(6):
                    vals = {a: int(rng.randint((O, H, W)[a])) for a in given_axes}
                    L, ok = fc.legal_axis(dense, axis, vals)
                    assert ok and np.array_equal(L, _reference_mask(am, axis, vals).astype(bool))
        for bad in (-1, H, H + 7):
            L, ok = fc.legal_axis(dense, 2, {1: bad})
            assert not ok and not L.any()


@pytest.mark.parametrize("O, H, W", GEOMETRIES)
def test_chains_of_draws_end_on_legal_actions(O, H, W):
    clean, _ = _rows(O, H, W)
    rng = np.random.RandomState(5)
    sizes = (O, H, W)
    for r, c in enumerate(clean):
        dense = fc.dense_legal(c, O, H, W)
        for order in fc.ALL_ORDERS:
            vals = {}
            for axis, given_axes in fc.stages_of(order):
                L, ok = fc.legal_axis(dense, axis, {a: vals[a] for a in given_axes})
                logits = lc.tame(rng, L[None])[0]
                v, lp, ent, bits = fc.sample(logits, L, ok, fc.hi32_axis(11, r, 2, axis))
                assert bits == 0
                assert L[v] if L.any() else v == 0
                if L.any():
                    assert np.isfinite(lp) and lp <= 0 and 0 <= ent <= np.log(sizes[axis]) + 1e-12
                vals[axis] = v
            if dense.any():
                assert dense[vals[0], vals[1], vals[2]], (order, vals)


@pytest.mark.parametrize("O, H, W", [g for g in GEOMETRIES if g[0] * g[1] * g[2] <= 400])
def test_stage_probabilities_multiply_to_a_distribution(O, H, W):
    clean, _ = _rows(O, H, W)
    rng = np.random.RandomState(9)
    sizes = (O, H, W)
    for c in clean:
        dense = fc.dense_legal(c, O, H, W)
        if not dense.any():
            continue
        for order in fc.ALL_ORDERS:
            # a fixed "network": logits of a stage depend on the given values only
            table = {}

            def logits_of(axis, vals):
                key = (axis, tuple(sorted(vals.items())))
                if key not in table:
                    table[key] = rng.randn(sizes[axis]) * 3.0
                return table[key]
            total = 0.0
            for o, x, y in np.argwhere(dense):
                triple, p = (int(o), int(x), int(y)), 0.0
                for axis, given_axes in fc.stages_of(order):
                    vals = {a: triple[a] for a in given_axes}
                    L, _ = fc.legal_axis(dense, axis, vals)
                    p += fc.log_prob(logits_of(axis, vals), L, triple[axis])
                total += np.exp(p)
            assert abs(total - 1.0) <= 1e-12, (order, total)


@pytest.mark.parametrize("O, H, W", GEOMETRIES)
def test_constant_logits_give_the_uniform_pick(O, H, W):
    clean, _ = _rows(O, H, W)
    rng = np.random.RandomState(13)
    sizes = (O, H, W)
    for r, c in enumerate(clean):
        dense = fc.dense_legal(c, O, H, W)
        for axis in range(3):
            for given_axes in ((), ((axis + 1) % 3,), ((axis + 1) % 3, (axis + 2) % 3)):
                vals = {a: int(rng.randint(sizes[a])) for a in given_axes}
                L, ok = fc.legal_axis(dense, axis, vals)
                if not L.any():
                    assert fc.sample(np.zeros(sizes[axis]), L, ok, 123) == (0, 0.0, 0.0, 0)
                    continue
                const = np.full(sizes[axis], rng.choice([0.0, 3.25, -7.5]))
                n = int(L.sum())
                for step in range(4):
                    h = fc.hi32_axis(11, r, step, axis)
                    v, lp, ent, bits = fc.sample(const, L, ok, h)
                    assert v == fc.uniform_pick(L, h) == int(np.flatnonzero(L)[(h * n) >> 32]) and bits == 0
                    lo, hi = fc.prefix_interval(const, L, v)
                    assert lo <= h / 2.0 ** 32 < hi
                    assert lp == pytest.approx(-np.log(n), rel=1e-12, abs=1e-15) and ent == pytest.approx(np.log(n), rel=1e-12, abs=1e-15)


def test_salt_separates_the_stages_and_keeps_the_base_hash():
    import sampling_contract as sc
    hs = {fc.hi32_axis(5, 1000, 3, a) for a in range(3)} | {sc.hi32(5, 1000, 3)}
    assert len(hs) == 4
    rnd = sc.mix64((sc.mix64(5 ^ ((sc.GOLDEN * 1001) & sc.M64)) + 3) & sc.M64)
    assert rnd >> 32 == sc.hi32(5, 1000, 3)
    assert fc.hi32_axis(5, 1000, 3, 1) == sc.mix64((rnd + 2 * sc.GOLDEN) & sc.M64) >> 32


def test_error_cases_are_data():
    L = np.array([False, True, True, False, True])
    nan = np.array([np.nan, 0.0, np.nan, 0.0, 1.0])
    assert fc.sample(nan, L, True, 1 << 31)[0] == 2 and fc.sample(nan, L, True, 1 << 31)[3] == fc.ERR_NONFINITE
    assert fc.sample(nan, L, True, 1 << 31, greedy_mode=True)[0] == 2  # the uniform pick in both modes
    neg = np.full(5, -np.inf)
    v, lp, ent, bits = fc.sample(neg, L, True, 0)
    assert (v, bits) == (1, fc.ERR_ALL_NEG_INF) and lp == -np.log(3) and ent == np.log(3)
    assert not fc.gradient(neg, L, 1, 1.0, 1.0).any()
    ok_l = np.array([9.0, 1.0, 2.0, 9.0, 2.0])
    assert fc.greedy(ok_l, L) == 2
    lp, ent, bits = fc.evaluate(ok_l, L, True, 3)
    assert (lp, bits) == (0.0, fc.ERR_VALUE) and ent == pytest.approx(fc.entropy(ok_l, L))
    assert fc.evaluate(ok_l, L, True, 7)[2] == fc.ERR_VALUE
    g = fc.gradient(ok_l, L, 3, 1.0, 0.0)  # the one-hot term is dropped: the row sums to -1
    assert g.sum() == pytest.approx(-1.0) and g[0] == g[3] == 0.0
    assert fc.gradient(ok_l, L, 2, 1.0, 0.5).sum() == pytest.approx(0.0, abs=1e-12)
    empty = np.zeros(5, bool)
    assert fc.sample(ok_l, empty, False, 5) == (0, 0.0, 0.0, fc.ERR_GIVEN)
    assert fc.evaluate(ok_l, empty, True, 1) == (0.0, 0.0, 0)
