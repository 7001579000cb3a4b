"""Float64 host restatement of the pcbenv_sample_axis / pcbenv_evaluate_axis / pcbenv_evaluate_axis_backward contract
(include/pcbenv.h), independent of how the kernels derive a stage's legal set, scan and reduce: the dense legal mask
from a row's bit rows, the per-axis legal set L of a stage, the salted uniform u_axis, and -- over L -- the draw, the
greedy pick, log-probability, entropy and the gradient formula.  Pinned to the reference's formulation
(utils/agent/factorized_action_distributions.py:107-818), not to the kernels: tests/test_factor_contract.py checks L
against the reduce_max / gather chain on the unpacked mask."""
import numpy as np

import sampling_contract as sc

AXIS_O, AXIS_X, AXIS_Y = 0, 1, 2
ERR_NONFINITE, ERR_ALL_NEG_INF, ERR_VALUE, ERR_GIVEN = 1, 2, 4, 8
# the stages (axis, given axes) of the two orders the reference ships, and all six orders of the three axes
ORDERS = {"orientation": ((0, ()), (1, (0,)), (2, (0, 1))), "coordinates": ((1, ()), (2, (1,)), (0, (1, 2)))}
ALL_ORDERS = [(0, 1, 2), (0, 2, 1), (1, 0, 2), (1, 2, 0), (2, 0, 1), (2, 1, 0)]


def stages_of(order):
    """(a, b, c) -> ((a, ()), (b, (a,)), (c, (a, b)))."""
    return tuple((ax, tuple(order[:i])) for i, ax in enumerate(order))


def given_bits(given) -> int:
    return sum(1 << a for a in given)


def dense_legal(bits, O: int, H: int, W: int) -> np.ndarray:
    """bits: uint64 [2, H, WW] -> bool [O, H, W]: (o, x, y) is legal when bit y % 64 of word [o & 1, x, y // 64] is set
    (columns >= W never count; O == 1 never looks at plane 1)."""
    bits = np.asarray(bits).view(np.uint64)
    out = np.zeros((O, H, W), bool)
    for o in range(O):
        for y in range(W):
            out[o, :, y] = (bits[o & 1, :, y // 64] >> np.uint64(y % 64)) & np.uint64(1)
    return out


def legal_axis(dense: np.ndarray, axis: int, given: dict):
    """The stage's legal set, bool [n], and whether every given value is inside its axis (False: L is empty, error bit
    3).  given: {axis: value}.  L = the values v of `axis` for which some legal (o, x, y) has coordinate `axis` = v and
    agrees with every given value."""
    n = dense.shape[axis]
    for a, v in given.items():
        if not 0 <= int(v) < dense.shape[a]:
            return np.zeros(n, bool), False
    keep = [slice(None)] * 3
    for a, v in given.items():
        keep[a] = slice(int(v), int(v) + 1)  # the cells that agree with the given value
    return dense[tuple(keep)].any(axis=tuple(a for a in range(3) if a != axis)), True


def hi32_axis(seed: int, genv: int, step: int, axis: int) -> int:
    """hi32(rnd_axis), rnd_axis = mix64(rnd + GOLDEN * (axis + 1)), rnd the value pcbenv_sample_actions uses."""
    seed, genv, step = int(seed), int(genv), int(step)
    rnd = sc.mix64((sc.mix64(seed ^ ((sc.GOLDEN * (genv + 1)) & sc.M64)) + step) & sc.M64)
    return sc.mix64((rnd + sc.GOLDEN * (axis + 1)) & sc.M64) >> 32


def u_axis(seed: int, genv: int, step: int, axis: int) -> float:
    return hi32_axis(seed, genv, step, axis) / 2.0 ** 32


def uniform_pick(L: np.ndarray, h32: int) -> int:
    """Member number (h32 * |L|) >> 32 of L (0 when L is empty)."""
    idx = np.flatnonzero(L)
    return int(idx[(int(h32) * idx.size) >> 32]) if idx.size else 0


def status(logits, L) -> int:
    """0, or the error bit of a row that is not a distribution: 1 a NaN / +inf in L, 2 every logit of L -inf."""
    l = np.asarray(logits, np.float64)[L]
    if l.size == 0:
        return 0
    if not (l < np.inf).all():
        return ERR_NONFINITE
    return ERR_ALL_NEG_INF if (l == -np.inf).all() else 0


def _weights(logits, L):
    l = np.asarray(logits, np.float64)
    M = l[L].max()
    w = np.zeros(l.shape)
    with np.errstate(all="ignore"):
        w[L] = np.exp(l[L] - M)
    return l, M, w, w.sum()


def prefix_interval(logits, L, v: int):
    """(C[v-1] / Z, C[v] / Z): the interval of u that selects v on the inverse CDF over L."""
    _, _, w, Z = _weights(logits, L)
    c = np.cumsum(w)
    return (c[v - 1] / Z if v > 0 else 0.0), c[v] / Z


def draw(logits, L, u: float) -> int:
    """The first v in L, in increasing v, whose prefix sum exceeds u * Z; never a value of weight 0."""
    _, _, w, Z = _weights(logits, L)
    hit = np.flatnonzero((np.cumsum(w) > u * Z) & L & (w > 0))
    return int(hit[0]) if hit.size else int(np.flatnonzero(L & (w > 0))[-1])


def greedy(logits, L) -> int:
    """The lowest argmax over L."""
    l = np.where(L, np.asarray(logits, np.float64), -np.inf)
    return int(np.flatnonzero(L & (l == l[L].max()))[0])


def log_prob(logits, L, v: int) -> float:
    l, M, _, Z = _weights(logits, L)
    return float(l[v] - M - np.log(Z))


def entropy(logits, L) -> float:
    """log Z - sum p_v (l_v - M); a zero weight contributes 0."""
    l, M, w, Z = _weights(logits, L)
    live = L & (w > 0)
    return float(np.log(Z) - np.sum(w[live] / Z * (l[live] - M)))


def sample(logits, L, given_ok: bool, h32: int, greedy_mode: bool = False):
    """What pcbenv_sample_axis returns for one row: (value, log_prob, entropy, error bits)."""
    bits = 0 if given_ok else ERR_GIVEN
    n = int(L.sum())
    if n == 0:
        return 0, 0.0, 0.0, bits
    st = status(logits, L)
    if st:
        return uniform_pick(L, h32), -np.log(n), np.log(n), bits | st
    v = greedy(logits, L) if greedy_mode else draw(logits, L, h32 / 2.0 ** 32)
    return v, log_prob(logits, L, v), entropy(logits, L), bits


def evaluate(logits, L, given_ok: bool, a: int):
    """What pcbenv_evaluate_axis returns for one row: (log_prob, entropy, error bits)."""
    bits = 0 if given_ok else ERR_GIVEN
    n = int(L.sum())
    if n == 0:
        return 0.0, 0.0, bits
    st = status(logits, L)
    if st:
        return -np.log(n), np.log(n), bits | st
    if not (0 <= int(a) < L.size and L[int(a)]):
        return 0.0, entropy(logits, L), bits | ERR_VALUE
    return log_prob(logits, L, int(a)), entropy(logits, L), bits


def gradient(logits, L, a: int, g_lp: float, g_h: float) -> np.ndarray:
    """g_v = g_lp (1[v = a] - p_v) - g_H p_v (log p_v + Hrow) on L (p_v = 0: the second term is 0), 0 elsewhere; a zero
    row where L is empty or the row is no distribution; no one-hot term where a is not in L."""
    g = np.zeros(L.size)
    if not L.any() or status(logits, L):
        return g
    l, M, w, Z = _weights(logits, L)
    p = w / Z
    Hrow = entropy(logits, L)
    with np.errstate(all="ignore"):
        logp = np.where(p > 0, l - M - np.log(Z), 0.0)
    g = np.where(L, -g_lp * p - g_h * np.where(p > 0, p * (logp + Hrow), 0.0), 0.0)
    if 0 <= int(a) < L.size and L[int(a)]:
        g[int(a)] += g_lp
    return g
