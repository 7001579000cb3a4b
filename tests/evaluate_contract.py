"""Float64 host restatement of the pcbenv_evaluate_logits / pcbenv_evaluate_logits_backward contract
(include/pcbenv.h), independent of how the kernels scan and reduce: log-probability and entropy of stored actions under
the masked categorical, their gradient with respect to the logits, and the edge cases that are data.  The legal set is
`sampling_contract.legal_flat` of a row's mask bits.  Pinned to the reference's formula (masked logits + RLlib
Categorical logp / entropy), not to the kernels: tests/test_evaluate_logits_abi.py checks it against torch float64
autograd through that chain."""
import numpy as np

import sampling_contract as sc

ERR_NONFINITE, ERR_ALL_NEG_INF, ERR_ACTION = 1, 2, 4
ROW_OK, ROW_ZERO, ROW_NO_ONE_HOT = 0, 1, 2


def legal_rows(bits, num_orientations: int, H: int, W: int) -> np.ndarray:
    """bits: [N, 2, H, WW] (int64 or uint64) -> bool [N, O*H*W]."""
    bits = np.asarray(bits).view(np.uint64)
    return np.stack([sc.legal_flat(bits[r], num_orientations, H, W) for r in range(bits.shape[0])])


def flat_actions(actions, H: int, W: int) -> np.ndarray:
    a = np.asarray(actions).astype(np.int64)
    if a.ndim == 1:
        return a
    return a[:, 0] * H * W + a[:, 1] * W + a[:, 2]


def tuple_in_range(actions, O: int, H: int, W: int) -> np.ndarray:
    a = np.asarray(actions).astype(np.int64)
    if a.ndim == 1:
        return (a >= 0) & (a < O * H * W)
    return (a[:, 0] >= 0) & (a[:, 0] < O) & (a[:, 1] >= 0) & (a[:, 1] < H) & (a[:, 2] >= 0) & (a[:, 2] < W)


def _rows(logits, legal, a, in_range):
    """The per-row pieces every function below needs."""
    l = np.asarray(logits, np.float64)
    legal = np.asarray(legal, bool)
    N, A = l.shape
    a = np.asarray(a, np.int64)
    in_range = (a >= 0) & (a < A) if in_range is None else np.asarray(in_range, bool) & (a >= 0) & (a < A)
    rows = np.arange(N)
    n = legal.sum(1)
    with np.errstate(all="ignore"):
        nonfinite = (legal & ~(l < np.inf)).any(1)  # a legal NaN or +inf
        M = np.where(legal & (l < np.inf), l, -np.inf).max(1) if A else np.full(N, -np.inf)
        all_neg = (n > 0) & ~nonfinite & (M == -np.inf)
        ok = (n > 0) & ~nonfinite & ~all_neg
        live = legal & (l > -np.inf) & ok[:, None]
        d = np.where(live, l - np.where(ok, M, 0.0)[:, None], 0.0)
        w = np.where(live, np.exp(d), 0.0)
        Z = np.where(ok, w.sum(1), 1.0)
        logZ = np.log(Z)
        ent = logZ - (w * d).sum(1) / Z
        a_ok = in_range & legal[rows, np.clip(a, 0, A - 1)]
        la = l[rows, np.clip(a, 0, A - 1)]
    return dict(l=l, legal=legal, n=n, nonfinite=nonfinite, all_neg=all_neg, ok=ok, live=live, d=d, w=w, Z=Z, logZ=logZ,
                M=M, ent=ent, a=a, a_ok=a_ok, la=la, rows=rows)


def evaluate(logits, legal, a, in_range=None):
    """logits [N, A], legal bool [N, A], a int [N] flat (in_range: False where a tuple action was out of range) ->
    (log_prob [N], entropy [N], error bits, row status [N]), float64."""
    r = _rows(logits, legal, a, in_range)
    N = r["l"].shape[0]
    lp, ent, status = np.zeros(N), np.zeros(N), np.full(N, ROW_ZERO)
    bits = 0
    with np.errstate(all="ignore"):
        bad = r["nonfinite"] | r["all_neg"]          # both need n > 0 by construction of all_neg; nonfinite implies n > 0
        logn = np.log(np.maximum(r["n"], 1))
        lp[bad], ent[bad] = -logn[bad], logn[bad]
        if r["nonfinite"].any():
            bits |= ERR_NONFINITE
        if r["all_neg"].any():
            bits |= ERR_ALL_NEG_INF
        ok = r["ok"]
        ent[ok] = r["ent"][ok]
        good = ok & r["a_ok"]
        lp[good] = (r["la"] - r["M"] - r["logZ"])[good]
        status[good] = ROW_OK
        miss = ok & ~r["a_ok"]
        status[miss] = ROW_NO_ONE_HOT
        if miss.any():
            bits |= ERR_ACTION
    return lp, ent, bits, status


def gradient(logits, legal, a, g_lp, g_h, in_range=None):
    """d(sum g_lp log_prob + sum g_h entropy) / d logits, float64 [N, A]:
    g_i = g_lp (1[i = a] - p_i) - g_H p_i (log p_i + Hrow) on the legal set (p_i = 0: the second term is 0), 0 elsewhere;
    zero rows where no action is legal or the row is an error case; no one-hot term where the stored action is not a
    legal one."""
    r = _rows(logits, legal, a, in_range)
    N, A = r["l"].shape
    g_lp = np.zeros(N) if g_lp is None else np.asarray(g_lp, np.float64)
    g_h = np.zeros(N) if g_h is None else np.asarray(g_h, np.float64)
    with np.errstate(all="ignore"):
        p = r["w"] / r["Z"][:, None]
        logp = np.where(p > 0, r["d"] - r["logZ"][:, None], 0.0)
        g = -g_lp[:, None] * p - g_h[:, None] * np.where(p > 0, p * (logp + r["ent"][:, None]), 0.0)
        hot = r["ok"] & r["a_ok"]
        g[r["rows"][hot], r["a"][hot]] += g_lp[hot]
        g = np.where(r["legal"] & r["ok"][:, None], g, 0.0)
    return g
