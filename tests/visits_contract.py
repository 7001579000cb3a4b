"""Float64 host restatement of the pcbenv_evaluate_visits / pcbenv_evaluate_visits_backward contract
(include/pcbenv_train.h), independent of how the kernels scan and reduce: the cross entropy of the masked categorical
against a sparse visit target, the entropy, their gradient with respect to the logits, the row status and the edge cases
that are data.  The distribution is `evaluate_contract._rows`; what is new here is the target.  Pinned to torch float64
autograd through masked_logits + log_softmax with the dense scattered target (tests/test_visits_contract.py), not to the
kernels.  `target_rows` is what csrc/pcb_visit_targets.h must give entry by entry (tests/test_visit_targets_model.py)."""
import numpy as np

import evaluate_contract as ec

ERR_NONFINITE, ERR_ALL_NEG_INF, ERR_TARGET = 1, 2, 4
ROW_OK, ROW_ZERO, ROW_NO_TARGET = 0, 1, 2


def flat_targets(target_actions, O: int, H: int, W: int):
    """int [N, C, 3] or [N, C] -> (flat index int64 [N, C], in range bool [N, C]); out of range: index 0."""
    a = np.asarray(target_actions).astype(np.int64)
    if a.ndim == 3:
        ok = (a[..., 0] >= 0) & (a[..., 0] < O) & (a[..., 1] >= 0) & (a[..., 1] < H) & (a[..., 2] >= 0) & (a[..., 2] < W)
        a = a[..., 0] * H * W + a[..., 1] * W + a[..., 2]
    else:
        ok = (a >= 0) & (a < O * H * W)
    return np.where(ok, a, 0), ok


def target_rows(legal, visits, idx, in_range):
    """The target side alone, whatever the logits are: (index int64 [N, C], -1 where the entry is not valid; kept int64
    [N, C], the visits of the valid entries, 0 elsewhere; pi float32 [N, C], the weight of the logit entry c names --
    float32(the visits of every valid entry with that index / T) -- 0 where not valid; T int64 [N]; bad bool [N]: an entry
    with negative visits, or visited with an action out of range or not legal)."""
    legal = np.asarray(legal, bool)
    v = np.asarray(visits).astype(np.int64)
    rows = np.arange(v.shape[0])[:, None]
    valid = (v > 0) & in_range & legal[rows, idx]
    bad = ((v < 0) | ((v > 0) & ~valid)).any(1)
    kept = np.where(valid, v, 0)
    T = kept.sum(1)
    index = np.where(valid, idx, -1)
    named = ((index[:, :, None] == index[:, None, :]) * kept[:, None, :]).sum(2)  # entries with the same action add up
    with np.errstate(all="ignore"):
        pi = np.where(valid, named.astype(np.float64) / np.maximum(T, 1)[:, None].astype(np.float64), 0.0).astype(np.float32)
    return index, kept, pi, T, bad


def _targets(r, visits, idx, in_range):
    """Dense float64 pi [N, A] and the per-row pieces; r: evaluate_contract._rows of the logits."""
    N, A = r["l"].shape
    index, _, _, T, bad = target_rows(r["legal"], visits, idx, in_range)
    v = np.asarray(visits).astype(np.float64)
    pi = np.zeros((N, A))
    for n in range(N):
        for c in range(index.shape[1]):
            if index[n, c] >= 0:
                pi[n, index[n, c]] += v[n, c] / float(T[n])  # entries with the same action add up
    return pi, T, bad


def evaluate(logits, legal, visits, idx, in_range):
    """logits [N, A], legal bool [N, A], visits int [N, C], idx / in_range from flat_targets ->
    (cross_entropy [N], entropy [N], error bits, row status [N]), float64."""
    r = ec._rows(logits, legal, np.zeros(len(logits), np.int64), None)
    pi, T, bad_target = _targets(r, visits, idx, in_range)
    N = r["l"].shape[0]
    ce, ent, status = np.zeros(N), np.zeros(N), np.full(N, ROW_ZERO)
    bits = 0
    with np.errstate(all="ignore"):
        bad = r["nonfinite"] | r["all_neg"]
        logn = np.log(np.maximum(r["n"], 1))
        ce[bad], ent[bad] = logn[bad], logn[bad]
        if r["nonfinite"].any():
            bits |= ERR_NONFINITE
        if r["all_neg"].any():
            bits |= ERR_ALL_NEG_INF
        ok = r["ok"]
        ent[ok] = r["ent"][ok]
        if (ok & bad_target).any():
            bits |= ERR_TARGET
        hit = ok & (T > 0)
        # log Z - sum pi (l - M); a target on a legal -inf logit: +inf
        lm = np.where(pi > 0, r["l"] - np.where(ok, r["M"], 0.0)[:, None], 0.0)
        ce[hit] = (r["logZ"] - (pi * lm).sum(1))[hit]
        status[hit] = ROW_OK
        status[ok & (T == 0)] = ROW_NO_TARGET
    return ce, ent, bits, status


def gradient(logits, legal, visits, idx, in_range, g_ce, g_h):
    """d(sum g_ce cross_entropy + sum g_h entropy) / d logits, float64 [N, A]:
    g_i = g_ce (p_i - pi_i) - g_H p_i (log p_i + Hrow) on the legal set (p_i = 0: the second term is 0), 0 elsewhere; zero
    rows where no action is legal or the row is an error case; no g_ce term where T == 0."""
    r = ec._rows(logits, legal, np.zeros(len(logits), np.int64), None)
    pi, T, _ = _targets(r, visits, idx, in_range)
    N, A = r["l"].shape
    g_ce = np.zeros(N) if g_ce is None else np.asarray(g_ce, np.float64)
    g_h = np.zeros(N) if g_h is None else np.asarray(g_h, np.float64)
    g_ce = np.where(T > 0, g_ce, 0.0)
    with np.errstate(all="ignore"):
        p = r["w"] / r["Z"][:, None]
        logp = np.where(p > 0, r["d"] - r["logZ"][:, None], 0.0)
        g = g_ce[:, None] * (p - pi) - g_h[:, None] * np.where(p > 0, p * (logp + r["ent"][:, None]), 0.0)
        g = np.where(r["legal"] & r["ok"][:, None], g, 0.0)
    return g
