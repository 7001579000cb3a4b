"""What the tests of pcbenv_evaluate_visits share (tests/test_visits_contract.py, tests/test_visit_targets_model.py on the
CPU, tests/test_evaluate_visits_gpu.py on the GPU): visit targets drawn from a legal set, the two action formats, and the
rows of the edge-case table of include/pcbenv_train.h.  A plain module: nothing here touches a device."""
import numpy as np


def draw_targets(rng, legal, C, max_visits=50):
    """(visits int32 [N, C], flat index int64 [N, C]): C entries per row drawn from the row's legal set with replacement
    (so duplicates occur once C approaches the legal count), about a fifth of them unvisited (visits 0), at least one
    visited per row that has a legal action.  Rows without one: all zero."""
    N = legal.shape[0]
    visits, idx = np.zeros((N, C), np.int32), np.zeros((N, C), np.int64)
    for r in range(N):
        ids = np.flatnonzero(legal[r])
        if ids.size == 0:
            continue
        idx[r] = ids[rng.randint(ids.size, size=C)]
        v = rng.randint(1, max_visits + 1, size=C)
        v[rng.rand(C) < 0.2] = 0
        v[rng.randint(C)] = max(1, v[0])
        visits[r] = v
    return visits, idx


def as_actions(idx, H, W, fmt):
    """flat index int [N, C] -> int32 [N, C] ("flat") or [N, C, 3] ("tuple")."""
    idx = np.asarray(idx, np.int64)
    if fmt == "flat":
        return idx.astype(np.int32)
    HW = H * W
    return np.stack([idx // HW, (idx % HW) // W, idx % W], -1).astype(np.int32)


def planes_legal(rng, O, H, W, N, p=0.5):
    """(cells bool [N, 2, H, W], legal bool [N, O*H*W]): random planes and the flat legal set they mean (orientation o
    reads plane o & 1; O == 1: plane 0 only, plane 1 left empty)."""
    cells = rng.rand(N, 2, H, W) < p
    if O == 1:
        cells[:, 1] = False
    legal = np.stack([cells[:, o & 1] for o in range(O)], 1).reshape(N, O * H * W)
    return cells, legal


# ---- the edge-case table: one row per line of include/pcbenv_train.h ------------------------------------------------
EDGE_ROWS = ("no_legal", "nan", "pos_inf", "all_neg_inf", "plain", "zero_visits_entry", "negative_visits", "illegal_action",
             "out_of_range", "no_target", "duplicates", "target_on_neg_inf")


def edge_batch(rng, legal, l, C, A):
    """One batch holding every row of the table: legal / l are [len(EDGE_ROWS), A] with a legal action in every row and at
    least 2 + an illegal position; returns (legal, logits float32, visits int32 [N, C], flat index int64 [N, C]) modified
    row by row.  C >= 3.  Out-of-range entries carry index A + 5."""
    legal, l = legal.copy(), l.astype(np.float32).copy()
    visits, idx = draw_targets(rng, legal, C)
    visits = np.maximum(visits, 1).astype(np.int32)  # every entry visited, so that what a row changes is all that differs
    row = {n: i for i, n in enumerate(EDGE_ROWS)}
    first = lambda r: np.flatnonzero(legal[r])
    legal[row["no_legal"]] = False
    l[row["nan"], first(row["nan"])[-1]] = np.nan
    l[row["pos_inf"], first(row["pos_inf"])[0]] = np.inf
    l[row["all_neg_inf"], legal[row["all_neg_inf"]]] = -np.inf
    visits[row["zero_visits_entry"], 1] = 0
    visits[row["negative_visits"], 0] = -3
    idx[row["illegal_action"], 2] = np.flatnonzero(~legal[row["illegal_action"]])[0]
    idx[row["out_of_range"], 1] = A + 5
    visits[row["no_target"]] = 0
    idx[row["duplicates"], :] = first(row["duplicates"])[0]
    idx[row["duplicates"], -1] = first(row["duplicates"])[1]
    r = row["target_on_neg_inf"]
    l[r, idx[r, 0]] = -np.inf
    keep = first(r)[first(r) != idx[r, 0]][0]
    l[r, keep] = 0.5  # a finite legal logit remains
    idx[r, 1:] = keep
    return legal, l, visits, idx
