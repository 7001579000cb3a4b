"""What the tests of pcbenv_top_priors rest on (tests/test_top_priors_cases.py checks it on the CPU,
tests/test_top_priors_model.py runs csrc/pcb_topk.h over it, tests/test_top_priors_gpu.py the kernel): the float64
contract of include/pcbenv_priors.h in numpy, and the case table -- the ragged configurations, the synthetic bit rows and
the logit regimes of tests/logits_cases.py, the regimes a selection needs on top (ties at the K-th boundary, signed
zeros, denormals, -inf tails, bad rows) and bit rows with a legal count around K.  A plain module: nothing here touches a
device."""
import os
import subprocess
import zlib

import numpy as np
import torch

import evaluate_contract as ec
import logits_cases as lc
import model_harness
from pcbenv.rollout import masked_logits

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KS = (1, 3, 16, 64)
GEOMETRIES = tuple(lc.RAGGED)
ERR_BAD, ERR_ALL_NEG_INF = 1, 2
TINY = float(np.finfo(np.float32).tiny)


def rng_for(*key):
    return np.random.RandomState(zlib.crc32(repr(key).encode()) & 0x7FFFFFFF)


def geometry(name):
    """-> (cfg, O, H, W) of a ragged configuration."""
    cfg = lc.RAGGED[name]()
    return cfg, cfg.num_orientations, cfg.height, cfg.width


def wavefronts(name):
    return lc.EXPECTED[name][4]


def to_dtype(l32, bf16):
    """The values a kernel reads: the float32 logits, or their bfloat16 rounding widened back (exact)."""
    return torch.from_numpy(l32).to(torch.bfloat16).to(torch.float32).numpy() if bf16 else np.asarray(l32, np.float32)


# ---- the contract ---------------------------------------------------------------------------------------------------

def contract(l32, legal, K, H, W):
    """include/pcbenv_priors.h in float64 on float32 logits [N, A] and legal bool [N, A] -> (count int32 [N], actions
    int32 [N, K, 3], prior float64 [N, K], error bits).  Good rows: np.lexsort((index, -v)) on the legal set, prior =
    exp(v - M) / Z over all of it.  Bad rows (a legal NaN / +inf: bit 0; every legal logit -inf: bit 1): the first k legal
    actions in flat order, each float32(1.0 / n).  Entries behind count are zero."""
    N = legal.shape[0]
    count, flat, prior, errors = np.zeros(N, np.int32), np.zeros((N, K), np.int64), np.zeros((N, K), np.float64), 0
    for r in range(N):
        idx = np.flatnonzero(legal[r])
        n = idx.size
        k = count[r] = min(K, n)
        if n == 0:
            continue
        v = l32[r, idx].astype(np.float32)
        nonfinite, all_neg = bool((np.isnan(v) | (v == np.inf)).any()), bool((v == -np.inf).all())
        if nonfinite or all_neg:
            errors |= ERR_BAD if nonfinite else ERR_ALL_NEG_INF
            flat[r, :k], prior[r, :k] = idx[:k], np.float64(np.float32(1.0 / n))
            continue
        v64 = v.astype(np.float64)
        order = np.lexsort((idx, -v64))[:k]
        M = v64.max()
        with np.errstate(under="ignore"):
            Z = np.exp(v64 - M).sum()
            flat[r, :k], prior[r, :k] = idx[order], np.exp(v64[order] - M) / Z
    actions = np.stack([flat // (H * W), (flat % (H * W)) // W, flat % W], axis=2).astype(np.int32)
    return count, actions, prior, errors


def flat_of(actions, H, W):
    a = np.asarray(actions, np.int64)
    return (a[..., 0] * H + a[..., 1]) * W + a[..., 2]


def chain32_probabilities(l32, legal):
    """torch's float32 chain on the CPU: masked_logits, then a float32 softmax -> float32 [N, A]."""
    x = torch.tensor(np.where(legal, l32, 0.0), dtype=torch.float32)
    return torch.softmax(masked_logits(x, torch.from_numpy(legal)), dim=1).numpy()


def chain32_priors(l32, legal, flat, count):
    """That chain gathered at the contract's actions `flat` [N, K] (so it does not depend on torch's sort) -> float64
    [N, K], zero behind count.  The source of e_ref."""
    out = np.take_along_axis(chain32_probabilities(l32, legal).astype(np.float64), flat, axis=1)
    out[np.arange(flat.shape[1])[None, :] >= np.asarray(count)[:, None]] = 0.0
    return out


# ---- bit rows -------------------------------------------------------------------------------------------------------

def synthetic(name):
    """The mask classes of tests/logits_cases.py at this geometry -> (legal bool [n, A], int64 bit rows [n, 2, H, WW], the
    class name of every row)."""
    cfg, O, H, W = geometry(name)
    classes = lc.mask_classes(cfg.kind, O, H, W, rng_for("masks", name))
    clean = np.concatenate([b for _, b, _ in classes])
    names = [c for c, b, _ in classes for _ in range(b.shape[0])]
    return ec.legal_rows(clean, O, H, W), clean.view(np.int64), names


def counted(name, K):
    """Bit rows with a legal count around K -> (legal, bit rows, the counts).  The targets are 0, 1, K - 1, K, K + 1; with
    four orientations one bit is two actions, so an odd target gets the even counts on either side."""
    cfg, O, H, W = geometry(name)
    rng = rng_for("counted", name, K)
    per_bit = 2 if O == 4 else 1
    targets = sorted({t for n in (0, 1, K - 1, K, K + 1) for t in ((n,) if n % per_bit == 0 else (n - 1, n + 1))})
    planes = 1 if O == 1 else 2
    cells = np.zeros((len(targets), 2, H, W), bool)
    for r, n in enumerate(targets):
        picks = rng.choice(planes * H * W, n // per_bit, replace=False)
        cells[r].reshape(2, -1)[picks // (H * W), picks % (H * W)] = True
    clean = lc._pack(cells)
    legal = ec.legal_rows(clean, O, H, W)
    assert legal.sum(1).tolist() == targets
    return legal, clean.view(np.int64), targets


# ---- the regimes of the selection: (rng, legal bool [N, A]) -> float32 [N, A] -----------------------------------------
# Every value below is a bfloat16 as well, so a regime keeps what it is for in either dtype.

def constant(rng, legal):
    return np.full(legal.shape, 0.5, np.float32)


def four_values(rng, legal):
    return rng.choice(np.array([-1.5, 0.25, 0.75, 2.0], np.float32), size=legal.shape)


def signed_zeros(rng, legal):
    return rng.choice(np.array([-0.0, 0.0, -1.0], np.float32), size=legal.shape, p=[0.45, 0.45, 0.1])


DENORMALS = np.array([np.ldexp(1.0, -133), np.ldexp(3.0, -132), np.ldexp(1.0, -130), np.ldexp(5.0, -129)], np.float32)


def denormals_negative(rng, legal):
    return -rng.choice(np.concatenate([DENORMALS, np.array([TINY, 1.0, 3.0], np.float32)]), size=legal.shape)


def denormals_mixed(rng, legal):
    mag = rng.choice(np.concatenate([DENORMALS, np.array([0.0, TINY], np.float32)]), size=legal.shape)
    return np.where(rng.rand(*legal.shape) < 0.5, -mag, mag).astype(np.float32)


def few_finite(rng, legal):
    """At most two finite legal logits per row, the rest -inf: with K >= 3 the list ends in -inf entries in index order."""
    l = np.full(legal.shape, -np.inf, np.float32)
    for e in range(legal.shape[0]):
        idx = np.flatnonzero(legal[e])
        if idx.size:
            keep = rng.choice(idx, min(2, idx.size), replace=False)
            l[e, keep] = rng.randn(keep.size).astype(np.float32)
    return l


def bad_rows(rng, legal):
    """Row r by r % 3: a legal NaN, a legal +inf, every legal logit -inf (illegal ones finite)."""
    l = rng.randn(*legal.shape).astype(np.float32)
    for e in range(legal.shape[0]):
        idx = np.flatnonzero(legal[e])
        if idx.size == 0:
            continue
        if e % 3 == 2:
            l[e, idx] = -np.inf
        else:
            l[e, idx[rng.randint(idx.size)]] = np.nan if e % 3 == 0 else np.inf
    return l


OWN = {"constant": constant, "four_values": four_values, "signed_zeros": signed_zeros, "denormals_negative": denormals_negative,
       "denormals_mixed": denormals_mixed, "few_finite": few_finite, "bad_rows": bad_rows}
REGIMES = {**lc.REGIMES, **OWN}
# where pcbenv/search.py:top_priors (float32 probabilities, stable sort) must give the contract's actions: the regimes
# without collapsed probabilities, scale30 up to K = 16
TORCH_AGREES = {"tame": 64, "peaked30": 64, "near_uniform": 64, "underflow": 64, "huge_spread": 64, "scale30": 16}


def logits(name, regime, legal, bf16=False):
    """The float32 values a kernel reads at this (geometry, regime, dtype): seeded by all three."""
    return to_dtype(REGIMES[regime](rng_for("logits", name, regime), legal), bf16)


def threshold_ties(l32, legal, K):
    """Per row: the flat indices of the legal logits equal to the K-th candidate's value (empty if the row has fewer than K
    or K takes them all), and how many of them the list keeps."""
    out = []
    for r in range(legal.shape[0]):
        idx = np.flatnonzero(legal[r])
        v = l32[r, idx].astype(np.float64)
        if idx.size <= K or np.isnan(v).any():
            out.append((idx[:0], 0))
            continue
        kth = np.sort(-v)[K - 1]
        out.append((idx[-v == kth], int(K - (-v < kth).sum())))
    return out


def segment_of(a, O, H, W):
    """The segment (csrc/pcb_policy_common.h) flat action a belongs to: (orientation, row) major, then the mask word."""
    WW = (W + 63) // 64
    return (a // W) * WW + (a % W) // 64


# ---- csrc/pcb_topk.h on the CPU ---------------------------------------------------------------------------------------
def program():
    """tools/topk_model_check.cpp as tests/model_harness.py:tool builds it; None without g++."""
    return model_harness.tool("topk_model_check")


def model(O, H, W, bits, l32, Ks):
    """The model's lists for rows (int64 bit rows [N, 2, H, WW], float32 logits [N, A]) -> {K: (count int32 [N], actions
    int32 [N, K, 3], prior float32 [N, K], error bits [N])}.  Raises on anything the program or a sanitizer reports."""
    N = l32.shape[0]
    head = np.array([O, H, W, N, len(Ks), *Ks], np.int64).tobytes()
    body = b"".join(np.ascontiguousarray(bits[r]).tobytes() + np.ascontiguousarray(l32[r], np.float32).tobytes() for r in range(N))
    run = subprocess.run([program()], input=head + body, capture_output=True)
    assert run.returncode == 0 and run.stderr == b"", run.stderr.decode()
    words, out, at = np.frombuffer(run.stdout, np.int64), {}, 0
    for K in Ks:
        rows = words[at:at + N * (2 + 4 * K)].reshape(N, 2 + 4 * K)
        at += rows.size
        out[K] = (rows[:, 0].astype(np.int32), rows[:, 2:2 + 3 * K].reshape(N, K, 3).astype(np.int32),
                  rows[:, 2 + 3 * K:].astype(np.uint32).view(np.float32).reshape(N, K), rows[:, 1].astype(np.int64))
    assert at == words.size
    return out
