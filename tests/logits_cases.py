"""What the edge tests of the three logits kernels rest on (tests/test_logits_edges_gpu.py; checked on the CPU by
tests/test_logits_cases.py): ragged configurations with the template instantiation each selects, synthetic legal-action
bit rows with their dirty twins, logit regimes, and torch's float32 chain on the CPU, whose error against the float64
contract scales every tolerance.  A plain module: nothing here touches a device."""
import numpy as np
import torch

from pcbenv import EnvConfig
from pcbenv.config import KIND_SQUARE
from pcbenv.rollout import masked_logits

# name -> constructor.  H != W everywhere; 64 < W < 128 gives a partial second mask word (100: 36 columns, 65: one,
# 70: six with a 2-column tail chunk, 68: four); W % 4 != 0 takes one load per legal logit (VEC false); A >= 4096 four
# wavefronts (NW 4).
RAGGED = {
    "spatial_7x100": lambda: EnvConfig.spatial(7, 100, 5, 5, 2, 7, 2, 7, 10, 1, 1, 4, 6, 2, "both", 2, 0.5),
    "pin_100x9": lambda: EnvConfig.pin(100, 9, 5, 5, 2, 6, 2, 6, 12, 3, 2, 4, 6, 2, "centroid", 2, 0.5),
    "rect_33x65": lambda: EnvConfig.rect(33, 65, 1, 9, 1, 9, 40, 5),
    "rect_9x70": lambda: EnvConfig.rect(9, 70, 2, 6, 2, 6, 8, 2),
    "rect_20x68": lambda: EnvConfig.rect(20, 68, 2, 6, 2, 6, 8, 2),
    "pin_40x48": lambda: EnvConfig.pin(40, 48, 7, 6, 2, 6, 2, 5, 14, 8, 3, 7, 9, 2, "both", 4, 0.3),
    "rect_128x36": lambda: EnvConfig.rect(128, 36, 2, 6, 2, 6, 8, 2),
    "square_3x128": lambda: EnvConfig.square(3, 128, 3),
    "square_70x12": lambda: EnvConfig.square(70, 12, 2),
}
# (O, H, W, VEC, NW) with 16- / 8-byte aligned pointers, as select_launch (csrc/pcb_policy_common.h) decides
EXPECTED = {
    "spatial_7x100": (4, 7, 100, True, 1), "pin_100x9": (4, 100, 9, False, 1), "rect_33x65": (2, 33, 65, False, 4),
    "rect_9x70": (2, 9, 70, False, 1), "rect_20x68": (2, 20, 68, True, 1), "pin_40x48": (4, 40, 48, True, 4),
    "rect_128x36": (2, 128, 36, True, 4), "square_3x128": (1, 3, 128, True, 1), "square_70x12": (1, 70, 12, True, 1),
}
# the ragged environments the sampler's tests run whole episodes of
SAMPLER_RAGGED = ("spatial_7x100", "pin_100x9", "rect_33x65", "rect_9x70", "square_3x128", "pin_40x48")
NW4_MIN_A = 4096


def launch_path(cfg, aligned=True):
    """(VEC, NW) of a launch at this geometry; aligned: the logits (and gradient) pointers sit on 4 elements."""
    A = cfg.num_orientations * cfg.height * cfg.width
    return (cfg.width % 4 == 0 and aligned), (4 if A >= NW4_MIN_A else 1)


# ---- synthetic bit rows --------------------------------------------------------------------------------------------

def _pack(cells):
    """bool [n, 2, H, W] -> uint64 [n, 2, H, WW], bit y % 64 of word y // 64 = column y."""
    n, P, H, W = cells.shape
    out = np.zeros((n, P, H, (W + 63) // 64), np.uint64)
    for y in range(W):
        out[..., y // 64] |= cells[..., y].astype(np.uint64) << np.uint64(y % 64)
    return out


def _count(cells, O):
    """Legal flat actions of bool [n, 2, H, W]: orientation o reads plane o & 1, the square kind plane 0 only."""
    per_plane = cells.reshape(cells.shape[0], 2, -1).sum(2)
    return sum(per_plane[:, o & 1] for o in range(O)).astype(np.int64)


def mask_classes(kind, O, H, W, rng):
    """-> [(class name, clean uint64 [n, 2, H, WW], the legal count each row claims [n])].  Plane 1 of the square kind is
    left zero in the clean rows.  Classes that need a column the grid lacks (63, 64, word 1) or a second plane are left
    out."""
    planes = 1 if kind == KIND_SQUARE else 2
    out = []

    def add(name, cells):
        cells = np.asarray(cells, bool)
        cells[:, planes:] = False
        out.append((name, _pack(cells), _count(cells, O)))

    def one(plane, x, y):
        c = np.zeros((1, 2, H, W), bool)
        c[0, plane, x, y] = True
        return c
    for p in (0.02, 0.5, 0.98):
        add(f"density_{p}", rng.rand(2, 2, H, W) < p)
    add("full", np.ones((1, 2, H, W), bool))
    add("none", np.zeros((1, 2, H, W), bool))
    add("last_bit", one((O - 1) & 1, H - 1, W - 1))
    if W > 63:
        add("col63", one(0, H // 2, 63))
    if W > 64:
        add("col64", one(0, H // 2, 64))
        c = rng.rand(2, 2, H, W) < 0.5
        c[..., :64] = False
        add("word1_only", c)
    if planes == 2:
        c = rng.rand(2, 2, H, W) < 0.5
        c[:, 0] = False
        add("plane1_only", c)
    return out


def bits(kind, O, H, W, rng):
    """The clean rows of every class, int64 [N, 2, H, WW] (the dtype mask_bits() returns)."""
    return np.concatenate([b for _, b, _ in mask_classes(kind, O, H, W, rng)]).view(np.int64)


def dirty_twin(clean, kind, W, rng):
    """The same legal set: every bit of columns >= W set and, for the square kind, garbage in plane 1."""
    d = np.array(clean).view(np.uint64).copy()
    WW = d.shape[-1]
    if kind == KIND_SQUARE:
        d[:, 1] = rng.randint(0, 1 << 62, size=d[:, 1].shape).astype(np.uint64) * np.uint64(5) + np.uint64(1)
    if W < 64 * WW:
        d[..., WW - 1] |= ~np.uint64(0) << np.uint64(W - 64 * (WW - 1))
    return d.view(np.int64)


# ---- logit regimes: (rng, legal bool [N, A]) -> float32 [N, A] ------------------------------------------------------

def tame(rng, legal, scale=3.0, p_neg_inf=0.05):
    """The distribution of the existing tests: randn * 3, 5 % -inf, one finite legal logit kept per row."""
    B, A = legal.shape
    l = (rng.randn(B, A) * scale).astype(np.float32)
    l[rng.rand(B, A) < p_neg_inf] = -np.inf
    for e in range(B):
        idx = np.flatnonzero(legal[e])
        if idx.size and not np.isfinite(l[e, idx]).any():
            l[e, idx[0]] = 0.0
    return l


def _scaled(scale):
    return lambda rng, legal: (rng.randn(*legal.shape) * scale).astype(np.float32)


def _peaked(gap):
    def f(rng, legal):
        l = rng.randn(*legal.shape).astype(np.float32)
        for e in range(legal.shape[0]):
            idx = np.flatnonzero(legal[e])
            if idx.size:
                l[e, idx[rng.randint(idx.size)]] += np.float32(gap)
        return l
    return f


def underflow(rng, legal):
    return np.where(rng.rand(*legal.shape) < 0.5, 0.0, -120.0).astype(np.float32)


def near_uniform(rng, legal):
    return (1.0 + 1e-4 * rng.randn(*legal.shape)).astype(np.float32)


HUGE = 3.0e38


def huge_equal(rng, legal):
    return np.full(legal.shape, HUGE, np.float32)


def huge_spread(rng, legal):
    """+-3.0e38 at random, at least one of each among the legal logits of a row that has two."""
    l = np.where(rng.rand(*legal.shape) < 0.5, HUGE, -HUGE).astype(np.float32)
    for e in range(legal.shape[0]):
        idx = np.flatnonzero(legal[e])
        if idx.size == 1:
            l[e, idx] = HUGE
        elif idx.size:
            i, j = rng.choice(idx.size, 2, replace=False)
            l[e, idx[i]], l[e, idx[j]] = HUGE, -HUGE
    return l


REGIMES = {"tame": tame, "scale30": _scaled(30.0), "scale300": _scaled(300.0), "peaked10": _peaked(10.0),
           "peaked30": _peaked(30.0), "underflow": underflow, "near_uniform": near_uniform, "huge_equal": huge_equal,
           "huge_spread": huge_spread}


def offset_pair(rng, legal, bf16):
    """(base, shifted, shift): values on a dyadic grid coarse enough that base + shift is exact in the dtype, so every
    l - M is the same float in both.  float32: multiples of 2^-10 in +-8, shift 4096; bf16: multiples of 1/4 in +-4,
    shift 32."""
    if bf16:
        base, shift = rng.randint(-16, 17, size=legal.shape).astype(np.float32) / np.float32(4.0), np.float32(32.0)
    else:
        base, shift = rng.randint(-8192, 8193, size=legal.shape).astype(np.float32) / np.float32(1024.0), np.float32(4096.0)
    return base, base + shift, float(shift)


def stored_actions(rng, legal, l, peak_rows=False):
    """A random legal action with a finite logit per row (0 where the row has none).  peak_rows: every even row stores
    its largest legal logit and every odd row another one."""
    a = np.zeros(legal.shape[0], np.int64)
    for r in range(legal.shape[0]):
        idx = np.flatnonzero(legal[r])
        fin = idx[np.isfinite(l[r, idx])]
        if fin.size and peak_rows:
            top = int(np.argmax(l[r, fin]))
            a[r] = fin[top] if r % 2 == 0 or fin.size == 1 else np.delete(fin, top)[rng.randint(fin.size - 1)]
        elif fin.size:
            a[r] = fin[rng.randint(fin.size)]
        elif idx.size:
            a[r] = idx[0]
    return a


# ---- torch's float32 chain on the CPU: the source of every e_ref ----------------------------------------------------

def chain32(l, legal, a, g_lp, g_h):
    """masked_logits + Categorical in float32 with autograd -> (log_prob [N], entropy [N], gradient [N, A], finite [N])
    as float64; finite: the rows where all three are finite."""
    x = torch.tensor(np.where(legal, l, 0.0), dtype=torch.float32, requires_grad=True)
    d = torch.distributions.Categorical(logits=masked_logits(x, torch.from_numpy(legal)), validate_args=False)
    lp, ent = d.log_prob(torch.from_numpy(np.asarray(a, np.int64))), d.entropy()
    (lp * torch.from_numpy(np.asarray(g_lp)).float() + ent * torch.from_numpy(np.asarray(g_h)).float()).sum().backward()
    lp, ent, g = lp.detach().double().numpy(), ent.detach().double().numpy(), x.grad.double().numpy()
    return lp, ent, g, np.isfinite(lp) & np.isfinite(ent) & np.isfinite(g).all(1)


def ulp32(x):
    """One float32 ulp at |x| (0 where x is not finite)."""
    x32 = np.abs(np.asarray(x, np.float64)).astype(np.float32)
    with np.errstate(all="ignore"):
        return np.where(np.isfinite(x32), np.spacing(np.where(np.isfinite(x32), x32, np.float32(0))), 0.0).astype(np.float64)
