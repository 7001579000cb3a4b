"""Float64 host restatement of the pcbenv_sample_logits contract (include/pcbenv.h), independent of how the kernel
scans, reduces and selects: the legal flat set from mask_bits(), the counter-based uniform u, the masked
distribution (prefix sums, log-probability, entropy) and the greedy pick."""
import numpy as np

M64 = (1 << 64) - 1
GOLDEN = 0x9E3779B97F4A7C15


def mix64(z: int) -> int:
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
    return z ^ (z >> 31)


def hi32(seed: int, genv: int, step: int) -> int:
    """hi32(rnd), rnd = mix64(mix64(seed ^ GOLDEN*(genv+1)) + step): what pcbenv_sample_actions draws with."""
    seed, genv, step = int(seed), int(genv), int(step)
    return mix64((mix64(seed ^ ((GOLDEN * (genv + 1)) & M64)) + step) & M64) >> 32


def u_of(seed: int, genv: int, step: int) -> float:
    return hi32(seed, genv, step) / 2.0 ** 32


def legal_flat(bits: np.ndarray, num_orientations: int, H: int, W: int) -> np.ndarray:
    """bits: uint64 [2, H, WW] (one environment's mask_bits()) -> bool [O*H*W] in flat action order; orientation o
    reads plane o & 1 (square: plane 0)."""
    bits = np.asarray(bits).view(np.uint64)
    planes = []
    for p in range(min(2, num_orientations)):
        cols = np.arange(W)
        words = bits[p][:, cols // 64]                                   # [H, W]
        planes.append(((words >> (cols % 64).astype(np.uint64)) & np.uint64(1)).astype(bool))
    return np.concatenate([planes[o & 1].reshape(-1) for o in range(num_orientations)])


def uniform_pick(legal: np.ndarray, h32: int) -> int:
    """pcbenv_sample_actions' pick: the (hi32 * n >> 32)-th legal flat action (0 when none is legal)."""
    idx = np.flatnonzero(legal)
    if idx.size == 0:
        return 0
    return int(idx[(h32 * idx.size) >> 32])


def masked(logits: np.ndarray, legal: np.ndarray):
    """-> (M, w, Z): w_i = exp(l_i - M) on the legal set, 0 elsewhere (float64)."""
    l = np.asarray(logits, np.float64)
    M = l[legal].max()
    w = np.zeros(l.shape, np.float64)
    w[legal] = np.exp(l[legal] - M)
    return M, w, w.sum()


def prefix_interval(logits, legal, a: int):
    """(C[a-1] / Z, C[a] / Z): the interval of u that selects flat action a on the inverse CDF."""
    _, w, Z = masked(logits, legal)
    c = np.cumsum(w)
    return (c[a - 1] / Z if a > 0 else 0.0), c[a] / Z


def draw(logits, legal, u: float) -> int:
    """The first legal i whose prefix sum exceeds u * Z."""
    _, w, Z = masked(logits, legal)
    c = np.cumsum(w)
    hit = np.flatnonzero((c > u * Z) & legal & (w > 0))
    return int(hit[0]) if hit.size else int(np.flatnonzero(legal & (w > 0))[-1])


def log_prob(logits, legal, a: int) -> float:
    M, _, Z = masked(logits, legal)
    return float(np.float64(logits[a]) - M - np.log(Z))


def entropy(logits, legal) -> float:
    """log Z - sum p_i (l_i - M) (factorized_action_distributions.py:49-59); a -inf legal logit contributes 0."""
    l = np.asarray(logits, np.float64)
    M, w, Z = masked(l, legal)
    live = legal & (w > 0)
    return float(np.log(Z) - np.sum(w[live] / Z * (l[live] - M)))


def greedy(logits, legal) -> int:
    """argmax over the legal set, the lowest flat index on ties."""
    l = np.where(legal, np.asarray(logits, np.float64), -np.inf)
    return int(np.flatnonzero(l == l[legal].max())[0])
