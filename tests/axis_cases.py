"""What the GPU tests of the axis kernels share (tests/test_sample_axis_gpu.py, tests/test_evaluate_axis_gpu.py): the
configurations that reach each path of the kernels, the dense legal mask of a live environment, a stage's legal sets for
a batch of rows and the vectorised float64 distribution over them.  A plain module: the device is touched only through
the environment handed in."""
import numpy as np
import torch

import factor_contract as fc
from logits_cases import RAGGED
from pcbenv import EnvConfig, named_config
from pcbenv.batched_env import BatchedPlacementEnv
from pcbenv.config import KIND_SQUARE

# n < 64 with O = 2 / 1; n = 64 exactly with mirrored planes; a second candidate per lane in y and in x, a partial second
# word, 128 rows, 128 columns; O = 4 on 128 x 128
CONFIGS = {"rect_6x6": lambda: EnvConfig.rect(6, 6, 2, 4, 2, 4, 4, 2), "square_5x5": lambda: EnvConfig.square(5, 5, 2),
           "c3": lambda: named_config("c3"), "c5": lambda: named_config("c5")}
CONFIGS.update({name: RAGGED[name] for name in ("spatial_7x100", "pin_100x9", "rect_128x36", "square_3x128")})
# (configuration, environments): 61 leaves the last workgroup of four rows partial
CASES = [(name, 32 if name == "c5" else 64) for name in CONFIGS] + [("pin_100x9", 61)]
SEED = 7


def make_env(cfg, B, **kw):
    env = BatchedPlacementEnv(cfg, B, queue_depth=kw.pop("queue_depth", 2), run_seed=SEED, **kw)
    env.generate_instances()
    env.reset()
    return env


def episode_steps(cfg):
    return (cfg.max_num_components if cfg.kind != KIND_SQUARE else 6) + 3


def sizes(cfg):
    return cfg.num_orientations, cfg.height, cfg.width


def dense_of_bits(bits, cfg):
    """uint64 / int64 [N, 2, H, WW] -> bool [N, O, H, W]; row 0 is checked against the contract's own unpacking."""
    O, H, W = sizes(cfg)
    bits = np.asarray(bits).view(np.uint64)
    cols = np.arange(W)
    planes = ((bits[:, :, :, cols // 64] >> (cols % 64).astype(np.uint64)) & np.uint64(1)).astype(bool)
    dense = np.stack([planes[:, o & 1] for o in range(O)], axis=1)
    if len(bits):
        assert np.array_equal(dense[0], fc.dense_legal(bits[0], O, H, W))
    return dense


def dense_of(env):
    """bool [B, O, H, W] from the bit rows, checked against the action_mask tensor."""
    dense = dense_of_bits(env.mask_bits().cpu().numpy(), env.cfg)
    assert np.array_equal(dense.reshape(env.num_envs, -1), env.action_mask.reshape(env.num_envs, -1).cpu().numpy().astype(bool))
    return dense


def legal_sets(dense, axis, given, actions):
    """-> (L bool [N, n], given_ok bool [N]) of a stage: row r reads the given columns of actions[r]."""
    out = [fc.legal_axis(dense[r], axis, {a: int(actions[r, a]) for a in given}) for r in range(len(dense))]
    return np.stack([L for L, _ in out]), np.array([ok for _, ok in out])


def host_dist(l, L):
    """Vectorised float64 restatement over [N, n]: (M, Z, prefix C / Z, entropy); rows with an empty L are not compared."""
    with np.errstate(all="ignore"):
        lm = np.where(L, l, -np.inf)
        M = lm.max(1, keepdims=True)
        live = L & (lm > -np.inf)
        d = np.where(live, lm - M, 0.0)
        w = np.where(live, np.exp(d), 0.0)
        Z = w.sum(1, keepdims=True)
        ent = np.log(Z[:, 0]) - (w / Z * d).sum(1)
        return M[:, 0], Z[:, 0], np.cumsum(w, 1) / Z, ent


def as_read(l32, dtype, device):
    """float32 [N, n] -> (the device tensor in `dtype`, float64 of what the kernel reads from it)."""
    dev = torch.from_numpy(l32).to(device).to(dtype).contiguous()
    return dev, dev.float().cpu().numpy().astype(np.float64)


class GridEncoder(torch.nn.Module):
    """A small encoder with the interface FactorisedPolicy asks for: `.encode(obs)` and `.enc_dim`."""
    enc_dim = 16

    def __init__(self, cfg):
        super().__init__()
        self.net = torch.nn.Linear(cfg.height * cfg.width, self.enc_dim)

    def encode(self, obs):
        return torch.tanh(self.net(obs["grid"].float().flatten(1)))
