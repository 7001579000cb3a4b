"""Cases and the CPU oracle of pcbenv_playout (plain module, no test; needs no GPU).

A case is a handle configuration, a number of roots and a run seed.  `Roots` brings the roots of a case to different
depths on the CPU alone -- a HandleModel stepped with the actions the device's uniform sampler would draw
(sampling_contract), rows reset at planned launches -- so that the expectation of a playout exists before any device call
and a test can assert the mix of roots and ends it needs.  `oracle_playout` is the contract of include/pcbenv.h restated
on the oracle: reset_packed(inst), a replay of hist, then draw / step_raw until the first done."""
import numpy as np

from pcbenv import EnvConfig, named_config
from pcbenv.config import KIND_PIN, KIND_SPATIAL, KIND_SQUARE

import sampling_contract as sc
from handle_model import HandleModel

# name -> (configuration, handle keywords, roots, run seed).  The seeds of the small grids were picked with this module
# alone (Roots + oracle_playouts, no device): both ends of an episode occur among the playouts after either number of launches.
CASES = {
    "c1": (lambda: named_config("c1"), {}, 12, 3),
    "rect_11x10": (lambda: EnvConfig.rect(11, 10, 3, 5, 3, 5, 8, 4), {}, 12, 6),
    "c2": (lambda: named_config("c2"), {}, 12, 3),
    "small_pin": (lambda: EnvConfig.pin(10, 10, 3, 4, 2, 4, 2, 4, 6, 1, 2, 4, 5, 2, "centroid", 2, 0.5), {}, 12, 2),
    "small_spatial": (lambda: EnvConfig.spatial(10, 10, 3, 4, 2, 4, 2, 4, 6, 1, 2, 4, 5, 2, "both", 2, 0.5), {}, 12, 2),
    "c3_centroid": (lambda: named_config("c3", "centroid"), {}, 12, 3),
    "c3_beam": (lambda: named_config("c3", "beam"), {}, 12, 3),
    "c3_both": (lambda: named_config("c3", "both"), {}, 12, 3),
    "c4": (lambda: named_config("c4"), {}, 12, 3),
    "c3_both_t256": (lambda: named_config("c3", "both"), {"threads_per_env": 256}, 12, 3),
    "c4_t64": (lambda: named_config("c4"), {"threads_per_env": 64}, 12, 3),
    "c5": (lambda: named_config("c5"), {}, 4, 3),
}
SMALL_GRIDS = ("rect_11x10", "small_pin", "small_spatial")  # where an episode can end with no legal cell left
K = 5
STEP0 = 1000  # step index of a playout's first draw (the roots' own steps use 0, 1, ...)


def max_steps(cfg):
    return (cfg.height // cfg.component_n) * (cfg.width // cfg.component_n) if cfg.kind == KIND_SQUARE else cfg.max_num_components


def action_mask_of(env):
    """The oracle environment's action_mask alone, float64 [O * H * W] (obs() copies every tensor)."""
    import ctypes as C
    from oracle import oracle as orc
    n = C.c_int64()
    p = env._L.orc_obs(env._h, orc._OBS["action_mask"], C.byref(n))
    return np.ctypeslib.as_array(p, shape=(n.value,))


def mask_bits_of(cfg, action_mask):
    """The oracle's action_mask as one environment's bit rows, uint64 [2, H, WW] (what mask_bits() returns)."""
    H, W, WW = cfg.height, cfg.width, (cfg.width + 63) // 64
    m = np.zeros((2, H, 64 * WW), np.uint8)
    planes = (np.asarray(action_mask).reshape(-1, H, W)[:2] != 0)
    m[:planes.shape[0], :, :W] = planes
    return np.packbits(m, axis=-1, bitorder="little").view(np.uint64)


def draw(cfg, env, seed, genv, step):
    """The action pcbenv_sample_actions draws for oracle environment `env`: (o, x, y)."""
    H, W = cfg.height, cfg.width
    legal = sc.legal_flat(mask_bits_of(cfg, action_mask_of(env)), cfg.num_orientations, H, W)
    f = sc.uniform_pick(legal, sc.hi32(seed, genv, step))
    return np.array([f // (H * W), (f % (H * W)) // W, f % W], np.int32)


def decode_flat(cfg, a):
    """A flat action as the wrappers decode it; out of range: no such action."""
    H, W = cfg.height, cfg.width
    if a < 0 or a >= cfg.num_orientations * H * W:
        return np.array([-1, 0, 0], np.int32)
    return np.array([a // (H * W), (a % (H * W)) // W, a % W], np.int32)


class Roots:
    """P roots of a case after `launches` step launches, on the CPU: row i was last reset `depth[i]` launches before the
    end (rows that were never reset again have played the whole time: their episodes are over).  plan[t] is the reset mask
    applied after launch t (None: no reset), actions[t] the actions of launch t."""

    def __init__(self, name, launches):
        cfg_fn, self.kw, self.P, self.seed = CASES[name]
        self.cfg, P = cfg_fn(), CASES[name][2]
        self.launches = launches
        L = max_steps(self.cfg)
        assert launches >= L, "row 0 must have finished its episode"
        # depths: finished, 0, the last transition of a full-length episode, then a spread (the same for both parities of `launches`)
        depth = [launches, 0, L - 1] + [1 + (3 * i) % max(L - 1, 1) for i in range(P - 3)]
        self.depth = np.array(depth[:P])
        self.model = HandleModel(self.cfg, P, 1, 3, False, self.seed)
        self.model.reset()
        self.plan, self.actions = [], []
        for t in range(launches):
            a = np.stack([draw(self.cfg, self.model.ob.env(i), self.seed, i, t) for i in range(P)])
            self.model.step(a)
            self.actions.append(a)
            mask = (self.depth == launches - 1 - t).astype(np.uint8)
            if mask.any():
                self.model.reset(mask)
            self.plan.append(mask if mask.any() else None)
        self.inst, self.hist = self.model.inst, self.model.hist

    def status(self):
        """Per root: 'fresh' (depth 0), 'finished', 'last' (the last component is the current one) or 'mid'."""
        out = []
        for i in range(self.P):
            e = self.model.ob.env(i)
            if self.cfg.kind == KIND_SQUARE:
                done = not (action_mask_of(e) != 0).any()
                out.append("finished" if done else "fresh" if not self.hist[i] else "mid")
                continue
            cur = e.current_component
            legal = (action_mask_of(e) != 0).any()
            if cur < 0 or not legal:
                out.append("finished")
            elif not self.hist[i]:
                out.append("fresh")
            else:
                out.append("last" if self.num_components(i) - 1 == cur else "mid")
        return out

    def num_components(self, i):
        """Components of root i's instance: rect marks them in component_mask, the pin kinds' placement_mask is 0 on padding only."""
        o = self.model.ob.env(i).obs()
        return int((o["component_mask" if "component_mask" in o else "placement_mask"] != 0).sum())


def oracle_playout(cfg, inst, hist, seed, genv, step0, limit, first_action=None):
    """-> dict(reward, done, length, info [2] (NaN where empty), actions [length, 3], placed_all)."""
    from oracle import oracle as orc
    ob = orc.OracleBatch(cfg, 1)
    e = ob.env(0)
    if cfg.kind == KIND_SQUARE:
        e.reset()
    else:
        ob.reset_packed(np.asarray(inst)[None])
    for a in hist:
        e.step_raw(a)
    acts, r, d, inf = [], 0.0, False, {}
    for t in range(limit):
        a = np.asarray(first_action, np.int32) if (t == 0 and first_action is not None) else draw(cfg, e, seed, genv, step0 + t)
        r, d, inf = e.step_raw(a)
        acts.append(a)
        if d:
            break
    info = np.array([inf["wirelength"], inf["num_intersections"]] if inf else [np.nan, np.nan], np.float64)
    placed_all = cfg.kind != KIND_SQUARE and e.current_component < 0
    return dict(reward=np.float64(r), done=int(d), length=len(acts), info=info, actions=np.array(acts, np.int32).reshape(-1, 3),
                placed_all=bool(placed_all))


def oracle_playouts(roots, root_of, step0=STEP0, limit=None, first_env_index=0, first_actions=None):
    """Playout i from root root_of[i]; first_actions: [n, 3] tuples or None."""
    limit = limit or max_steps(roots.cfg)
    return [oracle_playout(roots.cfg, roots.inst[r], roots.hist[r], roots.seed, first_env_index + i, step0, limit,
                           None if first_actions is None else first_actions[i]) for i, r in enumerate(root_of)]


def has_info(cfg):
    return cfg.kind in (KIND_PIN, KIND_SPATIAL)
