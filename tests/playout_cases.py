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
from logits_cases import RAGGED

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


def _spatial_max():
    return EnvConfig.spatial(128, 128, 9, 9, 2, 8, 2, 8, 64, 40, 8, 16, 16, 4, "both", 4, 0.5)


# The shapes at which k_playout takes another path than at the named configurations, same format.  The seeds were picked
# the same way (`edge_mix` below, no device): the first of 3, 2, 6, ... whose roots and playouts, after either number of
# launches, contain what tests/test_playout_gpu.py::test_edge_shapes asserts of the case.  spatial_7x100 also has to give
# test_forced_first_actions four live roots with a bad action and a forced legal action that does not end the playout:
# 3 gives three such roots, 2 only legal actions on a last component, 6 five roots and four playouts that go on.
EDGE_CASES = {
    "spatial_7x100": (RAGGED["spatial_7x100"], {}, 12, 6),                              # WW = 2 on one wavefront, routed, padding bits behind column 100
    "spatial_7x100_t256": (RAGGED["spatial_7x100"], {"threads_per_env": 256}, 12, 6),   # WW = 2, four wavefronts, routed
    "pin_100x9": (RAGGED["pin_100x9"], {}, 12, 3),                                      # 100 rows on 64 lanes: the fold is staged in LDS
    "rect_33x65": (RAGGED["rect_33x65"], {}, 8, 3),                                     # one valid bit in word 1; 40 components
    "pin_40x48_both_k4": (RAGGED["pin_40x48"], {}, 12, 3),                              # beam width 4, W not a power of two
    "rect_128_huge": (lambda: EnvConfig.rect(128, 128, 1, 128, 1, 128, 6, 1), {}, 8, 3),  # placements >= 64 wide, spanning both words
    "spatial_max": (_spatial_max, {}, 4, 3),                                            # 64 components, 256 pins, beam width 4
    "spatial_max_t64": (_spatial_max, {"threads_per_env": 64}, 4, 3),                   # 128 rows and 256 pins on 64 lanes
    "rect_1x1": (lambda: EnvConfig.rect(6, 6, 1, 1, 1, 1, 3, 1), {}, 8, 3),             # 1x1 components
    "rect_4x4_full": (lambda: EnvConfig.rect(4, 4, 4, 4, 4, 4, 2, 2), {}, 8, 3),        # the first placement fills the grid
}
SMALL_GRIDS = ("rect_11x10", "small_pin", "small_spatial")  # where an episode can end with no legal cell left
K = 5
STEP0 = 1000  # step index of a playout's first draw (the roots' own steps use 0, 1, ...)


def case(name):
    """(configuration constructor, handle keywords, roots, run seed) of a case of either table."""
    return CASES[name] if name in CASES else EDGE_CASES[name]


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

    def __init__(self, name, launches, seed=None):
        cfg_fn, self.kw, self.P, self.seed = case(name)
        if seed is not None:  # (a seed search: edge_mix)
            self.seed = seed
        self.cfg, P = cfg_fn(), self.P
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


def placements(roots, root_of, expected):
    """The accepted placements of the playouts of a kind with components: (playout, o, x, y, rows, columns on the grid).
    Every action of a playout is drawn from the legal ones and so accepted -- except from a finished root, which has
    none.  Transition t of a playout from root r places component len(hist[r]) + t; an odd orientation swaps the sides."""
    from pcbenv.instances import unpack_instances
    out, status = [], roots.status()
    for i, (r, e) in enumerate(zip(root_of, expected)):
        if status[r] == "finished":
            continue
        ins = unpack_instances(roots.cfg, np.asarray(roots.inst[r])[None])[0]
        for t in range(e["length"]):
            c = len(roots.hist[r]) + t
            assert c < ins.num_components
            o, x, y = (int(v) for v in e["actions"][t])
            h, w = int(ins.comp_h[c]), int(ins.comp_w[c])
            out.append((i, o, x, y, w if o & 1 else h, h if o & 1 else w))
    return out


def edge_mix(name, roots, expected, k=K):
    """What test_edge_shapes asserts of a case, from the CPU plan alone -> (the figures, the conditions that do not hold)."""
    from collections import Counter
    from pcbenv.instances import unpack_instances
    cfg, P = roots.cfg, roots.P
    root_of = [i // k for i in range(P * k)]
    status = roots.status()
    st = Counter(status)
    ends = Counter("placed" if e["placed_all"] else "stuck" for e in expected)
    lengths = sorted({e["length"] for e in expected})
    mix = dict(status=dict(st), ends=dict(ends), lengths=lengths)
    need = {"a fresh root": st["fresh"] >= 1, "a finished root": st["finished"] >= 1,
            "every playout done": all(e["done"] for e in expected)}
    if name == "rect_4x4_full":
        # the first placement fills the grid and ends the episode: a root is fresh or finished and nothing between
        need["no root between fresh and finished"] = st["mid"] + st["last"] == 0
        need["every end stuck"] = ends["stuck"] == len(expected)
        need["length 1 from every unfinished root"] = all(e["length"] == 1 for e, r in zip(expected, root_of) if status[r] != "finished")
    else:
        need["a mid or last root"] = st["mid"] + st["last"] >= 1
    if P == 12:
        need["3 distinct lengths"] = len(lengths) >= 3
    if name == "rect_33x65":
        need["both ends"] = ends["placed"] >= 1 and ends["stuck"] >= 1
    if name == "rect_128_huge":
        pl = placements(roots, root_of, expected)
        mix.update(wide=sum(pw >= 64 for *_, pw in pl), spanning=sum(y < 64 < y + pw for _, _, _, y, _, pw in pl),
                   tall=sum(ph > 64 for *_, ph, _ in pl))
        need.update({"a placement 64 or more wide": mix["wide"] >= 1, "a placement over both words": mix["spanning"] >= 1,
                     "a placement taller than 64": mix["tall"] >= 1})
    if name.startswith("spatial_max"):
        npins = [unpack_instances(cfg, np.asarray(roots.inst[r])[None])[0].num_pins for r in range(P)]
        routed = [i for i, e in enumerate(expected) if e["placed_all"] and e["info"][0] < cfg.max_wirelength]
        mix.update(pins=npins, routed_over_128_pins=sum(npins[root_of[i]] > 128 for i in routed))
        need["a routed end with more than 128 pins"] = mix["routed_over_128_pins"] >= 1
    return mix, [k for k, v in need.items() if not v]
