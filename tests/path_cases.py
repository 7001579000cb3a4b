"""Cases and the CPU oracle of pcbenv_playout_paths (plain module, no test; needs no GPU), built on playout_cases.

`oracle_path_playout` is the contract of include/pcbenv.h restated on the oracle: the root's episode, then transition
t < len(path) applies path[t] and every later one draws with the key (seed, genv, step0 + t), until the first done; `leaf`
is the legal mask before transition len(path), or after the last transition if the episode ended earlier.

`Plan` gives every root of a playout_cases case K = 5 playouts, playout i = r * K + j with a path chosen by j:
  j = 0  an empty path
  j = 1  the first ceil(len / 2) actions of its own path-less playout
  j = 2  all of them
  j = 3  the first max(1, len / 2) actions of its sibling (j + 1) % K
  j = 4  the sibling's first action three times: the second is illegal (the cell is now occupied, or the component
         cursor has moved on), so the episode ends inside the path
path_steps is the longest path, path_len is per playout.  Because the draw key depends on t and not on the path, j = 0, 1, 2
must reproduce the path-less playout; j = 3 follows another playout's prefix and then draws with its own keys.

The run seeds are those of playout_cases: every case used by tests/test_playout_paths_gpu.py contains, with them, what
`mix` asks for (tests/test_path_cases.py checks it on the CPU), so none had to be chosen here."""
import numpy as np

import playout_cases as pc

K = 5
STEP0 = pc.STEP0
GPU_CASES = ("c1", "rect_11x10", "small_pin", "small_spatial", "c3_centroid", "c3_both_t256", "spatial_7x100", "spatial_7x100_t256",
             "pin_100x9", "rect_4x4_full")
BOTH_PARITIES = ("c3_centroid", "spatial_7x100")  # run after an even and an odd number of step launches


def leaf_of(cfg, env):
    """The oracle environment's legal mask as bit rows, uint64 [2, H, WW]."""
    return pc.mask_bits_of(cfg, pc.action_mask_of(env)).copy()


def oracle_path_playout(cfg, inst, hist, seed, genv, step0, limit, path):
    """-> what playout_cases.oracle_playout returns, plus leaf (uint64 [2, H, WW])."""
    from oracle import oracle as orc
    ob = orc.OracleBatch(cfg, 1)
    e = ob.env(0)
    if cfg.kind == pc.KIND_SQUARE:
        e.reset()
    else:
        ob.reset_packed(np.asarray(inst)[None])
    for a in hist:
        e.step_raw(a)
    path = np.asarray(path, np.int32).reshape(-1, 3)
    acts, r, d, inf, leaf = [], 0.0, False, {}, None
    for t in range(limit):
        if t == len(path):
            leaf = leaf_of(cfg, e)
        a = path[t] if t < len(path) else pc.draw(cfg, e, seed, genv, step0 + t)
        r, d, inf = e.step_raw(a)
        acts.append(np.asarray(a, np.int32))
        if d:
            break
    if leaf is None:  # the episode ended on the path, or was cut at its end
        leaf = leaf_of(cfg, e)
    info = np.array([inf["wirelength"], inf["num_intersections"]] if inf else [np.nan, np.nan], np.float64)
    placed_all = cfg.kind != pc.KIND_SQUARE and e.current_component < 0
    return dict(reward=np.float64(r), done=int(d), length=len(acts), info=info, actions=np.array(acts, np.int32).reshape(-1, 3),
                placed_all=bool(placed_all), leaf=leaf)


def paths_of(base, P, k=K):
    """The plan's path of every playout from the path-less playouts `base` (P * k of them)."""
    assert k == K
    out = []
    for i in range(P * k):
        r, j = divmod(i, k)
        own = base[i]["actions"]
        sib = base[r * k + (j + 1) % k]["actions"]
        if j == 0:
            p = own[:0]
        elif j == 1:
            p = own[:(len(own) + 1) // 2]
        elif j == 2:
            p = own
        elif j == 3:
            p = sib[:max(1, len(sib) // 2)]
        else:
            p = np.repeat(sib[:1], 3, axis=0)
        out.append(np.asarray(p, np.int32).reshape(-1, 3))
    return out


class Plan:
    """Roots of a case after max_steps + parity launches, their path-less playouts, the plan's paths and the oracle's
    expectation of every playout, all on the CPU."""

    def __init__(self, name, parity=0):
        cfg = pc.case(name)[0]()
        self.name = name
        self.roots = pc.Roots(name, pc.max_steps(cfg) + parity)
        self.cfg, self.P = self.roots.cfg, self.roots.P
        self.n = self.P * K
        self.root_of = [i // K for i in range(self.n)]
        self.base = pc.oracle_playouts(self.roots, self.root_of, step0=STEP0)
        self.paths = paths_of(self.base, self.P)
        self.path_len = np.array([len(p) for p in self.paths], np.int32)
        self.path_steps = int(self.path_len.max())
        self.limit = max(pc.max_steps(cfg), self.path_steps)  # (rect_4x4_full: episodes of at most 2 transitions, paths of 3)
        self.expected = self.playouts(self.paths, self.limit)

    def playouts(self, paths, limit, root_of=None, first_env_index=0):
        ro, rt = self.root_of if root_of is None else root_of, self.roots
        return [oracle_path_playout(self.cfg, rt.inst[r], rt.hist[r], rt.seed, first_env_index + i, STEP0, limit, paths[i])
                for i, r in enumerate(ro)]

    def path_tensor(self, paths=None, steps=None, fill=0):
        """The paths as int32 [path_steps, n, 3]; rows behind a path's end hold `fill` (they are never read)."""
        paths = self.paths if paths is None else paths
        steps = max(len(p) for p in paths) if steps is None else steps
        t = np.full((steps, len(paths), 3), fill, np.int32)
        for i, p in enumerate(paths):
            t[:len(p), i] = p
        return t

    def flat(self, tuples):
        """[..., 3] tuples as flat actions (all of the plan's path actions are in range)."""
        H, W = self.cfg.height, self.cfg.width
        return (tuples[..., 0].astype(np.int64) * H * W + tuples[..., 1] * W + tuples[..., 2]).astype(np.int32)


def mix(plan):
    """What a plan contains -> (the figures, the conditions of tests/test_path_cases.py that do not hold)."""
    at_end = inside = after = differing = empty = 0
    for i, (e, b) in enumerate(zip(plan.expected, plan.base)):
        n = int(plan.path_len[i])
        if n == 0:
            empty += 1
        elif e["length"] < n:
            inside += 1
        elif e["length"] == n:
            at_end += 1
        else:
            after += 1
            differing += not (e["length"] == b["length"] and np.array_equal(e["actions"], b["actions"]))
    figures = dict(at_end=at_end, inside=inside, after=after, differing=differing, empty=empty)
    need = {"an empty path": empty >= 1, "ended exactly at its path's end": at_end >= 1, "ended inside its path": inside >= 1}
    if plan.name != "rect_4x4_full":  # its first placement ends the episode: nothing is ever drawn behind a path
        need["drew after a non-empty path"] = after >= 1
        need["a continuation that differs from the path-less twin"] = differing >= 1
    return figures, [k for k, v in need.items() if not v]
