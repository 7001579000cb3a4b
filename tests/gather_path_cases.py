"""Cases and the CPU oracle of pcbenv_gather_paths (plain module, no test; needs no GPU), built on path_cases.

The plans are path_cases.Plan of path_cases.GPU_CASES: per root an empty path, two prefixes of the root's path-less
playout (the second one whole: it ends the episode with its last action), a prefix of a sibling and a path whose second
action is illegal.  What pcbenv_gather_paths must make of playout i of a plan is the NODE its path names:

`oracle_node` is the contract of include/pcbenv.h restated on the oracle -- the root's instance, a replay of its history,
then the path's actions up to and including the first that reports done -- and gives the node's observation, the
outputs of the last transition applied (None where none was: the source row's then) and the number applied.

`apply_paths` is the same on a HandleModel, after `model.gather(...)`: it is what keeps a handle_model.Run next to a
destination handle, so that Run.compare_oracle checks every bound tensor of every row.

`mix` says what a plan contains of the ends the GPU tests need (tests/test_gather_path_cases.py asserts it on the CPU)."""
import numpy as np

import path_cases as pa
import playout_cases as pc

K, STEP0, GPU_CASES, BOTH_PARITIES = pa.K, pa.STEP0, pa.GPU_CASES, pa.BOTH_PARITIES
NO_ACTION = -9  # what path rows behind a path's end hold on the GPU: no action of any kind


def _info(inf):
    return np.array([inf["wirelength"], inf["num_intersections"]] if inf else [np.nan, np.nan], np.float64)


def oracle_node(cfg, inst, hist, path):
    """-> dict(length, reward, done, info (None x 3 with length 0), obs, leaf, placed_all, valid_last)."""
    from oracle import oracle as orc
    ob = orc.OracleBatch(cfg, 1)
    e = ob.env(0)
    if cfg.kind == pc.KIND_SQUARE:
        e.reset()
    else:
        ob.reset_packed(np.asarray(inst)[None])
    for a in hist:
        e.step_raw(a)
    n, r, d, inf, valid = 0, None, None, None, None
    for a in np.asarray(path, np.int32).reshape(-1, 3):
        before = pa.leaf_of(cfg, e)
        o, x, y = (int(v) for v in a)
        in_range = 0 <= o < cfg.num_orientations and 0 <= x < cfg.height and 0 <= y < cfg.width
        valid = bool(in_range and (before[o & 1, x, y // 64] >> np.uint64(y % 64)) & np.uint64(1))
        r, d, inf = e.step_raw(a)
        n += 1
        if d:
            break
    return dict(length=n, reward=None if n == 0 else np.float64(r), done=None if n == 0 else int(d),
                info=None if n == 0 else _info(inf), obs=e.obs(), leaf=pa.leaf_of(cfg, e),
                placed_all=bool(cfg.kind != pc.KIND_SQUARE and e.current_component < 0), valid_last=valid)


def nodes_of(plan, paths=None, path_len=None):
    """The node of every playout of a plan (paths / path_len: other paths than the plan's, as lists per playout)."""
    paths = plan.paths if paths is None else paths
    out = []
    for i, r in enumerate(plan.root_of):
        p = np.asarray(paths[i], np.int32).reshape(-1, 3)
        if path_len is not None:
            p = p[:int(path_len[i])]
        out.append(oracle_node(plan.cfg, plan.roots.inst[r], plan.roots.hist[r], p))
    return out


def apply_paths(model, taken, paths, path_len):
    """The model of a destination handle behind `model.gather(...)`: row i of `taken` makes transitions t < path_len[i]
    with paths[t, i] ([D, B, 3]) alone, stopping behind the first done; reward / done / info of the selected slot follow
    the last transition applied.  Returns the number of transitions applied per row, int32 [B]."""
    s = model.slot
    length = np.zeros(model.B, np.int32)
    for i in np.flatnonzero(np.asarray(taken, bool)):
        e = model.ob.env(int(i))
        for t in range(int(path_len[i])):
            a = np.ascontiguousarray(paths[t, i], np.int32)
            r, d, inf = e.step_raw(a)
            model.hist[i].append(a.copy())
            model.R[s, i], model.D[s, i], model.I[s, i] = r, d, _info(inf)
            length[i] = t + 1
            if d:
                break
    return length


def decode_flat_paths(cfg, flat):
    """Flat path actions [D, B] as the tuples the wrappers decode them to ([D, B, 3]; out of range: no such action)."""
    return np.stack([np.stack([pc.decode_flat(cfg, int(a)) for a in row]) for row in flat]).astype(np.int32)


def mix(plan, nodes):
    """What a plan contains -> (the figures, the conditions that do not hold)."""
    routed_kind = pc.has_info(plan.cfg)
    empty = inside = placed = routed = stuck = illegal = unread = 0
    for i, nd in enumerate(nodes):
        n, applied = int(plan.path_len[i]), nd["length"]
        if n == 0:
            empty += 1
            continue
        unread += applied < n or n < plan.path_steps
        if applied == n and not nd["done"]:
            inside += 1
        elif nd["done"] and nd["valid_last"]:
            placed += nd["placed_all"]
            stuck += not nd["placed_all"]
            # (routed: the wirelength of the routes, below the worst case an unfinished episode is given)
            routed += bool(nd["placed_all"] and routed_kind and nd["info"][0] < plan.cfg.max_wirelength)
        elif nd["done"]:
            illegal += 1
    figures = dict(empty=empty, inside=inside, placed=placed, routed=routed, stuck=stuck, illegal=illegal, unread=unread)
    need = {"a path of length 0": empty >= 1, "a path ended by an illegal action": illegal >= 1,
            "a row behind whose end path rows are left unread": unread >= 1}
    if plan.name == "rect_4x4_full":
        # its first placement fills the grid: no path ends inside an episode, and every legal end is "no legal cell left"
        need["a path that ends the episode by a legal placement"] = stuck >= 1
    else:
        need["a path that ends inside the episode"] = inside >= 1
        if routed_kind:
            need["a path that ends the episode by placing the last component (a routed reward)"] = routed >= 1
        elif plan.cfg.kind == pc.KIND_SQUARE:
            need["a path that ends the episode by a legal placement"] = stuck >= 1  # the square kind only ends with no legal cell left
        else:
            need["a path that ends the episode by placing the last component"] = placed >= 1
    return figures, [k for k, v in need.items() if not v]
