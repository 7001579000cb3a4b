"""Monte-Carlo lookahead over forked episodes: the first consumer of `BatchedPlacementEnv.gather_`.

A caller of the reference forks an episode with `copy.deepcopy(env)`, plays it out and keeps the best try.  Here
`best_of_k` forks every root environment into k children of a planner batch with one device-side gather, plays every
child to the end of its episode with the on-device uniform sampler (one `rollout_step` launch per step) and picks, per
root, the child with the highest terminal reward -- with tensor ops only, no host round trip.  The caller then applies
the best child's first action to the root and searches again from the next state (receding-horizon lookahead).

`best_of_k_playouts` gives the same result without the planner batch: `BatchedPlacementEnv.playout` plays the k forks of
every root in one kernel launch that writes no observation (pcbenv_playout).  `action_values` scores candidate first
actions the same way: k playouts behind each candidate, the forced first action of the playout call.

`tree_search` goes deeper than one ply: a batched UCT whose nodes are named by their path from the root and evaluated by
`BatchedPlacementEnv.playout(paths=...)` (pcbenv_playout_paths) -- one launch per iteration for all roots, no planner
batch, no node ever materialised.  `tree_search_device` is the same search with the tree kept by the device
(pcbenv_tree_advance): two launches per iteration and no tensor operation between them.

`policy_backend` replaces the uniform rollout of either search by a policy's: the node a path names is materialised
in a planner batch by `gather_(paths=...)` (pcbenv_gather_paths, one launch), and the rollout behind it draws from the
logits a network gives for the planner's observations.
"""
from __future__ import annotations

from dataclasses import dataclass

import torch


@dataclass
class BestOfK:
    reward: torch.Tensor   # [P] float64: terminal reward of the best child of every root
    child: torch.Tensor    # [P] int64: its index in the planner batch (root p's children are p * k .. p * k + k - 1)
    actions: torch.Tensor  # [T, P, 3] int32: the actions it took, T = max_num_components (rows behind its end: don't care)
    length: torch.Tensor   # [P] int64: steps up to and including its terminal transition
    child_rewards: torch.Tensor  # [P, k] float64: the terminal reward of every child


def child_index(P: int, k: int, device="cpu") -> torch.Tensor:
    """Planner environment i plays root i // k: the gather index arange(P).repeat_interleave(k), int32 [P * k]."""
    return torch.arange(P, dtype=torch.int32, device=device).repeat_interleave(k)


def pick_best(final_reward: torch.Tensor, k: int):
    """Per root, the child with the highest terminal reward (the first such child on ties): (reward [P], planner index [P])."""
    r = final_reward.view(-1, k)
    best = r.argmax(dim=1)
    P = r.shape[0]
    return r.gather(1, best[:, None])[:, 0], torch.arange(P, device=r.device) * k + best


def best_of_k(root, planner, k: int, step_index: int) -> BestOfK:
    """root: P environments; planner: P * k environments of the same definition with auto_reset=False.  Forks every
    root episode k times into the planner (`gather_`), plays every child to its first `done` with the fused sampler
    (draws for steps step_index, step_index + 1, ... -- the children of one root differ by their global environment
    index), and returns the best child per root.  At most max_num_components launches: every transition places a
    component or ends the episode."""
    P = root.num_envs
    if planner.num_envs != P * k:
        raise ValueError(f"the planner needs {P} x {k} = {P * k} environments, it has {planner.num_envs}")
    if planner.auto_reset:
        raise ValueError("the planner must be created with auto_reset=False (a child's episode ends at its first done)")
    dev, n = planner.device, planner.num_envs
    planner.gather_(child_index(P, k, dev), source=root)
    T = root.cfg.max_num_components
    actions = torch.zeros((T, n, 3), dtype=torch.int32, device=dev)
    final = torch.zeros(n, dtype=torch.float64, device=dev)
    length = torch.zeros(n, dtype=torch.int64, device=dev)
    finished = torch.zeros(n, dtype=torch.bool, device=dev)
    for t in range(T):
        _, r, d, _, _ = planner.rollout_step(step_index + t, out=actions[t])
        first = d.bool() & ~finished
        final = torch.where(first, r, final)
        length = torch.where(first, torch.full_like(length, t + 1), length)
        finished |= first
    reward, child = pick_best(final, k)
    return BestOfK(reward, child, actions[:, child], length[child], final.view(P, k))


def select_best(final_reward: torch.Tensor, length: torch.Tensor, actions: torch.Tensor, k: int) -> BestOfK:
    """The tensor half of a best-of-k search (any device): per-child terminal rewards [P * k], lengths [P * k] and actions
    [T, P * k, 3] -> the best child per root, its actions and length, and every child's reward as [P, k]."""
    reward, child = pick_best(final_reward, k)
    return BestOfK(reward, child, actions[:, child], length.to(torch.int64)[child], final_reward.view(-1, k))


def best_of_k_playouts(root, k: int, step_index: int) -> BestOfK:
    """`best_of_k(root, planner, k, step_index)` for a planner with the root's run_seed and first_env_index = 0, without the
    planner: one `root.playout` launch plays the k forks of every root to their end (the same draws, the same
    transitions), and the selection is the same.  Same fields, same values; `actions` rows behind a child's end are zero."""
    po = root.playout(k=k, step_index=step_index, max_steps=root.cfg.max_num_components)
    return select_best(po.reward, po.length, po.actions, k)


@dataclass
class ActionValues:
    mean: torch.Tensor       # [P, A] float64: mean playout reward behind every candidate
    max: torch.Tensor        # [P, A] float64: the best playout reward behind every candidate
    cut_share: torch.Tensor  # 0-dim float64: the share of playouts that were cut before their episode ended


def aggregate_values(reward: torch.Tensor, done: torch.Tensor, P: int, A: int, k: int) -> ActionValues:
    """The tensor half of `action_values` (any device): playout rewards and done flags [P * A * k], playout
    (p * A + a) * k + j being try j of candidate a of root p."""
    r = reward.view(P, A, k)
    return ActionValues(r.mean(dim=2), r.max(dim=2).values, (done == 0).to(torch.float64).mean())


def action_values(root, candidates: torch.Tensor, k: int, step_index: int, max_steps=None) -> ActionValues:
    """Monte-Carlo values of candidate first actions: candidates int32 [P, A, 3]; behind candidate a of root p run k playouts
    that take it as their first action and draw uniformly afterwards (one `root.playout` launch of P * A * k playouts).
    The value is the playouts' final reward (pin kinds: the terminal routing reward; an illegal candidate gives the
    worst-case reward).  Returns the mean and the max per candidate and the share of playouts cut at max_steps."""
    P = root.num_envs
    if candidates.dim() != 3 or candidates.shape[0] != P or candidates.shape[2] != 3:
        raise ValueError(f"candidates must have shape [{P}, A, 3], got {list(candidates.shape)}")
    A = candidates.shape[1]
    first = candidates.to(device=root.device, dtype=torch.int32).repeat_interleave(k, dim=1).reshape(P * A * k, 3)
    po = root.playout(k=A * k, step_index=step_index, first_actions=first, max_steps=max_steps, actions_steps=0)
    return aggregate_values(po.reward, po.done, P, A, k)


@dataclass
class TreeSearch:
    """What `tree_search` returns.  P roots, N = iterations + 1 node slots per root (slot 0 is the root, slots are filled in
    the order the nodes were created), C = max_children."""
    action: torch.Tensor         # [P, 3] int32: the most-visited first action (ties: the lowest child slot)
    child_visits: torch.Tensor   # [P, C] int64: visits of the root's children, 0 where there is none
    child_actions: torch.Tensor  # [P, C, 3] int32: their actions
    best_reward: torch.Tensor    # [P] float64: the reward of the best playout seen (the first such playout on ties)
    best_actions: torch.Tensor   # [T, P, 3] int32: its actions (rows behind its end: don't care)
    best_length: torch.Tensor    # [P] int64
    num_nodes: torch.Tensor      # [P] int64: node slots in use
    parent: torch.Tensor         # [P, N] int64, -1 for the root and for unused slots
    depth: torch.Tensor          # [P, N] int64
    node_action: torch.Tensor    # [P, N, 3] int32: the action that leads from the parent to the node
    visits: torch.Tensor         # [P, N] int64
    value_sum: torch.Tensor      # [P, N] float64: sum of the final rewards of the playouts through the node
    value_max: torch.Tensor      # [P, N] float64: the best of them, -inf for unused slots
    terminal: torch.Tensor       # [P, N] bool: the episode is over at the node
    children: torch.Tensor       # [P, N, C] int64: node slots of the children in the order they were created, -1 = none


def tree_search(root, iterations: int, step_index: int, c_uct: float = 1.0, max_children: int = 4, backend=None,
                max_steps=None) -> TreeSearch:
    """Batched UCT over all P = root.num_envs roots in lock-step, the tree in tensors, one playout launch per iteration and
    no host synchronisation inside the loop.  Iteration m:
      selection  from the root, descend to the child with the highest q + c_uct * sqrt(ln(visits of the node) / visits of
                 the child), q = the child's mean playout reward normalised per root by the smallest and largest playout
                 reward seen so far (0 while they are equal), ties to the lowest child slot; stop at a terminal node or at
                 a node with fewer than max_children children;
      launch     backend(paths, path_len, step_index + m * max_steps): P playouts, playout p forced along the path of root
                 p's selected node (paths int32 [max_steps, P, 3], path_len int32 [P] = the node's depth) and drawing
                 uniformly behind it -- `root.playout(k=1, paths=..., path_len=..., max_steps=max_steps)` by default;
      expansion  the action the playout itself drew at row `depth` becomes a new child of the selected node, or revisits the
                 child that already has that action (no extra sampling launch); the child is terminal if the playout ended
                 with that transition.  A terminal node is never expanded: its playout replays the path and ends on it;
      backup     the playout's final reward is added to visits / value_sum / value_max of the leaf and all its ancestors.
    max_steps: the most transitions of an episode (default: that of root.cfg); it bounds the depth loops.  The playouts of
    iteration m use step indices step_index + m * max_steps + t, so every draw of a search has its own key and a search is
    a function of (the roots, run_seed, step_index).  Needs iterations >= 1.  `backend` may be any callable with that
    signature returning a `Playout` with reward, length and actions (tests: a CPU oracle); everything else is tensor code
    for any device."""
    from .batched_env import default_max_steps
    P, C, M = int(root.num_envs), int(max_children), int(iterations)
    if M < 1 or C < 1:
        raise ValueError("tree_search needs iterations >= 1 and max_children >= 1")
    T = default_max_steps(root.cfg) if max_steps is None else int(max_steps)
    if backend is None:
        backend = lambda paths, path_len, s: root.playout(k=1, step_index=s, paths=paths, path_len=path_len, max_steps=T)
    dev = getattr(root, "device", "cpu")
    N = M + 1
    i64 = dict(dtype=torch.int64, device=dev)
    # one slot, one child column and one path row more than used: where a root has nothing to write, the write goes there
    parent = torch.full((P, N + 1), -1, **i64)
    depth = torch.zeros((P, N + 1), **i64)
    node_action = torch.zeros((P, N + 1, 3), dtype=torch.int32, device=dev)
    visits = torch.zeros((P, N + 1), **i64)
    vsum = torch.zeros((P, N + 1), dtype=torch.float64, device=dev)
    vmax = torch.full((P, N + 1), float("-inf"), dtype=torch.float64, device=dev)
    terminal = torch.zeros((P, N + 1), dtype=torch.bool, device=dev)
    children = torch.full((P, N + 1, C + 1), -1, **i64)
    nchild = torch.zeros((P, N + 1), **i64)
    count = torch.ones(P, **i64)
    lo = torch.full((P,), float("inf"), dtype=torch.float64, device=dev)
    hi = torch.full((P,), float("-inf"), dtype=torch.float64, device=dev)
    best_reward = torch.full((P,), float("-inf"), dtype=torch.float64, device=dev)
    best_actions = torch.zeros((T, P, 3), dtype=torch.int32, device=dev)
    best_length = torch.zeros(P, **i64)
    rows = torch.arange(P, **i64)
    trash = torch.full((P,), N, **i64)
    zero_r = torch.zeros(P, dtype=torch.float64, device=dev)
    ninf_r = torch.full((P,), float("-inf"), dtype=torch.float64, device=dev)
    for m in range(M):
        # selection
        node = torch.zeros(P, **i64)
        paths = torch.zeros((T + 1, P, 3), dtype=torch.int32, device=dev)
        span = torch.where(hi > lo, hi - lo, torch.ones_like(hi))
        for d in range(min(T, m)):  # (iteration m finds no node deeper than m: a bound the host knows without asking the device)
            stop = terminal[rows, node] | (nchild[rows, node] < C)
            ch = children[rows, node, :C]                          # [P, C], all >= 0 where the descent goes on
            chc = ch.clamp(min=0)
            n_c = visits[rows[:, None], chc].clamp(min=1).to(torch.float64)
            q = (vsum[rows[:, None], chc] / n_c - lo[:, None]) / span[:, None]
            q = torch.where((hi > lo)[:, None], q, torch.zeros_like(q))
            n_p = visits[rows, node].clamp(min=1).to(torch.float64)
            ucb = q + c_uct * torch.sqrt(torch.log(n_p)[:, None] / n_c)
            ucb = torch.where(ch >= 0, ucb, torch.full_like(ucb, float("-inf")))
            nxt = chc[rows, ucb.argmax(dim=1)]                     # the first maximum: the lowest child slot
            node = torch.where(stop, node, nxt)
            paths[torch.where(stop, torch.full_like(node, T), torch.full_like(node, d)), rows] = node_action[rows, node]
        dsel = depth[rows, node]
        # launch
        po = backend(paths[:T], dsel.to(torch.int32), int(step_index) + m * T)
        r, L = po.reward.to(torch.float64), po.length.to(torch.int64)
        # expansion: the action drawn at row `depth` (there is one unless the episode ended on the path)
        drew = (L > dsel) & ~terminal[rows, node]
        a = po.actions[dsel.clamp(max=T - 1), rows].to(torch.int32)          # [P, 3]
        ch = children[rows, node, :C]
        same = (ch >= 0) & (node_action[rows[:, None], ch.clamp(min=0)] == a[:, None, :]).all(dim=2) & drew[:, None]
        found = same.any(dim=1)
        old = ch.clamp(min=0)[rows, same.to(torch.int64).argmax(dim=1)]
        make = drew & ~found & (nchild[rows, node] < C)
        slot = torch.where(make, count, trash)
        parent[rows, slot] = torch.where(make, node, torch.full_like(node, -1))
        depth[rows, slot] = torch.where(make, dsel + 1, torch.zeros_like(dsel))
        node_action[rows, slot] = torch.where(make[:, None], a, torch.zeros_like(a))
        terminal[rows, slot] = make & (L <= dsel + 1)
        children[rows, node, torch.where(make, nchild[rows, node], torch.full_like(node, C))] = slot
        nchild[rows, node] += make.to(torch.int64)
        count += make.to(torch.int64)
        leaf = torch.where(found, old, torch.where(make, slot, node))
        # backup
        lo, hi = torch.minimum(lo, r), torch.maximum(hi, r)
        cur = leaf
        for _ in range(min(T, m + 1) + 1):  # the leaf is at depth m + 1 at most
            on = cur >= 0
            idx = torch.where(on, cur, trash)[:, None]
            visits.scatter_add_(1, idx, on.to(torch.int64)[:, None])
            vsum.scatter_add_(1, idx, torch.where(on, r, zero_r)[:, None])
            vmax.scatter_reduce_(1, idx, torch.where(on, r, ninf_r)[:, None], reduce="amax")
            cur = torch.where(on, parent[rows, idx[:, 0]], torch.full_like(cur, -1))
        better = r > best_reward
        best_reward = torch.where(better, r, best_reward)
        best_length = torch.where(better, L, best_length)
        best_actions = torch.where(better[None, :, None], po.actions[:T].to(torch.int32), best_actions)
    ch = children[:, 0, :C]
    child_visits = torch.where(ch >= 0, visits[rows[:, None], ch.clamp(min=0)], torch.zeros_like(ch))
    child_actions = torch.where((ch >= 0)[:, :, None], node_action[rows[:, None], ch.clamp(min=0)], torch.zeros((P, C, 3), dtype=torch.int32, device=dev))
    action = child_actions[rows, child_visits.argmax(dim=1)]
    return TreeSearch(action, child_visits, child_actions, best_reward, best_actions, best_length, count,
                      parent[:, :N], depth[:, :N], node_action[:, :N], visits[:, :N], vsum[:, :N], vmax[:, :N], terminal[:, :N],
                      children[:, :N, :C])


def policy_backend(root, planner, logits_fn, greedy=False):
    """A `backend` for `tree_search` / `tree_search_device` that plays the rollout behind the path with a POLICY instead
    of the uniform draw: `(paths, path_len, step_index0) -> Playout`.  planner: P = root.num_envs environments of the
    root's definition with auto_reset=False, the root's run_seed and first_env_index 0.  logits_fn(obs) -> logits as
    `planner.sample_logits` takes them (a network on the planner's observation dict).

    One call: `planner.gather_(arange(P), source=root, paths=paths, path_len=path_len)` materialises the P nodes the paths
    name (pcbenv_gather_paths, one launch); then for every absolute transition index t = 0 .. max_steps - 1 (max_steps =
    paths.shape[0]) one `logits_fn`, one `planner.sample_logits(..., step_index=step_index0 + t)` and one `planner.step`
    -- a fixed number of launches and no host synchronisation, as in `best_of_k`.  Row i takes part from t = path_len[i]
    on: before that it is handed an action that is no action, (-1, -1, -1), which leaves its state and observations as
    they are (an invalid action is a terminal transition with the state unchanged, and there is no done latch); its
    reward / done of those launches are not looked at.  The draw of transition t has the key (run_seed, i, step_index0 +
    t), that of `root.playout(paths=...)`: constant logits give that call's playouts bit for bit.

    Returns Playout(reward, done, length, info, actions): reward / length / info of each row's first `done` (rows that
    ended on the path report what `gather_` reported; a row cut at max_steps reports its last transition and done = 0);
    actions[t] is the path as given for t < path_len, the action drawn for path_len <= t < length, zero behind."""
    from .batched_env import Playout
    from .config import KIND_PIN, KIND_SPATIAL
    P = int(planner.num_envs)
    if P != int(root.num_envs):
        raise ValueError(f"the planner needs {int(root.num_envs)} environments, it has {P}")
    if planner.auto_reset:
        raise ValueError("the planner must be created with auto_reset=False (a row's episode ends at its first done)")
    if planner.run_seed != root.run_seed or planner.first_env_index != 0:
        raise ValueError("the planner must have the root's run_seed and first_env_index 0 (the keys of the draws)")

    def backend(paths, path_len, step_index0):
        dev, T = planner.device, int(paths.shape[0])
        planner.gather_(torch.arange(P, dtype=torch.int32, device=dev), source=root, paths=paths, path_len=path_len)
        plen = path_len.to(device=dev, dtype=torch.int64)
        pins = getattr(getattr(planner, "cfg", None), "kind", None) in (KIND_PIN, KIND_SPATIAL)  # the kinds with an info row
        length = planner.gather_length.to(torch.int64)
        finished = (length > 0) & planner.done.bool()  # the episode ended on the path
        reward, done = planner.reward.clone(), finished.clone()
        info = planner.info_raw.clone() if pins else None
        actions = paths.to(device=dev, dtype=torch.int32).clone()
        no_action = torch.full((P, 3), -1, dtype=torch.int32, device=dev)
        for t in range(T):
            drawn, _, _ = planner.sample_logits(logits_fn(planner.obs), step_index=int(step_index0) + t, greedy=greedy)
            held = plen > t
            _, r, d, _ = planner.step(torch.where(held[:, None], no_action, drawn))
            live = ~held & ~finished
            actions[t] = torch.where(held[:, None], actions[t], torch.where(live[:, None], drawn, torch.zeros_like(drawn)))
            reward = torch.where(live, r, reward)
            if pins:
                info = torch.where(live[:, None], planner.info_raw, info)
            length = torch.where(live, torch.full_like(length, t + 1), length)
            first = live & d.bool()
            done |= first
            finished |= first
        return Playout(reward, done.to(torch.uint8), length.to(torch.int32), info, actions)
    return backend


@dataclass
class DeviceTreeSearch(TreeSearch):
    """What `tree_search_device` returns: `TreeSearch`, and the error word of the launches."""
    errors: torch.Tensor         # 0-dim int32: bit 0 = the tree was full when a node was due (capacity < iterations + 1)


def ln_table(N: int) -> torch.Tensor:
    """ln n for n = 0 .. N as `tree_search` computes it (torch's float64 log on the CPU), entry 0 set to 0: float64 [N + 1]."""
    ln = torch.log(torch.arange(N + 1, dtype=torch.float64))
    ln[0] = 0.0
    return ln


_LN_ON_DEVICE = {}


def ln_table_on(N: int, device) -> torch.Tensor:
    """`ln_table(N)` on `device`, uploaded once per (N, device) and kept: a search enqueues no host copy of its own."""
    key = (int(N), str(device))
    if key not in _LN_ON_DEVICE:
        _LN_ON_DEVICE[key] = ln_table(N).to(device)
    return _LN_ON_DEVICE[key]


def new_tree(P: int, N: int, C: int, T: int, device) -> dict:
    """The tensors of P trees of N node slots, C children per node and T steps, as `BatchedPlacementEnv.tree_request`
    takes them.  Uninitialised but for `paths`, `best_actions` and `errors_dev`: PCBENV_TREE_INIT fills the rest."""
    i32, f64 = dict(dtype=torch.int32, device=device), dict(dtype=torch.float64, device=device)
    tree = {n: torch.empty((P, N), **i32) for n in ("parent", "depth", "visits", "num_children")}
    tree.update({n: torch.empty((P, N), **f64) for n in ("value_sum", "value_max")})
    tree.update({n: torch.empty(P, **f64) for n in ("reward_lo", "reward_hi", "best_reward")})
    tree.update({n: torch.empty(P, **i32) for n in ("num_nodes", "best_length", "selected", "path_len")})
    tree.update(node_action=torch.empty((P, N, 3), **i32), children=torch.empty((P, N, C), **i32),
                terminal=torch.empty((P, N), dtype=torch.uint8, device=device), best_actions=torch.zeros((T, P, 3), **i32),
                paths=torch.zeros((T, P, 3), **i32), errors_dev=torch.zeros(1, **i32), ln_dev=ln_table_on(N, device))
    return tree


def tree_result(tree: dict) -> DeviceTreeSearch:
    """The tensors of a device tree in the form `tree_search` reports (int32 widened to int64, the root's children summed up)."""
    w = lambda n: tree[n].to(torch.int64)
    children, visits, node_action = w("children"), w("visits"), tree["node_action"]
    P, _, C = children.shape
    rows = torch.arange(P, dtype=torch.int64, device=children.device)
    ch = children[:, 0, :]
    child_visits = torch.where(ch >= 0, visits[rows[:, None], ch.clamp(min=0)], torch.zeros_like(ch))
    child_actions = torch.where((ch >= 0)[:, :, None], node_action[rows[:, None], ch.clamp(min=0)], torch.zeros_like(node_action[:, :1]).expand(P, C, 3))
    action = child_actions[rows, child_visits.argmax(dim=1)]
    return DeviceTreeSearch(action, child_visits, child_actions, tree["best_reward"], tree["best_actions"], w("best_length"), w("num_nodes"),
                            w("parent"), w("depth"), node_action, visits, tree["value_sum"], tree["value_max"], tree["terminal"].bool(),
                            children, tree["errors_dev"][0])


def tree_search_device(root, iterations: int, step_index: int, c_uct: float = 1.0, max_children: int = 4, max_steps=None,
                       capacity=None, backend=None) -> DeviceTreeSearch:
    """`tree_search` with the tree kept by the device: an iteration is two kernel launches, `root.tree_advance`
    (pcbenv_tree_advance: backup of the last playout, expansion, the next selection) and `root.playout(paths=...)`, with
    no tensor operation between them.  The same search as `tree_search(root, iterations, step_index, c_uct, max_children,
    max_steps=max_steps)` -- the same playouts, the same tree, field by field -- as long as no two UCT scores of one
    selection differ only by the rounding of a logarithm (the table of ln n is torch's float64 log on the CPU).
    capacity: node slots per root, default iterations + 1 (what the search can use at most).  A smaller tree stops growing
    when it is full -- later playouts are backed up into existing nodes -- and reports bit 0 in `errors`; ln n is then
    taken at n = capacity for larger n.  max_children is 64 at most.  backend: as in `tree_search` (for instance
    `policy_backend`), called in place of `root.playout`; its reward / length / actions must be on the root's device."""
    from . import _lib
    from .batched_env import default_max_steps
    P, C, M = int(root.num_envs), int(max_children), int(iterations)
    if M < 1 or C < 1:
        raise ValueError("tree_search_device needs iterations >= 1 and max_children >= 1")
    T = default_max_steps(root.cfg) if max_steps is None else int(max_steps)
    N = M + 1 if capacity is None else int(capacity)
    tree = new_tree(P, N, C, T, root.device)
    req = root.tree_request(tree, c_uct)
    root.tree_advance(req, _lib.TREE_INIT | _lib.TREE_SELECT)
    if backend is None:
        backend = lambda paths, path_len, s: root.playout(k=1, step_index=s, paths=paths, path_len=path_len, max_steps=T)
    for m in range(M):
        po = backend(tree["paths"], tree["path_len"], int(step_index) + m * T)
        root.tree_advance(req, _lib.TREE_ABSORB | (_lib.TREE_SELECT if m + 1 < M else 0), po.reward, po.length, po.actions)
    return tree_result(tree)
