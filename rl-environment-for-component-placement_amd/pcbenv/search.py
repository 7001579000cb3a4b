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

`puct_search` is the AlphaZero search -- a node is expanded with a policy's best legal actions and their priors, selected
by q + c * prior * sqrt(n) / (1 + n_c) and scored by a value -- and `puct_search_device` the same search with the tree
kept by the device (pcbenv_puct_advance, include/pcbenv_search.h): one launch per iteration next to the evaluation.
`network_evaluator` is the evaluation by a network on `gather_(paths=...)`'s observations; `top_priors` its candidates.
`puct_choose` and `puct_reroot` are what stands between two searches of an episode -- the move, greedy or drawn in
proportion to the visits, and the subtree below it as the next search's tree -- in tensor code, the specification of
pcbenv_puct_move (include/pcbenv_move.h); `puct_selfplay` plays episodes with them on the device, two launches per move
next to `step`.

Every PUCT function takes `leaves=L`: leaf-parallel selection with virtual visits -- a root descends L times before
anything is evaluated, each descent leaving a pending visit on its path, the evaluator sees P * L nodes at once and one
launch backs them up (pcbenv_puct_advance_leaves, include/pcbenv_leaves.h).  With leaves == 1 each of them does what it
did before that keyword existed.

`frontier_search` is a beam search over placements -- per root a frontier of W partial placements, each expanded by an
evaluator's K best legal actions, the W best of the W * K children kept per depth, the best finished placement the
result -- on `frontier_advance`, the specification in tensor code of pcbenv_frontier_advance
(include/pcbenv_frontier.h); `frontier_search_device` is the same search with one launch per depth.
`frontier_sample_search` is that search with the rows ordered by Gumbel-perturbed log-probabilities -- stochastic beam search,
W placements per root sampled without replacement -- on `frontier_sample_advance`, the specification of
pcbenv_frontier_sample (include/pcbenv_frontier_sample.h); `frontier_sample_search_device` has one launch per depth.

`policy_backend` replaces the uniform rollout of either search by a policy's: the node a path names is materialised
in a planner batch by `gather_(paths=...)` (pcbenv_gather_paths, one launch), and the rollout behind it draws from the
logits a network gives for the planner's observations.
"""
from __future__ import annotations

from dataclasses import dataclass
from types import SimpleNamespace

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


# ---- PUCT: priors in selection and expansion, a value at the leaf --------------------------------------------------
@dataclass
class Evaluation:
    """What an evaluator says of the P nodes the paths name (`evaluate(paths, path_len, step_index0) -> Evaluation`)."""
    value: torch.Tensor         # [P] float64, finite: the value backed up from the node
    terminal: torch.Tensor      # [P] uint8 / bool: the episode is over at the node
    cand_count: torch.Tensor    # [P] int32: candidates given (a count outside [0, K] is clamped)
    cand_actions: torch.Tensor  # [P, K, 3] int32: candidate actions in the tuple format `step` takes
    cand_prior: torch.Tensor    # [P, K] float32: their prior probabilities, used as given


PUCT_TREE_TENSORS = ("num_nodes", "parent", "depth", "visits", "num_children", "first_child", "node_action", "prior", "value_sum", "value_max",
                     "terminal", "reward_lo", "reward_hi")


@dataclass
class PuctSearch:
    """What `puct_search` and `puct_search_device` return.  P roots, N = capacity node slots per root (slot 0 is the root; the k
    children of a node are the slots first_child .. first_child + k - 1), C = max_children."""
    action: torch.Tensor         # [P, 3] int32: the most-visited root child's action (ties: the lowest slot; zero without children)
    child_visits: torch.Tensor   # [P, C] int64: visits of the root's children, 0 where there is none
    child_actions: torch.Tensor  # [P, C, 3] int32: their actions
    child_priors: torch.Tensor   # [P, C] float64: their priors
    root_value: torch.Tensor     # [P] float64: value_sum / visits of slot 0
    num_nodes: torch.Tensor      # [P] int64: node slots in use
    parent: torch.Tensor         # [P, N] int64, -1 for the root and for unused slots
    depth: torch.Tensor          # [P, N] int64
    visits: torch.Tensor         # [P, N] int64
    num_children: torch.Tensor   # [P, N] int64
    first_child: torch.Tensor    # [P, N] int64, -1 for a node not expanded
    node_action: torch.Tensor    # [P, N, 3] int32: the action that leads from the parent to the node
    prior: torch.Tensor          # [P, N] float64: the prior the node was given when its parent was expanded
    value_sum: torch.Tensor      # [P, N] float64: sum of the values backed up through the node
    value_max: torch.Tensor      # [P, N] float64: the largest of them, -inf for unused slots
    terminal: torch.Tensor       # [P, N] bool: the episode is over at the node
    reward_lo: torch.Tensor      # [P] float64: the smallest value seen (+inf before the first)
    reward_hi: torch.Tensor      # [P] float64: the largest
    errors: torch.Tensor         # 0-dim int32: bit 0 = the children of a node did not fit into the free slots


def new_puct_tree(P: int, N: int, T: int, device, leaves: int = 1) -> dict:
    """The tensors of P PUCT trees of N node slots and T steps, as `BatchedPlacementEnv.puct_request` takes them -- and,
    with `pending` [P, N] and the exchange tensors `selected`, `path_len` and `paths` of P * leaves rows, as
    `puct_leaves_request` does; `noised` [P] is `puct_noise_request`'s.  Uninitialised but for `paths`, `pending`, `noised` and
    `errors_dev`: PCBENV_TREE_INIT fills the rest."""
    i32, f64 = dict(dtype=torch.int32, device=device), dict(dtype=torch.float64, device=device)
    R = P * int(leaves)
    tree = {n: torch.empty((P, N), **i32) for n in ("parent", "depth", "visits", "num_children", "first_child")}
    tree.update({n: torch.empty((P, N), **f64) for n in ("prior", "value_sum", "value_max")})
    tree.update({n: torch.empty(P, **f64) for n in ("reward_lo", "reward_hi")})
    tree.update(num_nodes=torch.empty(P, **i32), selected=torch.empty(R, **i32), path_len=torch.empty(R, **i32))
    tree.update(node_action=torch.empty((P, N, 3), **i32), terminal=torch.empty((P, N), dtype=torch.uint8, device=device),
                paths=torch.zeros((T, R, 3), **i32), errors_dev=torch.zeros(1, **i32), pending=torch.zeros((P, N), **i32),
                noised=torch.zeros(P, **i32))
    return tree


def puct_result(tree: dict, max_children: int) -> PuctSearch:
    """The tensors of a PUCT tree in the form the searches report (int32 widened to int64, the root's children summed up)."""
    w = lambda n: tree[n].to(torch.int64)
    visits, node_action, prior = w("visits"), tree["node_action"], tree["prior"]
    P, N = visits.shape
    C = int(max_children)
    dev = visits.device
    rows = torch.arange(P, dtype=torch.int64, device=dev)
    lane = torch.arange(C, dtype=torch.int64, device=dev)
    have = lane[None, :] < w("num_children")[:, :1]
    ch = torch.where(have, w("first_child")[:, :1] + lane[None, :], torch.zeros((), dtype=torch.int64, device=dev)).clamp(0, N - 1)
    child_visits = torch.where(have, visits[rows[:, None], ch], torch.zeros_like(ch))
    child_actions = torch.where(have[:, :, None], node_action[rows[:, None], ch], torch.zeros_like(node_action[:, :1]).expand(P, C, 3))
    child_priors = torch.where(have, prior[rows[:, None], ch], torch.zeros_like(prior[:, :1]).expand(P, C))
    action = child_actions[rows, child_visits.argmax(dim=1)]
    return PuctSearch(action, child_visits, child_actions, child_priors, tree["value_sum"][:, 0] / visits[:, 0].to(torch.float64),
                      w("num_nodes"), w("parent"), w("depth"), visits, w("num_children"), w("first_child"), node_action, prior,
                      tree["value_sum"], tree["value_max"], tree["terminal"].bool(), tree["reward_lo"], tree["reward_hi"],
                      tree["errors_dev"][0])


def sqrt_rn(x: torch.Tensor) -> torch.Tensor:
    """The correctly rounded float64 square root of a count (x >= 1, integer-valued): what sqrt() of csrc/pcb_tree.h:root_of
    gives on the host and __dsqrt_rn on the device.  On a device this is torch.sqrt.  torch's CPU kernel is off by one unit
    in the last place for some arguments (2, 8, 19, 32, ...), which decides a PUCT selection whose two best scores tie, so
    on the CPU the result is corrected once: s * s as an exact sum p + e of two doubles (Dekker's product over Veltkamp's
    split), the residual x - p - e, and s + residual / (2 s)."""
    s = torch.sqrt(x)
    if x.device.type != "cpu":
        return s
    t = 134217729.0 * s
    hi = t - (t - s)
    lo = s - hi
    p = s * s
    e = ((hi * hi - p) + 2.0 * hi * lo) + lo * lo
    return s + ((x - p) - e) / (2.0 * s)


def _puct_arguments(root, iterations, max_children, max_steps, capacity, tree=None, leaves=1):
    from .batched_env import default_max_steps
    P, C, M = int(root.num_envs), int(max_children), int(iterations)
    if M < 1 or C < 1 or C > 64:
        raise ValueError("a PUCT search needs iterations >= 1 and max_children in [1, 64]")
    if int(leaves) < 1 or int(leaves) > 64:
        raise ValueError("a PUCT search needs leaves in [1, 64]")
    T = default_max_steps(root.cfg) if max_steps is None else int(max_steps)
    N = 1 + M * int(leaves) * C if capacity is None else int(capacity)
    if tree is not None:  # the search goes on in the tree it is given: the capacity is that tree's
        if tuple(tree["parent"].shape[:1]) != (P,) or tree["parent"].dim() != 2:
            raise ValueError(f"tree: parent must be [{P}, N], got {list(tree['parent'].shape)}")
        N = int(tree["parent"].shape[1])
    if T < 1 or N < 1:
        raise ValueError("a PUCT search needs max_steps >= 1 and capacity >= 1")
    return P, C, M, T, N


def puct_search(root, iterations: int, step_index: int, evaluate, c_puct: float = 1.0, max_children: int = 16, max_steps=None,
                capacity=None, tree=None, leaves: int = 1, root_noise=None, noise_seed=None, noise_first_root=None,
                noise_step_index=None, root_select=None, leaf_begin=None, leaf_end=None, level_select=None, pending_select=None) -> PuctSearch:
    """Batched PUCT (the AlphaZero search) over all P = root.num_envs roots in lock-step, the tree in tensors, one
    `evaluate` per iteration and no host synchronisation inside the loop: the specification of pcbenv_puct_advance
    (include/pcbenv_search.h), in tensor code for any device.  Iteration m:
      selection  from the root, descend to the child with the highest q + c_puct * prior * sqrt(max(visits of the node, 1)) /
                 (1 + visits of the child), q = the child's mean value normalised per root by the smallest and largest value
                 seen so far, 0 for a child without a visit or while the two are equal; ties to the lowest child; stop at a
                 terminal node or at one that has no children, after max_steps levels at the latest;
      evaluate   evaluate(paths, path_len, step_index + m * max_steps) -> Evaluation of the P selected nodes (paths int32
                 [max_steps, P, 3], path_len int32 [P] = the levels descended);
      expansion  a node the evaluation calls terminal is marked so, for good.  Any other node that has no children and is not
                 terminal gets k = clamp(cand_count, 0, min(K, max_children)) children at once, in consecutive slots, with the
                 candidates' actions and priors as given -- or none at all, and bit 0 of `errors`, if fewer than k slots are
                 free.  With k = 0 the node stays a leaf and is evaluated again when it is selected again;
      backup     the value is added to visits / value_sum / value_max of the node and all its ancestors.
    capacity: node slots per root, default 1 + iterations * max_children (what the search can use at most).  max_steps: the
    most transitions of an episode (default: that of root.cfg).  Needs iterations >= 1.
    tree: the search continues in this tree instead of an empty one -- a dict of PUCT_TREE_TENSORS (`search_tree` of an
    earlier result, or what `puct_reroot` returns), integer tensors of any width, which is not modified; capacity is then
    the tree's.  Such a tree may be deep from the first iteration on, so descent and backup are bounded by max_steps alone.
    leaves = L > 1: leaf-parallel selection with virtual visits, the specification of pcbenv_puct_advance_leaves
    (include/pcbenv_leaves.h).  Iteration m selects L times, leaf after leaf, before anything is evaluated.  A descent
    adds one pending visit to every node it passes, the root and the node it ends at included, and the next one scores a
    child with n_c = visits + pending, q * (visits / n_c) in the place of q -- a pending visit counts as one that returned
    the smallest value seen -- and sqrt(max(visits + pending of the node, 1)).  A descent that ends at a node that is not
    terminal, has no children and has a pending visit already is a repeat: it takes its pending visits back, and this and
    all later leaves of the root are no leaf -- path_len -1, their evaluation is not looked at.  Then ONE evaluate(paths
    [max_steps, P * L, 3], path_len [P * L], step_index + m * max_steps), row p * L + l the leaf l of root p, and the
    leaves are expanded and backed up in the same order, each backup taking the pending visit off its chain.  capacity
    defaults to 1 + iterations * L * max_children.
    root_noise = (alpha, eps): exploration noise on the root's priors, `puct_root_noise` with the key (noise_seed,
    noise_first_root + p, step_index), once per root and search: before the first selection in a tree that is kept, and
    again after the first iteration's expansion for the roots that had no children then (a fresh root, whose first
    evaluation has just expanded it).  A root that is still without children after that stays without noise for this
    search.  noise_seed defaults to root.run_seed ^ 0x6e6f6973 and noise_first_root to root.first_env_index; a root that
    is no BatchedPlacementEnv gives the seed explicitly (the first root then defaults to 0).  noise_step_index: the step
    index of the key where it is not the search's own (move j of `puct_selfplay` has step_index + j).  None: no noise.
    root_select: another rule for level 0 (`gumbel_search`'s): root_select(tree, stopped, nxt) -> the node every root goes to
    from slot 0, given the tree as it stands (a dict of views that must not be modified), the roots that stop at slot 0 and
    the node PUCT would go to; it is called once per leaf.  None: PUCT at every level.  With leaves > 1 such a rule has a
    budget to keep, so it comes with two more hooks: leaf_begin(l, tree, alive) -> alive, called before the descent of leaf l
    with the roots that have had no repeat so far, returns those that take this leaf -- the others get no leaf from here on,
    as behind a repeat, and add no pending visit -- and leaf_end(l, alive), called behind the descent with the roots whose
    leaf l is a leaf: a repeat is not among them, so what root_select proposed for it is not committed.
    level_select: another rule for every level (`gumbel_search(full=True)`'s): level_select(d, tree, node, stopped, nxt) -> the
    node every root goes to from `node` [P] at level d, given the tree as it stands (views, not to be modified), the roots
    that stop there and the node PUCT would go to; at level 0 root_select is asked after it.  None: PUCT.  Such a rule reads
    no pending visit: with leaves > 1 it raises ValueError.
    pending_select: `level_select` for a rule that counts pending visits (`gumbel_search(node_rule="gumbel", leaves=L)`'s):
    pending_select(d, tree, node, stopped, nxt), where `tree` also has `pending` [P, N] as the leaves before this one left it.
    It goes with any leaves; at level 0 root_select is asked after it.  None: PUCT."""
    P, C, M, T, N = _puct_arguments(root, iterations, max_children, max_steps, capacity, tree, leaves)
    L = int(leaves)
    if level_select is not None and L != 1:
        raise ValueError("level_select does not go with leaves > 1")
    if root_select is not None and L != 1 and (leaf_begin is None or leaf_end is None):
        raise ValueError("root_select with leaves > 1 needs leaf_begin and leaf_end")
    noise = _noise_arguments(root, root_noise, noise_seed, noise_first_root)
    dev = getattr(root, "device", "cpu")
    i64, f64 = dict(dtype=torch.int64, device=dev), dict(dtype=torch.float64, device=dev)
    # one slot and one path row more than used: where a root has nothing to write, the write goes there
    parent, first_child = torch.full((P, N + 1), -1, **i64), torch.full((P, N + 1), -1, **i64)
    depth, visits, nchild = torch.zeros((P, N + 1), **i64), torch.zeros((P, N + 1), **i64), torch.zeros((P, N + 1), **i64)
    node_action = torch.zeros((P, N + 1, 3), dtype=torch.int32, device=dev)
    prior, vsum = torch.zeros((P, N + 1), **f64), torch.zeros((P, N + 1), **f64)
    vmax = torch.full((P, N + 1), float("-inf"), **f64)
    terminal = torch.zeros((P, N + 1), dtype=torch.bool, device=dev)
    count = torch.ones(P, **i64)
    pending = torch.zeros((P, N + 1), **i64)  # zero between iterations: every selection is absorbed
    lo, hi = torch.full((P,), float("inf"), **f64), torch.full((P,), float("-inf"), **f64)
    errors = torch.zeros(1, dtype=torch.int32, device=dev)
    if tree is not None:
        given = lambda n, like: tree[n].to(device=dev, dtype=like.dtype)
        for n, t in (("parent", parent), ("first_child", first_child), ("depth", depth), ("visits", visits), ("num_children", nchild),
                     ("node_action", node_action), ("prior", prior), ("value_sum", vsum), ("value_max", vmax), ("terminal", terminal)):
            t[:, :N] = given(n, t)
        count, lo, hi = given("num_nodes", count).clone(), given("reward_lo", lo).clone(), given("reward_hi", hi).clone()
        if tree.get("errors_dev") is not None:
            errors = tree["errors_dev"].to(device=dev, dtype=torch.int32).reshape(1).clone()
    deepest = (lambda m: min(T, m)) if tree is None else (lambda m: T)  # an empty tree has no node deeper than m in iteration m
    rows, lane = torch.arange(P, **i64), torch.arange(C, **i64)
    trash = torch.full((P,), N, **i64)
    zero_r, ninf_r = torch.zeros(P, **f64), torch.full((P,), float("-inf"), **f64)
    none = torch.full((P,), -1, **i64)
    noised = torch.zeros(P, dtype=torch.int32, device=dev)

    def view():  # the tree as it stands, for a hook
        return dict(num_nodes=count, parent=parent[:, :N], depth=depth[:, :N], visits=visits[:, :N], num_children=nchild[:, :N],
                    first_child=first_child[:, :N], node_action=node_action[:, :N], prior=prior[:, :N], value_sum=vsum[:, :N],
                    value_max=vmax[:, :N], terminal=terminal[:, :N], reward_lo=lo, reward_hi=hi)

    def add_noise(noised, errors):
        now = dict(num_children=nchild[:, :N], first_child=first_child[:, :N], prior=prior[:, :N])
        prior[:, :N], done = puct_root_noise(now, noised, C, noise[0], noise[1], noise[2], step_index if noise_step_index is None else noise_step_index,
                                             noise[3])
        return done, errors | puct_noise_errors(now, noised, C)
    if noise is not None and tree is not None:
        noised, errors = add_noise(noised, errors)
    for m in range(M):
        # selection (iteration m finds no node deeper than m: a bound the host knows without asking the device)
        paths = torch.zeros((T + 1, P, L, 3), dtype=torch.int32, device=dev)
        wide = hi > lo
        span = torch.where(wide, hi - lo, torch.ones_like(hi))
        alive = torch.ones(P, dtype=torch.bool, device=dev)  # no repeat so far
        chosen, levels = [], []
        for l in range(L):
            if leaf_begin is not None:
                alive = leaf_begin(l, view(), alive)
            node = torch.zeros(P, **i64)
            plen = torch.zeros(P, **i64)
            stopped = ~alive
            for d in range(deepest(m)):
                k = nchild[rows, node]
                stopped = stopped | terminal[rows, node] | (k == 0)
                fc = first_child[rows, node]
                mine = (lane[None, :] < k[:, None]) & ~stopped[:, None]
                ch = torch.where(mine, fc[:, None] + lane[None, :], trash[:, None])
                n_c = visits[rows[:, None], ch]
                n_vf = n_c.to(torch.float64)
                n_cf = (n_c + pending[rows[:, None], ch]).to(torch.float64)
                q = ((vsum[rows[:, None], ch] / n_vf.clamp(min=1.0) - lo[:, None]) / span[:, None]) * (n_vf / n_cf)
                q = torch.where((n_c > 0) & wide[:, None], q, torch.zeros_like(q))
                n_p = (visits[rows, node] + pending[rows, node]).clamp(min=1).to(torch.float64)
                u = c_puct * prior[rows[:, None], ch] * sqrt_rn(n_p)[:, None] / (1.0 + n_cf)
                score = torch.where(mine, q + u, torch.full_like(q, float("-inf")))
                nxt = fc + score.argmax(dim=1)                         # the first maximum: the lowest child
                if level_select is not None:
                    nxt = level_select(d, view(), node, stopped, nxt)
                if pending_select is not None:
                    nxt = pending_select(d, dict(view(), pending=pending[:, :N]), node, stopped, nxt)
                if root_select is not None and d == 0:
                    nxt = root_select(view(), stopped, nxt)
                pending[rows, torch.where(stopped, trash, node)] += 1  # the node the descent leaves
                node = torch.where(stopped, node, nxt)
                paths[torch.where(stopped, torch.full_like(node, T), torch.full_like(node, d)), rows, l] = node_action[rows, node]
                plen = plen + (~stopped).to(torch.int64)
            # a repeat takes back what it added above the node it ended at, and ends the selection of its root
            repeat = alive & ~terminal[rows, node] & (nchild[rows, node] == 0) & (pending[rows, node] > 0)
            cur = torch.where(repeat, parent[rows, node], none)
            for _ in range(deepest(m)):
                on = cur >= 0
                idx = torch.where(on, cur, trash)
                pending[rows, idx] -= on.to(torch.int64)
                cur = torch.where(on, parent[rows, idx], none)
            alive = alive & ~repeat
            if leaf_end is not None:
                leaf_end(l, alive)
            pending[rows, torch.where(alive, node, trash)] += 1
            chosen.append(torch.where(alive, node, none))
            levels.append(torch.where(alive, plen, none))
        # evaluation
        ev = evaluate(paths[:T].reshape(T, P * L, 3), torch.stack(levels, dim=1).reshape(P * L).to(torch.int32), int(step_index) + m * T)
        K = int(ev.cand_prior.shape[1])
        Kc = min(K, C)
        ev_value = ev.value.to(device=dev, dtype=torch.float64).reshape(P, L)
        ev_over = ev.terminal.to(device=dev).bool().reshape(P, L)
        ev_count = ev.cand_count.to(device=dev, dtype=torch.int64).reshape(P, L)
        ev_actions = ev.cand_actions.to(device=dev, dtype=torch.int32).reshape(P, L, K, 3)
        ev_prior = ev.cand_prior.to(device=dev, dtype=torch.float32).reshape(P, L, K)
        for l in range(L):
            live = chosen[l] >= 0
            node = chosen[l].clamp(min=0)
            value = torch.where(live, ev_value[:, l], zero_r)
            over = ev_over[:, l] & live
            # expansion: all the children at once, or none
            terminal[rows, node] = terminal[rows, node] | over
            k = ev_count[:, l].clamp(0, Kc)
            due = live & ~over & (nchild[rows, node] == 0) & ~terminal[rows, node] & (k > 0)
            fits = count + k <= N
            make = due & fits
            errors = errors | ((due & ~fits).any().to(torch.int32) * 1)
            on = make[:, None] & (lane[None, :Kc] < k[:, None])
            slot = torch.where(on, count[:, None] + lane[None, :Kc], trash[:, None])
            parent[rows[:, None], slot] = torch.where(on, node[:, None], torch.full_like(slot, -1))
            depth[rows[:, None], slot] = torch.where(on, depth[rows, node][:, None] + 1, torch.zeros_like(slot))
            acts = ev_actions[:, l, :Kc]
            node_action[rows[:, None], slot] = torch.where(on[:, :, None], acts, torch.zeros_like(acts))
            pri = ev_prior[:, l, :Kc].to(torch.float64)
            prior[rows[:, None], slot] = torch.where(on, pri, torch.zeros_like(pri))
            at = torch.where(make, node, trash)
            first_child[rows, at] = torch.where(make, count, torch.full_like(count, -1))
            nchild[rows, at] = torch.where(make, k, torch.zeros_like(k))
            count = count + torch.where(make, k, torch.zeros_like(k))
            # backup
            lo, hi = torch.where(live, torch.minimum(lo, value), lo), torch.where(live, torch.maximum(hi, value), hi)
            cur = torch.where(live, node, none)
            for _ in range(deepest(m) + 1):  # the node is at depth m at most
                on = cur >= 0
                idx = torch.where(on, cur, trash)[:, None]
                visits.scatter_add_(1, idx, on.to(torch.int64)[:, None])
                vsum.scatter_add_(1, idx, torch.where(on, value, zero_r)[:, None])
                vmax.scatter_reduce_(1, idx, torch.where(on, value, ninf_r)[:, None], reduce="amax")
                pending.scatter_add_(1, idx, -on.to(torch.int64)[:, None])
                cur = torch.where(on, parent[rows, idx[:, 0]], torch.full_like(cur, -1))
        if noise is not None and m == 0:  # the first expansion has given a fresh root its children
            noised, errors = add_noise(noised, errors)
    tree = dict(num_nodes=count, parent=parent[:, :N], depth=depth[:, :N], visits=visits[:, :N], num_children=nchild[:, :N],
                first_child=first_child[:, :N], node_action=node_action[:, :N], prior=prior[:, :N], value_sum=vsum[:, :N],
                value_max=vmax[:, :N], terminal=terminal[:, :N], reward_lo=lo, reward_hi=hi, errors_dev=errors)
    return puct_result(tree, C)


def _puct_iterations(root, req, tree, M, T, evaluate, step_index, first_phases, leaves=1, noise=None):
    """The launches of one device search of M iterations on `tree`: `first_phases` (INIT | SELECT, or SELECT alone in a tree
    that is kept), then per iteration `evaluate` followed by ABSORB | SELECT, the last iteration by ABSORB alone.  With
    leaves > 1 the launches are pcbenv_puct_advance_leaves' and `req` is a `puct_leaves_request`.
    noise = (noise request, alpha, eps, seed, step index of the key): `noised` is zeroed, NOISE (pcbenv_puct_root_noise)
    goes before the first SELECT of a tree that is kept, and the first iteration is ABSORB alone, NOISE, SELECT."""
    from . import _lib
    advance = root.puct_advance if int(leaves) == 1 else root.puct_advance_leaves
    if noise is not None:
        tree["noised"].zero_()
        if not first_phases & _lib.TREE_INIT:
            root.puct_root_noise(*noise)
    advance(req, first_phases)
    for m in range(M):
        ev = evaluate(tree["paths"], tree["path_len"], int(step_index) + m * T)
        over = ev.terminal.view(torch.uint8) if ev.terminal.dtype == torch.bool else ev.terminal
        fused = noise is None or m > 0
        advance(req, _lib.TREE_ABSORB | (_lib.TREE_SELECT if m + 1 < M and fused else 0), ev.value, over, ev.cand_count, ev.cand_actions, ev.cand_prior)
        if not fused:
            root.puct_root_noise(*noise)
            if m + 1 < M:
                advance(req, _lib.TREE_SELECT)


def puct_search_device(root, iterations: int, step_index: int, evaluate, c_puct: float = 1.0, max_children: int = 16, max_steps=None,
                       capacity=None, tree=None, leaves: int = 1, root_noise=None, noise_seed=None, noise_step_index=None) -> PuctSearch:
    """`puct_search` with the tree kept by the device: an iteration is `evaluate` and one kernel launch,
    `root.puct_advance` (pcbenv_puct_advance: expansion, backup, the next selection), with no tensor operation between
    them: INIT | SELECT first, then per iteration `evaluate(tree paths, path_len, step_index + m * max_steps)` followed by
    ABSORB | SELECT, the last iteration by ABSORB alone.  The same search as `puct_search` with the same arguments -- the
    same evaluations, the same tree, field by field, floats by their bits: the score has no logarithm, every operation of
    it is a single IEEE one on either side.  The evaluation's tensors must be on the root's device, contiguous, of the
    dtypes `Evaluation` names (`terminal` may be bool).
    tree: the search continues in this tree, in place -- the tensors of `new_puct_tree` as an earlier search or
    `puct_move(MOVE_REROOT)` left them; capacity is then the tree's, INIT is skipped and the first launch is SELECT alone.
    leaves = L > 1: `puct_search(leaves=L)` with `root.puct_advance_leaves` (pcbenv_puct_advance_leaves,
    include/pcbenv_leaves.h) as the one launch per iteration; `evaluate` sees P * L rows, row p * L + l the leaf l of root
    p, path_len -1 where there is no leaf.  A tree that is kept is one of `new_puct_tree(leaves=L)`.
    root_noise = (alpha, eps), noise_seed, noise_step_index: `puct_search`'s, as launches of `root.puct_root_noise` (pcbenv_puct_root_noise,
    include/pcbenv_noise.h) on the tree's `noised`: one before the first SELECT of a tree that is kept; the first iteration
    is ABSORB alone, NOISE, SELECT.  None: no noise, and the launches are what they are without this argument."""
    from . import _lib
    P, C, M, T, N = _puct_arguments(root, iterations, max_children, max_steps, capacity, tree, leaves)
    L = int(leaves)
    kept = tree is not None
    if not kept:
        tree = new_puct_tree(P, N, T, root.device, L)
    req = root.puct_request(tree, c_puct, C) if L == 1 else root.puct_leaves_request(tree, c_puct, C, L)
    noise = _noise_arguments(root, root_noise, noise_seed, None)
    if noise is not None:
        noise = (root.puct_noise_request(tree, C), noise[0], noise[1], noise[2], int(step_index if noise_step_index is None else noise_step_index))
    _puct_iterations(root, req, tree, M, T, evaluate, step_index, _lib.TREE_SELECT if kept else _lib.TREE_INIT | _lib.TREE_SELECT, L, noise)
    return puct_result(tree, C)


# ---- the move of a searched game: the choice, and the subtree that stays ---------------------------------------------
MOVE_GREEDY, MOVE_PROPORTIONAL = 0, 1  # include/pcbenv_move.h
_M64, _GOLDEN = (1 << 64) - 1, 0x9E3779B97F4A7C15


def _i64(x: int) -> int:
    """The int64 with the bits of x mod 2^64."""
    x &= _M64
    return x - (1 << 64) if x >> 63 else x


def _shr(z: torch.Tensor, k: int) -> torch.Tensor:
    """Logical shift right of int64 bits."""
    return (z >> k) & ((1 << (64 - k)) - 1)


def _mix64(z: torch.Tensor) -> torch.Tensor:
    """The splitmix64 finaliser on the bits of an int64 tensor (products wrap)."""
    z = (z ^ _shr(z, 30)) * _i64(0xBF58476D1CE4E5B9)
    z = (z ^ _shr(z, 27)) * _i64(0x94D049BB133111EB)
    return z ^ _shr(z, 31)


def draw_hi32(seed: int, genv: torch.Tensor, step_index: int) -> torch.Tensor:
    """hi32(mix64(mix64(seed ^ GOLDEN * (genv + 1)) + step_index)) per entry of genv (int64): the library's draw hash, int64 in [0, 2^32)."""
    inner = _mix64((genv.to(torch.int64) + 1) * _i64(_GOLDEN) ^ _i64(int(seed)))
    return _shr(_mix64(inner + _i64(int(step_index))), 32)


def search_tree(ps: PuctSearch) -> dict:
    """The tree of a search result as the dict `puct_search(tree=)`, `puct_choose` and `puct_reroot` take."""
    tree = {n: getattr(ps, n) for n in PUCT_TREE_TENSORS}
    tree["errors_dev"] = ps.errors.reshape(1)
    return tree


def new_move_tensors(P: int, N: int, C: int, device) -> dict:
    """The tensors pcbenv_puct_move writes, as `BatchedPlacementEnv.puct_move_request` takes them next to a tree's."""
    i32 = dict(dtype=torch.int32, device=device)
    return dict(move_slot=torch.empty(P, **i32), move_action=torch.empty((P, 3), **i32), child_visits=torch.empty((P, C), **i32),
                child_actions=torch.empty((P, C, 3), **i32), root_value=torch.empty(P, dtype=torch.float64, device=device),
                remap=torch.empty((P, N), **i32))


def puct_choose(tree: dict, max_children: int, mode: int = MOVE_GREEDY, seed: int = 0, step_index: int = 0, first_root: int = 0) -> dict:
    """The move of every root of a PUCT tree: the specification of pcbenv_puct_move's CHOOSE (include/pcbenv_move.h) in
    tensor code for any device, no host synchronisation.  -> dict(move_slot int32 [P], move_action int32 [P, 3],
    child_visits int32 [P, C], child_actions int32 [P, C, 3], root_value float64 [P]).  The children of the root, their
    visits and root_value are `puct_result`'s.  MOVE_GREEDY: the most-visited child, ties to the lowest -- `puct_result`'s
    `action`.  MOVE_PROPORTIONAL: with total = the sum of the children's visits and h = draw_hi32(seed, first_root + p,
    step_index), the least child whose inclusive prefix sum of visits exceeds (h * total) >> 32 -- integers only; greedy
    where total is 0.  A root without children: move_slot -1, action (0, 0, 0).  The tree is healthy (this is not where
    damage is checked)."""
    ps = puct_result(dict(tree, errors_dev=torch.zeros(1, dtype=torch.int32, device=tree["visits"].device)), max_children)
    cv, ca = ps.child_visits, ps.child_actions
    P = cv.shape[0]
    rows = torch.arange(P, dtype=torch.int64, device=cv.device)
    c = cv.argmax(dim=1)
    if int(mode) == MOVE_PROPORTIONAL:
        total = cv.sum(dim=1)
        at = (draw_hi32(seed, rows + int(first_root), step_index) * total) >> 32
        drawn = (cv.cumsum(dim=1) > at[:, None]).to(torch.int64).argmax(dim=1)
        c = torch.where(total > 0, drawn, c)
    has = ps.num_children[:, 0] > 0
    slot = torch.where(has, ps.first_child[:, 0] + c, torch.full_like(c, -1))
    action = torch.where(has[:, None], ca[rows, c], torch.zeros_like(ca[:, 0]))
    return dict(move_slot=slot.to(torch.int32), move_action=action, child_visits=cv.to(torch.int32), child_actions=ca, root_value=ps.root_value)


def puct_reroot(tree: dict, move_slot: torch.Tensor, reset=None):
    """The subtree of node move_slot[p] as the tree of root p: the specification of pcbenv_puct_move's REROOT
    (include/pcbenv_move.h) in tensor code for any device, no host synchronisation.  tree: a dict of PUCT_TREE_TENSORS
    (healthy trees whose unused slots hold the INIT values), not modified.  -> (the new tree, tensors of the dtypes given,
    and remap int32 [P, N]).  A slot is kept if it is move_slot or a descendant of it (pointer doubling over `parent`,
    ceil(log2 N) rounds); remap is its rank among the kept slots and -1 elsewhere; a kept node moves to that slot with
    parent and first_child renamed through remap and its depth taken from the new root, which gets parent -1, action 0
    and prior 0; every other slot holds the INIT values.  reward_lo / reward_hi stay.  move_slot == 0 is the identity.
    move_slot == -1, or reset[p] != 0: an empty tree (what PCBENV_TREE_INIT leaves) and remap -1."""
    dev = tree["parent"].device
    w = lambda n: tree[n].to(torch.int64)
    parent, depth, visits, nchild, fchild, count = w("parent"), w("depth"), w("visits"), w("num_children"), w("first_child"), w("num_nodes")
    P, N = parent.shape
    i64 = dict(dtype=torch.int64, device=dev)
    rows, slots = torch.arange(P, **i64), torch.arange(N, **i64)
    m = move_slot.to(device=dev, dtype=torch.int64)
    empty = m < 0
    if reset is not None:
        empty = empty | (reset.to(dev) != 0)
    mc = m.clamp(0, N - 1)
    below = slots[None, :] == mc[:, None]          # s is m or has m among its ancestors, so far
    up = parent.clamp(min=0)                       # the root points at itself
    for _ in range(max(1, (N - 1).bit_length())):
        below = below | below.gather(1, up)
        up = up.gather(1, up)
    kept = below & (slots[None, :] < count[:, None]) & ~empty[:, None]
    rank = kept.to(torch.int64).cumsum(dim=1) - 1
    remap = torch.where(kept, rank, torch.full_like(rank, -1))
    to = torch.where(kept, rank, torch.full_like(rank, N))    # a slot that is not kept writes into the spare column
    is_root = kept & (slots[None, :] == mc[:, None])

    def moved(values, init, dtype):
        out = torch.full((P, N + 1) + tuple(values.shape[2:]), init, dtype=dtype, device=dev)
        out[rows[:, None], to] = values.to(dtype)
        return out[:, :N].contiguous()
    new_parent = torch.where(is_root, torch.full_like(parent, -1), remap.gather(1, parent.clamp(min=0)))
    new_first = torch.where(nchild > 0, remap.gather(1, fchild.clamp(0, N - 1)), torch.full_like(fchild, -1))
    new_depth = depth - depth[rows, mc][:, None]
    action = torch.where(is_root[:, :, None], torch.zeros_like(tree["node_action"]), tree["node_action"])
    prior = torch.where(is_root, torch.zeros_like(tree["prior"]), tree["prior"])
    like = lambda n: tree[n].dtype
    inf = float("inf")
    new = dict(num_nodes=torch.where(empty, torch.ones_like(count), kept.sum(dim=1)).to(like("num_nodes")),
               parent=moved(new_parent, -1, like("parent")), depth=moved(new_depth, 0, like("depth")), visits=moved(visits, 0, like("visits")),
               num_children=moved(nchild, 0, like("num_children")), first_child=moved(new_first, -1, like("first_child")),
               node_action=moved(action, 0, like("node_action")), prior=moved(prior, 0.0, like("prior")),
               value_sum=moved(tree["value_sum"], 0.0, like("value_sum")), value_max=moved(tree["value_max"], -inf, like("value_max")),
               terminal=moved(tree["terminal"], 0, like("terminal")),
               reward_lo=torch.where(empty, torch.full_like(tree["reward_lo"], inf), tree["reward_lo"]),
               reward_hi=torch.where(empty, torch.full_like(tree["reward_hi"], -inf), tree["reward_hi"]))
    for n in tree:
        if n not in new:
            new[n] = tree[n]
    return new, remap.to(torch.int32)


# ---- exploration noise on the root's priors ---------------------------------------------------------------------------
# ln, exp and the square root in IEEE + - * / alone: csrc/pcb_ieee_math.h, line by line.  torch's own differ from libm's and
# ocml's in the last place; these are the same bits on every device.
_LN2_HI, _LN2_LO = 6.93147180369123816490e-01, 1.90821492927058770002e-10
_LOG2_E, _SQRT_HALF = 1.44269504088896338700e+00, 7.07106781186547524401e-01
NOISE_ATTEMPTS, NOISE_BOOST_DRAW = 32, 96
NOISE_ALPHA_MIN, NOISE_ALPHA_MAX = 0.01, 100.0


def _pow2(k: torch.Tensor) -> torch.Tensor:
    """2^k for an integer tensor, -1022 <= k <= 1023, through the bits."""
    return ((k.to(torch.int64) + 1023) << 52).view(torch.float64)


def ieee_ln(x: torch.Tensor) -> torch.Tensor:
    """ln of positive normal float64 numbers: csrc/pcb_ieee_math.h:ieee_ln, the same operations."""
    m, e = torch.frexp(x)
    low = m < _SQRT_HALF
    m = torch.where(low, 2.0 * m, m)
    e = e - low.to(e.dtype)
    t = (m - 1.0) / (m + 1.0)
    t2 = t * t
    p = (1.0 / 27.0) * t2 + 1.0 / 25.0
    for n in (23.0, 21.0, 19.0, 17.0, 15.0, 13.0, 11.0, 9.0, 7.0, 5.0, 3.0, 1.0):
        p = p * t2 + 1.0 / n
    ef = e.to(torch.float64)
    return ef * _LN2_HI + (ef * _LN2_LO + (2.0 * t) * p)


def ieee_exp(x: torch.Tensor) -> torch.Tensor:
    """exp of float64 numbers <= 0, exactly 0 below -708: csrc/pcb_ieee_math.h:ieee_exp, the same operations."""
    under = x < -708.0
    x = torch.where(under, torch.zeros_like(x), x)
    kf = (x * _LOG2_E - 0.5).to(torch.int64).to(torch.float64)  # the conversion cuts towards 0
    r = (x - kf * _LN2_HI) - kf * _LN2_LO
    p = (1.0 / 6227020800.0) * r + 1.0 / 479001600.0
    for f in (39916800.0, 3628800.0, 362880.0, 40320.0, 5040.0, 720.0, 120.0, 24.0, 6.0, 2.0, 1.0, 1.0):
        p = p * r + 1.0 / f
    return torch.where(under, torch.zeros_like(x), p * _pow2(kf))


def ieee_sqrt(x: torch.Tensor) -> torch.Tensor:
    """The square root of positive normal float64 numbers: csrc/pcb_ieee_math.h:ieee_sqrt, the same operations."""
    m, e = torch.frexp(x)
    odd = (e & 1) != 0
    m = torch.where(odd, 2.0 * m, m)
    e = e - odd.to(e.dtype)
    y = torch.ones_like(m)
    for _ in range(6):
        y = 0.5 * (y + m / y)
    return y * _pow2(torch.div(e, 2, rounding_mode="floor"))


def noise_uniform(base: torch.Tensor, c: torch.Tensor, t: int) -> torch.Tensor:
    """Draw number t of child c under `base` (int64 bits): ((w >> 12) + 0.5) * 2^-52, w = mix64(base + GOLDEN * (64 t + c + 1))."""
    w = _mix64(base + (c + (64 * int(t) + 1)) * _i64(_GOLDEN))
    return (_shr(w, 12).to(torch.float64) + 0.5) * (1.0 / 4503599627370496.0)


def noise_base(seed: int, genv: torch.Tensor, step_index: int) -> torch.Tensor:
    """The 64 bits behind the library's draw for (seed, genv, step_index): `draw_hi32` before its shift."""
    return _mix64(_mix64((genv.to(torch.int64) + 1) * _i64(_GOLDEN) ^ _i64(int(seed))) + _i64(int(step_index)))


def noise_gammas(base: torch.Tensor, c: torch.Tensor, alpha: float):
    """Gamma(alpha) draws for the children c (int64, broadcast against base): csrc/pcb_puct_noise.h:gamma_draw as
    NOISE_ATTEMPTS masked rounds.  -> (g float64, exhausted bool: no attempt accepted and g = d)."""
    alpha = float(alpha)
    a = alpha if alpha >= 1.0 else alpha + 1.0
    d = a - 1.0 / 3.0
    cc = (1.0 / 3.0) / ieee_sqrt(torch.full((), d, dtype=torch.float64, device=base.device))
    g = torch.full(torch.broadcast_shapes(base.shape, c.shape), d, dtype=torch.float64, device=base.device)
    done = torch.zeros_like(g, dtype=torch.bool)
    for t in range(NOISE_ATTEMPTS):
        v1, v2 = 2.0 * noise_uniform(base, c, 3 * t) - 1.0, 2.0 * noise_uniform(base, c, 3 * t + 1) - 1.0
        s = v1 * v1 + v2 * v2
        inside = s < 1.0
        s = torch.where(inside, s, torch.full_like(s, 0.5))
        x = v1 * ieee_sqrt((-2.0 * ieee_ln(s)) / s)
        w = 1.0 + cc * x
        v = (w * w) * w
        positive = v > 0.0
        lnv = ieee_ln(torch.where(positive, v, torch.ones_like(v)))
        accept = ieee_ln(noise_uniform(base, c, 3 * t + 2)) < ((0.5 * (x * x) + d) - d * v) + d * lnv
        now = inside & positive & accept & ~done
        g = torch.where(now, d * v, g)
        done = done | now
    if alpha < 1.0:
        g = g * ieee_exp(ieee_ln(noise_uniform(base, c, NOISE_BOOST_DRAW)) / alpha)
    return g, ~done


def _noise_roots(tree, noised, C):
    """(k, fc, due, ok) of slot 0 of every root: the root is due (not noised yet, has children) and its child range is one."""
    k, fc = tree["num_children"][:, 0].to(torch.int64), tree["first_child"][:, 0].to(torch.int64)
    N = tree["prior"].shape[1]
    due = (noised.to(k.device) == 0) & (k >= 1)
    return k, fc, due, (k <= C) & (fc >= 1) & (fc <= N - k)


def puct_noise_errors(tree: dict, noised: torch.Tensor, max_children: int) -> torch.Tensor:
    """The error bits of `puct_root_noise` on the same arguments, int32 [1]: bit 1 (value 2) if a root that is due has a
    child range outside the tree."""
    _, _, due, ok = _noise_roots(tree, noised, int(max_children))
    return ((due & ~ok).any().to(torch.int32) * 2).reshape(1)


def puct_root_noise(tree: dict, noised: torch.Tensor, max_children: int, alpha: float, eps: float, seed: int, step_index: int,
                    first_root: int = 0):
    """Dirichlet noise on the priors of every root's children: the specification of pcbenv_puct_root_noise
    (include/pcbenv_noise.h) in tensor code for any device, no host synchronisation, which the kernel matches bit for bit.
    tree: a dict with `num_children`, `first_child` (integers of any width) and `prior` float64, [P, N]; noised: integers
    [P].  Neither is modified.  -> (prior float64 [P, N], noised int32 [P]).  A root with noised 0 and k >= 1 children in a
    healthy range gets prior(fc + c) = float32((1 - eps) * prior(fc + c) + eps * eta_c), eta = g / (g_0 + ... + g_(k-1))
    summed in that order (1 / k if the sum is not a finite number > 0), g_c a Gamma(alpha) draw by Marsaglia and Tsang's
    method with at most 32 attempts from the uniform stream of (seed, first_root + p, step_index, c) -- every elementary
    function in IEEE + - * / (`ieee_ln`, `ieee_exp`, `ieee_sqrt`) -- and noised 1.  Every other root is left as it is."""
    C, alpha, eps = int(max_children), float(alpha), float(eps)
    if not (NOISE_ALPHA_MIN <= alpha <= NOISE_ALPHA_MAX) or not (0.0 <= eps <= 1.0) or C < 1 or C > 64:
        raise ValueError("puct_root_noise needs alpha in [0.01, 100], eps in [0, 1] and max_children in [1, 64]")
    prior = tree["prior"]
    dev = prior.device
    P, N = prior.shape
    i64 = dict(dtype=torch.int64, device=dev)
    k, fc, due, ok = _noise_roots(tree, noised, C)
    handled = due & ok
    rows, lane = torch.arange(P, **i64), torch.arange(C, **i64)
    g, _ = noise_gammas(noise_base(seed, rows + int(first_root), step_index)[:, None], lane[None, :], alpha)
    S = torch.zeros(P, dtype=torch.float64, device=dev)
    for c in range(C):  # in this order: it is the contract
        S = torch.where(c < k, S + g[:, c], S)
    kf = k.clamp(min=1).to(torch.float64)
    eta = torch.where(((S > 0.0) & (S <= 1.7976931348623157e308))[:, None], g / S[:, None], (1.0 / kf)[:, None].expand(P, C))
    mine = handled[:, None] & (lane[None, :] < k[:, None])
    ch = torch.where(mine, fc[:, None] + lane[None, :], torch.full((), N, **i64))
    wide = torch.cat([prior, torch.zeros((P, 1), dtype=prior.dtype, device=dev)], dim=1)  # a spare column for what is not written
    old = wide[rows[:, None], ch]
    new = ((1.0 - eps) * old + eps * eta).to(torch.float32).to(torch.float64)
    wide[rows[:, None], ch] = torch.where(mine, new, old)
    return wide[:, :N].contiguous(), torch.where(handled, torch.ones_like(k), noised.to(dev).to(torch.int64)).to(torch.int32)


def _noise_arguments(root, root_noise, noise_seed, first_root):
    """(alpha, eps, seed, first root) of a search's `root_noise=` / `noise_seed=`, None without noise."""
    if root_noise is None:
        return None
    alpha, eps = (float(v) for v in root_noise)
    if not (NOISE_ALPHA_MIN <= alpha <= NOISE_ALPHA_MAX) or not (0.0 <= eps <= 1.0):
        raise ValueError("root_noise = (alpha, eps) needs alpha in [0.01, 100] and eps in [0, 1]")
    if noise_seed is None and not hasattr(root, "run_seed"):
        raise ValueError("root_noise: a root without run_seed needs noise_seed")
    seed = (int(root.run_seed) ^ 0x6e6f6973) if noise_seed is None else int(noise_seed)
    return alpha, eps, seed, int(getattr(root, "first_env_index", 0) if first_root is None else first_root)


# ---- Gumbel root search with sequential halving (include/pcbenv_gumbel.h) ---------------------------------------------
GUMBEL_BEGIN, GUMBEL_ABSORB, GUMBEL_SELECT, GUMBEL_CHOOSE = 1, 2, 4, 8
GUMBEL_DRAW = 128             # the number of the Gumbel draw in a child's uniform stream; the noise draws are 0 .. 96
GUMBEL_PRIOR_FLOOR = 2.0 ** -149
GUMBEL_WEIGHT_ONE = 16777216.0


def considered_visits(max_considered: int, simulations: int) -> torch.Tensor:
    """The table of Sequential Halving, int32 [Mc + 1, n] on the CPU: row m, simulation t -> the number of simulations a root
    child must have had to be considered at t, for m candidates and n simulations (csrc/pcb_gumbel.h:considered_row, the
    schedule of "Policy improvement by planning with Gumbel").  Row 0 is zeros, row 1 is 0 .. n - 1; otherwise, with e the
    least integer with 2^e >= m, visits[0 .. m) = 0 and nc = m, until n entries exist: extra = max(1, n // (e * nc)); extra
    times, append visits[0 .. nc) and add 1 to each of them; nc = max(2, nc // 2)."""
    Mc, n = int(max_considered), int(simulations)
    if Mc < 1 or Mc > 64 or n < 1:
        raise ValueError("considered_visits needs max_considered in [1, 64] and simulations >= 1")
    rows = [[0] * n, list(range(n))]
    for m in range(2, Mc + 1):
        e = (m - 1).bit_length()
        visits, nc, row = [0] * m, m, []
        while len(row) < n:
            for _ in range(max(1, n // (e * nc))):
                row += visits[:nc]
                visits[:nc] = [v + 1 for v in visits[:nc]]
            nc = max(2, nc // 2)
        rows.append(row[:n])
    return torch.tensor(rows[:Mc + 1], dtype=torch.int32)


def _gumbel_rule(max_children, c_visit, c_scale):
    C, c_visit, c_scale = int(max_children), float(c_visit), float(c_scale)
    if C < 1 or C > 64 or not (0.0 <= c_visit < float("inf")) or not (0.0 <= c_scale < float("inf")):
        raise ValueError("the Gumbel rule needs max_children in [1, 64] and finite c_visit, c_scale >= 0")
    return C, c_visit, c_scale


def gumbel_scores(tree: dict, max_children: int, c_visit: float, c_scale: float, seed: int, step_index: int, first_root: int = 0,
                  full: bool = False) -> dict:
    """The quantities of every root's children under the Gumbel rule: the specification of include/pcbenv_gumbel.h's
    "quantities of a root" in tensor code for any device, no host synchronisation, which csrc/pcb_gumbel.h and the kernel
    match bit for bit.  tree: a dict with `num_children`, `first_child`, `visits` (integers of any width), `prior`,
    `value_sum` float64 [P, N] and `reward_lo`, `reward_hi` float64 [P]; not modified.  -> dict(k, fc int64 [P]; ok bool [P]:
    the root has children in a healthy range; mine bool [P, C]: child c exists; g, logit, qhat, sigma, x = logit + sigma,
    score = (g + logit) + sigma float64 [P, C], meaningless where mine is False; actions int32 [P, C, 3], zero there).
    g_c = -ln(-ln u) with u draw number 128 of child c in the uniform stream of (seed, first_root + p, step_index) --
    `noise_uniform`'s; logit_c = ln(min(prior, 1)), a prior that is not above 2^-149 at that floor; qhat_c = the child's mean
    value -- the root's where the child has no visit, reward_lo where the root has none either -- normalised by
    [reward_lo, reward_hi], 0 while that is no range; sigma_c = ((c_visit + the most visits among the children) * c_scale)
    * qhat_c.  ln is `ieee_ln`.
    full=True: the quantities of include/pcbenv_gumbel_tree.h -- qhat, sigma, x and score are `gumbel_node_scores`' at slot 0,
    where a child without a visit is completed with v_mix in the place of the root's mean; g and logit are the same."""
    C, c_visit, c_scale = _gumbel_rule(max_children, c_visit, c_scale)
    prior, vsum = tree["prior"], tree["value_sum"]
    dev = prior.device
    P, N = prior.shape
    i64 = dict(dtype=torch.int64, device=dev)
    visits = tree["visits"].to(torch.int64)
    k, fc = tree["num_children"][:, 0].to(torch.int64), tree["first_child"][:, 0].to(torch.int64)
    ok = (k >= 1) & (k <= C) & (fc >= 1) & (fc <= N - k)
    rows, lane = torch.arange(P, **i64), torch.arange(C, **i64)
    mine = ok[:, None] & (lane[None, :] < k[:, None])
    ch = torch.where(mine, fc[:, None] + lane[None, :], torch.zeros((), **i64))
    n_c = visits[rows[:, None], ch]
    most = torch.where(mine, n_c, torch.full((), -2 ** 31, **i64)).max(dim=1).values
    lo, hi = tree["reward_lo"], tree["reward_hi"]
    n_0 = visits[:, 0]
    vbar = torch.where(n_0 > 0, vsum[:, 0] / n_0.clamp(min=1).to(torch.float64), lo)
    mean = torch.where(n_c > 0, vsum[rows[:, None], ch] / n_c.clamp(min=1).to(torch.float64), vbar[:, None])
    wide = hi > lo
    span = torch.where(wide, hi - lo, torch.ones_like(hi))
    lo_ = torch.where(wide, lo, torch.zeros_like(lo))
    qhat = torch.where(wide[:, None], (mean - lo_[:, None]) / span[:, None], torch.zeros_like(mean))
    pr = prior[rows[:, None], ch]
    floor = torch.full_like(pr, GUMBEL_PRIOR_FLOOR)
    logit = ieee_ln(torch.where(pr > floor, torch.where(pr < 1.0, pr, torch.ones_like(pr)), floor))
    sigma = ((c_visit + most.to(torch.float64)) * c_scale)[:, None] * qhat
    if full:
        at_root = gumbel_node_scores(tree, torch.zeros(P, **i64), C, c_visit, c_scale)
        qhat, sigma = at_root["qhat"], at_root["sigma"]
    u = noise_uniform(noise_base(seed, rows + int(first_root), step_index)[:, None], lane[None, :], GUMBEL_DRAW)
    g = -ieee_ln(-ieee_ln(u))
    na = tree.get("node_action")
    actions = None if na is None else torch.where(mine[:, :, None], na[rows[:, None], ch], torch.zeros_like(na[:, :1]).expand(P, C, 3))
    return dict(k=k, fc=fc, ok=ok, mine=mine, g=g, logit=logit, qhat=qhat, sigma=sigma, x=logit + sigma, score=(g + logit) + sigma, actions=actions)


def _best_of(score, within):
    """The first maximum of score over `within` [P, C] (bool), per row: the lowest child on ties."""
    return torch.where(within, score, torch.full_like(score, float("-inf"))).argmax(dim=1)


def gumbel_select_root(tree: dict, sim_index: torch.Tensor, sim_visits: torch.Tensor, considered: torch.Tensor, max_children: int,
                       c_visit: float, c_scale: float, seed: int, step_index: int, first_root: int = 0, full: bool = False) -> dict:
    """Level 0 of pcbenv_gumbel_advance's SELECT: its specification in tensor code for any device, no host synchronisation.
    tree: `gumbel_scores`' and `terminal` [P, N]; sim_index [P], sim_visits [P, C] integers; considered int32 [Mc + 1, n]
    (`considered_visits`) on the tree's device.  Nothing is modified.  -> dict(scheduled bool [P]: the root makes a scheduled
    simulation; child int64 [P]: the root child it goes to, 0 elsewhere; sim_index int32 [P], sim_visits int32 [P, C]: the
    counters afterwards; errors int32 [1]: bit 1 (value 2) if a root that does not stop at slot 0 has a child range outside
    the tree or a negative sim_index).  A root stops at slot 0 if it is terminal or has no children.  With t = sim_index,
    0 <= t < n: v = considered[min(Mc, k), t], S = the children with sim_visits == v, or all k if there is none, the child
    is the argmax of `gumbel_scores`' score over S, ties to the lowest; its counter and sim_index go up by one.  With t >= n
    the root level is PUCT's and the counters stay.
    full=True: level 0 of pcbenv_gumbel_tree_advance's SELECT -- `gumbel_scores(full=True)`; with t >= n the root level is
    `gumbel_select_node`'s."""
    sc = gumbel_scores(tree, max_children, c_visit, c_scale, seed, step_index, first_root, full)
    Mc, n = int(considered.shape[0]) - 1, int(considered.shape[1])
    k, ok, mine = sc["k"], sc["ok"], sc["mine"]
    dev = k.device
    t = sim_index.to(device=dev, dtype=torch.int64)
    sv = sim_visits.to(device=dev, dtype=torch.int64)
    goes = ~((tree["terminal"][:, 0] != 0) | (k == 0))
    scheduled = goes & ok & (t >= 0) & (t < n)
    v = considered.to(torch.int64)[k.clamp(0, Mc), t.clamp(0, n - 1)]
    at = mine & (sv == v[:, None])
    within = mine & (~at.any(dim=1, keepdim=True) | at)
    child = torch.where(scheduled, _best_of(sc["score"], within), torch.zeros_like(k))
    lane = torch.arange(sv.shape[1], dtype=torch.int64, device=dev)
    hit = scheduled[:, None] & (lane[None, :] == child[:, None])
    errors = ((goes & (~ok | (t < 0))).any().to(torch.int32) * 2).reshape(1)
    return dict(scheduled=scheduled, child=child, sim_index=(t + scheduled.to(torch.int64)).to(torch.int32),
                sim_visits=(sv + hit.to(torch.int64)).to(torch.int32), errors=errors)


def gumbel_choose(tree: dict, sim_visits: torch.Tensor, max_children: int, c_visit: float, c_scale: float, seed: int, step_index: int,
                  first_root: int = 0, full: bool = False) -> dict:
    """The move and the policy target of every root under the Gumbel rule: the specification of pcbenv_gumbel_advance's
    CHOOSE (include/pcbenv_gumbel.h) in tensor code for any device, no host synchronisation.  tree: `gumbel_scores`' and
    `node_action`; sim_visits [P, C] integers.  Nothing is modified.  -> dict(move_slot int32 [P], move_action int32 [P, 3],
    child_weights int32 [P, C], child_policy float32 [P, C], child_actions int32 [P, C, 3], root_value float64 [P], errors
    int32 [1]).  The move is the best score among the children with the most scheduled simulations, ties to the lowest.
    The target is pi = softmax(logit + sigma) over the k children: e_c = `ieee_exp`(x_c - max x), Z their sum in child
    order, pi_c = e_c / Z; child_policy = float32(pi), child_weights = int32(pi * 2^24 + 0.5), zero behind k.  A root
    without children, or with a child range outside the tree (bit 1 of errors): move_slot -1 and zeros.
    full=True: pcbenv_gumbel_tree_advance's CHOOSE -- `gumbel_scores(full=True)`."""
    sc = gumbel_scores(tree, max_children, c_visit, c_scale, seed, step_index, first_root, full)
    k, fc, ok, mine, x = sc["k"], sc["fc"], sc["ok"], sc["mine"], sc["x"]
    dev = k.device
    P, C = mine.shape
    sv = sim_visits.to(device=dev, dtype=torch.int64)
    most = torch.where(mine, sv, torch.full((), -2 ** 31, dtype=torch.int64, device=dev)).max(dim=1).values
    c = _best_of(sc["score"], mine & (sv == most[:, None]))
    mx = torch.where(mine, x, torch.full_like(x, float("-inf"))).max(dim=1).values
    e = torch.where(mine, ieee_exp(torch.where(mine, x - mx[:, None], torch.zeros_like(x))), torch.zeros_like(x))
    Z = torch.zeros(P, dtype=torch.float64, device=dev)
    for b in range(C):  # in this order: it is the contract
        Z = torch.where(mine[:, b], Z + e[:, b], Z)
    pi = torch.where(mine, e / torch.where(ok, Z, torch.ones_like(Z))[:, None], torch.zeros_like(e))
    rows = torch.arange(P, dtype=torch.int64, device=dev)
    slot = torch.where(ok, fc + c, torch.full_like(c, -1))
    action = torch.where(ok[:, None], sc["actions"][rows, c], torch.zeros_like(sc["actions"][:, 0]))
    errors = (((k != 0) & ~ok).any().to(torch.int32) * 2).reshape(1)
    return dict(move_slot=slot.to(torch.int32), move_action=action, child_weights=(pi * GUMBEL_WEIGHT_ONE + 0.5).to(torch.int32),
                child_policy=pi.to(torch.float32), child_actions=sc["actions"],
                root_value=tree["value_sum"][:, 0] / tree["visits"][:, 0].to(torch.float64), errors=errors)


def gumbel_node_scores(tree: dict, node: torch.Tensor, max_children: int, c_visit: float, c_scale: float, pending=None) -> dict:
    """The quantities of one node per root under the full Gumbel rule: the specification of include/pcbenv_gumbel_tree.h's
    "quantities of a node" in tensor code for any device, no host synchronisation, which csrc/pcb_gumbel_tree.h and the
    kernel match bit for bit.  tree: `gumbel_scores`'; node [P]: a slot of every root, integers; not modified.  -> dict(k, fc
    int64 [P]; ok bool [P]: the node has children in a healthy range; mine bool [P, C]: child c exists; n int64 [P, C]: its
    visits; Nsum int64 [P]; vhat, vmix float64 [P]; logit, qhat, sigma, x, pi, t float64 [P, C], meaningless where mine is
    False).  With ch the children of the node and n_c their visits: S = the sum of value_sum(ch), Wv and Qv the sums of pr_c
    and pr_c * q_c over the children with a visit, pr_c the prior clamped to [2^-149, 1] and q_c = value_sum(ch) / n_c; vhat =
    (value_sum(node) - S) / own with own = visits(node) - Nsum, the node's mean where own <= 0 and reward_lo where it has no
    visit either; vmix = (vhat + (Nsum / Wv) * Qv) / (1 + Nsum), vhat while no child has a visit; qhat_c = q_c, or vmix for a
    child without a visit, normalised by [reward_lo, reward_hi], 0 while that is no range; sigma_c = ((c_visit + the most
    visits among the children) * c_scale) * qhat_c; pi = softmax(logit + sigma) as `gumbel_choose` forms it; t_c = pi_c - n_c /
    (1 + Nsum).  Every sum is formed in child order from 0.0.  ln and exp are `ieee_ln` and `ieee_exp`.
    pending [P, N] integers (not modified): the rule of include/pcbenv_gumbel_tree_leaves.h -- a pending visit counts as a visit
    in t and enters nothing else: with m_c = n_c + pending(ch) and Msum their sum, t_c = pi_c - m_c / (1 + Msum), a NaN (Msum ==
    -1: damaged counts only) counting as -inf; the dict also has m int64 [P, C] and Msum int64 [P].  pi and everything before
    it read no pending visit.  None: what the function returns without the argument."""
    C, c_visit, c_scale = _gumbel_rule(max_children, c_visit, c_scale)
    prior, vsum = tree["prior"], tree["value_sum"]
    dev = prior.device
    P, N = prior.shape
    i64 = dict(dtype=torch.int64, device=dev)
    visits = tree["visits"].to(torch.int64)
    rows, lane = torch.arange(P, **i64), torch.arange(C, **i64)
    a = node.to(**i64)
    k, fc = tree["num_children"].to(torch.int64)[rows, a], tree["first_child"].to(torch.int64)[rows, a]
    ok = (k >= 1) & (k <= C) & (fc >= 1) & (fc <= N - k)
    mine = ok[:, None] & (lane[None, :] < k[:, None])
    ch = torch.where(mine, fc[:, None] + lane[None, :], torch.zeros((), **i64))
    n_c = visits[rows[:, None], ch]
    seen = mine & (n_c > 0)
    zero_i = torch.zeros((), **i64)
    Nsum = torch.where(mine, n_c, zero_i).sum(dim=1)
    most = torch.where(mine, n_c, torch.full((), -2 ** 31, **i64)).max(dim=1).values
    pr = prior[rows[:, None], ch]
    floor = torch.full_like(pr, GUMBEL_PRIOR_FLOOR)
    pr = torch.where(pr > floor, torch.where(pr < 1.0, pr, torch.ones_like(pr)), floor)
    vs = vsum[rows[:, None], ch]
    q_c = vs / torch.where(seen, n_c, torch.ones((), **i64)).to(torch.float64)
    wq = pr * q_c
    S = torch.zeros(P, dtype=torch.float64, device=dev)
    Wv, Qv = torch.zeros_like(S), torch.zeros_like(S)
    for b in range(C):  # in this order: it is the contract
        S = torch.where(mine[:, b], S + vs[:, b], S)
        Wv = torch.where(seen[:, b], Wv + pr[:, b], Wv)
        Qv = torch.where(seen[:, b], Qv + wq[:, b], Qv)
    lo, hi = tree["reward_lo"], tree["reward_hi"]
    n_a, sum_a = visits[rows, a], vsum[rows, a]
    own = n_a - Nsum
    Nf = Nsum.to(torch.float64)
    vhat = torch.where(own > 0, (sum_a - S) / own.clamp(min=1).to(torch.float64), torch.where(n_a > 0, sum_a / n_a.clamp(min=1).to(torch.float64), lo))
    mixes = (Nsum > 0) & (Wv > 0.0)
    vmix = torch.where(mixes, (vhat + (Nf / torch.where(mixes, Wv, torch.ones_like(Wv))) * Qv) / (1.0 + Nf), vhat)
    wide = hi > lo
    span = torch.where(wide, hi - lo, torch.ones_like(hi))
    lo_ = torch.where(wide, lo, torch.zeros_like(lo))
    qhat = torch.where(wide[:, None], (torch.where(seen, q_c, vmix[:, None]) - lo_[:, None]) / span[:, None], torch.zeros_like(q_c))
    logit = ieee_ln(pr)
    sigma = ((c_visit + most.to(torch.float64)) * c_scale)[:, None] * qhat
    x = logit + sigma
    mx = torch.where(mine, x, torch.full_like(x, float("-inf"))).max(dim=1).values
    e = torch.where(mine, ieee_exp(torch.where(mine, x - mx[:, None], torch.zeros_like(x))), torch.zeros_like(x))
    Z = torch.zeros(P, dtype=torch.float64, device=dev)
    for b in range(C):  # in this order: it is the contract
        Z = torch.where(mine[:, b], Z + e[:, b], Z)
    pi = torch.where(mine, e / torch.where(ok, Z, torch.ones_like(Z))[:, None], torch.zeros_like(e))
    out = dict(k=k, fc=fc, ok=ok, mine=mine, n=n_c, Nsum=Nsum, vhat=vhat, vmix=vmix, logit=logit, qhat=qhat, sigma=sigma, x=x, pi=pi)
    if pending is None:
        out["t"] = pi - n_c.to(torch.float64) / (1.0 + Nf)[:, None]
        return out
    m_c = n_c + pending.to(**i64)[rows[:, None], ch]
    Msum = torch.where(mine, m_c, zero_i).sum(dim=1)
    t = pi - m_c.to(torch.float64) / (1.0 + Msum.to(torch.float64))[:, None]
    out.update(m=m_c, Msum=Msum, t=torch.where(t == t, t, torch.full_like(t, float("-inf"))))
    return out


def gumbel_select_node(tree: dict, node: torch.Tensor, max_children: int, c_visit: float, c_scale: float, pending=None) -> dict:
    """The non-root rule of pcbenv_gumbel_tree_advance's SELECT at one node per root, in tensor code for any device, no host
    synchronisation: -> dict(child int64 [P]: the argmax of `gumbel_node_scores`' t over the node's children, ties to the
    lowest, 0 where the node has none in a healthy range; ok bool [P]: it has; errors int32 [1]: bit 1 (value 2) if a node
    that does not stop -- it is not terminal and num_children != 0 -- has a child range outside the tree).  The rule is
    deterministic and has no exploration constant; the visit counts it produces track pi.
    pending [P, N]: pcbenv_gumbel_tree_advance_leaves' rule -- `gumbel_node_scores(pending=)`'s t, in which a pending visit
    counts as a visit, so that the descents of one launch track pi as visits do.  None: as without the argument."""
    ns = gumbel_node_scores(tree, node, max_children, c_visit, c_scale, pending)
    rows = torch.arange(node.shape[0], dtype=torch.int64, device=ns["k"].device)
    a = node.to(device=rows.device, dtype=torch.int64)
    goes = ~((tree["terminal"][rows, a] != 0) | (ns["k"] == 0))
    child = torch.where(ns["ok"], _best_of(ns["t"], ns["mine"]), torch.zeros_like(ns["k"]))
    return dict(child=child, ok=ns["ok"], errors=((goes & ~ns["ok"]).any().to(torch.int32) * 2).reshape(1))


def new_gumbel_tensors(P: int, C: int, max_considered: int, simulations: int, device) -> dict:
    """The tensors pcbenv_gumbel_advance takes next to a PUCT tree's, as `BatchedPlacementEnv.gumbel_request` does: the budget
    of a move `sim_index` [P], `sim_visits` [P, C] (BEGIN zeroes them), the table `considered` [Mc + 1, n], and what CHOOSE
    writes: `move_slot`, `move_action`, `child_weights`, `child_policy` float32, `child_actions`, `root_value` float64."""
    i32 = dict(dtype=torch.int32, device=device)
    return dict(sim_index=torch.zeros(P, **i32), sim_visits=torch.zeros((P, C), **i32), considered=considered_visits(max_considered, simulations).to(device),
                move_slot=torch.empty(P, **i32), move_action=torch.empty((P, 3), **i32), child_weights=torch.empty((P, C), **i32),
                child_policy=torch.empty((P, C), dtype=torch.float32, device=device), child_actions=torch.empty((P, C, 3), **i32),
                root_value=torch.empty(P, dtype=torch.float64, device=device))


@dataclass
class GumbelSearch:
    """What `gumbel_search` and `gumbel_search_device` return."""
    search: PuctSearch           # the tree after the search, as `puct_search` reports it
    sim_index: torch.Tensor      # [P] int32: scheduled simulations made
    sim_visits: torch.Tensor     # [P, C] int32: of them, per root child
    move_slot: torch.Tensor      # [P] int32: the slot of the move's child, -1 for a root without children
    move_action: torch.Tensor    # [P, 3] int32
    child_weights: torch.Tensor  # [P, C] int32: the policy target in units of 2^-24
    child_policy: torch.Tensor   # [P, C] float32: the policy target
    child_actions: torch.Tensor  # [P, C, 3] int32
    root_value: torch.Tensor     # [P] float64


def _gumbel_arguments(root, simulations, max_considered, seed, first_root):
    n, Mc = int(simulations), int(max_considered)
    if n < 1 or Mc < 1 or Mc > 64:
        raise ValueError("a Gumbel search needs simulations >= 1 and max_considered in [1, 64]")
    if seed is None and not hasattr(root, "run_seed"):
        raise ValueError("a root without run_seed needs seed")
    return n, Mc, (int(root.run_seed) ^ 0x67756d62) if seed is None else int(seed), int(getattr(root, "first_env_index", 0) if first_root is None else first_root)


def _gumbel_launches(simulations, leaves, launches):
    """(L, the evaluations of a Gumbel search of n simulations with L leaves per launch): `launches`, or ceil(n / L) + 1 --
    n + 1 with one leaf, one evaluation per simulation and the root's own."""
    L = int(leaves)
    if L < 1 or L > 64:
        raise ValueError("a Gumbel search needs leaves in [1, 64]")
    E = -(-int(simulations) // L) + 1 if launches is None else int(launches)
    if E < 1:
        raise ValueError("a Gumbel search needs launches >= 1")
    return L, E


def _gumbel_node_rule(node_rule, full, leaves, launches):
    """True if every level below the root is the Gumbel node rule: full=True, which does not go with leaves > 1 or launches=,
    or node_rule="gumbel", which goes with any."""
    if node_rule not in ("puct", "gumbel"):
        raise ValueError('node_rule must be "puct" or "gumbel"')
    if full and (int(leaves) != 1 or launches is not None):
        raise ValueError("full=True does not go with leaves > 1 or launches=")
    return bool(full) or node_rule == "gumbel"


def gumbel_search(root, simulations: int, step_index: int, evaluate, max_considered: int = 16, c_visit: float = 50.0, c_scale: float = 1.0,
                  c_puct: float = 1.0, max_children: int = 16, max_steps=None, capacity=None, tree=None, seed=None, first_root=None,
                  gumbel_step_index=None, leaves: int = 1, launches=None, full: bool = False, node_rule: str = "puct") -> GumbelSearch:
    """The search of one move under the Gumbel rule, the whole of it as specification: `puct_search` with n + 1 =
    simulations + 1 evaluations whose level 0 is `gumbel_select_root`'s while the budget lasts, then `gumbel_choose`.  A fresh
    root spends evaluation 0 on its own expansion and then makes exactly n scheduled simulations; a kept root (tree=) makes n
    scheduled simulations and one PUCT descent.  Below the root every level is PUCT's.  The draws have the key (seed,
    first_root + p, gumbel_step_index), defaulting to root.run_seed ^ 0x67756d62, root.first_env_index and step_index;
    capacity defaults to 1 + (n + 1) * max_children.
    leaves = L > 1: several simulations per evaluation, the specification of pcbenv_gumbel_advance_leaves
    (include/pcbenv_gumbel_leaves.h): `puct_search(leaves=L)` with `launches` evaluations of P * L rows, default ceil(n / L) + 1.
    Leaf after leaf a root takes the next simulation of its schedule -- `gumbel_select_root` on the counters as the leaves
    before left them; its scores read no pending visit, so they are the same for every leaf -- and descends from the child
    by the pending-visit score.  A repeat consumes no simulation and ends the root's leaves of this evaluation, as does the
    end of the budget at a leaf behind the first; with the budget spent, the first leaf is one PUCT descent.  A root that is
    terminal or has no children has one leaf, itself.  A root whose repeats left sim_index < n when the launches are over
    is chosen as it stands: `sim_index` tells the share of the budget spent.  capacity defaults to 1 + launches * L *
    max_children.
    full=True: the specification of pcbenv_gumbel_tree_advance (include/pcbenv_gumbel_tree.h) -- level 0 once the budget is
    spent and every level below the root are `gumbel_select_node`'s, and `gumbel_select_root` and `gumbel_choose` complete a
    child without a visit with v_mix (full=True); c_puct is not read.  With leaves > 1 or launches= it raises ValueError: the
    rule reads no pending visit.
    node_rule="gumbel": the full rule with any leaves and launches.  With leaves = 1 and no launches= it is full=True, bit for
    bit.  Otherwise it is the specification of pcbenv_gumbel_tree_advance_leaves (include/pcbenv_gumbel_tree_leaves.h): the
    leaf loop above with `gumbel_select_root(full=True)` at the root and, at every level below it and at level 0 once the
    budget is spent, `gumbel_select_node(pending=)` -- a pending visit counts as a visit of the child and enters nothing else;
    `gumbel_choose(full=True)`; c_puct is not read.  "puct", the default: the search is what it is without this argument."""
    n, Mc, seed, first = _gumbel_arguments(root, simulations, max_considered, seed, first_root)
    full = _gumbel_node_rule(node_rule, full, leaves, launches)
    C, c_visit, c_scale = _gumbel_rule(max_children, c_visit, c_scale)
    key = int(step_index if gumbel_step_index is None else gumbel_step_index)
    P, dev = int(root.num_envs), getattr(root, "device", "cpu")
    table = considered_visits(Mc, n).to(dev)
    state = dict(sim_index=torch.zeros(P, dtype=torch.int32, device=dev), sim_visits=torch.zeros((P, C), dtype=torch.int32, device=dev))
    L, E = _gumbel_launches(n, leaves, launches)

    def root_select(now, stopped, nxt):
        sel = gumbel_select_root(now, state["sim_index"], state["sim_visits"], table, C, c_visit, c_scale, seed, key, first, full)
        state.update(sim_index=sel["sim_index"], sim_visits=sel["sim_visits"])
        return torch.where(sel["scheduled"], now["first_child"][:, 0].to(torch.int64) + sel["child"], nxt)

    def level_select(d, now, node, stopped, nxt):
        rows = torch.arange(P, dtype=torch.int64, device=node.device)
        return now["first_child"][rows, node].to(torch.int64) + gumbel_select_node(now, node, C, c_visit, c_scale)["child"]
    if L == 1 and launches is None:
        ps = puct_search(root, n + 1, step_index, evaluate, c_puct=c_puct, max_children=C, max_steps=max_steps, capacity=capacity, tree=tree,
                         root_select=root_select, level_select=level_select if full else None)
    else:
        proposed = {}

        def leaf_begin(l, now, alive):  # a root that takes no descent, or has no simulation left, has its one leaf and no more
            proposed.clear()
            if l == 0:
                return alive
            k, fc, t = now["num_children"][:, 0], now["first_child"][:, 0], state["sim_index"].to(torch.int64)
            ok = (k >= 1) & (k <= C) & (fc >= 1) & (fc <= int(now["prior"].shape[1]) - k)
            return alive & ~(now["terminal"][:, 0] != 0) & ok & (t >= 0) & (t < n)

        def propose(now, stopped, nxt):  # the counters move when the leaf has turned out to be one
            sel = proposed["sel"] = gumbel_select_root(now, state["sim_index"], state["sim_visits"], table, C, c_visit, c_scale, seed, key, first, full)
            return torch.where(sel["scheduled"], now["first_child"][:, 0].to(torch.int64) + sel["child"], nxt)

        def leaf_end(l, alive):
            sel = proposed.get("sel")
            if sel is not None:
                keep = alive & sel["scheduled"]
                state.update(sim_index=torch.where(keep, sel["sim_index"], state["sim_index"]),
                             sim_visits=torch.where(keep[:, None], sel["sim_visits"], state["sim_visits"]))

        def pending_select(d, now, node, stopped, nxt):
            rows = torch.arange(P, dtype=torch.int64, device=node.device)
            return now["first_child"][rows, node].to(torch.int64) + gumbel_select_node(now, node, C, c_visit, c_scale, now["pending"])["child"]
        ps = puct_search(root, E, step_index, evaluate, c_puct=c_puct, max_children=C, max_steps=max_steps, capacity=capacity, tree=tree, leaves=L,
                         root_select=propose, leaf_begin=leaf_begin, leaf_end=leaf_end, pending_select=pending_select if full else None)
    ch = gumbel_choose(search_tree(ps), state["sim_visits"], C, c_visit, c_scale, seed, key, first, full)
    return GumbelSearch(ps, state["sim_index"], state["sim_visits"], ch["move_slot"], ch["move_action"], ch["child_weights"], ch["child_policy"],
                        ch["child_actions"], ch["root_value"])


def _gumbel_iterations(root, greq, tree, n, T, evaluate, step_index, seed, key, full=False):
    """The launches of one device Gumbel search on `tree`: BEGIN | SELECT, then n + 1 times `evaluate` followed by ABSORB |
    SELECT, the last time by ABSORB alone -- pcbenv_gumbel_advance every one, pcbenv_gumbel_tree_advance with full."""
    advance = root.gumbel_tree_advance if full else root.gumbel_advance
    advance(greq, GUMBEL_BEGIN | GUMBEL_SELECT, seed=seed, step_index=key)
    for m in range(n + 1):
        ev = evaluate(tree["paths"], tree["path_len"], int(step_index) + m * T)
        over = ev.terminal.view(torch.uint8) if ev.terminal.dtype == torch.bool else ev.terminal
        advance(greq, GUMBEL_ABSORB | (GUMBEL_SELECT if m < n else 0), ev.value, over, ev.cand_count, ev.cand_actions, ev.cand_prior,
                seed=seed, step_index=key)


def _gumbel_leaves_iterations(root, greq, tree, E, T, evaluate, step_index, seed, key, full=False):
    """The launches of one device Gumbel search with leaves on `tree`: BEGIN | SELECT, then E times `evaluate` followed by
    ABSORB | SELECT, the last time by ABSORB alone -- pcbenv_gumbel_advance_leaves every one, pcbenv_gumbel_tree_advance_leaves
    with full."""
    advance = root.gumbel_tree_advance_leaves if full else root.gumbel_advance_leaves
    advance(greq, GUMBEL_BEGIN | GUMBEL_SELECT, seed=seed, step_index=key)
    for m in range(E):
        ev = evaluate(tree["paths"], tree["path_len"], int(step_index) + m * T)
        over = ev.terminal.view(torch.uint8) if ev.terminal.dtype == torch.bool else ev.terminal
        advance(greq, GUMBEL_ABSORB | (GUMBEL_SELECT if m + 1 < E else 0), ev.value, over, ev.cand_count, ev.cand_actions, ev.cand_prior, seed=seed,
                step_index=key)


def gumbel_search_device(root, simulations: int, step_index: int, evaluate, max_considered: int = 16, c_visit: float = 50.0, c_scale: float = 1.0,
                         c_puct: float = 1.0, max_children: int = 16, max_steps=None, capacity=None, tree=None, seed=None,
                         gumbel_step_index=None, leaves: int = 1, launches=None, full: bool = False, node_rule: str = "puct") -> GumbelSearch:
    """`gumbel_search` with the tree kept by the device: `root.gumbel_advance` (pcbenv_gumbel_advance) is the one launch per
    evaluation, with no tensor operation between them: BEGIN | SELECT first -- a fresh tree gets `puct_advance(INIT)` before
    it -- then n + 1 times `evaluate(tree paths, path_len, step_index + m * max_steps)` followed by ABSORB | SELECT, the last
    time by ABSORB alone, then CHOOSE.  The same search as `gumbel_search` with the same arguments: the same evaluations, the
    same tree, counters, move and target, field by field, floats by their bits.
    tree: the search continues in this tree, in place -- the tensors of `new_puct_tree` and `new_gumbel_tensors` (for this
    max_considered and simulations) as an earlier search or `puct_move(MOVE_REROOT)` left them.
    leaves = L > 1, launches: `gumbel_search(leaves=L, launches=)` with `root.gumbel_advance_leaves`
    (pcbenv_gumbel_advance_leaves, include/pcbenv_gumbel_leaves.h) as the one launch per evaluation: BEGIN | SELECT first -- a
    fresh tree gets `puct_advance_leaves(INIT)` before it, so that `pending` is zero -- then `launches` times `evaluate` and
    ABSORB | SELECT, the last time ABSORB alone, then CHOOSE; `evaluate` sees P * L rows, path_len -1 where there is no leaf.  A
    tree that is kept is one of `new_puct_tree(leaves=L)`.
    full=True: `gumbel_search(full=True)` with `root.gumbel_tree_advance` (pcbenv_gumbel_tree_advance,
    include/pcbenv_gumbel_tree.h) as the one launch per evaluation and as CHOOSE, on the same tensors; not with leaves > 1 or
    launches= (ValueError).  Without it the launches are what they are without this argument.
    node_rule="gumbel": `gumbel_search(node_rule="gumbel")`.  With leaves = 1 and no launches= the launches are full=True's,
    pcbenv_gumbel_tree_advance; otherwise every launch, CHOOSE included, is `root.gumbel_tree_advance_leaves`
    (pcbenv_gumbel_tree_advance_leaves, include/pcbenv_gumbel_tree_leaves.h) on the tensors of leaves = L.  Without it the
    launches are what they are without this argument."""
    from . import _lib
    n, Mc, seed, _ = _gumbel_arguments(root, simulations, max_considered, seed, None)
    full = _gumbel_node_rule(node_rule, full, leaves, launches)
    L, E = _gumbel_launches(n, leaves, launches)
    key = int(step_index if gumbel_step_index is None else gumbel_step_index)
    kept = tree is not None
    if L != 1 or launches is not None:
        P, C, M, T, N = _puct_arguments(root, E, max_children, max_steps, capacity, tree, L)
        if not kept:
            tree = new_puct_tree(P, N, T, root.device, L)
            tree.update(new_gumbel_tensors(P, C, Mc, n, root.device))
            root.puct_advance_leaves(root.puct_leaves_request(tree, c_puct, C, L), _lib.TREE_INIT)
        greq = root.gumbel_leaves_request(tree, c_puct, C, c_visit, c_scale, L)
        _gumbel_leaves_iterations(root, greq, tree, E, T, evaluate, step_index, seed, key, full)
        (root.gumbel_tree_advance_leaves if full else root.gumbel_advance_leaves)(greq, GUMBEL_CHOOSE, seed=seed, step_index=key)
        return GumbelSearch(puct_result(tree, C), tree["sim_index"], tree["sim_visits"], tree["move_slot"], tree["move_action"], tree["child_weights"],
                            tree["child_policy"], tree["child_actions"], tree["root_value"])
    P, C, M, T, N = _puct_arguments(root, n + 1, max_children, max_steps, capacity, tree)
    if not kept:
        tree = new_puct_tree(P, N, T, root.device)
        tree.update(new_gumbel_tensors(P, C, Mc, n, root.device))
        root.puct_advance(root.puct_request(tree, c_puct, C), _lib.TREE_INIT)
    greq = root.gumbel_request(tree, c_puct, C, c_visit, c_scale)
    _gumbel_iterations(root, greq, tree, n, T, evaluate, step_index, seed, key, full)
    (root.gumbel_tree_advance if full else root.gumbel_advance)(greq, GUMBEL_CHOOSE, seed=seed, step_index=key)
    return GumbelSearch(puct_result(tree, C), tree["sim_index"], tree["sim_visits"], tree["move_slot"], tree["move_action"], tree["child_weights"],
                        tree["child_policy"], tree["child_actions"], tree["root_value"])


@dataclass
class SelfPlay:
    """What `puct_selfplay` returns: per move (the leading extent M = moves) and root."""
    actions: torch.Tensor        # [M, P, 3] int32: the move played (zero for a root without children)
    child_visits: torch.Tensor   # [M, P, C] int32: the visit counts of the root's children -- the policy target of the move
    child_actions: torch.Tensor  # [M, P, C, 3] int32: their actions
    root_value: torch.Tensor     # [M, P] float64: value_sum / visits of the root after the move's search
    reward: torch.Tensor         # [M, P] float64: what `step` reported for the move
    done: torch.Tensor           # [M, P] uint8
    kept_visits: torch.Tensor    # [M, P] int32: the visits the next move's root started with (0: a fresh tree)
    errors: torch.Tensor         # 0-dim int32: bit 0 = the children of a node did not fit into the free slots, bit 1 = a damaged tree
    tree: dict                   # the tree and move tensors as the last move left them


def puct_selfplay(root, evaluate, moves: int, iterations: int, step_index: int = 0, c_puct: float = 1.0, max_children: int = 16,
                  max_steps=None, capacity=None, mode: int = MOVE_GREEDY, seed=None, on_move=None, leaves: int = 1, root_noise=None,
                  noise_seed=None, gumbel=None, gumbel_seed=None, gumbel_full: bool = False, gumbel_node_rule: str = "puct") -> SelfPlay:
    """Plays `moves` moves of every root environment with a PUCT search whose tree stays on the device and is kept from
    move to move.  Per move: `iterations` of search on the kept tree (`evaluate` and one pcbenv_puct_advance launch each,
    as `puct_search_device(tree=)`); `root.puct_move(MOVE_CHOOSE)` -- the visit distribution of the root and the move,
    greedy or in proportion to the visits (`mode`); `root.step(move_action)`; `root.puct_move(MOVE_REROOT, reset=done)` --
    the subtree of the move becomes the tree, an episode that ended gets an empty one.  Two launches per move next to
    `step`, nothing allocated inside the loop but the results' rows, no host synchronisation.
    Iteration m of move j calls evaluate(paths, path_len, step_index + (j * iterations + m) * max_steps); the proportional
    draw of move j has the key (seed, first_env_index + p, step_index + j), seed defaulting to run_seed ^ 0x6d6f7665 so that
    it shares no key with the environment's own draws.
    capacity: node slots per root, default 1 + 2 * iterations * max_children.  A kept subtree and the children the next
    search adds have to fit: an overflow shows as bit 0 of `errors`, as in `puct_search_device`, and the search goes on in
    the full tree.  The bound that can never overflow is 1 + moves * iterations * max_children.
    on_move: called as on_move(j, tree) after move j's REROOT with the dict of the tree and move tensors (`remap` among
    them), which the next move overwrites: a trainer copies what it keeps.
    leaves = L > 1: every iteration selects and evaluates L leaves per root (`puct_search_device(leaves=L)`); `evaluate`
    sees P * L rows and the default capacity is 1 + 2 * iterations * L * max_children.  `pending` is zero after every
    search, so the move's two launches take the tree as it is.
    root_noise = (alpha, eps): exploration noise on the root's priors, once per root and move
    (`puct_search_device(root_noise=)`): the kept, expanded root of a move before its first descent, a fresh one as soon as
    its first evaluation has expanded it.  The draws of move j have the key (noise_seed, first_env_index + p, step_index
    + j), noise_seed defaulting to run_seed ^ 0x6e6f6973, so they share no key with the step draws or the move draw.
    gumbel = (max_considered, c_visit, c_scale): every move is a Gumbel search (`gumbel_search_device`) of n = `iterations`
    simulations, n + 1 evaluations -- iteration m of move j calls evaluate(paths, path_len, step_index + (j * (n + 1) + m) *
    max_steps) -- and pcbenv_gumbel_advance's CHOOSE stands in the place of `puct_move(MOVE_CHOOSE)`: the move is the best
    of the most-simulated root children, `child_visits` holds `child_weights`, the policy target softmax(logit +
    sigma(completed q)) in units of 2^-24, which `visit_targets.cross_entropy` takes as it takes visit counts.  `mode` is not
    read: the choice is the sample.  The draws of move j have the key (gumbel_seed, first_env_index + p, step_index + j),
    gumbel_seed defaulting to run_seed ^ 0x67756d62.  The default capacity is 1 + 2 * (n + 1) * max_children; together with
    root_noise it raises ValueError.  With leaves = L > 1 every move is `gumbel_search_device(leaves=L)`: ceil(n / L) + 1
    evaluations of P * L rows and pcbenv_gumbel_advance_leaves launches, the default capacity 1 + 2 * (ceil(n / L) + 1) * L *
    max_children; `pending` is zero after the last ABSORB, so REROOT takes the tree as it is.
    gumbel_full=True: every move is `gumbel_search_device(full=True)`, the launches pcbenv_gumbel_tree_advance's
    (include/pcbenv_gumbel_tree.h) on the same tensors; it needs gumbel= and leaves = 1 (ValueError otherwise).
    gumbel_node_rule="gumbel": every move is `gumbel_search_device(node_rule="gumbel", leaves=L)` -- gumbel_full=True's launches
    with leaves = 1, pcbenv_gumbel_tree_advance_leaves' (include/pcbenv_gumbel_tree_leaves.h) with more; it needs gumbel=
    (ValueError otherwise).  "puct", the default: the game is what it is without this argument.
    `evaluate` must be callable: ValueError otherwise, before anything is allocated."""
    from . import _lib, _move_lib
    L = int(leaves)
    if gumbel_full and (gumbel is None or L != 1):
        raise ValueError("gumbel_full=True needs gumbel= and leaves = 1")
    if gumbel_node_rule not in ("puct", "gumbel") or (gumbel_node_rule == "gumbel" and gumbel is None):
        raise ValueError('gumbel_node_rule must be "puct" or "gumbel", and "gumbel" needs gumbel=')
    gumbel_full = bool(gumbel_full) or gumbel_node_rule == "gumbel"
    if not callable(evaluate):
        raise ValueError("puct_selfplay needs an evaluate(paths, path_len, step_index0) to call")
    if gumbel is not None and root_noise is not None:
        raise ValueError("gumbel= does not go with root_noise")
    E = int(iterations) + 1 if gumbel is not None else int(iterations)  # evaluations per move
    if gumbel is not None and L != 1:
        E = _gumbel_launches(_gumbel_arguments(root, iterations, gumbel[0], gumbel_seed, None)[0], L, None)[1]
    P, C, M, T, N = _puct_arguments(root, E, max_children, max_steps, 1 + 2 * E * L * int(max_children) if capacity is None else capacity, leaves=L)
    J = int(moves)
    if J < 1:
        raise ValueError("puct_selfplay needs moves >= 1")
    dev = root.device
    tree = new_puct_tree(P, N, T, dev, L)
    tree.update(new_move_tensors(P, N, C, dev))
    greq = None
    if gumbel is not None:
        n, Mc, gseed, _ = _gumbel_arguments(root, iterations, gumbel[0], gumbel_seed, None)
        tree.update(new_gumbel_tensors(P, C, Mc, n, dev))
        greq = root.gumbel_request(tree, c_puct, C, gumbel[1], gumbel[2]) if L == 1 else root.gumbel_leaves_request(tree, c_puct, C, gumbel[1], gumbel[2], L)
    req, mreq = root.puct_request(tree, c_puct, C) if L == 1 else root.puct_leaves_request(tree, c_puct, C, L), root.puct_move_request(tree, C)
    if gumbel is not None:
        (root.puct_advance if L == 1 else root.puct_advance_leaves)(req, _lib.TREE_INIT)
    seed = (root.run_seed ^ 0x6d6f7665) if seed is None else int(seed)
    noise = _noise_arguments(root, root_noise, noise_seed, None)
    nreq = root.puct_noise_request(tree, C) if noise is not None else None
    i32 = dict(dtype=torch.int32, device=dev)
    out = SelfPlay(torch.empty((J, P, 3), **i32), torch.empty((J, P, C), **i32), torch.empty((J, P, C, 3), **i32),
                   torch.empty((J, P), dtype=torch.float64, device=dev), torch.empty((J, P), dtype=torch.float64, device=dev),
                   torch.empty((J, P), dtype=torch.uint8, device=dev), torch.empty((J, P), **i32), tree["errors_dev"][0], tree)
    for j in range(J):
        if gumbel is not None and L != 1:
            _gumbel_leaves_iterations(root, greq, tree, M, T, evaluate, int(step_index) + j * M * T, gseed, int(step_index) + j, gumbel_full)
            (root.gumbel_tree_advance_leaves if gumbel_full else root.gumbel_advance_leaves)(greq, GUMBEL_CHOOSE, seed=gseed, step_index=int(step_index) + j)
        elif gumbel is not None:
            _gumbel_iterations(root, greq, tree, n, T, evaluate, int(step_index) + j * M * T, gseed, int(step_index) + j, gumbel_full)
            (root.gumbel_tree_advance if gumbel_full else root.gumbel_advance)(greq, GUMBEL_CHOOSE, seed=gseed, step_index=int(step_index) + j)
        else:
            _puct_iterations(root, req, tree, M, T, evaluate, int(step_index) + j * M * T, _lib.TREE_SELECT if j else _lib.TREE_INIT | _lib.TREE_SELECT, L,
                             None if noise is None else (nreq, noise[0], noise[1], noise[2], int(step_index) + j))
            root.puct_move(mreq, _move_lib.MOVE_CHOOSE, mode=mode, seed=seed, step_index=int(step_index) + j)
        _, reward, done, _ = root.step(tree["move_action"])
        out.actions[j], out.child_visits[j], out.child_actions[j], out.root_value[j] = (tree["move_action"], tree["child_weights" if gumbel is not None else "child_visits"],
                                                                                         tree["child_actions"], tree["root_value"])
        out.reward[j], out.done[j] = reward, done
        root.puct_move(mreq, _move_lib.MOVE_REROOT, reset=done)
        out.kept_visits[j] = tree["visits"][:, 0]
        if on_move is not None:
            on_move(j, tree)
    return out


def top_priors(logits: torch.Tensor, action_mask: torch.Tensor, K: int):
    """The K most probable legal actions of a masked policy: (cand_count int32 [P], cand_actions int32 [P, K, 3],
    cand_prior float32 [P, K]).  logits [P, A] in flat action order (a = o*H*W + x*W + y), action_mask [P, O, H, W] (or
    [P, H, W]: one orientation), non-zero = legal.  The probabilities are the float32 softmax over the legal logits,
    exp(l - max) / sum; a stable descending sort puts equal probabilities in flat-index order, the first K are kept
    (cand_count = min(K, legal count); the entries behind it are zero) and come back in the tuple format `step` takes.
    A torch chain for any device, no host synchronisation."""
    P = logits.shape[0]
    legal = action_mask.reshape(P, -1) != 0
    A = legal.shape[1]
    H, W = int(action_mask.shape[-2]), int(action_mask.shape[-1])
    l32 = logits.reshape(P, A).to(torch.float32)
    ninf = torch.full_like(l32, float("-inf"))
    top = torch.where(legal, l32, ninf).max(dim=1, keepdim=True).values
    e = torch.where(legal, torch.exp(l32 - torch.where(legal.any(dim=1, keepdim=True), top, torch.zeros_like(top))), torch.zeros_like(l32))
    p = e / e.sum(dim=1, keepdim=True).clamp(min=torch.finfo(torch.float32).tiny)
    K = int(K)
    order = torch.sort(torch.where(legal, p, torch.full_like(p, -1.0)), dim=1, descending=True, stable=True).indices[:, :K]
    if order.shape[1] < K:  # fewer actions than candidates asked for
        order = torch.cat([order, torch.zeros((P, K - order.shape[1]), dtype=order.dtype, device=order.device)], dim=1)
    count = legal.sum(dim=1).clamp(max=K)
    kept = torch.arange(K, device=logits.device)[None, :] < count[:, None]
    flat = torch.where(kept, order, torch.zeros_like(order))
    prior = torch.where(kept, p.gather(1, flat), torch.zeros((), dtype=torch.float32, device=p.device))
    o, rem = torch.div(flat, H * W, rounding_mode="floor"), flat % (H * W)
    actions = torch.stack([o, torch.div(rem, W, rounding_mode="floor"), rem % W], dim=2).to(torch.int32)
    return count.to(torch.int32), actions.contiguous(), prior.contiguous()


def network_evaluator(root, planner, logits_fn, value_fn=None, max_children: int = 16, priors: str = "torch", leaves: int = 1):
    """An `evaluate` for `puct_search` / `puct_search_device` that scores a node with a network:
    `(paths, path_len, step_index0) -> Evaluation`.  planner: P = root.num_envs environments of the root's definition
    with auto_reset=False, the root's run_seed and first_env_index 0 (the constraints of `policy_backend`).

    One call: `planner.gather_(arange(P), source=root, paths=paths, path_len=path_len)` materialises the P nodes the paths
    name (pcbenv_gather_paths, one launch); a node is terminal if a transition of its path reported done, `(gather_length
    > 0) & done`.  The candidates are `top_priors(logits_fn(planner.obs), planner.obs["action_mask"], max_children)`.  The
    value is `planner.reward` where the node is terminal; elsewhere `value_fn(planner.obs)` [P], or, without a value_fn,
    the final reward of a uniform rollout from the node: `root.playout(k=1, step_index=step_index0, paths=paths,
    path_len=path_len, max_steps=paths.shape[0])` (pcbenv_playout_paths, one launch).  No host synchronisation.

    priors="device": the candidates are `planner.top_priors(logits_fn(planner.obs), max_children)` instead
    (pcbenv_top_priors, one launch): the legal set is read from the planner's state, no mask is copied and nothing is
    sorted.  The two differ where float32 `exp` makes unequal logits equally probable, or zero: there the torch chain,
    which orders probabilities, falls back to index order, and the device, which orders the logits themselves, keeps logit
    order; the priors differ in their last bits (the device forms them in float64 and rounds once).  With constant logits
    the two are bit-identical: Z = n exactly and every prior is float32(1 / n) on both sides.

    leaves = L > 1, for the searches' `leaves=L`: the planner has P * L environments, row p * L + l forks root p
    (`gather_` with the index arange(P * L) // L), and the rollout without a value_fn is `root.playout(k=L, paths=...)`.
    A row with path_len == -1 is no leaf: it keeps its episode, and what comes back for it is ignored by the search."""
    if priors not in ("torch", "device"):
        raise ValueError(f'priors must be "torch" or "device", got {priors!r}')
    L = int(leaves)
    P = int(planner.num_envs)
    if L < 1 or P != int(root.num_envs) * L:
        raise ValueError(f"the planner needs {int(root.num_envs)}" + (f" x {L}" if L != 1 else "") + f" environments, it has {P}")
    if planner.auto_reset:
        raise ValueError("the planner must be created with auto_reset=False (a node's episode ends at its first done)")
    if planner.run_seed != root.run_seed or planner.first_env_index != 0:
        raise ValueError("the planner must have the root's run_seed and first_env_index 0 (the keys of the draws)")
    K = int(max_children)

    def evaluate(paths, path_len, step_index0):
        dev, T = planner.device, int(paths.shape[0])
        index = torch.arange(P, dtype=torch.int32, device=dev) if L == 1 else child_index(P // L, L, dev)
        planner.gather_(index, source=root, paths=paths, path_len=path_len)
        obs = planner.obs
        over = (planner.gather_length > 0) & planner.done.bool()
        if priors == "device":
            count, actions, prior = planner.top_priors(logits_fn(obs).reshape(P, -1), K)
        else:
            count, actions, prior = top_priors(logits_fn(obs), obs["action_mask"], K)
        if value_fn is not None:
            leaf = value_fn(obs).to(torch.float64).reshape(P)
        else:
            leaf = root.playout(k=L, step_index=int(step_index0), paths=paths, path_len=path_len, max_steps=T).reward
        value = torch.where(over, planner.reward.to(torch.float64), leaf)
        return Evaluation(value, over.to(torch.uint8), count, actions, prior)
    return evaluate


# ---- the frontier: a beam search over placements ---------------------------------------------------------------------
FRONTIER_INIT, FRONTIER_ADVANCE = 1, 2  # include/pcbenv_frontier.h
MAX_FRONTIER_WIDTH, MAX_FRONTIER_CANDIDATES, MAX_FRONTIER_ROWS = 64, 64, 1024
FRONTIER_ERR_ROW = 2  # bit 1 of the error word: a path_len outside [-1, T] in the rows read


def new_frontier_tensors(P: int, W: int, K: int, T: int, device) -> dict:
    """The tensors of P frontiers of W * K rows and T steps, as `BatchedPlacementEnv.frontier_request` takes them: the two
    sets of rows `paths_s` [T, P * W * K, 3], `path_len_s` and `cum_logp_s` [P * W * K], s = 0, 1, which a search swaps
    between depths, `parent_row`, `live`, the accumulators `best_value`, `best_len`, `best_path` and `errors_dev`.
    Uninitialised but for the paths, `best_path`, `cum_logp_s` and `errors_dev`: FRONTIER_INIT fills the rest."""
    i32, f64 = dict(dtype=torch.int32, device=device), dict(dtype=torch.float64, device=device)
    R = int(P) * int(W) * int(K)
    ft = {}
    for s in (0, 1):
        ft.update({f"paths_{s}": torch.zeros((T, R, 3), **i32), f"path_len_{s}": torch.empty(R, **i32), f"cum_logp_{s}": torch.zeros(R, **f64)})
    ft.update(parent_row=torch.empty(R, **i32), live=torch.empty(P, **i32), best_value=torch.empty(P, **f64), best_len=torch.empty(P, **i32),
              best_path=torch.zeros((T, P, 3), **i32), errors_dev=torch.zeros(1, **i32))
    return ft


def log_prior(prior: torch.Tensor) -> torch.Tensor:
    """float64 ln of float32 priors as csrc/pcb_frontier.h:log_prior gives it: `ieee_ln` of a prior that is a positive,
    finite, normal float32 -- read off its bits -- and -inf of any other."""
    b = prior.contiguous().view(torch.int32)
    e = (b >> 23) & 0xff
    ok = (b >= 0) & (e >= 1) & (e <= 254)
    x = torch.where(ok, prior, torch.ones_like(prior)).to(torch.float64)
    return torch.where(ok, ieee_ln(x), torch.full_like(x, float("-inf")))


def _frontier_rows(ft: dict, width: int, num_candidates: int, evaluation, swap: bool):
    """Steps 1 and 2 of `frontier_advance` -- the live rows, bit 1 of the error word and the best finished row -- and the
    tensors the later steps read, as a namespace."""
    W, K = int(width), int(num_candidates)
    F = W * K
    T, P = int(ft["best_path"].shape[0]), int(ft["best_path"].shape[1])
    a, b = (1, 0) if swap else (0, 1)
    paths_in, len_in, cum_in = ft[f"paths_{a}"], ft[f"path_len_{a}"], ft[f"cum_logp_{a}"]
    paths_out, len_out, cum_out = ft[f"paths_{b}"], ft[f"path_len_{b}"], ft[f"cum_logp_{b}"]
    dev = len_in.device
    slot = torch.arange(F, dtype=torch.int64, device=dev)
    ev = evaluation
    f64 = dict(dtype=torch.float64, device=dev)
    ninf = torch.full((), float("-inf"), **f64)
    length = len_in.view(P, F).to(torch.int64)
    live = (length >= 0) & (length <= T)
    damaged = (length < -1) | (length > T)
    if ft.get("errors_dev") is not None:
        ft["errors_dev"] |= (damaged.any().to(torch.int32) * FRONTIER_ERR_ROW)
    value = ev.value.to(**f64).view(P, F)
    over = ev.terminal.to(dev).view(P, F) != 0
    k = ev.cand_count.to(device=dev, dtype=torch.int64).view(P, F).clamp(0, K)
    cand_actions = ev.cand_actions.to(device=dev, dtype=torch.int32).view(P, F, K, 3)
    cand_prior = ev.cand_prior.to(device=dev, dtype=torch.float32).view(P, F, K)
    rows = torch.arange(P, dtype=torch.int64, device=dev)
    pin = paths_in.view(T, P, F, 3)
    # finished rows: the first of those with the largest value is the one a walk in increasing i ends with
    fin = live & over
    v = torch.where(fin & ~torch.isnan(value), value, ninf)
    top = v.max(dim=1, keepdim=True).values
    first = torch.where(fin & (v == top), slot[None, :], F).min(dim=1).values.clamp(max=F - 1)
    v_first, len_first = v[rows, first], length[rows, first]
    better = fin.any(dim=1) & ((ft["best_len"] == -1) | (v_first > ft["best_value"]))
    ft["best_value"].copy_(torch.where(better, v_first, ft["best_value"]))
    ft["best_len"].copy_(torch.where(better, len_first.to(torch.int32), ft["best_len"]))
    step = torch.arange(T, dtype=torch.int64, device=dev)
    taken = better[None, :] & (step[:, None] < len_first[None, :])                                    # [T, P]
    ft["best_path"].copy_(torch.where(taken[:, :, None], pin[:, rows, first], ft["best_path"]))
    expandable = live & ~over & (length < T) & (k > 0)
    cum = cum_in.view(P, F)
    return SimpleNamespace(**locals())


def _frontier_children(ft: dict, x, kept: torch.Tensor, n: torch.Tensor):
    """Step 4 of `frontier_advance` for the rows and tensors `x` of `_frontier_rows`: the children of the kept rows `kept`
    [P, W] (slots of the in set, in rank order), of which the first `n` [P] count, into the out set.  -> (child, parent, c),
    [P, F] bool, [P, F] and [F]: which out slots hold a child, the in slot of their parent, and their candidate."""
    W, K, F, T, P, dev, slot, length, k, cum, rows, pin, step = x.W, x.K, x.F, x.T, x.P, x.dev, x.slot, x.length, x.k, x.cum, x.rows, x.pin, x.step
    len_out, cum_out, paths_out, cand_prior, cand_actions = x.len_out, x.cum_out, x.paths_out, x.cand_prior, x.cand_actions
    w, c = torch.div(slot, K, rounding_mode="floor"), slot % K
    parent = kept[:, w]                                                                                # [P, F]
    child = (w[None, :] < n[:, None]) & (c[None, :] < k.gather(1, parent))
    plen = length.gather(1, parent)
    len_out.view(P, F).copy_(torch.where(child, plen + 1, -1))
    ft["parent_row"].view(P, F).copy_(torch.where(child, parent, -1))
    lp = log_prior(cand_prior[rows[:, None], parent, c[None, :]])
    cum_out.view(P, F).copy_(torch.where(child, cum.gather(1, parent) + lp, cum_out.view(P, F)))
    pout = paths_out.view(T, P, F, 3)
    inherited = pin.gather(2, parent[None, :, :, None].expand(T, P, F, 3))
    own = cand_actions[rows[:, None], parent, c[None, :]]                                              # [P, F, 3]
    at = step[:, None, None]
    new = torch.where((child[None] & (at < plen[None]))[..., None], inherited,
                      torch.where((child[None] & (at == plen[None]))[..., None], own[None].expand(T, P, F, 3), pout))
    pout.copy_(new)
    ft["live"].copy_(child.sum(dim=1))
    return child, parent, c


def frontier_advance(ft: dict, phases: int, width: int, num_candidates: int, prior_weight: float = 0.0, evaluation=None, swap: bool = False) -> None:
    """One depth of a beam search over placements, in tensor code for any device and without a host synchronisation: the
    specification of pcbenv_frontier_advance (include/pcbenv_frontier.h), on the tensors of `new_frontier_tensors`, in
    place.  swap=False reads set 0 as `in` and writes set 1 as `out`; swap=True the other way round.  W = width, K =
    num_candidates, F = W * K rows per root, row p * F + i the slot i of root p.
    FRONTIER_INIT writes the out set and nothing else: path_len 0 for slot 0 of every root and -1 for the others, cum_logp
    of slot 0 = 0.0, parent_row = -1, live = 1, best_len = -1 and best_value = -inf; the paths and best_path are untouched.
    FRONTIER_ADVANCE takes `evaluation`, the `Evaluation` of the in rows, in four steps per root.
      live rows        path_len in [0, T]; a value outside [-1, T] is no row and sets bit 1 of `errors_dev`.
      finished rows    live rows the evaluation calls terminal, taken in increasing i with v = value, a NaN counted as -inf:
                       one with best_len == -1 or v > best_value becomes the root's best -- best_value = v, best_len = its
                       length, best_path rows d < that length = its path.  A finished row is never expanded.
      the order        live, unfinished rows with path_len < T and k = clamp(cand_count, 0, K) > 0 are expandable, the
                       others are dropped.  Their score is value if prior_weight == 0, and value + prior_weight * cum_logp
                       otherwise (two operations), a NaN counted as -inf; the order is the score descending, ties -- -0.0
                       with +0.0 among them -- to the lower i; the first n = min(W, expandable) rows are kept.
      the children     child c < k of the kept row of rank w goes to slot w * K + c of the out set: the parent's path and
                       cand_actions[parent, c] behind it, path_len + 1, cum_logp of the parent + `log_prior` of the
                       candidate's prior, parent_row = the parent's slot i.  Every other slot gets path_len = parent_row =
                       -1 and nothing else; live = the child rows written."""
    W, K, ph = int(width), int(num_candidates), int(phases)
    if ph not in (FRONTIER_INIT, FRONTIER_ADVANCE):
        raise ValueError("phases must be FRONTIER_INIT or FRONTIER_ADVANCE")
    if W < 1 or W > MAX_FRONTIER_WIDTH or K < 1 or K > MAX_FRONTIER_CANDIDATES or W * K > MAX_FRONTIER_ROWS:
        raise ValueError(f"width and num_candidates must be in [1, 64] and their product at most {MAX_FRONTIER_ROWS}, got {W} and {K}")
    F = W * K
    T, P = int(ft["best_path"].shape[0]), int(ft["best_path"].shape[1])
    a, b = (1, 0) if swap else (0, 1)
    paths_in, len_in, cum_in = ft[f"paths_{a}"], ft[f"path_len_{a}"], ft[f"cum_logp_{a}"]
    paths_out, len_out, cum_out = ft[f"paths_{b}"], ft[f"path_len_{b}"], ft[f"cum_logp_{b}"]
    dev = len_in.device
    if P == 0:
        return
    slot = torch.arange(F, dtype=torch.int64, device=dev)
    if ph == FRONTIER_INIT:
        first = (slot == 0)[None, :].expand(P, F)
        len_out.view(P, F).copy_(torch.where(first, 0, -1))
        cum_out.view(P, F)[:, 0] = 0.0
        ft["parent_row"].fill_(-1)
        ft["live"].fill_(1)
        ft["best_len"].fill_(-1)
        ft["best_value"].fill_(float("-inf"))
        return
    x = _frontier_rows(ft, W, K, evaluation, swap)
    # the order of the expandable rows
    score = x.value if float(prior_weight) == 0.0 else x.value + float(prior_weight) * torch.where(x.expandable, x.cum, torch.zeros_like(x.cum))
    score = torch.where(x.expandable & ~torch.isnan(score), score, x.ninf) + 0.0  # + 0.0: -0.0 and +0.0 are one key to any sort
    by_score = torch.sort(score, dim=1, descending=True, stable=True).indices
    behind = (~x.expandable).gather(1, by_score).to(torch.int8)
    order = by_score.gather(1, torch.sort(behind, dim=1, stable=True).indices)  # the expandable rows first, each part in the order it had
    n = x.expandable.sum(dim=1).clamp(max=W)
    _frontier_children(ft, x, order[:, :W], n)


@dataclass
class FrontierSearch:
    """What `frontier_search` and `frontier_search_device` return.  P roots, F = width * max_children rows per root."""
    best_path: torch.Tensor   # [T, P, 3] int32: the path of the best finished placement (rows >= best_len: don't care)
    best_len: torch.Tensor    # [P] int32: its length, -1 if no row of the root finished
    best_value: torch.Tensor  # [P] float64: its value, -inf if none
    action: torch.Tensor      # [P, 3] int32: best_path[0], zero where best_len < 1
    live: torch.Tensor        # [P] int32: the rows of the final frontier
    errors: torch.Tensor      # 0-dim int32: bit 1 = a path_len outside [-1, T] was read
    paths: torch.Tensor       # [T, P * F, 3] int32: the final frontier, as the last ADVANCE wrote it
    path_len: torch.Tensor    # [P * F] int32, -1 = no row
    cum_logp: torch.Tensor    # [P * F] float64
    parent_row: torch.Tensor  # [P * F] int32: the slot of a row's parent in the frontier before, -1 = no row


def _frontier_arguments(root, evaluate, width, max_children, prior_weight, max_steps, depth):
    from .batched_env import default_max_steps
    P, W, K = int(root.num_envs), int(width), int(max_children)
    if W < 1 or W > MAX_FRONTIER_WIDTH or K < 1 or K > MAX_FRONTIER_CANDIDATES or W * K > MAX_FRONTIER_ROWS:
        raise ValueError(f"a frontier search needs width and max_children in [1, 64] and their product at most {MAX_FRONTIER_ROWS}")
    if P * W * K > 2 ** 31 - 1:
        raise ValueError("a frontier search needs num_envs * width * max_children <= 2^31 - 1")
    if not callable(evaluate):
        raise ValueError("evaluate must be callable: (paths, path_len, step_index0) -> Evaluation")
    pw = float(prior_weight)
    if pw != pw or pw in (float("inf"), float("-inf")):
        raise ValueError("prior_weight must be finite")
    T = default_max_steps(root.cfg) if max_steps is None else int(max_steps)
    D = T + 1 if depth is None else int(depth)
    if T < 1 or D < 1 or D > T + 1:
        raise ValueError("a frontier search needs max_steps >= 1 and depth in [1, max_steps + 1]")
    return P, W, K, pw, T, D


def frontier_result(ft: dict, last: int) -> FrontierSearch:
    """The tensors of a frontier search in the form the searches report; `last`: the set the last ADVANCE wrote."""
    best_path, best_len = ft["best_path"], ft["best_len"]
    action = torch.where((best_len >= 1)[:, None], best_path[0], torch.zeros_like(best_path[0]))
    return FrontierSearch(best_path, best_len, ft["best_value"], action, ft["live"], ft["errors_dev"][0], ft[f"paths_{last}"], ft[f"path_len_{last}"],
                          ft[f"cum_logp_{last}"], ft["parent_row"])


def frontier_search(root, evaluate, width: int, max_children: int, step_index: int, prior_weight: float = 0.0, max_steps=None,
                    depth=None) -> FrontierSearch:
    """A beam search over placements for all P = root.num_envs roots in lock-step, on the specification `frontier_advance`:
    tensor code for any device, one `evaluate` per depth and no host synchronisation.  Per root a frontier of at most W =
    width partial placements is kept; INIT makes it the root alone, and depth d = 0, 1, ... is
      evaluate   evaluate(paths, path_len, step_index + d * max_steps) -> `Evaluation` of the P * W * K rows of the frontier's
                 children (K = max_children; path_len -1: no row, what comes back for it is not looked at);
      advance    `frontier_advance`: the finished rows compete for best_path, the W best of the others by value +
                 prior_weight * cum_logp are kept, and each gives its k <= K candidates as the next rows.
    depth: the number of depths, default and at most max_steps + 1 (then every row has finished or was dropped).
    max_steps: the most transitions of an episode (default: that of root.cfg).  With prior_weight = 0 the search orders
    by the evaluator's value alone -- a network's value head, or a uniform rollout from the node -- and with a constant
    value and prior_weight = 1 by the cumulative log-prior.  `network_evaluator(..., leaves=W * K)` is such an `evaluate`."""
    P, W, K, pw, T, D = _frontier_arguments(root, evaluate, width, max_children, prior_weight, max_steps, depth)
    ft = new_frontier_tensors(P, W, K, T, getattr(root, "device", "cpu"))
    frontier_advance(ft, FRONTIER_INIT, W, K, pw, swap=True)  # writes set 0
    for d in range(D):
        cur = d % 2
        ev = evaluate(ft[f"paths_{cur}"], ft[f"path_len_{cur}"], int(step_index) + d * T)
        frontier_advance(ft, FRONTIER_ADVANCE, W, K, pw, ev, swap=cur == 1)
    return frontier_result(ft, D % 2)


def frontier_search_device(root, evaluate, width: int, max_children: int, step_index: int, prior_weight: float = 0.0, max_steps=None,
                           depth=None) -> FrontierSearch:
    """`frontier_search` with the frontier step on the device: a depth is `evaluate` and one kernel launch,
    `root.frontier_advance` (pcbenv_frontier_advance, include/pcbenv_frontier.h), with no tensor operation between them.
    The same search as `frontier_search` with the same arguments, field by field, floats by their bits: the score is two
    IEEE operations and the logarithm is `ieee_ln` on either side.  The evaluation's tensors must be on the root's device,
    contiguous, of the dtypes `Evaluation` names (`terminal` may be bool)."""
    P, W, K, pw, T, D = _frontier_arguments(root, evaluate, width, max_children, prior_weight, max_steps, depth)
    ft = new_frontier_tensors(P, W, K, T, root.device)
    req = root.frontier_request(ft, W, K, pw)
    root.frontier_advance(req, FRONTIER_INIT, swap=True)  # writes set 0
    for d in range(D):
        cur = d % 2
        ev = evaluate(ft[f"paths_{cur}"], ft[f"path_len_{cur}"], int(step_index) + d * T)
        root.frontier_advance(req, FRONTIER_ADVANCE, ev, swap=cur == 1)
    return frontier_result(ft, D % 2)


# ---- the stochastic frontier: sampling placements without replacement ------------------------------------------------
FRONTIER_ERR_SET = 4          # bit 2 of the error word: a set_len outside [-1, T]
FRONTIER_SAMPLE_DRAWS = 256   # csrc/pcb_frontier_sample.h:GUMBEL_DRAWS: draw 256 + i of child c is the Gumbel of child c of the parent in slot i
FRONTIER_SAMPLE_SET = ("set_len", "set_gumbel", "set_logp", "set_value", "set_path")


def new_frontier_sample_tensors(P: int, W: int, K: int, T: int, device) -> dict:
    """The tensors of `new_frontier_tensors` and what `BatchedPlacementEnv.frontier_sample_request` takes beside them:
    `gumbel_s` float64 [P * W * K], s = 0, 1, the third member of the two sets of rows, and the sample set of W slots per
    root, `set_len` [P * W], `set_gumbel`, `set_logp`, `set_value` float64 [P * W] and `set_path` [T, P * W, 3]."""
    i32, f64 = dict(dtype=torch.int32, device=device), dict(dtype=torch.float64, device=device)
    R, S = int(P) * int(W) * int(K), int(P) * int(W)
    ft = new_frontier_tensors(P, W, K, T, device)
    ft.update(gumbel_0=torch.zeros(R, **f64), gumbel_1=torch.zeros(R, **f64), set_len=torch.empty(S, **i32), set_gumbel=torch.zeros(S, **f64),
              set_logp=torch.zeros(S, **f64), set_value=torch.zeros(S, **f64), set_path=torch.zeros((T, S, 3), **i32))
    return ft


def _is_finite(x: torch.Tensor) -> torch.Tensor:
    return (x - x) == 0.0


def truncated_gumbel(G_S: torch.Tensor, phi: torch.Tensor, G_c: torch.Tensor, Z: torch.Tensor) -> torch.Tensor:
    """csrc/pcb_frontier_sample.h:child_gumbel, the same operations: the perturbed log-probability of a child with
    log-probability phi and G_c = phi + g_c, given its parent's G_S and Z, the largest G_c among its siblings."""
    zero, one = torch.zeros_like(G_c), torch.ones_like(G_c)
    ok = _is_finite(phi) & _is_finite(G_S)
    gs, gc = torch.where(ok, G_S, zero), torch.where(ok, G_c, zero)
    a = torch.where(ok, G_c - Z, zero)
    d = 1.0 - ieee_exp(a)
    same = (a == 0.0) | (d <= 0.0)
    v = (gs - gc) + ieee_ln(torch.where(same, one, d))
    top, mag = torch.where(v > 0.0, v, zero), torch.where(v < 0.0, -v, v)
    out = (gs - top) - ieee_ln(1.0 + ieee_exp(-mag))
    ninf = torch.full_like(G_c, float("-inf"))
    return torch.where(_is_finite(phi), torch.where(_is_finite(G_S) & ~same, out, G_S), ninf)


def _ranked(mask: torch.Tensor, values: torch.Tensor):
    """Along dim 1: the `values` where `mask` holds, moved to the front in their order -> (those, how many)."""
    P, W = mask.shape
    rank = mask.to(torch.int64).cumsum(dim=1) - 1
    front = torch.zeros((P, W + 1), dtype=values.dtype, device=values.device)
    front.scatter_(1, torch.where(mask, rank, W), values)
    return front[:, :W], mask.sum(dim=1)


def frontier_sample_advance(ft: dict, phases: int, width: int, num_candidates: int, seed: int, step_index: int, first_root: int = 0,
                            evaluation=None, swap: bool = False) -> None:
    """One depth of a stochastic beam search over placements (Kool, van Hoof and Welling, ICML 2019), in tensor code for any
    device and without a host synchronisation: the specification of pcbenv_frontier_sample
    (include/pcbenv_frontier_sample.h), on the tensors of `new_frontier_sample_tensors`, in place; swap as in
    `frontier_advance`.
    FRONTIER_INIT is `frontier_advance`'s, and gumbel of slot 0 = 0.0 and set_len = -1 everywhere.
    FRONTIER_ADVANCE: the live rows and the best finished row as in `frontier_advance`.  Then
      the contenders   set slots with set_len in [0, T] (outside [-1, T]: bit 2 of `errors_dev`), id j, key set_gumbel; live
                       rows that are finished or expandable, id W + i, key gumbel; a NaN key counts as -inf.
      the winners      the first min(W, contenders) by key descending, ties -- -0.0 with +0.0 among them -- to the lower id.
                       A set entry that did not win gets set_len -1.  The m-th finished winner goes into the m-th lowest
                       slot without a surviving entry: set_len, set_gumbel = its key, set_logp = its cum_logp, set_value =
                       its value, set_path = its path.  The expandable winners are the kept rows, in rank order.
      the children     as in `frontier_advance`, and gumbel = `truncated_gumbel` of the parent's key, the child's cum_logp
                       phi, phi + g with g = -ln(-ln u), u draw number 256 + the parent's slot of child c under (seed,
                       first_root + p, step_index), and Z, the largest phi + g over the parent's children with finite phi."""
    W, K, ph = int(width), int(num_candidates), int(phases)
    if ph not in (FRONTIER_INIT, FRONTIER_ADVANCE):
        raise ValueError("phases must be FRONTIER_INIT or FRONTIER_ADVANCE")
    if W < 1 or W > MAX_FRONTIER_WIDTH or K < 1 or K > MAX_FRONTIER_CANDIDATES or W * K > MAX_FRONTIER_ROWS:
        raise ValueError(f"width and num_candidates must be in [1, 64] and their product at most {MAX_FRONTIER_ROWS}, got {W} and {K}")
    F = W * K
    T, P = int(ft["best_path"].shape[0]), int(ft["best_path"].shape[1])
    if P == 0:
        return
    a, b = (1, 0) if swap else (0, 1)
    gum_in, gum_out = ft[f"gumbel_{a}"].view(P, F), ft[f"gumbel_{b}"].view(P, F)
    if ph == FRONTIER_INIT:
        frontier_advance(ft, FRONTIER_INIT, W, K, swap=swap)
        gum_out[:, 0] = 0.0
        ft["set_len"].fill_(-1)
        return
    x = _frontier_rows(ft, W, K, evaluation, swap)
    dev, ninf, length = x.dev, x.ninf, x.length
    # the contenders
    set_len = ft["set_len"].view(P, W).to(torch.int64)
    entry = (set_len >= 0) & (set_len <= T)
    if ft.get("errors_dev") is not None:
        ft["errors_dev"] |= (((set_len < -1) | (set_len > T)).any().to(torch.int32) * FRONTIER_ERR_SET)
    set_gumbel = ft["set_gumbel"].view(P, W)
    key_set = torch.where(entry & ~torch.isnan(set_gumbel), set_gumbel, ninf)
    contender = x.fin | x.expandable
    key_row = torch.where(contender & ~torch.isnan(gum_in), gum_in, ninf)
    key = torch.cat([key_set, key_row], dim=1) + 0.0  # + 0.0: -0.0 and +0.0 are one key to any sort
    valid = torch.cat([entry, contender], dim=1)
    by_key = torch.sort(key, dim=1, descending=True, stable=True).indices
    behind = (~valid).gather(1, by_key).to(torch.int8)
    order = by_key.gather(1, torch.sort(behind, dim=1, stable=True).indices)  # the contenders first, each part in the order it had
    # the winners
    won = order[:, :W]
    is_winner = torch.arange(W, dtype=torch.int64, device=dev)[None, :] < valid.sum(dim=1).clamp(max=W)[:, None]
    from_set = is_winner & (won < W)
    row = (won - W).clamp(min=0)
    finished = is_winner & ~from_set & x.fin.gather(1, row)
    survivor = torch.zeros((P, W + 1), dtype=torch.bool, device=dev)
    survivor.scatter_(1, torch.where(from_set, won, W), torch.ones_like(from_set))
    survivor = survivor[:, :W]
    entered, count = _ranked(finished, row)
    vacant = ~survivor
    rank = vacant.to(torch.int64).cumsum(dim=1) - 1
    takes = vacant & (rank < count[:, None])
    src = entered.gather(1, rank.clamp(min=0))                                                        # [P, W]
    src_len = length.gather(1, src)
    ft["set_len"].view(P, W).copy_(torch.where(takes, src_len, torch.where(entry & ~survivor, -1, set_len)))
    set_gumbel.copy_(torch.where(takes, key_row.gather(1, src), set_gumbel))
    ft["set_logp"].view(P, W).copy_(torch.where(takes, x.cum.gather(1, src), ft["set_logp"].view(P, W)))
    ft["set_value"].view(P, W).copy_(torch.where(takes, x.value.gather(1, src), ft["set_value"].view(P, W)))
    set_path = ft["set_path"].view(T, P, W, 3)
    moved = x.pin.gather(2, src[None, :, :, None].expand(T, P, W, 3))
    set_path.copy_(torch.where((takes[None] & (x.step[:, None, None] < src_len[None]))[..., None], moved, set_path))
    # the children
    kept, n = _ranked(is_winner & ~from_set & ~finished, row)
    child, parent, c = _frontier_children(ft, x, kept, n)
    phi = x.cum_out.view(P, F)
    genv = int(first_root) + torch.arange(P, dtype=torch.int64, device=dev)
    base = noise_base(int(seed), genv, int(step_index))[:, None]
    word = _mix64(base + (64 * (FRONTIER_SAMPLE_DRAWS + parent) + c[None, :] + 1) * _i64(_GOLDEN))
    u = (_shr(word, 12).to(torch.float64) + 0.5) * (1.0 / 4503599627370496.0)
    G_c = phi + -ieee_ln(-ieee_ln(u))
    counts = child & _is_finite(phi)
    Z = torch.where(counts, G_c, ninf).view(P, W, K).max(dim=2, keepdim=True).values.expand(P, W, K).reshape(P, F)
    G = truncated_gumbel(key_row.gather(1, parent), torch.where(child, phi, ninf), G_c, Z)
    gum_out.copy_(torch.where(child, G, gum_out))


@dataclass
class FrontierSampleSearch:
    """What `frontier_sample_search` and `frontier_sample_search_device` return.  P roots, W = width slots per root, slot
    p * W + j; the entries of a root in descending `set_gumbel` are its sample, in the order they were drawn."""
    best_path: torch.Tensor   # [T, P, 3] int32: the path of the finished placement with the largest value (rows >= best_len: don't care)
    best_len: torch.Tensor    # [P] int32: its length, -1 if no row of the root finished
    best_value: torch.Tensor  # [P] float64: its value, -inf if none
    action: torch.Tensor      # [P, 3] int32: best_path[0], zero where best_len < 1
    live: torch.Tensor        # [P] int32: the rows of the final frontier (0: the set is complete)
    errors: torch.Tensor      # 0-dim int32: bit 1 = a path_len, bit 2 = a set_len out of range was read
    set_len: torch.Tensor     # [P * W] int32: the length of the placement in a slot, -1 = free
    set_gumbel: torch.Tensor  # [P * W] float64: its perturbed log-probability
    set_logp: torch.Tensor    # [P * W] float64: its log-probability under the policy restricted to the candidates
    set_value: torch.Tensor   # [P * W] float64: its value
    set_path: torch.Tensor    # [T, P * W, 3] int32: its path (rows >= set_len: don't care)


def frontier_sample_result(ft: dict) -> FrontierSampleSearch:
    """The tensors of a stochastic frontier search in the form the searches report."""
    r = frontier_result(ft, 0)
    return FrontierSampleSearch(r.best_path, r.best_len, r.best_value, r.action, r.live, r.errors, *(ft[n] for n in FRONTIER_SAMPLE_SET))


def frontier_sample_search(root, evaluate, width: int, max_children: int, step_index: int, seed: int, first_root: int = 0, max_steps=None,
                           depth=None) -> FrontierSampleSearch:
    """A stochastic beam search over placements for all P = root.num_envs roots in lock-step, on the specification
    `frontier_sample_advance`: `frontier_search` with the rows ordered by Gumbel-perturbed log-probabilities, which returns
    W = width complete placements per root sampled without replacement from the policy `evaluate` gives (its K =
    max_children candidates per node), each with its value and its log-probability, next to the best of them by value.
    Depth d is `evaluate(paths, path_len, step_index + d * max_steps)` and one step with that step index; the draws depend
    on (seed, first_root + p, step index) alone.  depth: the number of depths, default and at most max_steps + 1 (then
    live == 0 and the set is complete)."""
    P, W, K, _, T, D = _frontier_arguments(root, evaluate, width, max_children, 0.0, max_steps, depth)
    ft = new_frontier_sample_tensors(P, W, K, T, getattr(root, "device", "cpu"))
    frontier_sample_advance(ft, FRONTIER_INIT, W, K, seed, int(step_index), first_root, swap=True)  # writes set 0
    for d in range(D):
        cur = d % 2
        ev = evaluate(ft[f"paths_{cur}"], ft[f"path_len_{cur}"], int(step_index) + d * T)
        frontier_sample_advance(ft, FRONTIER_ADVANCE, W, K, seed, int(step_index) + d * T, first_root, ev, swap=cur == 1)
    return frontier_sample_result(ft)


def frontier_sample_search_device(root, evaluate, width: int, max_children: int, step_index: int, seed: int, first_root: int = 0, max_steps=None,
                                  depth=None) -> FrontierSampleSearch:
    """`frontier_sample_search` with the frontier step on the device: a depth is `evaluate` and one kernel launch,
    `root.frontier_sample` (pcbenv_frontier_sample, include/pcbenv_frontier_sample.h), with no tensor operation between
    them.  The same search as `frontier_sample_search` with the same arguments, field by field, floats by their bits."""
    P, W, K, _, T, D = _frontier_arguments(root, evaluate, width, max_children, 0.0, max_steps, depth)
    ft = new_frontier_sample_tensors(P, W, K, T, root.device)
    req = root.frontier_sample_request(ft, W, K, seed, first_root)
    root.frontier_sample(req, FRONTIER_INIT, int(step_index), swap=True)  # writes set 0
    for d in range(D):
        cur = d % 2
        ev = evaluate(ft[f"paths_{cur}"], ft[f"path_len_{cur}"], int(step_index) + d * T)
        root.frontier_sample(req, FRONTIER_ADVANCE, int(step_index) + d * T, ev, swap=cur == 1)
    return frontier_sample_result(ft)
