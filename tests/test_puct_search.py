"""pcbenv.search.puct_search on the CPU: an evaluator stub over the toy game of tests/test_tree_search.py, a function of the
path alone (and of the root, for the scale of the values).

The game: an action is (0, 0, b), b in {0, 1}; an episode has three transitions, except that b0 = b1 = 1 ends it at the
second.  A finished episode is worth REWARD[b0, b1, b2] (REWARD[1, 1, 0] for the short one), an unfinished one VALUE[path];
the policy gives b = 0 and b = 1 the probabilities PRIOR[path], except at the path (0, 1), where it gives no candidate at
all although the episode goes on.  Values are scaled per root; root 3 is over before its first transition.  Every tree
below can be worked out by hand, and is: EXPECT_ROOT0 was filled in on paper, and `reference` is the same search written
as a plain loop over dicts, for the roots and iteration counts not done on paper.

Also `top_priors` on hand-made logits and masks, and `network_evaluator` against a stand-in planner."""
import math
from types import SimpleNamespace

import pytest
import torch

from pcbenv.search import Evaluation, network_evaluator, puct_search, top_priors

T = 3
REWARD = [[[0.10, 0.90], [0.50, 0.50]], [[0.30, 0.20], [0.70, 0.70]]]
VALUE = {(): 0.4, (0,): 0.6, (1,): 0.3, (0, 0): 0.5, (0, 1): 0.5, (1, 0): 0.25}
PRIOR = {(): (0.25, 0.75), (0,): (0.75, 0.25), (1,): (0.5, 0.5), (0, 0): (0.25, 0.75), (0, 1): None, (1, 0): (0.5, 0.5)}  # of b = 0, b = 1
SCALE = (1.0, -1.0, 4.0, 1.0)  # root 1 prefers what root 0 avoids; root 2 is root 0 on another scale (the normalisation); root 3 is terminal
CASES = [(5, 1.0, 2, 2), (24, 1.0, 2, 2), (24, 0.3, 2, 2), (16, 1.0, 1, 2), (12, 2.0, 3, 1), (24, 1.5, 3, 2)]  # iterations, c_puct, C, K


def node_of(p, path, K):
    """-> (value, terminal, [(b, prior), ...] at most K candidates, the more probable first, b = 0 first on ties)."""
    path = tuple(path)
    if p == 3:
        return 0.125, True, []
    if len(path) == 3 or path[:2] == (1, 1):
        b = path + (0,)
        return REWARD[b[0]][b[1]][b[2]] * SCALE[p], True, []
    pri = PRIOR[path]
    cands = [] if pri is None else sorted(((0, pri[0]), (1, pri[1])), key=lambda c: -c[1])[:K]
    return VALUE[path] * SCALE[p], False, cands


def evaluator_for(P, K, calls=None):
    def evaluate(paths, path_len, step_index0):
        assert paths.shape == (T, P, 3) and paths.dtype == torch.int32 and path_len.shape == (P,) and path_len.dtype == torch.int32
        if calls is not None:
            calls.append((paths.clone(), path_len.clone(), step_index0))
        value, over, count = torch.zeros(P, dtype=torch.float64), torch.zeros(P, dtype=torch.uint8), torch.zeros(P, dtype=torch.int32)
        actions, prior = torch.zeros((P, K, 3), dtype=torch.int32), torch.zeros((P, K), dtype=torch.float32)
        for p in range(P):
            v, t, cands = node_of(p, [int(paths[d, p, 2]) for d in range(int(path_len[p]))], K)
            value[p], over[p], count[p] = v, int(t), len(cands)
            for c, (b, pr) in enumerate(cands):
                actions[p, c, 2], prior[p, c] = b, pr
        return Evaluation(value, over, count, actions, prior)
    return evaluate


def reference(p, iterations, c_puct, max_children, K):
    """The same search as a plain loop, one root."""
    nodes = [dict(parent=-1, depth=0, b=0, prior=0.0, visits=0, vsum=0.0, vmax=-math.inf, terminal=False, children=[])]
    lo, hi = math.inf, -math.inf
    for m in range(iterations):
        n, d = 0, 0
        while d < T and not nodes[n]["terminal"] and nodes[n]["children"]:
            def score(c):
                k = nodes[c]
                q = (k["vsum"] / k["visits"] - lo) / (hi - lo) if k["visits"] > 0 and hi > lo else 0.0
                return q + c_puct * k["prior"] * math.sqrt(max(nodes[n]["visits"], 1)) / (1.0 + k["visits"])
            scores = [score(c) for c in nodes[n]["children"]]
            n, d = nodes[n]["children"][scores.index(max(scores))], d + 1  # the first maximum
        path, k = [], n
        while k > 0:
            path.insert(0, nodes[k]["b"]); k = nodes[k]["parent"]
        assert len(path) == d
        v, term, cands = node_of(p, path, K)
        if term:
            nodes[n]["terminal"] = True
        elif not nodes[n]["children"] and not nodes[n]["terminal"]:
            for b, pr in cands[:max_children]:
                nodes.append(dict(parent=n, depth=d + 1, b=b, prior=pr, visits=0, vsum=0.0, vmax=-math.inf, terminal=False, children=[]))
                nodes[n]["children"].append(len(nodes) - 1)
        lo, hi = min(lo, v), max(hi, v)
        k = n
        while k >= 0:
            nodes[k]["visits"] += 1; nodes[k]["vsum"] += v; nodes[k]["vmax"] = max(nodes[k]["vmax"], v); k = nodes[k]["parent"]
    return nodes, lo, hi


def run(P, iterations, c_puct=1.0, max_children=2, K=2, **kw):
    root = SimpleNamespace(num_envs=P, device="cpu")
    return puct_search(root, iterations, 0, evaluator_for(P, K, **kw), c_puct=c_puct, max_children=max_children, max_steps=T)


# Root 0, c_puct = 1, max_children = 2, K = 2, worked out on paper:
#  m=0  the root has no child: it is evaluated, 0.4, and gets slots 1 = (b=1, prior 0.75) and 2 = (b=0, 0.25): the more probable
#       first.  lo = hi = 0.4
#  m=1  n(root) = 1, no child visited: score = prior * sqrt(1) / 1; the prior decides: slot 1.  Path [1] is worth 0.3; slots 3 =
#       (b=0, 0.5) and 4 = (b=1, 0.5) under slot 1.  lo = 0.3
#  m=2  n(root) = 2.  Slot 1: q = (0.3 - 0.3) / 0.1 = 0, u = 0.75 * sqrt(2) / 2 = 0.530; slot 2: u = 0.25 * sqrt(2) = 0.354: slot 1.
#       There n = 1 and slots 3 and 4 score 0.5 * 1 / 1 each: the tie goes to slot 3.  Path [1, 0] is worth 0.25; slots 5, 6
#       under slot 3.  lo = 0.25
#  m=3  n(root) = 3.  Slot 1: mean 0.275, q = 0.025 / 0.15 = 0.167, u = 0.75 * sqrt(3) / 3 = 0.433; slot 2: u = 0.25 * sqrt(3) =
#       0.433, q = 0: slot 1.  There n = 2: slot 3: q = 0, u = 0.5 * sqrt(2) / 2 = 0.354; slot 4: u = 0.5 * sqrt(2) = 0.707: slot
#       4.  Path [1, 1] ends the episode: 0.7, slot 4 is terminal.  hi = 0.7
#  m=4  n(root) = 4.  Slot 1: mean 1.25 / 3, q = (0.41667 - 0.25) / 0.45 = 0.370, u = 0.75 * 2 / 4 = 0.375; slot 2: u = 0.25 * 2 =
#       0.5: slot 1.  There n = 3: slot 3: q = 0, u = 0.5 * sqrt(3) / 2 = 0.433; slot 4: q = 1, u = 0.433: slot 4, terminal:
#       the descent stops, the node is evaluated again, 0.7, and not expanded
EXPECT_ROOT0 = dict(
    parent=[-1, 0, 0, 1, 1, 3, 3], depth=[0, 1, 1, 2, 2, 3, 3], b=[0, 1, 0, 0, 1, 0, 1], prior=[0.0, 0.75, 0.25, 0.5, 0.5, 0.5, 0.5],
    visits=[5, 4, 0, 1, 2, 0, 0], num_children=[2, 2, 0, 2, 0, 0, 0], first_child=[1, 3, -1, 5, -1, -1, -1],
    value_sum=[0.4 + 0.3 + 0.25 + 0.7 + 0.7, 0.3 + 0.25 + 0.7 + 0.7, 0.0, 0.25, 0.7 + 0.7, 0.0, 0.0],
    value_max=[0.7, 0.7, -math.inf, 0.25, 0.7, -math.inf, -math.inf], terminal=[False, False, False, False, True, False, False])


def test_five_iterations_by_hand():
    calls = []
    ps = run(1, 5, calls=calls)
    e = EXPECT_ROOT0
    n = len(e["parent"])
    assert ps.num_nodes.tolist() == [n] and ps.parent.shape == (1, 1 + 5 * 2)
    for f in ("parent", "depth", "visits", "num_children", "first_child", "prior", "value_sum", "value_max", "terminal"):
        assert getattr(ps, f)[0, :n].tolist() == e[f], f  # the sums in the order the values arrived: bit for bit
    assert ps.node_action[0, :n, 2].tolist() == e["b"] and not ps.node_action[0, :, :2].any()
    assert (ps.parent[0, n:] == -1).all() and (ps.first_child[0, n:] == -1).all() and not ps.visits[0, n:].any()
    assert [c[1].tolist() for c in calls] == [[0], [1], [2], [2], [2]]  # the prior decided m=1, the tie of m=2 went to slot 3, m=4 revisits the terminal leaf
    assert [c[0][:int(c[1][0]), 0, 2].tolist() for c in calls] == [[], [1], [1, 0], [1, 1], [1, 1]]
    assert [c[2] for c in calls] == [m * T for m in range(5)]  # step_index0 = step_index + m * max_steps
    assert ps.child_visits.tolist() == [[4, 0]] and ps.child_actions[0, :, 2].tolist() == [1, 0] and ps.child_priors.tolist() == [[0.75, 0.25]]
    assert ps.action.tolist() == [[0, 0, 1]] and ps.root_value.tolist() == [(0.4 + 0.3 + 0.25 + 0.7 + 0.7) / 5]
    assert ps.reward_lo.tolist() == [0.25] and ps.reward_hi.tolist() == [0.7] and int(ps.errors) == 0


def check_against_reference(ps, P, iterations, c_puct, max_children, K):
    for p in range(P):
        nodes, lo, hi = reference(p, iterations, c_puct, max_children, K)
        n = len(nodes)
        assert int(ps.num_nodes[p]) == n
        assert ps.parent[p, :n].tolist() == [k["parent"] for k in nodes] and (ps.parent[p, n:] == -1).all()
        assert ps.depth[p, :n].tolist() == [k["depth"] for k in nodes]
        assert ps.node_action[p, :n, 2].tolist() == [k["b"] for k in nodes]
        assert ps.prior[p, :n].tolist() == [k["prior"] for k in nodes]
        assert ps.visits[p, :n].tolist() == [k["visits"] for k in nodes] and not ps.visits[p, n:].any()
        assert ps.value_sum[p, :n].tolist() == [k["vsum"] for k in nodes]
        assert ps.value_max[p, :n].tolist() == [k["vmax"] for k in nodes]
        assert ps.terminal[p, :n].tolist() == [k["terminal"] for k in nodes]
        assert ps.num_children[p, :n].tolist() == [len(k["children"]) for k in nodes]
        assert ps.first_child[p, :n].tolist() == [k["children"][0] if k["children"] else -1 for k in nodes]
        for k in nodes:
            assert k["children"] == list(range(k["children"][0], k["children"][0] + len(k["children"]))) if k["children"] else True
            assert len(k["children"]) <= min(max_children, K) and not (k["terminal"] and k["children"]), "a terminal node was expanded"
        assert float(ps.reward_lo[p]) == lo and float(ps.reward_hi[p]) == hi
        visits = [nodes[c]["visits"] for c in nodes[0]["children"]]
        assert ps.child_visits[p, :len(visits)].tolist() == visits and not ps.child_visits[p, len(visits):].any()
        if visits:
            assert int(ps.action[p, 2]) == nodes[nodes[0]["children"][visits.index(max(visits))]]["b"]
        assert float(ps.root_value[p]) == nodes[0]["vsum"] / nodes[0]["visits"]
    assert int(ps.errors) == 0


@pytest.mark.parametrize("iterations, c_puct, max_children, K", CASES)
def test_four_roots_in_lock_step(iterations, c_puct, max_children, K):
    """Roots on different reward scales descend differently in one batch.  max_children = 1 < K = 2 truncates the candidates to
    the most probable one and makes the tree a chain; K = 1 < max_children = 3 gives one child however many are allowed."""
    calls = []
    ps = run(4, iterations, c_puct, max_children, K, calls=calls)
    check_against_reference(ps, 4, iterations, c_puct, max_children, K)
    assert [c[2] for c in calls] == [m * T for m in range(iterations)]
    assert int(ps.num_children.max()) == min(max_children, K, 2)
    # the terminal root: never expanded, evaluated every time
    assert ps.num_nodes[3] == 1 and ps.terminal[3, 0] and ps.visits[3, 0] == iterations and ps.action[3].tolist() == [0, 0, 0]
    if iterations >= 12:
        assert (ps.terminal[:3, 1:] & (ps.visits[:3, 1:] > 1)).any(), "no terminal leaf was visited twice"
    if min(max_children, K) == 1:
        assert (ps.num_children[:3] <= 1).all() and int(ps.num_nodes[:3].max()) <= T + 1
        assert ps.node_action[0, 1, 2] == 1 and ps.prior[0, 1] == 0.75  # the one kept is the most probable


def test_a_live_node_without_candidates_is_evaluated_again_and_never_expanded():
    """The path (0, 1) goes on but the policy names no candidate there: cand_count == 0.  With c_puct = 2 the search of root 0
    comes back to it."""
    ps = run(1, 40, 2.0, 2, 2)
    p = 0
    slot = [s for s in range(int(ps.num_nodes[p])) if ps.depth[p, s] == 2 and ps.node_action[p, s, 2] == 1
            and ps.node_action[p, int(ps.parent[p, s]), 2] == 0]
    assert len(slot) == 1
    s = slot[0]
    assert ps.visits[p, s] > 1 and ps.num_children[p, s] == 0 and ps.first_child[p, s] == -1 and not ps.terminal[p, s]
    assert float(ps.value_sum[p, s]) == sum([0.5] * int(ps.visits[p, s]))


def test_ties_go_to_the_lowest_slot():
    """Equal values everywhere and equal priors: q is 0 for every child (hi == lo), equal visits tie, and the descent takes
    the lowest slot; the most-visited action of a tie is the lowest slot's too."""
    def evaluate(paths, path_len, s):
        over = (path_len == T).to(torch.uint8)
        acts = torch.zeros((1, 2, 3), dtype=torch.int32)
        acts[0, 1, 2] = 1
        return Evaluation(torch.full((1,), 0.25, dtype=torch.float64), over, torch.full((1,), 2, dtype=torch.int32), acts, torch.full((1, 2), 0.5))
    root = SimpleNamespace(num_envs=1, device="cpu")
    ps = puct_search(root, 3, 0, evaluate, max_children=2, max_steps=T)   # root, then slot 1 (tie), then slot 2 (0.5 * sqrt(2) / 2 < 0.5 * sqrt(2))
    assert ps.child_visits.tolist() == [[1, 1]] and ps.action.tolist() == [[0, 0, 0]]
    ps = puct_search(root, 4, 0, evaluate, max_children=2, max_steps=T)   # the tie between the two again: slot 1
    assert ps.child_visits.tolist() == [[2, 1]]


def test_capacity_all_or_nothing():
    ps = puct_search(SimpleNamespace(num_envs=4, device="cpu"), 12, 0, evaluator_for(4, 2), max_children=2, max_steps=T, capacity=4)
    assert ps.parent.shape == (4, 4) and int(ps.errors) == 1
    assert ps.num_nodes.tolist() == [3, 3, 3, 1]  # the root's two children fit, a third pair would need slots 3 and 4
    assert ps.visits[:, 0].tolist() == [12] * 4  # every evaluation was backed up all the same


def test_nothing_synchronises_inside_the_loop(monkeypatch):
    """No .item(), .cpu(), .tolist(), .numpy(), nonzero() or bool(tensor) while the search runs (each would be a host
    synchronisation on a device)."""
    fixed = []
    record = evaluator_for(3, 2)
    root = SimpleNamespace(num_envs=3, device="cpu")
    puct_search(root, 12, 0, lambda a, b, s: fixed.append(record(a, b, s)) or fixed[-1], max_children=2, max_steps=T)
    replayed = iter(fixed)  # the same search sees the same evaluations: the stub itself reads its arguments on the host

    def refuse(name):
        def f(*a, **k):
            raise AssertionError(f"puct_search called Tensor.{name}")
        return f
    for name in ("item", "cpu", "tolist", "numpy", "nonzero", "__bool__", "__int__", "__float__", "__index__"):
        monkeypatch.setattr(torch.Tensor, name, refuse(name))
    ps = puct_search(root, 12, 0, lambda a, b, s: next(replayed), max_children=2, max_steps=T)
    monkeypatch.undo()
    check_against_reference(ps, 3, 12, 1.0, 2, 2)


def test_arguments():
    root = SimpleNamespace(num_envs=2, device="cpu")
    for kw in (dict(iterations=0), dict(iterations=4, max_children=0), dict(iterations=4, max_children=65), dict(iterations=4, capacity=0)):
        with pytest.raises(ValueError):
            puct_search(root, kw.pop("iterations"), 0, evaluator_for(2, 2), max_steps=T, **kw)


# ---- top_priors ------------------------------------------------------------------------------------------------------
def test_top_priors_by_hand():
    """Two orientations on a 2 x 3 grid: A = 12, a = o * 6 + x * 3 + y."""
    ln = math.log
    logits = torch.zeros((4, 12))
    mask = torch.zeros((4, 2, 2, 3), dtype=torch.uint8)
    # row 0: legal 1, 4, 7, 10 with probabilities 0.5, 0.125, 0.25, 0.125: the tie of 4 and 10 in flat-index order; an illegal logit is huge
    for a, pr in ((1, 0.5), (4, 0.125), (7, 0.25), (10, 0.125)):
        mask.view(4, 12)[0, a], logits[0, a] = 1, ln(pr)
    logits[0, 0] = 1e30
    # row 1: every action legal, constant logits; row 2: two legal, fewer than K; row 3: none
    mask[1] = 1
    mask.view(4, 12)[2, 11], mask.view(4, 12)[2, 2] = 1, 1
    logits[2, 11] = 5.0
    count, actions, prior = top_priors(logits, mask, 3)
    assert count.dtype == torch.int32 and actions.dtype == torch.int32 and prior.dtype == torch.float32
    assert count.tolist() == [3, 3, 2, 0] and actions.shape == (4, 3, 3) and prior.shape == (4, 3)
    assert actions[0].tolist() == [[0, 0, 1], [1, 0, 1], [0, 1, 1]]          # 1, 7, 4 (before 10)
    assert torch.allclose(prior[0], torch.tensor([0.5, 0.25, 0.125]), rtol=1e-6, atol=0)
    assert actions[1].tolist() == [[0, 0, 0], [0, 0, 1], [0, 0, 2]] and prior[1].tolist() == [float(torch.tensor(1.0) / 12)] * 3
    assert actions[2].tolist() == [[1, 1, 2], [0, 0, 2], [0, 0, 0]] and prior[2, 2] == 0 and prior[2, 0] > 0.99 and prior[2, 1] > 0
    assert not actions[3].any() and not prior[3].any()
    count, actions, prior = top_priors(logits, mask, 16)  # more candidates asked for than there are actions
    assert count.tolist() == [4, 12, 2, 0] and actions.shape == (4, 16, 3) and not prior[:, 12:].any()
    assert actions[0, 3].tolist() == [1, 1, 1] and float(prior[1].sum()) == pytest.approx(1.0)
    c1, a1, p1 = top_priors(logits.to(torch.bfloat16)[1:2].reshape(1, 2, 2, 3), mask[1:2].bool(), 3)  # any dtype and shape of the same extent
    assert c1.tolist() == [3] and a1.tolist() == actions[1:2, :3].tolist() and p1.tolist() == prior[1:2, :3].tolist()
    one = top_priors(torch.zeros((1, 6)), torch.tensor([[[0, 1, 0], [0, 0, 1]]]), 2)  # [P, H, W]: one orientation
    assert one[0].tolist() == [2] and one[1].tolist() == [[[0, 0, 1], [0, 1, 2]]] and one[2].tolist() == [[0.5, 0.5]]


# ---- network_evaluator against a stand-in planner --------------------------------------------------------------------
class ToyPlanner:
    """The toy game as the planner network_evaluator drives: gather_ with paths, obs (with an action_mask [P, 1, 1, 2]),
    reward, done, gather_length."""

    def __init__(self, P):
        self.num_envs, self.device, self.auto_reset, self.run_seed, self.first_env_index = P, "cpu", False, 0, 0
        self.gathers = 0

    def gather_(self, index, source=None, check=False, paths=None, path_len=None):
        P = self.num_envs
        assert index.tolist() == list(range(P)) and index.dtype == torch.int32 and source is not None
        self.gathers += 1
        self.b = [[int(paths[t, i, 2]) for t in range(int(path_len[i]))] for i in range(P)]
        self.reward, self.done = torch.zeros(P, dtype=torch.float64), torch.zeros(P, dtype=torch.uint8)
        self.gather_length = torch.tensor([len(b) for b in self.b], dtype=torch.int32)
        for i, b in enumerate(self.b):
            v, over, _ = node_of(i, b, 2)
            if over:
                self.reward[i], self.done[i] = v, 1
        return self.obs

    @property
    def obs(self):
        mask = torch.ones((self.num_envs, 1, 1, 2), dtype=torch.uint8)
        for i, b in enumerate(self.b):
            if node_of(i, b, 2)[1] or PRIOR[tuple(b)] is None:
                mask[i] = 0
        return {"action_mask": mask, "path": self.b}


def test_network_evaluator_one_call_by_hand():
    """P = 3: the root, a path of one step, and a path that ends the short episode (b0 = b1 = 1)."""
    P = 3
    planner = ToyPlanner(P)
    rollouts = []

    def playout(k, step_index, paths, path_len, max_steps):
        rollouts.append((k, step_index, max_steps))
        return SimpleNamespace(reward=torch.tensor([9.0, 8.0, 7.0], dtype=torch.float64))
    root = SimpleNamespace(num_envs=P, device="cpu", run_seed=0, playout=playout)
    logits_fn = lambda obs: torch.log(torch.tensor([list(PRIOR.get(tuple(b)) or (0.5, 0.5)) for b in obs["path"]]))
    value_fn = lambda obs: torch.tensor([VALUE.get(tuple(b), 0.0) * SCALE[i] for i, b in enumerate(obs["path"])], dtype=torch.float32)
    paths = torch.zeros((T, P, 3), dtype=torch.int32)
    paths[0, 1, 2] = 1
    paths[0, 2, 2], paths[1, 2, 2] = 1, 1
    plen = torch.tensor([0, 1, 2], dtype=torch.int32)
    ev = network_evaluator(root, planner, logits_fn, value_fn, max_children=2)(paths, plen, 30)
    assert ev.terminal.tolist() == [0, 0, 1] and ev.terminal.dtype == torch.uint8 and ev.value.dtype == torch.float64
    assert ev.value.tolist() == [float(torch.tensor(0.4)), float(torch.tensor(-0.3)), 0.7 * 4.0]  # value_fn's float32, the reward where terminal
    assert ev.cand_count.tolist() == [2, 2, 0] and ev.cand_actions[:2, :, 2].tolist() == [[1, 0], [0, 1]] and not ev.cand_actions[2].any()
    assert torch.allclose(ev.cand_prior, torch.tensor([[0.75, 0.25], [0.5, 0.5], [0.0, 0.0]]), rtol=1e-6, atol=0)
    assert planner.gathers == 1 and not rollouts
    ev = network_evaluator(root, planner, logits_fn, max_children=1)(paths, plen, 30)  # no value_fn: a uniform rollout from the leaf
    assert ev.value.tolist() == [9.0, 8.0, 0.7 * 4.0] and rollouts == [(1, 30, T)]
    assert ev.cand_count.tolist() == [1, 1, 0] and ev.cand_actions.shape == (P, 1, 3) and ev.cand_actions[:, 0, 2].tolist() == [1, 0, 0]
    for bad in (SimpleNamespace(num_envs=P + 1, device="cpu", run_seed=0), SimpleNamespace(num_envs=P, device="cpu", run_seed=1)):
        with pytest.raises(ValueError):
            network_evaluator(bad, planner, logits_fn)


@pytest.mark.parametrize("iterations, max_children", [(12, 2), (9, 1)])
def test_network_evaluator_in_the_search(iterations, max_children):
    """puct_search(evaluate=network_evaluator(...)) on the stand-in grows the tree the stub's evaluations grow, given the
    same priors: the stub is handed network_evaluator's float32 softmax in place of its table."""
    P = 3
    planner = ToyPlanner(P)
    root = SimpleNamespace(num_envs=P, device="cpu", run_seed=0)
    logits_fn = lambda obs: torch.log(torch.tensor([list(PRIOR.get(tuple(b)) or (0.5, 0.5)) for b in obs["path"]]))
    value_fn = lambda obs: torch.tensor([node_of(i, b, 2)[0] for i, b in enumerate(obs["path"])], dtype=torch.float64)
    evaluate = network_evaluator(root, planner, logits_fn, value_fn, max_children=2)
    stub = evaluator_for(P, 2)

    def with_softmax_priors(paths, path_len, s):
        want, got = stub(paths, path_len, s), evaluate(paths, path_len, s)
        assert want.terminal.tolist() == got.terminal.tolist() and want.value.tolist() == got.value.tolist()
        assert want.cand_count.tolist() == got.cand_count.tolist() and torch.equal(want.cand_actions, got.cand_actions)
        assert torch.allclose(want.cand_prior, got.cand_prior, rtol=1e-6, atol=0)
        return got
    got = puct_search(root, iterations, 0, evaluate, max_children=max_children, max_steps=T)
    want = puct_search(root, iterations, 0, with_softmax_priors, max_children=max_children, max_steps=T)
    for f in want.__dataclass_fields__:
        a, b = getattr(got, f), getattr(want, f)
        assert a.dtype == b.dtype and torch.equal(a, b), f
    assert planner.gathers == 2 * iterations
