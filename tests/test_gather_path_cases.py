"""The plans of tests/gather_path_cases.py on the CPU oracle alone, and pcbenv.search.policy_backend on the toy game of
tests/test_tree_search.py.  No GPU.

The node a path names is stated twice -- gather_path_cases.oracle_node (a fresh oracle: the root's instance, its history,
the path up to the first done) and gather_path_cases.apply_paths on a HandleModel behind a gather (what the GPU tests
keep next to the destination handle) -- and both against what path_cases already knows of the same paths: the leaf mask,
and the outputs of a playout that ends on its path.  Every plan must hold every end the GPU tests need."""
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import gather_path_cases as gp
import path_cases as pa
from handle_model import HandleModel, _same_info
from pcbenv.search import policy_backend, tree_search

from test_tree_search import REWARD, SCALE, T, backend_for, drawn

_PLANS = {}


def plan(name, parity=0):
    if (name, parity) not in _PLANS:
        p = pa.Plan(name, parity)
        _PLANS[name, parity] = (p, gp.nodes_of(p))
    return _PLANS[name, parity]


@pytest.mark.parametrize("name, parity", [(n, 0) for n in gp.GPU_CASES] + [(n, 1) for n in gp.BOTH_PARITIES])
def test_every_plan_has_every_end(name, parity):
    p, nodes = plan(name, parity)
    figures, missing = gp.mix(p, nodes)
    print(f"GATHER-PATH-MIX {name} parity {parity}: {figures}")
    assert not missing, (missing, figures)
    assert figures["empty"] == p.P


@pytest.mark.parametrize("name", gp.GPU_CASES)
def test_the_node_is_what_the_path_playout_starts_from(name):
    """oracle_node against path_cases.oracle_path_playout: the same leaf mask; a playout that ended on its path reports
    the node's outputs; one that went on applied the whole path without a done."""
    p, nodes = plan(name)
    for i, (nd, e) in enumerate(zip(nodes, p.expected)):
        n = int(p.path_len[i])
        assert np.array_equal(nd["leaf"], e["leaf"]), i
        assert nd["length"] == min(n, e["length"]), i
        if n == 0:
            assert nd["reward"] is None and nd["done"] is None and nd["info"] is None
        elif e["length"] <= n:
            assert nd["done"] == e["done"] == 1 and nd["reward"].tobytes() == e["reward"].tobytes() and _same_info(nd["info"], e["info"]), i
            assert nd["placed_all"] == e["placed_all"], i
        else:
            assert nd["done"] == 0 and nd["length"] == n, i
            assert nd["reward"] == (1.0 if not gp.pc.has_info(p.cfg) else 0.0) and np.isnan(nd["info"]).all(), i


@pytest.mark.parametrize("name", ["small_spatial", "rect_4x4_full", "c1"])
def test_apply_paths_on_a_handle_model_gives_the_same_nodes(name):
    """A destination model of n rows: gather(child index, source = the roots' model), then apply_paths -- every row's
    observation, outputs and length are oracle_node's; rows refused or kept stay as they were."""
    p, nodes = plan(name)
    src = p.roots.model
    dst = HandleModel(p.cfg, p.n, 1, 3, False, p.roots.seed)
    dst.reset()
    idx = np.array(p.root_of, np.int64)
    idx[3], idx[7] = -1, p.P  # kept, out of range
    before = {i: dst.ob.env(i).obs() for i in (3, 7)}
    taken = dst.gather(idx, src)
    assert not taken[3] and not taken[7] and taken.sum() == p.n - 2
    root_rdi = (dst.R[0].copy(), dst.D[0].copy(), dst.I[0].copy())
    length = gp.apply_paths(dst, taken, p.path_tensor(fill=gp.NO_ACTION), p.path_len)
    for i, nd in enumerate(nodes):
        got = dst.ob.env(i).obs()
        if not taken[i]:
            assert length[i] == 0 and all(np.array_equal(got[k], before[i][k]) for k in got), i
            continue
        assert length[i] == nd["length"], i
        assert set(got) == set(nd["obs"]) and all(np.array_equal(got[k], nd["obs"][k]) for k in got), i
        if nd["length"] == 0:  # the source row's outputs, as the gather copied them
            r = p.root_of[i]
            assert dst.R[0, i] == src.R[0, r] == root_rdi[0][i] and dst.D[0, i] == src.D[0, r] and _same_info(dst.I[0, i], src.I[0, r]), i
        else:
            assert dst.R[0, i].tobytes() == nd["reward"].tobytes() and dst.D[0, i] == nd["done"] and _same_info(dst.I[0, i], nd["info"]), i
        assert len(dst.hist[i]) == len(src.hist[p.root_of[i]]) + nd["length"], i


def test_decode_flat_paths():
    cfg = pa.pc.case("rect_11x10")[0]()
    H, W, A = cfg.height, cfg.width, cfg.num_orientations * cfg.height * cfg.width
    flat = np.array([[0, W + 2, H * W + 5, A - 1], [-1, A, A + 77, 3]], np.int32)
    got = gp.decode_flat_paths(cfg, flat)
    assert got.shape == (2, 4, 3)
    assert got[0].tolist() == [[0, 0, 0], [0, 1, 2], [1, 0, 5], [cfg.num_orientations - 1, H - 1, W - 1]]
    assert (got[1, :3, 0] == -1).all() and got[1, 3].tolist() == [0, 0, 3]


# ---- policy_backend on the toy game of tests/test_tree_search.py ---------------------------------------------------
class ToyPlanner:
    """The game of tests/test_tree_search.py as the planner policy_backend drives: gather_ with paths, obs, sample_logits,
    step, reward, done, gather_length.  An action is (0, 0, b); (-1, -1, -1), or any action behind the episode's end, is
    invalid: done with the worst reward and the state unchanged, and no done latch."""
    WORST = -99.0

    def __init__(self, P):
        self.num_envs, self.device, self.auto_reset, self.run_seed, self.first_env_index = P, "cpu", False, 0, 0
        self.scale = torch.tensor(SCALE[:P], dtype=torch.float64)
        self.b = [[] for _ in range(P)]
        self.reward, self.done = torch.zeros(P, dtype=torch.float64), torch.zeros(P, dtype=torch.uint8)
        self.launches, self.steps_asked = 0, []

    def _over(self, i):
        b = self.b[i]
        return len(b) == 3 or b[:2] == [1, 1]

    def _transition(self, i, a):
        o, x, b = (int(v) for v in a)
        if (o, x) != (0, 0) or b not in (0, 1) or self._over(i):
            self.reward[i], self.done[i] = self.WORST, 1
            return True
        self.b[i].append(b)
        over = self._over(i)
        bb = self.b[i] + [0]
        self.reward[i] = float(REWARD[bb[0], bb[1], bb[2]]) * float(self.scale[i]) if over else 0.0
        self.done[i] = int(over)
        return over

    def gather_(self, index, source=None, check=False, paths=None, path_len=None):
        assert index.tolist() == list(range(self.num_envs)) and source is not None
        self.b = [[] for _ in range(self.num_envs)]
        self.reward, self.done = torch.zeros_like(self.reward), torch.zeros_like(self.done)
        self.gather_length = torch.zeros(self.num_envs, dtype=torch.int32)
        for i in range(self.num_envs):
            for t in range(int(path_len[i])):
                self.gather_length[i] = t + 1
                if self._transition(i, paths[t, i]):
                    break
        return self.obs

    @property
    def obs(self):
        return {"depth": torch.tensor([len(b) for b in self.b])}

    def sample_logits(self, logits, step_index, greedy=False):
        self.steps_asked.append(int(step_index))
        a = torch.zeros((self.num_envs, 3), dtype=torch.int32)
        a[:, 2] = logits.argmax(dim=1).to(torch.int32)
        return a, None, None

    def step(self, actions):
        self.launches += 1
        self.reward, self.done = self.reward.clone(), self.done.clone()
        for i in range(self.num_envs):
            self._transition(i, actions[i])
        return self.obs, self.reward, self.done, {}


@pytest.mark.parametrize("P, iterations, max_children", [(1, 5, 2), (3, 12, 2), (3, 9, 1)])
def test_policy_backend_on_the_toy_game(P, iterations, max_children):
    """With a logits_fn that reproduces `drawn`, tree_search(backend=policy_backend(...)) gives the tree backend_for gives,
    field by field: T launches per iteration, the draw of transition t asked with step index step_index0 + t."""
    root = SimpleNamespace(num_envs=P, device="cpu", run_seed=0)
    planner = ToyPlanner(P)
    calls = [0]

    def logits_fn(obs):
        assert set(obs) == {"depth"}
        step = calls[0]  # the backend asks T times per iteration, iteration m with step_index0 = m * T
        calls[0] += 1
        logits = torch.zeros((P, 2))
        logits[:, drawn(step - step % T, step % T)] = 1.0
        return logits
    got = tree_search(root, iterations, 0, max_children=max_children, backend=policy_backend(root, planner, logits_fn), max_steps=T)
    want = tree_search(root, iterations, 0, max_children=max_children, backend=backend_for(P), max_steps=T)
    for f in want.__dataclass_fields__:
        a, b = getattr(got, f), getattr(want, f)
        assert a.dtype == b.dtype and torch.equal(a, b), f
    assert planner.launches == iterations * T and planner.steps_asked == list(range(iterations * T))


def test_policy_backend_one_call_by_hand():
    """One call, P = 3: an empty path, a path of one step, and a path that ends the short episode (b0 = b1 = 1)."""
    P = 3
    root = SimpleNamespace(num_envs=P, device="cpu", run_seed=0)
    planner = ToyPlanner(P)
    backend = policy_backend(root, planner, lambda obs: torch.tensor([[0.0, 1.0]] * P))  # always b = 1
    paths = torch.zeros((T, P, 3), dtype=torch.int32)
    paths[0, 1, 2] = 0
    paths[0, 2, 2], paths[1, 2, 2] = 1, 1
    po = backend(paths, torch.tensor([0, 1, 2], dtype=torch.int32), 30)
    # row 0 draws 1, 1 and ends at 2; row 1 plays 0, then 1, 1; row 2 ended on its path and reports what gather_ reported
    assert po.length.tolist() == [2, 3, 2] and po.length.dtype == torch.int32 and po.done.tolist() == [1, 1, 1]
    want = [float(REWARD[1, 1, 0]) * SCALE[0], float(REWARD[0, 1, 1]) * SCALE[1], float(REWARD[1, 1, 0]) * SCALE[2]]
    assert po.reward.tolist() == want and po.info is None
    assert po.actions[:, :, 2].tolist() == [[1, 0, 1], [1, 1, 1], [0, 1, 0]]
    assert planner.steps_asked == [30, 31, 32]
    with pytest.raises(ValueError):
        policy_backend(SimpleNamespace(num_envs=P + 1, device="cpu", run_seed=0), planner, None)
    with pytest.raises(ValueError):
        policy_backend(SimpleNamespace(num_envs=P, device="cpu", run_seed=1), planner, None)
