"""pcbenv.search.tree_search on the GPU: the device backend (one pcbenv_playout_paths launch per iteration) and a backend
that plays the same playouts on the CPU oracle must grow identical trees -- every draw is keyed by (run_seed, root, step
index), so the search is deterministic and any difference in one playout's reward, length or drawn action shows up in the
tree.  12 roots at different depths (path_cases.Plan), 24 iterations."""
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from pcbenv.batched_env import Playout
from pcbenv.search import tree_search

import path_cases as pa
import playout_cases as pc
from test_playout_gpu import device_roots

pytestmark = pytest.mark.gpu

ITERATIONS, STEP_INDEX = 24, 5000


def oracle_backend(roots, T, calls):
    cfg, P = roots.cfg, roots.P

    def backend(paths, path_len, step_index0):
        paths, path_len = paths.cpu().numpy(), path_len.cpu().numpy()
        calls.append(int(path_len.max()))
        acts = np.zeros((T, P, 3), np.int32)
        reward, done, length = np.zeros(P), np.zeros(P, np.uint8), np.zeros(P, np.int32)
        for p in range(P):
            e = pa.oracle_path_playout(cfg, roots.inst[p], roots.hist[p], roots.seed, p, step_index0, T, paths[:path_len[p], p])
            reward[p], done[p], length[p] = e["reward"], e["done"], e["length"]
            acts[:e["length"], p] = e["actions"]
        return Playout(torch.from_numpy(reward), torch.from_numpy(done), torch.from_numpy(length), None, torch.from_numpy(acts))
    return backend


def _bits(t):
    return t.cpu().numpy().view(np.uint64)


@pytest.mark.parametrize("name", ["small_pin", "c3_centroid"])
def test_device_and_oracle_backends_grow_the_same_tree(name):
    roots = pa.Plan(name).roots
    cfg, P, T = roots.cfg, roots.P, pc.max_steps(roots.cfg)
    assert P == 12
    calls = []
    want = tree_search(SimpleNamespace(num_envs=P, cfg=cfg, device="cpu"), ITERATIONS, STEP_INDEX, c_uct=0.7, max_children=3,
                       backend=oracle_backend(roots, T, calls))
    assert len(calls) == ITERATIONS and max(calls) >= 2  # the search went deeper than one ply
    assert int(want.num_nodes.max()) > 4 and bool(want.terminal.any())
    run = device_roots(roots)
    got = tree_search(run.env, ITERATIONS, STEP_INDEX, c_uct=0.7, max_children=3)
    for f in ("num_nodes", "parent", "depth", "node_action", "visits", "terminal", "children", "child_visits", "child_actions", "action",
              "best_length"):
        assert torch.equal(getattr(got, f).cpu(), getattr(want, f)), f
    for f in ("value_sum", "value_max", "best_reward"):
        assert np.array_equal(_bits(getattr(got, f)), _bits(getattr(want, f))), f
    L = want.best_length
    for p in range(P):
        assert torch.equal(got.best_actions[:int(L[p]), p].cpu(), want.best_actions[:int(L[p]), p]), p
    run.compare_oracle("the roots after the search")
    run.close()
