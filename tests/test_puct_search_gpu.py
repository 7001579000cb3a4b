"""The PUCT search through the whole stack on real roots: `puct_search_device` -- pcbenv_puct_advance next to
`network_evaluator` (pcbenv_gather_paths, `top_priors`, pcbenv_playout_paths) -- against `puct_search`, the specification,
run on the same handles with the same evaluator: the specification's tree tensors and arithmetic are on the CPU and the
evaluator's outputs are copied over.  The evaluator is a function of its arguments, so both searches see the same
evaluations and must grow identical trees, field by field, floats by their bits; the roots are untouched afterwards.

For the (paths, path_len) of that run the evaluator itself is held to the CPU oracle (tests/gather_path_cases.py): the
terminal flag, with constant logits the candidates -- the K lowest legal flat actions of the oracle's node, each with prior
float32(1 / n) -- and the value of a terminal leaf."""
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from pcbenv.batched_env import BatchedPlacementEnv
from pcbenv.search import Evaluation, network_evaluator, puct_search, puct_search_device

import gather_path_cases as gp
import path_cases as pa
import playout_cases as pc
from test_playout_gpu import device_roots

pytestmark = pytest.mark.gpu

STEP_INDEX, C_PUCT = 7000, 1.25
FIELDS = ("parent", "depth", "visits", "num_children", "first_child", "node_action", "prior", "value_sum", "value_max", "terminal",
          "reward_lo", "reward_hi", "num_nodes", "action", "child_visits", "child_actions", "child_priors", "root_value", "errors")


def constant_logits(cfg, P, dev):
    zeros = torch.zeros((P, cfg.num_orientations * cfg.height * cfg.width), dtype=torch.float32, device=dev)
    return lambda obs: zeros


def linear_logits(cfg, P, dev):
    """A fixed seeded linear map of action_mask: logits[a] = b[a] + v[a] * sum over a' of u[a'] * mask[a'] (a reduction and
    elementwise operations only: the same mask gives the same bits every time)."""
    A = cfg.num_orientations * cfg.height * cfg.width
    g = torch.Generator().manual_seed(20)
    b, v, u = (torch.randn(A, generator=g).to(dev) for _ in range(3))
    return lambda obs: b[None, :] + v[None, :] * (obs["action_mask"].reshape(P, A).to(torch.float32) * (u / A)[None, :]).sum(dim=1, keepdim=True)


def same(a, b):
    a, b = a.cpu(), b.cpu()
    return a.dtype == b.dtype and a.shape == b.shape and a.numpy().tobytes() == b.numpy().tobytes()


@pytest.mark.parametrize("name, iterations, C, logits", [
    ("small_pin", 24, 3, constant_logits), ("small_pin", 12, 16, constant_logits), ("spatial_7x100_t256", 12, 16, constant_logits),
    ("c3_centroid", 16, 3, constant_logits), ("small_pin", 16, 16, linear_logits)])
def test_device_search_is_the_specification_on_real_roots(name, iterations, C, logits):
    roots = pa.Plan(name).roots
    cfg, P, T = roots.cfg, roots.P, pc.max_steps(roots.cfg)
    assert P == 12 or name == "spatial_7x100_t256"
    run = device_roots(roots)
    dev = run.env.device
    planner = BatchedPlacementEnv(cfg, P, queue_depth=2, run_seed=roots.seed, auto_reset=False, **roots.kw)
    planner.generate_instances()
    planner.reset()
    evaluate = network_evaluator(run.env, planner, logits(cfg, P, dev), max_children=C)
    recorded = []

    def copied_over(paths, path_len, step_index0):
        ev = evaluate(paths.to(dev), path_len.to(dev), step_index0)
        ev = Evaluation(*(getattr(ev, f).cpu() for f in ("value", "terminal", "cand_count", "cand_actions", "cand_prior")))
        recorded.append((paths.numpy().copy(), path_len.numpy().copy(), ev))
        return ev
    want = puct_search(SimpleNamespace(num_envs=P, cfg=cfg, device="cpu"), iterations, STEP_INDEX, copied_over, c_puct=C_PUCT, max_children=C, max_steps=T)
    got = puct_search_device(run.env, iterations, STEP_INDEX, evaluate, c_puct=C_PUCT, max_children=C, max_steps=T)
    assert int(want.errors) == 0 and int(want.num_nodes.max()) > 1 + C and int(want.depth.max()) >= 2
    for f in FIELDS:
        assert same(getattr(got, f), getattr(want, f)), f
    run.compare_oracle("the roots after the searches")
    # the evaluator against the CPU oracle, every distinct node of the run once
    H, W = cfg.height, cfg.width
    seen, terminals = set(), 0
    for paths, path_len, ev in recorded:
        for p in range(P):
            path = paths[:path_len[p], p]
            key = (p, path.tobytes())
            if key in seen:
                continue
            seen.add(key)
            nd = gp.oracle_node(cfg, roots.inst[p], roots.hist[p], path)
            over = nd["length"] > 0 and nd["done"] == 1
            assert bool(ev.terminal[p]) == over, (p, path)
            if over:
                terminals += 1
                assert np.float64(ev.value[p]).tobytes() == nd["reward"].tobytes(), (p, path)
            legal = np.flatnonzero(np.asarray(nd["obs"]["action_mask"]).reshape(-1))
            n, k = len(legal), int(ev.cand_count[p])
            assert k == min(C, n), (p, path)
            a = ev.cand_actions[p].numpy().astype(np.int64)
            flat = (a[:, 0] * H + a[:, 1]) * W + a[:, 2]
            assert not a[k:].any() and not ev.cand_prior[p, k:].any()
            if logits is constant_logits and k:
                assert flat[:k].tolist() == legal[:k].tolist(), (p, path)
                assert (ev.cand_prior[p, :k].numpy() == np.float32(1.0) / np.float32(n)).all(), (p, path)
            elif k:  # legal, distinct, the more probable first
                assert set(flat[:k].tolist()) <= set(legal.tolist()) and len(set(flat[:k].tolist())) == k
                pr = ev.cand_prior[p, :k].numpy()
                assert (pr[:-1] >= pr[1:]).all() and (k < 2 or n <= C or flat[:k].tolist() != legal[:k].tolist())
    assert len(seen) > iterations  # the roots went different ways
    if logits is linear_logits:
        assert any(len(set(ev.cand_prior[p, :int(ev.cand_count[p])].tolist())) > 1 for _, _, ev in recorded for p in range(P))
    print(f"PUCT-SEARCH {name} C={C}: {len(seen)} distinct nodes evaluated, {terminals} terminal, at most {int(want.num_nodes.max())} slots in use, "
          f"depth {int(want.depth.max())}")
    planner.close()
    run.close()
