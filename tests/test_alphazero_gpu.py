"""pcbenv/alphazero.py on the GPU: self-play collects what the update needs, the update with the device loss
(pcbenv_evaluate_visits and its backward) agrees with the update through the torch chain, and the loop goes round.
The 10x10 spatial configuration of tests/test_evaluate_logits_gpu.py:_ppo_setup, 32 roots, pcbenv/policy.py's model with
its initial weights, 2 moves of 4 search iterations per collect, 8 candidates per node."""
import copy

import numpy as np
import pytest
import torch

from pcbenv import EnvConfig
from pcbenv.alphazero import AlphaZeroConfig, AlphaZeroTrainer
from pcbenv.batched_env import BatchedPlacementEnv
from pcbenv.masked_categorical import unpack_mask_bits
from pcbenv.visit_targets import dense_targets

pytestmark = pytest.mark.gpu

P, MOVES, ITERATIONS, C = 32, 2, 4, 8


def _setup():
    cfg = EnvConfig.spatial(10, 10, 9, 9, 2, 2, 2, 2, 5, 5, 3, 3, 6, 6, "centroid", 2, 0.75)
    root = BatchedPlacementEnv(cfg, P, queue_depth=4, auto_reset=True)
    planner = BatchedPlacementEnv(cfg, P, queue_depth=1)
    for e in (root, planner):
        e.generate_instances()
        e.reset()
    return cfg, root, planner


def test_collect_and_the_two_updates():
    from pcbenv.policy import SpatialPolicy
    torch.manual_seed(0)
    cfg, root, planner = _setup()
    dev = root.device
    policy = SpatialPolicy(cfg).to(dev)
    # two epochs: the statistics reported are those of the second, behind one optimiser step on the first's gradient
    kw = dict(moves=MOVES, iterations=ITERATIONS, max_children=C, epochs=2, minibatches=1, entropy_coef=0.01)
    collector = AlphaZeroTrainer(root, planner, copy.deepcopy(policy), AlphaZeroConfig(device_loss=True, **kw))
    for t in range(3):  # episodes have 5 moves: three uniform ones first, so that the batch holds moves 3 and 4 and every episode ends in it
        root.step(root.sample_actions(t))
    batch = collector.collect()
    N, A = MOVES * P, cfg.num_orientations * cfg.height * cfg.width
    assert batch["mask_bits"].shape == (MOVES, P, 2, 10, 1) and batch["child_visits"].shape == (MOVES, P, C)
    assert batch["child_actions"].shape == (MOVES, P, C, 3) and batch["z"].shape == batch["weight"].shape == (MOVES, P)
    assert int(batch["errors"]) == 0
    assert not bool(batch["done"][0].any()) and bool(batch["done"][1].all())
    assert bool((batch["weight"] == 1).all())
    assert torch.equal(batch["z"][1], batch["reward"][1].float()) and torch.equal(batch["z"][0], batch["z"][1])  # carried back over the episode
    # the stored bits are the stored masks
    bits = batch["mask_bits"].reshape(N, 2, 10, 1)
    legal = unpack_mask_bits(cfg, bits)
    assert torch.equal(legal, batch["obs"]["action_mask"].reshape(N, -1).bool())
    # every row with T > 0 has its targets inside its legal set, and the kernel raises no bit 2
    visits, actions = batch["child_visits"].reshape(N, C), batch["child_actions"].reshape(N, C, 3)
    a = actions.long()
    flat = a[..., 0] * 100 + a[..., 1] * 10 + a[..., 2]
    assert bool((flat >= 0).all()) and bool((flat < A).all())
    assert bool((legal.gather(1, flat) | (visits == 0)).all()) and bool((visits >= 0).all())
    pi, T = dense_targets(cfg, legal, visits, actions)
    assert bool((T[:P] == ITERATIONS - 1).all())  # a fresh tree: every iteration but the first went through a child of the root
    assert bool((T[P:] >= ITERATIONS - 1).all())  # (a kept subtree adds its own)
    err = torch.zeros(1, dtype=torch.int32, device=dev)
    ce, ent = root.evaluate_visits_forward(torch.zeros((N, A), device=dev), bits.contiguous(), visits.contiguous(), actions.contiguous(), None, err)
    assert int(err.item()) == 0 and bool(torch.isfinite(ce).all())
    # from identical weights and this one batch, one update with device_loss off and one with it on
    stats = {}
    for on in (False, True):
        tr = AlphaZeroTrainer(root, planner, copy.deepcopy(policy), AlphaZeroConfig(device_loss=on, **kw))
        torch.manual_seed(123)  # the same permutation and BatchNorm refresh rows
        stats[on] = tr.update(batch)
    print("ALPHAZERO-UPDATE-AB", stats)
    assert set(stats[True]) == {"loss", "policy", "value", "entropy"}
    for k in stats[True]:
        assert abs(stats[False][k] - stats[True][k]) <= 1e-4, (k, stats)
    assert stats[True]["value"] > 0 and stats[True]["policy"] > 0
    # a second round, the collector's own loop: moves 0 and 1 of the next episodes, which end outside the batch
    second = collector.collect()
    assert not bool(second["done"].any()) and not bool(second["weight"].any())
    out = collector.update(second)
    assert all(np.isfinite(v) for v in out.values()) and out["value"] == 0.0, out
    for e in (root, planner):
        e.close()
