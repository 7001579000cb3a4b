"""The tensor halves of pcbenv.search's playout-based functions on hand-made CPU tensors: the selection of
best_of_k_playouts (select_best) and the aggregation of action_values (aggregate_values).  No device, no library call."""
import math

import torch

from pcbenv.search import ActionValues, BestOfK, aggregate_values, pick_best, select_best


def test_select_best_picks_the_first_best_child_and_its_trajectory():
    P, k, T = 3, 4, 5
    reward = torch.tensor([-3.0, -1.0, -2.0, -1.0,     # root 0: a tie between children 1 and 3 -> the first
                           -9.0, -8.0, -7.0, -6.5,     # root 1: the last child
                           0.0, -0.5, -0.25, -4.0],    # root 2: the first child
                          dtype=torch.float64)
    length = torch.tensor([5, 4, 3, 2, 1, 2, 3, 4, 5, 5, 5, 5], dtype=torch.int32)
    actions = torch.arange(T * P * k * 3, dtype=torch.int32).view(T, P * k, 3)
    res = select_best(reward, length, actions, k)
    assert isinstance(res, BestOfK)
    assert res.child.tolist() == [1, 7, 8] and res.child.dtype == torch.int64
    assert res.reward.tolist() == [-1.0, -6.5, 0.0] and res.reward.dtype == torch.float64
    assert res.length.tolist() == [4, 4, 5] and res.length.dtype == torch.int64
    assert res.actions.shape == (T, P, 3) and torch.equal(res.actions, actions[:, [1, 7, 8]])
    assert res.child_rewards.shape == (P, k) and torch.equal(res.child_rewards.reshape(-1), reward)
    r, c = pick_best(reward, k)  # the selection is best_of_k's own
    assert torch.equal(r, res.reward) and torch.equal(c, res.child)


def test_select_best_with_one_child_per_root():
    reward = torch.tensor([-2.0, -1.0], dtype=torch.float64)
    res = select_best(reward, torch.tensor([3, 1], dtype=torch.int32), torch.zeros((4, 2, 3), dtype=torch.int32), 1)
    assert res.child.tolist() == [0, 1] and res.reward.tolist() == [-2.0, -1.0] and res.length.tolist() == [3, 1]


def test_aggregate_values_means_maxima_and_cut_share():
    P, A, k = 2, 3, 4
    reward = torch.arange(P * A * k, dtype=torch.float64) * 0.5 - 4.0   # playout (p * A + a) * k + j
    reward[5] = 10.0                                                    # try 1 of candidate 1 of root 0
    done = torch.ones(P * A * k, dtype=torch.uint8)
    done[[0, 7, 23]] = 0
    v = aggregate_values(reward, done, P, A, k)
    assert isinstance(v, ActionValues) and v.mean.shape == (P, A) and v.max.shape == (P, A)
    for p in range(P):
        for a in range(A):
            tries = reward[(p * A + a) * k:(p * A + a + 1) * k]
            assert v.mean[p, a].item() == tries.mean().item() and v.max[p, a].item() == tries.max().item()
    assert v.max[0, 1].item() == 10.0 and v.mean.dtype == torch.float64
    assert math.isclose(v.cut_share.item(), 3 / 24)
    assert aggregate_values(reward, torch.ones_like(done), P, A, k).cut_share.item() == 0.0
