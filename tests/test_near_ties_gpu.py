"""The witnesses and the real-valued searches of tests/near_tie_cases.py on the GPU.

1. Witness tables: for pcbenv_puct_advance, pcbenv_puct_advance_leaves and pcbenv_gumbel_advance at G = 4, 16 and 64, SELECT on
   the hand-built table -- two contending children per root whose scores part in the last bits, placed over the lanes
   where the butterfly argmax combines -- then ABSORB | SELECT with a scripted real-valued evaluation, for Gumbel CHOOSE
   before them.  After each call every tensor of the request equals the CPU model's, floats by their bits, through the
   guarded-tensor harnesses of the three kernels' own GPU tests.  tests/test_near_ties_model.py holds the model to the
   Python reference on the same tables and shows that each wrong arithmetic goes to the other child: a kernel that
   computes one of them -- a fused multiply-add, another root, a reciprocal -- differs from the model here.
2. Recorded searches on real-valued evaluations: the kernel equals the model after every call."""
import numpy as np
import pytest
import torch

from pcbenv import named_config
from pcbenv.batched_env import BatchedPlacementEnv

import near_tie_cases as nt
import puct_cases as pc
import test_gumbel_gpu as gumbel_gpu
import test_puct_advance_gpu as puct_gpu
import test_puct_leaves_gpu as leaves_gpu
from test_puct_advance_gpu import Guarded
from test_puct_leaves_gpu import GuardedLeaves

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def handle():
    env = BatchedPlacementEnv(named_config("c3"), 2, queue_depth=1, run_seed=1)  # the handle gives the device only
    yield env
    env.close()


@pytest.mark.parametrize("kernel, G", [(k, G) for k in ("puct", "leaves") for G in nt.WIDTHS])
def test_the_kernel_equals_the_model_on_the_witness_table(handle, kernel, G):
    t, seq, states = nt.puct_calls(kernel, G)
    if kernel == "puct":
        g = Guarded(t.P, t.N, nt.T, t.K, handle.device)
        req = handle.puct_request(g.t, t.c_puct, t.C)
    else:
        g = GuardedLeaves(t.P, t.N, nt.T, t.K, t.L, handle.device)
        req = handle.puct_leaves_request(g.t, t.c_puct, t.C, t.L)
        g.t["pending"].zero_()  # the model's load leaves nothing pending; the first call's pokes are the table's
    for f in pc.TREE_FIELDS:  # the load of the first call
        g.t[f].copy_(torch.from_numpy(np.ascontiguousarray(t.state[f])).to(g.t[f].dtype))
    before = g.snapshot()
    for i, (call, want) in enumerate(zip(seq, states)):
        if kernel == "puct":
            _, before = puct_gpu.advance_and_compare(handle, req, g, i, call, want, before)
        else:
            before = leaves_gpu.advance_and_compare(handle, req, g, i, call, want, before)
    first = states[0]["selected"][::t.L]
    assert all(first[p] == row["ref"] for p, row in enumerate(t.rows))  # what was compared is the reference's choice


@pytest.mark.parametrize("G", list(nt.WIDTHS))
def test_the_gumbel_kernel_equals_the_model_on_the_witness_table(handle, G):
    case, seq, states = nt.gumbel_calls(G)
    gumbel_gpu.assert_equals_the_model_after_every_call(handle, case, seq, states)


@pytest.mark.parametrize("G", list(nt.WIDTHS))
def test_the_gumbel_kernel_s_policy_target_equals_the_model_s_on_the_choose_table(handle, G):
    """Roots on which a Z summed in another order, a reciprocal of Z or a fused improved logit changes a child_weights
    integer or a child_policy float32 (tests/test_near_ties_model.py shows that they do)."""
    case, seq, states = nt.choose_calls(G)
    gumbel_gpu.assert_equals_the_model_after_every_call(handle, case, seq, states)


@pytest.mark.parametrize("name", list(nt.REAL_PUCT))
def test_puct_advance_equals_the_model_on_a_real_valued_search(handle, name):
    puct_gpu.assert_equals_the_model_after_every_call(handle, nt.real_puct(name))


@pytest.mark.parametrize("name", list(nt.REAL_LEAVES))
def test_puct_advance_leaves_equals_the_model_on_a_real_valued_search(handle, name):
    leaves_gpu.assert_equals_the_model_after_every_call(handle, nt.real_leaves(name))


@pytest.mark.parametrize("name", nt.REAL_GUMBEL)
def test_gumbel_advance_equals_the_model_on_a_real_valued_search(handle, name):
    case, seq, states, gs, calls = nt.real_gumbel(name)
    gumbel_gpu.assert_equals_the_model_after_every_call(handle, case, seq, states)
