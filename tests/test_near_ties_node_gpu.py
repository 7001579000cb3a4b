"""The witnesses and the real-valued searches of tests/near_tie_node_cases.py on the GPU: pcbenv_gumbel_advance_leaves,
pcbenv_gumbel_tree_advance and pcbenv_gumbel_tree_advance_leaves at G = 4, 16 and 64.

1. Witness tables: CHOOSE, SELECT and ABSORB | SELECT with a scripted real-valued evaluation on hand-built states -- two
   contending children per node whose t (or root score) part in the last bits, over the lanes where the butterfly argmax
   combines; pending visits preset and made by the launch itself; a witness that decides the second leaf of a launch.  After
   each call every tensor of the request equals the CPU model's, floats by their bits, through the guarded-tensor harnesses of the
   three kernels' own GPU tests, and what was compared at the first SELECT is the reference's choice.
   tests/test_near_ties_node_model.py holds the models to the Python reference on the same tables and shows that each wrong
   arithmetic -- a sum in butterfly order, a fused multiply-add, a reciprocal, a pending visit left out -- goes to the other child.
2. CHOOSE tables: roots on which such an arithmetic moves a child_weights integer or a child_policy float32.
3. Recorded searches on real-valued evaluations: the kernel equals the model after every call."""
import pytest

from pcbenv import named_config
from pcbenv.batched_env import BatchedPlacementEnv

import near_tie_node_cases as nn
import test_gumbel_leaves_gpu as leaves_gpu
import test_gumbel_tree_gpu as tree_gpu
import test_gumbel_tree_leaves_gpu as tree_leaves_gpu

pytestmark = pytest.mark.gpu
WIDTHS = list(nn.WIDTHS)
TREE_KERNELS = ("gumbel_tree", "gumbel_tree_leaves")


@pytest.fixture(scope="module")
def handle():
    env = BatchedPlacementEnv(named_config("c3"), 2, queue_depth=1, run_seed=1)  # the handle gives the device only
    yield env
    env.close()


def equals_the_model(handle, kernel, case, seq, states):
    if kernel == "gumbel_tree":
        assert case.levels == tree_gpu.gt.T
        tree_gpu.assert_equals_the_model_after_every_call(handle, case, seq, states)
    else:
        harness = leaves_gpu if kernel == "gumbel_leaves" else tree_leaves_gpu
        harness.assert_equals_the_model_after_every_call(handle, case, seq, states, levels=case.levels)


def first_leaves(states, case, leaf=0):
    """What the model -- which the kernel has just been held to -- selected at the first SELECT, per root."""
    per = getattr(case, "L", 1)
    return states[1]["selected"][leaf::per]


@pytest.mark.parametrize("G", WIDTHS)
@pytest.mark.parametrize("kernel", TREE_KERNELS)
def test_the_tree_kernels_equal_the_model_on_the_node_rule_table(handle, kernel, G):
    case, seq, states = nn.node_calls(kernel, G)
    equals_the_model(handle, kernel, case, seq, states)
    assert first_leaves(states, case).tolist() == [row["ref"] for row in nn.node_table(G).rows]


@pytest.mark.parametrize("G", WIDTHS)
def test_the_tree_leaves_kernel_equals_the_model_on_the_pending_table(handle, G):
    case, seq, states = nn.pending_calls(G)
    equals_the_model(handle, "gumbel_tree_leaves", case, seq, states)
    first, second = first_leaves(states, case), first_leaves(states, case, 1)
    for p, row in enumerate(nn.pending_table(G).rows):
        assert (second[p] if row["kind"] == "launched" else first[p]) == row["ref"], (p, row)


@pytest.mark.parametrize("G", WIDTHS)
@pytest.mark.parametrize("kernel", TREE_KERNELS)
def test_the_tree_kernels_equal_the_model_on_root_scores_completed_with_vmix(handle, kernel, G):
    case, seq, states = nn.root_calls(kernel, G)
    equals_the_model(handle, kernel, case, seq, states)
    assert first_leaves(states, case).tolist() == [row["ref"] for row in nn.root_table(G).rows]


@pytest.mark.parametrize("G", WIDTHS)
@pytest.mark.parametrize("which", ["first", "second"])
@pytest.mark.parametrize("kernel", ["gumbel_leaves", "gumbel_tree_leaves"])
def test_the_leaf_kernels_equal_the_model_on_the_root_score_witnesses(handle, kernel, which, G):
    """The witness decides the first leaf of the launch, or the second: from scores and counters kept in registers."""
    t, case, seq, states = nn.gumbel_rows_calls(kernel, G, which)
    equals_the_model(handle, kernel, case, seq, states)
    got = first_leaves(states, case, int(which == "second"))
    assert all(got[p] == row["ref"] for p, row in enumerate(t.rows) if row["score"] == "gumbel")


@pytest.mark.parametrize("G", WIDTHS)
def test_the_gumbel_leaves_kernel_equals_the_model_on_pending_visits_below_a_scheduled_root(handle, G):
    t, case, seq, states = nn.leaves_rows_calls(G)
    equals_the_model(handle, "gumbel_leaves", case, seq, states)
    got = first_leaves(states, case)
    assert all(got[p] == row["ref"] for p, row in enumerate(t.rows) if row["level"] == 1)


@pytest.mark.parametrize("G", WIDTHS)
@pytest.mark.parametrize("kernel", TREE_KERNELS)
def test_the_tree_kernels_policy_target_equals_the_model_s_on_the_choose_tables(handle, kernel, G):
    """Roots on which Qv in butterfly order or a fused vmix (some children have no visit), and Z in butterfly order, a reciprocal
    of Z or a fused improved logit (all have one), changes a child_weights integer or a child_policy float32."""
    equals_the_model(handle, kernel, *nn.choose_calls(kernel, G))
    equals_the_model(handle, kernel, *nn.root_rule_choose_calls(kernel, G))


@pytest.mark.parametrize("kernel, name, leaves", [(kernel, name, leaves) for kernel, Ls in nn.REAL_LEAVES.items() for name in nn.REAL for leaves in Ls])
def test_the_kernel_equals_the_model_on_a_real_valued_search(handle, kernel, name, leaves):
    case, seq, states, gs, calls = nn.real_search(kernel, name, leaves)
    equals_the_model(handle, kernel, case, seq, states)
