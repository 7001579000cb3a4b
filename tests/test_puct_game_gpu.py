"""A searched game on the GPU, call by call (tests/puct_game_cases.py has the games and the CPU model).

k_puct_advance and k_puct_move take turns on ONE set of guarded, sentinel-filled tensors -- both requests are built over the
same tree -- as puct_selfplay makes them: the searches of three moves, each on what the REROOT before it left, CHOOSE and
REROOT with a `reset`.  After EVERY call every tensor of the call's request equals the state of csrc/pcb_puct.h and
csrc/pcb_puct_move.h composed on the CPU, bit for bit, the guards keep their bytes, and the tensors that only the other
request names are left alone.  The handle has first_env_index = 3: the proportional draws are keyed by 3 + p.

What the games reach -- SELECT and ABSORB at G = 4, 16 and 64 on kept, reset and compacted trees in one wavefront, a full
tree that grows again into the slots REROOT gave up, a kept chain past slot 64 -- is asserted on the CPU
(puct_game_cases.check_game) before a kernel runs."""
import numpy as np
import pytest
import torch

from pcbenv import named_config
from pcbenv.batched_env import BatchedPlacementEnv

import puct_cases as pc
import puct_game_cases as gc
import puct_move_cases as mc
from test_puct_advance_gpu import Guarded, advance_and_compare
from test_puct_move_gpu import DTYPES as MOVE_DTYPES, move_and_compare

pytestmark = pytest.mark.gpu

MOVE_ONLY = gc.MOVE_FIELDS + ("reset",)
ADVANCE_ONLY = ("selected", "path_len", "paths") + pc.INPUTS


@pytest.fixture(scope="module")
def handle():
    env = BatchedPlacementEnv(named_config("c3"), 2, queue_depth=1, run_seed=1, first_env_index=gc.FIRST_ROOT)  # the device, and first_root
    yield env
    env.close()


@pytest.mark.parametrize("name", list(gc.GAMES))
def test_the_kernels_equal_the_model_after_every_call_of_a_game(handle, name):
    gc.check_game(name)
    m = gc.modelled(name)
    game = m.game
    P, N, C, T, K = game.P, game.N, game.C, game.T, game.K
    g = Guarded(P, N, T, K, handle.device)
    for f, shape in dict(mc.shapes(P, N, C), reset=(P,)).items():
        if f not in g.t:
            g.add(f, shape, MOVE_DTYPES.get(f, torch.int32))
    g.t["root_value"].fill_(-7.0)
    g.t["reset"].zero_()
    req, mreq = handle.puct_request(g.t, game.c_puct, C), handle.puct_move_request(g.t, C)
    assert req.parent == mreq.parent and req.num_nodes == mreq.num_nodes and req.errors_dev == mreq.errors_dev and handle.first_env_index == 3
    for i, (call, want) in enumerate(zip(m.seq, m.states)):
        if call["kind"] == gc.ADVANCE:
            g.t["errors_dev"].zero_()  # the model reports the bits of each call
            before, after = advance_and_compare(handle, req, g, i, call, want, g.snapshot())
            others = MOVE_ONLY
        else:
            before, after = move_and_compare(handle, mreq, g, i, call, want, first_root=gc.FIRST_ROOT)
            others = ADVANCE_ONLY
        for f in others:  # what only the other request names
            assert np.array_equal(after[f], before[f]), (i, f)
        for f in gc.STATE_FIELDS:  # and the whole state, whichever kernel ran
            got = g.inside(after, f)
            assert pc.same_bits(got, want[f]) if f in gc.FLOATS else np.array_equal(got.astype(np.int64), want[f]), (i, f)
