"""A searched game on the CPU: csrc/pcb_puct.h and csrc/pcb_puct_move.h, composed on one state by tools/puct_game_check.cpp
(AddressSanitizer + UBSan, a program of its own, nothing preloaded), against the specification's game -- puct_search(tree=),
puct_choose, puct_reroot of pcbenv/search.py -- move by move: every selection is the recorded one (the program checks it),
and after each move's last ABSORB, its CHOOSE and its REROOT the state is the specification's, field by field, floats by
their bits.  tests/puct_game_cases.py has the games; tests/test_puct_game_gpu.py holds the kernels to the model's states."""
import shutil

import numpy as np
import pytest

import puct_cases as pc
import puct_game_cases as gc
import puct_move_cases as mc
from pcbenv.search import search_tree

pytestmark = pytest.mark.skipif(shutil.which("g++") is None, reason="no g++")


def _same(state, f, t):
    t = t.numpy()
    if f in gc.FLOATS:
        assert pc.same_bits(state[f], t.astype(np.float64)), f
    else:
        assert np.array_equal(state[f], t.astype(np.int64)), f


@pytest.mark.parametrize("name", list(gc.GAMES))
def test_the_game_is_what_it_is_there_for(name):
    """Descents through kept nodes, reset and kept roots in one wavefront, a full tree compacted and grown again, ties in a
    kept tree, both modes, a draw that depends on first_root: puct_game_cases.check_game, from the model's states."""
    v = gc.check_game(name)
    assert v.errors == [0, pc.ERR_FULL] and gc.FIRST_ROOT == 3 and gc.J == 3
    if name == "chain":  # the kept chain passes slot 64, and the first SELECT walks all of it
        assert v.deepest_first_select >= 64
    else:
        assert gc.GAMES[name][2] == pc.WIDTH_T


def test_the_games_cover_the_widths():
    assert [pc.group_lanes(g[3]) for g in gc.GAMES.values()] == [4, 16, 64, 4]
    assert all(g[6] <= 1 + g[5] * g[3] for g in gc.GAMES.values())  # no roomier than a single search needs


@pytest.mark.parametrize("name", list(gc.GAMES))
def test_the_model_is_the_specification(name):
    m = gc.modelled(name)
    g, seq, states = m.game, m.seq, m.states
    errors = 0
    for j, mv in enumerate(g.moves):
        mine = [i for i, c in enumerate(seq) if c["move"] == j]
        assert [seq[i]["kind"] for i in mine[-2:]] == [gc.MOVE, gc.MOVE] and seq[mine[-3]]["phases"] == pc.ABSORB
        searched, chose, rerooted = (states[i] for i in mine[-3:])
        errors |= int(np.bitwise_or.reduce([states[i]["errors"] for i in mine]))
        for f in pc.TREE_FIELDS:  # the search went on in the kept tree as puct_search(tree=) does
            _same(searched, f, getattr(mv.ps, f))
        assert errors == int(mv.ps.errors)  # the specification's error word is the game's, the model's a call's
        for f in ("move_slot", "move_action", "child_visits", "child_actions", "root_value"):
            _same(chose, f, mv.chosen[f])
        for f in pc.TREE_FIELDS + ("selected", "path_len", "paths") + (("remap",) if j else ()):  # CHOOSE writes its five tensors only
            assert pc.same_bits(chose[f], searched[f]), f
        for f in pc.TREE_FIELDS:
            _same(rerooted, f, mv.tree[f])
        _same(rerooted, "remap", mv.remap)
        for f in ("selected", "path_len", "paths", "move_slot", "move_action", "child_visits", "child_actions", "root_value"):
            assert pc.same_bits(rerooted[f], chose[f]), f
        gone = (mv.done != 0) | (mv.chosen["move_slot"].numpy() < 0)
        assert (rerooted["num_nodes"][gone] == 1).all() and (rerooted["visits"][gone, 0] == 0).all() and np.isinf(rerooted["reward_lo"][gone]).all()
        assert gone.any() and not gone.all()
    first = states[0]
    assert (first["move_slot"] == mc.FILL).all() and (first["remap"] == mc.FILL).all() and (first["root_value"] == -7.0).all()
    assert int(search_tree(g.moves[-1].ps)["errors_dev"][0]) == errors
