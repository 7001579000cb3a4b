"""The plain transition of the geometry-fixed step builds (Team<>::plain_transition_from_rows, csrc/pcb_step.h: the grid
plane from the lane's register row before the rest of the update, the mask folded from the same register) at the
boundaries of that arm, c3 / c4 at B = 8 and B = 40: a `fixed_geometry=1` handle against a `fixed_geometry=0` twin -- every
bound tensor, reward, done, info, the actions, `mask_bits()` and the state blocks, bit for bit after every call -- and
against the host model of tests/handle_model.py.

The external actions are made on the host from the mask the device shows, so that every case meets: a placement at
(0, 0); one flush with the bottom and right edges (bit 63 of lane 63); both orientations of a component with h != w; a
next component with h == w (the second plane is a copy); an occupied cell and tuples or codes out of range in the same
launch as valid actions; the last-but-one and the last component.  Before every step the cell tensors and the marginals
of the rows about to take a valid action are filled with a marker byte: a byte the arm no longer wrote would keep it.

No play on a 64 x 64 grid leaves a component of at most 6 x 6 cells without a legal cell, so the episode that ends that
way starts from a checkpoint whose occupancy rows are edited on the host, the same way in both handles: everything is
occupied but the cells the next action fills.  The host model cannot follow that; the twin and direct checks do."""
import numpy as np
import pytest
import torch

from pcbenv import named_config

from emission_cases import SENTINEL
from handle_model import Run, _bytes_equal
from test_fixed_geometry_gpu import Pair, _same

pytestmark = pytest.mark.gpu

CASES = [(name, B) for name in ("c3", "c4") for B in (8, 40)]
H = W = 64
CELL_KEYS = ("grid", "action_mask", "pin_grid")


def _np(t):
    return t.cpu().numpy()


def _components(env):
    """Per environment: the cursor (-1: none), the number of components and their (h, w), from the feature tensors."""
    obs = env.obs_f64()
    pm, cf = _np(obs["placement_mask"]), _np(obs["all_components_feature"])
    cur = np.where((pm == 3.0).any(axis=1), (pm == 3.0).argmax(axis=1), -1)
    return cur, (pm != 0.0).sum(axis=1), cf[:, :, 0].astype(int), cf[:, :, 1].astype(int)


TERM_MARK = slice(56, 64)  # EnvHdr::term_seq, term_pos (csrc/pcb_records.h), the last two words of the 64-byte header


def _same_states(pair, tag):
    """The state blocks but for the environment's mark on the terminal list of the next launch: its place there is the order
    in which the launch's atomic adds arrived, and with more takers than a shard has entries so is who gets one at all.  The
    list is a scheduling hint no result depends on (Team<>::run_env)."""
    a, b = pair.both(lambda e: np.array(e.state_dict()["state"]).reshape(pair.B, -1))
    a[:, TERM_MARK] = b[:, TERM_MARK] = 0
    assert _bytes_equal(a, b), (tag, "state blocks", np.flatnonzero((a != b).any(axis=1))[:5].tolist())


def _fill_marker(pair, rows):
    """The cell tensors and the marginals of `rows`, in both handles, to the marker byte."""
    idx = torch.from_numpy(np.flatnonzero(rows))
    for e in (pair.fix, pair.run):
        idx_d = idx.to(e.device)
        for k in CELL_KEYS:
            if k in e.obs:
                e.obs[k][idx_d] = SENTINEL
        for v in e.mask_marginals.values():
            v[idx_d] = SENTINEL


def _check_against_model(run, a, r, d, tag):
    rr, dd, ii = run.model.step(a)
    assert np.array_equal(_np(d), dd), (tag, "done")
    assert _bytes_equal(_np(r), rr), (tag, "reward")
    inf = _np(run.env.info_raw)
    has = ~np.isnan(inf[:, 0])
    assert _bytes_equal(inf[has], ii[has]), (tag, "info")
    run.model.I[run.model.slot] = inf
    run.compare_oracle(tag)
    return dd


@pytest.mark.parametrize("name,B", CASES)
def test_crafted_external_actions_at_the_arm_boundaries(name, B):
    cfg = named_config(name)
    O, HW, A = cfg.num_orientations, H * W, cfg.num_orientations * H * W
    run = Run(cfg, B, mask_marginals=True, options={"fixed_geometry": 1})
    pair = Pair(cfg, B, fix=run.env)
    placed = np.zeros(B, int)  # components placed in the current episode
    met = dict(origin=0, flush=0, occupied=0, out_of_range=0, last_but_one=0, last=0, next_square=0, mixed_launch=0)
    oriented = set()           # orientations & 1 that components with h != w were placed with, over the batch
    # (step, environment) -> the invalid action it takes there
    invalid = {(2, 1): "occupied", (2, 2): (O, 0, 0), (4, 3): (0, H, 0), (5, 5): (0, -1, 0), (6, 4): (0, 0, W), (7, 6): (-1, 3, 3),
               (9, 1): "occupied"}
    try:
        for t in range(26):
            drawn = _np(run.env.sample_actions(t))
            assert np.array_equal(drawn, _np(pair.run.sample_actions(t))), t
            mask, grid = _np(run.env.obs["action_mask"]).reshape(B, O, H, W), _np(run.env.obs["grid"])
            cur, ncomp, ch, cw = _components(run.env)
            a = drawn.copy()
            valid = np.ones(B, bool)
            for i in range(B):
                assert cur[i] == placed[i] < ncomp[i], (t, i)  # reset_done() follows every step: nobody is past its end
                h, w = ch[i, cur[i]], cw[i, cur[i]]
                bad = invalid.get((t, i))
                if bad == "occupied":
                    x, y = np.argwhere(grid[i] != 0)[0]
                    a[i], valid[i] = (0, x, y), False
                    met["occupied"] += 1
                elif bad is not None:
                    a[i], valid[i] = bad, False
                    met["out_of_range"] += 1
                elif placed[i] == 0:  # an empty grid: the corners, in all four orientations over the batch
                    o = (0, 0, 1, 3)[i % 4]
                    cells = np.argwhere(mask[i, o] != 0)
                    x, y = cells[-1] if i % 4 in (1, 2) else cells[0]
                    a[i] = (o, x, y)
                    ph, pw = (w, h) if o & 1 else (h, w)
                    if i % 4 in (1, 2):
                        assert (x + ph, y + pw) == (H, W), (t, i)
                        met["flush"] += 1
                    else:
                        assert (x, y) == (0, 0), (t, i)
                        met["origin"] += 1
                if valid[i]:
                    if h != w:
                        oriented.add(int(a[i, 0]) & 1)
                    nxt = cur[i] + 1
                    met["last"] += nxt == ncomp[i]
                    met["last_but_one"] += nxt == ncomp[i] - 1
                    met["next_square"] += nxt < ncomp[i] and ch[i, nxt] == cw[i, nxt]
            met["mixed_launch"] += (not valid.all()) and valid.any()
            if t % 2:  # flat codes; a tuple out of range has none: a code out of range stands for it
                f = (a[:, 0].astype(np.int64) * HW + a[:, 1] * W + a[:, 2])
                for i in np.flatnonzero(~valid):
                    if invalid[(t, i)] != "occupied":
                        f[i] = (-1, A, A + 4, 2 ** 31 - 1)[(t // 2) % 4]
                acts = torch.from_numpy(f.astype(np.int32))
            else:
                acts = torch.from_numpy(a.astype(np.int32))
            _fill_marker(pair, valid)
            (_, r, d, _), _ = pair.both(lambda e: e.step(acts))
            dd = _check_against_model(run, a.astype(np.int32), r, d, ("step", t))
            pair.compare(("step", t))
            _same_states(pair, ("step", t))
            assert np.array_equal(dd[~valid] != 0, np.ones(int((~valid).sum()), bool)), t  # an invalid action ends the episode
            placed[valid] += 1
            placed[dd != 0] = 0
            run.reset_done()
            pair.run.reset_done()
            pair.compare(("reset_done", t))
            _same_states(pair, ("reset_done", t))
    finally:
        pair.run.close()
        run.close()
    assert all(met.values()), met
    assert oriented == {0, 1}, oriented


@pytest.mark.parametrize("variant", ["default", "stream", "incremental"])
@pytest.mark.parametrize("name,B", CASES)
def test_fused_sequence_across_two_resets(name, B, variant):
    """36 fused steps of episodes of 16 components: two resets, in the launch (default, streaming stores) or by reset_done()
    (PCBENV_FLAG_INCREMENTAL_OBS, where the arm must not be taken)."""
    cfg = named_config(name)
    inc = variant == "incremental"
    options = {"stream_threshold_bytes": 0} if variant == "stream" else {}
    kw = dict(incremental_obs=True) if inc else dict(auto_reset=True)
    run = Run(cfg, B, mask_marginals=True, options=dict(options, fixed_geometry=1), **kw)
    pair = Pair(cfg, B, fix=run.env, options=options, **kw)
    taken, fused_launch = [], run.env.rollout_step
    run.env.rollout_step = lambda t: taken.append(fused_launch(t)) or taken[-1]  # (Run.step keeps the actions to itself)
    terminal_launches = 0
    try:
        for t in range(36):
            dd = run.step(t, fused=True)
            x = pair.run.rollout_step(t)[-1]
            assert _same(taken[-1][-1], x), (("fused", t), "actions")
            pair.compare(("fused", t))
            _same_states(pair, ("fused", t))
            terminal_launches += bool(dd.any())
            if inc:
                run.reset_done()
                pair.run.reset_done()
                pair.compare(("reset_done", t))
    finally:
        pair.run.close()
        run.close()
    assert terminal_launches >= 2, terminal_launches


@pytest.mark.parametrize("auto_reset", [False, True])
@pytest.mark.parametrize("name,B", CASES)
def test_episode_ends_with_no_legal_cell_left(name, B, auto_reset):
    cfg = named_config(name)
    pair = Pair(cfg, B, auto_reset=auto_reset)
    victims = sorted({0, 3, B - 1})
    try:
        for t in range(3):
            pair.fused(t)
        acts = pair.fix.sample_actions(3)
        a = _np(acts)
        cur, ncomp, ch, cw = _components(pair.fix)
        assert (cur == 3).all() and (ncomp > 4).all()
        packed = np.packbits(_np(pair.fix.obs["grid"]), axis=-1, bitorder="little").reshape(B, H * 8)  # the occupancy rows of a state block
        for e in (pair.fix, pair.run):
            sd = e.state_dict()
            state = np.array(sd["state"]).reshape(B, -1)
            at = state[0].tobytes().find(packed[0].tobytes())
            assert at >= 0 and state[0].tobytes().find(packed[0].tobytes(), at + 1) < 0
            assert all(state[i, at:at + H * 8].tobytes() == packed[i].tobytes() for i in range(B))
            for i in victims:
                o, x, y = a[i]
                h, w = ch[i, 3], cw[i, 3]
                ph, pw = (w, h) if o & 1 else (h, w)
                full = np.ones((H, W), np.uint8)
                full[x:x + ph, y:y + pw] = 0  # legal now, so free now: the action fills the last free cells
                state[i, at:at + H * 8] = np.packbits(full, axis=-1, bitorder="little").ravel()
            sd["state"] = state.ravel()
            e.load_state_dict(sd)
        _same_states(pair, "edited")
        _fill_marker(pair, np.ones(B, bool))
        pair.both(lambda e: e.step(acts))
        pair.compare("step")
        _same_states(pair, "step")
        e = pair.fix
        done, info = _np(e.done), _np(e.info_raw)
        others = np.setdiff1d(np.arange(B), victims)
        assert (done[victims] == 1).all() and (done[others] == 0).all()
        assert (info[victims, 0] == cfg.max_wirelength).all() and (info[victims, 1] == cfg.max_num_intersections).all()  # the worst-case reward
        grid, mask = _np(e.obs["grid"]), _np(e.obs["action_mask"]).reshape(B, -1, H, W)
        for k in CELL_KEYS:
            if k in e.obs:
                assert int(_np(e.obs[k]).max()) <= 1, k  # no marker byte left anywhere
        if auto_reset:  # the reset has followed in the launch: an empty grid and the first component's mask
            assert not grid[victims].any() and mask[victims].any(axis=(1, 2, 3)).all()
        else:
            assert grid[victims].all() and not mask[victims].any()
        assert grid[others].any(axis=(1, 2)).all() and not grid[others].all(axis=(1, 2)).any()
    finally:
        pair.close()
