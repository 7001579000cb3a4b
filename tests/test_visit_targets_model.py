"""csrc/pcb_visit_targets.h -- which entries of a row's visit target are valid, their total, the weight of an entry and of
a logit several entries name, as plain C++ -- against tests/visits_contract.py:target_rows on the CPU:
tools/visit_targets_check.cpp (AddressSanitizer + UBSan, a program of its own, nothing preloaded) reduces a table of rows
in both action formats with C = 1 and 64 and returns every index, kept visit count, weight and bit, which must be the contract's, floats by
their bits.  tests/test_evaluate_visits_gpu.py then holds the kernels, which compile the same header, to the contract."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import model_harness
import visits_cases as vc
import visits_contract as vt
from logits_cases import _pack

pytestmark = pytest.mark.skipif(shutil.which("g++") is None, reason="no g++")

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GEOMETRIES = ((1, 3, 128), (2, 9, 70), (4, 6, 10))  # two full words; a ragged second word; planes shared by orientations 2 and 3


@pytest.fixture(scope="module")
def program():
    return model_harness.tool("visit_targets_check", include=True)


def _table(O, H, W, C, seed):
    """Rows drawn from the legal set, then damaged: duplicates, zero and negative visits, illegal and out-of-range
    actions, no visits at all, no legal action, visits near INT32_MAX (T needs 64 bits)."""
    rng = np.random.RandomState(seed)
    N, A = 14, O * H * W
    cells, legal = vc.planes_legal(rng, O, H, W, N)
    visits, idx = vc.draw_targets(rng, legal, C)
    idx[0, :] = idx[0, 0]
    visits[1, 0] = 0
    visits[2, 0] = -1
    idx[3, C - 1], visits[3, C - 1] = np.flatnonzero(~legal[3])[0], 4
    idx[4, 0], visits[4, 0] = A, 3
    idx[5, 0], visits[5, 0] = -1, 3
    visits[6] = 0
    cells[7], legal[7] = False, False
    visits[8] = np.int32(2 ** 31 - 1)
    idx[9, 0], visits[9, 0] = A + 7, 0  # out of range but unvisited: silent
    return cells, legal, visits, idx


def _run(program, O, H, W, fmt, C, cells, visits, actions):
    N = len(visits)
    bits = _pack(cells).view(np.int64).reshape(N, -1)
    body = np.concatenate([bits, visits.astype(np.int64), actions.astype(np.int64).reshape(N, -1)], axis=1)
    words = np.concatenate([np.array([O, H, W, 1 if fmt == "flat" else 0, C, N], np.int64), body.ravel()])
    done = subprocess.run([program], input=words.tobytes(), capture_output=True)
    assert done.returncode == 0 and done.stderr == b"", done.stderr.decode()
    out = np.frombuffer(done.stdout, np.int64).reshape(N, 2 + 3 * C)
    f32 = lambda w: w.astype(np.uint32).view(np.float32)
    return out[:, 0], out[:, 1], out[:, 2:2 + C], out[:, 2 + C:2 + 2 * C], f32(out[:, 2 + 2 * C:])


@pytest.mark.parametrize("fmt", ["tuple", "flat"])
@pytest.mark.parametrize("C", [1, 64])
@pytest.mark.parametrize("geometry", GEOMETRIES, ids=lambda g: "x".join(map(str, g)))
def test_the_header_is_the_contract(program, geometry, C, fmt):
    O, H, W = geometry
    cells, legal, visits, idx = _table(O, H, W, C, seed=C + W)
    actions = vc.as_actions(idx, H, W, fmt)
    if fmt == "tuple":  # ranges of the single coordinates
        actions[10, 0] = [0, H, 0]
        actions[11, 0] = [0, 0, W]
        actions[12, 0] = [O, 0, 0]
        actions[13, 0] = [0, -1, 0]
        visits[10:14, 0] = 5
    fi, in_range = vt.flat_targets(actions, O, H, W)
    want_index, want_kept, want_pi, want_T, want_bad = vt.target_rows(legal, visits, fi, in_range)
    bits, T, index, kept, pi = _run(program, O, H, W, fmt, C, cells, visits, actions)
    assert np.array_equal(index, want_index) and np.array_equal(kept, want_kept)
    assert np.array_equal(T, want_T)
    assert np.array_equal(bits, np.where(want_bad, vt.ERR_TARGET, 0))
    assert np.array_equal(pi.view(np.uint32), want_pi.view(np.uint32))  # one division in float64, rounded once
    # what the rows are there for
    assert want_bad[2] and want_bad[4] and want_bad[5] and not want_bad[1] and not want_bad[6] and not want_bad[9]
    assert want_T[6] == 0 and want_T[7] == 0 and want_bad[7]  # (a row without a legal action: the kernels never ask)
    if C == 64:
        assert want_T[8] > 2 ** 32 and want_bad[3] and (np.bincount(want_index[0][want_index[0] >= 0]).max() > 1)
    if fmt == "tuple":
        assert want_bad[10:14].all()
