"""The per-axis legal set of the factorised policies (csrc/pcb_axis_set.h) on the CPU: tools/axis_set_check.cpp compiles
the header the axis kernels compile and compares it with a brute-force scan of the dense mask, for every (axis, given)
pair, valid and out-of-range given values, on the mask classes of tests/logits_cases.py and their dirty twins.  Built
with AddressSanitizer + UBSan as a stand-alone program; nothing is loaded into this process."""
import os
import re
import subprocess

import numpy as np

import logits_cases as lc
import model_harness
from pcbenv.config import KIND_PIN, KIND_RECT, KIND_SQUARE

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GEOMETRIES = [(1, 8, 8), (2, 6, 6), (4, 10, 10), (4, 16, 64), (4, 5, 128), (2, 33, 65), (4, 100, 9), (2, 128, 36), (1, 3, 128)]
KIND_OF = {1: KIND_SQUARE, 2: KIND_RECT, 4: KIND_PIN}


def _rows_text():
    lines, rows = [], 0
    for O, H, W in GEOMETRIES:
        rng = np.random.RandomState(O * 100000 + H * 1000 + W)
        kind = KIND_OF[O]
        clean = np.concatenate([b for _, b, _ in lc.mask_classes(kind, O, H, W, rng)])
        dirty = lc.dirty_twin(clean, kind, W, rng).view(np.uint64)
        if W % 64 or kind == KIND_SQUARE:
            assert not np.array_equal(clean, dirty)
        lines.append(f"G {O} {H} {W} {len(clean)}")
        for c, d in zip(clean, dirty):
            lines.append(" ".join(f"{int(w):x}" for w in c.reshape(-1)))
            lines.append(" ".join(f"{int(w):x}" for w in d.reshape(-1)))
        rows += len(clean)
    return "\n".join(lines) + "\n", rows


def test_axis_set_check_program():
    exe = model_harness.tool("axis_set_check", include=True)
    text, rows = _rows_text()
    run = subprocess.run([exe], input=text, capture_output=True, text=True)
    assert run.returncode == 0, run.stdout + run.stderr
    assert run.stderr == "", run.stderr
    found = re.match(r"axis_set_check ok: (\d+) geometries, (\d+) rows, (\d+) queries", run.stdout)
    assert found, run.stdout
    assert int(found.group(1)) == len(GEOMETRIES) and int(found.group(2)) == rows
    assert int(found.group(3)) > 12 * rows
