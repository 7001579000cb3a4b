"""The register forms of the geometry-fixed step builds' plain transition (csrc/pcb_transition.h: a lane's occupancy row
after update_grid as an expression of its old row and the action, and the legal-mask window folded from rows held as
values) on the CPU: tools/step_dataflow_check.cpp compiles the header the kernels compile and checks both against
occupy_row and the window's definition.  Built with AddressSanitizer + UBSan as a stand-alone program; nothing is loaded
into this process."""
import re
import shutil
import subprocess

import pytest

import model_harness

N = 64                        # the fixed geometry: H = W = lanes of a wavefront
MAX_PINS_PER_COMPONENT = 64   # PCBENV_MAX_PINS_PER_COMPONENT
RANDOM_ROWS = 320             # old rows of the random part of the update sweep, 64 to a grid
GRIDS = 60
# windows beyond what a pin kind's component can be: the whole grid, one row, one column, the largest square that leaves
# a second one no room, and the two that leave one row or column
EXTRA_WINDOWS = ((64, 64), (64, 1), (1, 64), (33, 33), (63, 2), (2, 63))


@pytest.mark.skipif(shutil.which("g++") is None, reason="no g++")
def test_step_dataflow_check_program():
    exe = model_harness.tool("step_dataflow_check", include=True)
    lines = [f"U {RANDOM_ROWS} 7",
             f"F {GRIDS} 11 {len(EXTRA_WINDOWS)} " + " ".join(f"{h} {w}" for h, w in EXTRA_WINDOWS)]
    run = subprocess.run([exe], input="\n".join(lines) + "\n", capture_output=True, text=True)
    assert run.returncode == 0, run.stdout + run.stderr
    assert run.stderr == "", run.stderr
    found = re.match(r"step_dataflow_check ok: (\d+) rows after an update, (\d+) window folds \((\d+) with equal sides, "
                     r"(\d+) with no legal cell left\)", run.stdout)
    assert found, run.stdout
    print(run.stdout.strip())
    rows, folds, equal_sides, no_legal_cell = (int(g) for g in found.groups())
    rectangles = (N * (N + 1) // 2) ** 2  # (x, ph) times (y, pw) with the rectangle inside the grid
    assert rows == N * (2 * rectangles + RANDOM_ROWS // N * (N * (N + 1) // 2))  # nothing skipped: empty and full, then the random grids
    windows = [(h, w) for h in range(1, N + 1) for w in range(1, N + 1) if h * w <= MAX_PINS_PER_COMPONENT] + list(EXTRA_WINDOWS)
    assert folds == GRIDS * len(windows)
    assert equal_sides == GRIDS * sum(h == w for h, w in windows)
    assert 0 < no_legal_cell < folds  # windows that fit somewhere and windows that fit nowhere were both met
