"""The two scalar models the step kernel carries for the reference's traps -- CPython's set iteration order
(csrc/pcb_setmodel.h) and the hoisted intersection test with its integer extent pre-filter (csrc/pcb_geometry.h) -- on
the CPU: tools/kernel_models_check.cpp compiles the headers the kernels compile and checks them against the recorded
orders of tests/golden/setorder.npz, against live sets when this interpreter has the reference's set implementation,
and against the reference's own intersection formula.  Built with AddressSanitizer + UBSan as a stand-alone program;
nothing is loaded into this process."""
import os
import random
import re
import shutil
import subprocess
import sys

import numpy as np
import pytest

import model_harness

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _order_line(pts, vis_idx, order):
    flat = " ".join(f"{x} {y}" for x, y in pts)
    return f"S {len(pts)} {flat} {sum(1 << i for i in vis_idx)} {len(order)} " + " ".join(str(i) for i in order)


def _live_orders(count):
    """Orders of real sets, built as make_golden.record_setorder builds them, biased to <= 4 points left (the fast path)."""
    rng = random.Random(23)
    lines = []
    for _ in range(count):
        n = rng.randrange(1, 16)
        side = rng.choice([6, 10, 64, 128])
        pts = []
        while len(pts) < n:
            p = (rng.randrange(side), rng.randrange(side))
            if p not in pts:
                pts.append(p)
        k = max(0, n - rng.randrange(0, 5)) if rng.random() < 0.7 else rng.randrange(0, n + 1)
        vis_idx = rng.sample(range(n), k)
        visited = set()
        for i in vis_idx:  # built like beam_search does: visited | {neighbor}
            visited = visited | {pts[i]}
        lines.append(_order_line(pts, vis_idx, [pts.index(p) for p in set(pts) - visited]))
    return lines


@pytest.mark.skipif(shutil.which("g++") is None, reason="no g++")
def test_kernel_models_check_program():
    exe = model_harness.tool("kernel_models_check", include=True, more_checks=",float-cast-overflow")
    z = np.load(os.path.join(REPO, "tests", "golden", "setorder.npz"))
    lines = [f"H {int(x)} {int(y)} {int(h)}" for x, y, h in z["tuple_hash"]]
    for pts, mask, order in zip(z["points"], z["visited_mask"], z["order"]):
        n = int((pts[:, 0] >= 0).sum())
        lines.append(_order_line([(int(x), int(y)) for x, y in pts[:n]], [i for i in range(n) if int(mask) >> i & 1],
                                 [int(i) for i in order if i >= 0]))
    if sys.implementation.name == "cpython" and (3, 8) <= sys.version_info[:2] <= (3, 11):
        lines += _live_orders(20000)
    lines.append("G 1 2000000")
    run = subprocess.run([exe], input="\n".join(lines) + "\n", capture_output=True, text=True)
    assert run.returncode == 0, run.stdout + run.stderr
    assert run.stderr == "", run.stderr
    found = re.match(r"kernel_models_check ok: (\d+) tuple hashes, (\d+) set orders \((\d+) on the fast path\), (\d+) segment pairs", run.stdout)
    assert found, run.stdout
    hashes, orders, fast, pairs = (int(g) for g in found.groups())
    assert hashes == len(z["tuple_hash"]) and orders == len(lines) - 1 - hashes and pairs == 2000000
    assert fast > 0
