"""The scalar core of a transition (csrc/pcb_transition.h: action code, validate_action, update_grid, place_component with
its inverse, cursor and done) on the CPU: tools/transition_check.cpp compiles the header the kernels compile and replays
every recorded reference transition of tests/golden through it, with the lane strides of both team sizes, then runs
sweeps that need no recording.  Built with AddressSanitizer + UBSan as a stand-alone program; nothing is loaded into this
process."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import model_harness
from golden_util import case_names, load_case

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KIND = {"square": 0, "rect": 1, "pin": 2, "spatial": 3}
FILL_WIDTHS = (1, 63, 64, 65, 127, 128)
MAX_PINS_PER_COMPONENT = 64  # PCBENV_MAX_PINS_PER_COMPONENT


def _bit_rows(cells):
    """[..., W] cells of 0 / 1 -> the hexadecimal 64-bit words of the bit rows (bit b of word w = column 64 w + b)."""
    cells = np.asarray(cells) != 0
    ww = (cells.shape[-1] + 63) // 64
    padded = np.zeros(cells.shape[:-1] + (64 * ww,), np.uint8)
    padded[..., :cells.shape[-1]] = cells
    words = np.packbits(padded, axis=-1, bitorder="little").reshape(-1, 8).view("<u8").ravel()
    return " ".join(f"{int(w):x}" for w in words)


def _transition_lines():
    """One T line per recorded transition -> (lines, invalid transitions, pin rows, geometries)."""
    lines, invalid, pin_rows, geometries = [], 0, 0, set()
    for name in case_names():
        meta, cfg, episodes = load_case(name)
        kind, H, W = KIND[meta["kind"]], cfg.height, cfg.width
        for ep in episodes:
            grid, mask = ep.obs["grid"], ep.obs["action_mask"]
            if mask.ndim == 3:  # the square kind has no orientation axis
                mask = mask[:, None]
            O = mask.shape[1]
            geometries.add((O, H, W))
            assert len(grid) == len(ep.actions) + 1
            inst = ep.instance
            ncomp = 0 if inst is None else inst.num_components
            placed = 0  # valid transitions so far: the recording goes on past an invalid action, which changes nothing
            for t, action in enumerate(ep.actions):
                o, x, y = (int(v) for v in action)
                cur = 0 if kind == 0 else placed if placed < ncomp else -1
                ch, cw = (cfg.component_n,) * 2 if kind == 0 else (int(inst.comp_h[cur]), int(inst.comp_w[cur])) if cur >= 0 else (0, 0)
                pins = [] if kind < 2 else list(range(inst.num_pins))  # all of them: the pin loop picks the component's
                mine = [q for q in pins if int(inst.pin_comp[q]) == cur]
                # what the reference did: a valid action occupies at least one free cell, an invalid one leaves the grid alone
                valid = not np.array_equal(grid[t + 1], grid[t])
                invalid += not valid
                placed += valid
                planes = np.zeros((2, H, W))
                planes[:min(2, O)] = mask[t][:2]
                f = [kind, H, W, O, cfg.component_n, cur, ncomp, ch, cw, len(pins)]
                for q in pins:
                    f += [int(inst.pin_rel_x[q]), int(inst.pin_rel_y[q]), int(inst.pin_comp[q])]
                in_range = 0 <= o < O and 0 <= x < H and 0 <= y < W
                f += [o, x, y, (o * H + x) * W + y if in_range else -1, int(valid), int(mask[t + 1].any()), int(ep.done[t])]
                line = "T " + " ".join(str(v) for v in f) + " " + " ".join((_bit_rows(grid[t]), _bit_rows(planes), _bit_rows(grid[t + 1])))
                if kind == 3 and valid:
                    rows = ep.obs["all_pins_num_feature"][t + 1]
                    for q in mine:
                        line += " " + " ".join(str(int(v)) for v in rows[int(inst.pin_id[q])])
                    pin_rows += len(mine)
                lines.append(line)
    return lines, invalid, pin_rows, sorted(geometries)


@pytest.mark.skipif(shutil.which("g++") is None, reason="no g++")
def test_transition_check_program():
    exe = model_harness.tool("transition_check", include=True)
    lines, invalid, pin_rows, geometries = _transition_lines()
    transitions = len(lines)
    assert transitions > 0 and invalid > 0 and pin_rows > 0
    lines += [f"C {O} {H} {W}" for O, H, W in geometries] + [f"R {W}" for W in FILL_WIDTHS] + ["P"]
    run = subprocess.run([exe], input="\n".join(lines) + "\n", capture_output=True, text=True)
    assert run.returncode == 0, run.stdout + run.stderr
    assert run.stderr == "", run.stderr
    found = re.match(r"transition_check ok: (\d+) transitions \((\d+) invalid\), (\d+) pin rows, (\d+) action codes, (\d+) row fills, "
                     r"(\d+) rotations", run.stdout)
    assert found, run.stdout
    print(run.stdout.strip())
    got = tuple(int(g) for g in found.groups())
    codes = sum(O * H * W + 4 for O, H, W in geometries)
    fills = sum((W + 1) * (W + 2) // 2 for W in FILL_WIDTHS)  # y in [0, W], pw in [0, W - y]
    rotations = sum(4 * h * w for h in range(1, MAX_PINS_PER_COMPONENT + 1) for w in range(1, MAX_PINS_PER_COMPONENT // h + 1))
    assert got == (transitions, invalid, pin_rows, codes, fills, rotations)  # nothing skipped
