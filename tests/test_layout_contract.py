"""The host/kernel layout contract (csrc/pcb_layout.h) on the CPU: tools/layout_check.cpp sweeps the geometry and
asserts that every state-block and LDS zone, the feature cache and the terminal-list counters hold what their users
index.  Built with AddressSanitizer + UBSan as a stand-alone program; nothing is loaded into this process."""
import os
import shutil
import subprocess

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.skipif(shutil.which("g++") is None, reason="no g++")
def test_layout_check_program(tmp_path):
    exe = str(tmp_path / "layout_check")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-I", os.path.join(REPO, "include"),
                    "-I", os.path.join(REPO, "rl-environment-for-component-placement_amd", "csrc"),
                    "-o", exe, os.path.join(REPO, "tools", "layout_check.cpp")], check=True)
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0, run.stdout + run.stderr
    assert run.stdout.startswith("layout_check ok:"), run.stdout
