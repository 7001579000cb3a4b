"""The host/kernel layout contract (csrc/pcb_layout.h) on the CPU: tools/layout_check.cpp sweeps the geometry and
asserts that every state-block and LDS zone, the feature cache and the terminal-list counters hold what their users
index.  Built with AddressSanitizer + UBSan as a stand-alone program; nothing is loaded into this process."""
import os
import shutil
import subprocess

import pytest

import model_harness

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.skipif(shutil.which("g++") is None, reason="no g++")
def test_layout_check_program():
    exe = model_harness.tool("layout_check", include=True, fp_contract_off=False, frame_pointer=True)
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0, run.stdout + run.stderr
    assert run.stdout.startswith("layout_check ok:"), run.stdout
