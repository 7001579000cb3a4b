"""The predicate that chooses the geometry-fixed build of the step kernel (csrc/pcb_layout.h fixed_geometry_applies) on
the CPU: tools/fixed_geometry_check.cpp asserts that the 64 x 64 pin and spatial kinds on one wavefront, in place, select
it and that every near miss does not.  Built with AddressSanitizer + UBSan as a stand-alone program; nothing is loaded
into this process."""
import os
import shutil
import subprocess

import pytest

import model_harness

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.skipif(shutil.which("g++") is None, reason="no g++")
def test_fixed_geometry_check_program():
    exe = model_harness.tool("fixed_geometry_check", include=True, fp_contract_off=False, frame_pointer=True)
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0, run.stdout + run.stderr
    assert run.stdout.startswith("fixed_geometry_check ok:"), run.stdout
