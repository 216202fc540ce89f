"""The balanced schedule of the pipelined conv, on the CPU: the planner (csrc/conv_pipe_plan.h)
through its stand-alone check tests/native/pipe_plan.cpp, and the preconditions under which the
integer-valued cases of tests/test_conv_pipe_balanced_gpu.py are exact."""
import shutil
import subprocess
from pathlib import Path

import pytest

import exact_conv as ec
import pipe_balanced_cases as pc

HERE = Path(__file__).resolve().parent
needs_cxx = pytest.mark.skipif(shutil.which("g++") is None, reason="no host C++ compiler")


def _run(tmp_path, flags):
    exe = tmp_path / "pipe_plan"
    subprocess.run(["g++", "-std=c++17", "-O1", *flags, str(HERE / "native" / "pipe_plan.cpp"), "-o",
                    str(exe)], check=True, capture_output=True, text=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.strip() == "ok", r.stdout + r.stderr


@needs_cxx
def test_planner_covers_every_step_once(tmp_path):
    """Sweep of (T, S, G) plus the real layer-3 / layer-4 shapes at G = 256: every (tile, K step)
    exactly once, at most two contributors per tile, the eligibility rule (q < S, T <= G,
    ng > 1, SEG2 refused) and the automatic choice on the real shapes."""
    _run(tmp_path, [])


@needs_cxx
def test_planner_asan_ubsan(tmp_path):
    _run(tmp_path, ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"])


def test_gpu_case_shapes():
    """The tile / K-step counts the GPU cases are written for."""
    assert pc.tiles_steps(pc.FWD, False) == (5, 36)
    assert pc.tiles_steps(pc.L4, True) == (8, 72)
    assert pc.tiles_steps(pc.ALIGNED, False) == (4, 36) and 4 * 36 % 2 == 0 and 4 * 36 // 2 % 36 == 0
    assert pc.tiles_steps(pc.ONE_TAP, False) == (5, 4)
    # G = 4 on 5 x 36 steps: the ranges end inside tiles 1, 2 and 3
    assert [45 * w // 36 for w in (1, 2, 3)] == [1, 2, 3] and all(45 * w % 36 for w in (1, 2, 3))


@pytest.mark.parametrize("geom", pc.ALL, ids=ec.geom_id)
def test_gpu_cases_are_exact(geom):
    """bf16 results are integers of magnitude <= 256 and every fp32 sum of |terms| is below
    2^24, so any accumulation order gives the float64 reference."""
    seen = ec.exact_preconditions(ec.int_case(geom))
    assert seen["y"] > 0 and seen["dx"] > 0
