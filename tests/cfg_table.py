"""The conv kernel config tables (csrc/conv_cfg.h) as the native program
tests/native/cfg_table.cpp prints them: built with plain g++ once per session."""
import functools
import shutil
import subprocess
import tempfile
from pathlib import Path

import pytest

HERE = Path(__file__).resolve().parent


def _value(v):
    return int(v) if v.lstrip("-").isdigit() else v


@functools.lru_cache(maxsize=None)
def _lines():
    tmp = Path(tempfile.mkdtemp(prefix="cfg_table_"))
    try:
        exe = tmp / "cfg_table"
        subprocess.run(["g++", "-std=c++17", "-O1", str(HERE / "native" / "cfg_table.cpp"), "-o",
                        str(exe)], check=True, capture_output=True, text=True)
        r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=60)
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
    assert r.returncode == 0 and r.stdout.split("\n")[-2] == "ok", r.stdout + r.stderr
    return r.stdout.splitlines()[:-1]


def records():
    """({id: record}, {id: record}) of the forward-style and the weight-gradient table, each
    record a dict of the printed ``key=value`` pairs (ints, ``family`` a string)."""
    if shutil.which("g++") is None:
        pytest.skip("no host C++ compiler")
    out = {"fwd": {}, "wgrad": {}, "tile": {}}
    for line in _lines():
        kind, *pairs = line.split()
        rec = {k: _value(v) for k, v in (p.split("=") for p in pairs)}
        out[kind][rec["id"]] = rec
    return out["fwd"], out["wgrad"]
