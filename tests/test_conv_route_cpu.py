"""The conv routing rule (csrc/conv_cfg.h: conv_route / conv_route_multi / wgrad_route): which
kernel a launch runs on, for every cfg row and every combination of the rule's boolean inputs.

tests/native/conv_route.cpp prints the rule; the expected lines below are written out per id from
the documented behaviour (docs/KERNELS.md "Dispatch"), not computed from the function under test:
an igemm / v2 row runs its own tile, a specialised row its kernel where the geometry fits and
its fallback tile where it does not, res64 refuses what it does not fit, and no fallback is
taken with a fused pre-BN operand or the BN-backward reduction (RED) epilogue."""
import itertools
import shutil
import subprocess
from pathlib import Path

import pytest

HERE = Path(__file__).resolve().parent
REFUSE, LOOP = "refuse", "loop"
T64, T128 = -1, -2  # the fallback-only 256x64 / 256x128 igemm tiles

# ---- one geometry, no pre / red: id -> {fits: route}; a route is "family tile" or, where the
# tile depends on the column count, ("family tile @ 64 columns", "@ 128 columns").  60 (stem)
# also depends on ADD: {(fits, add): route}
PLAIN = {
    9: {0: "igemm 9", 1: "igemm 9"},
    10: {0: "igemm 10", 1: "igemm 10"},
    11: {0: "igemm 11", 1: "igemm 11"},
    12: {0: "igemm 12", 1: "igemm 12"},
    13: {0: "igemm 13", 1: "igemm 13"},
    14: {0: "igemm 14", 1: "igemm 14"},
    15: {0: "igemm 15", 1: "igemm 15"},
    16: {0: "igemm 16", 1: "igemm 16"},
    17: {0: "igemm 17", 1: "igemm 17"},
    39: {0: "igemm -1", 1: "halo 39"},
    41: {0: "igemm -1", 1: "halo 41"},
    42: {0: "igemm 12", 1: "halo 42"},
    60: {(0, 0): "igemm -1", (0, 1): "igemm -1", (1, 0): "stem 60", (1, 1): "igemm -1"},
    80: {0: REFUSE, 1: "res64 80"},
    90: {0: ("igemm -1", "igemm -2"), 1: "pipe 90"},
    91: {0: ("igemm -1", "igemm -2"), 1: "pipe 91"},
    92: {0: ("igemm -1", "igemm -2"), 1: "pipe 92"},
    93: {0: ("igemm -1", "igemm -2"), 1: "pipe 93"},
    T64: {0: "igemm -1", 1: "igemm -1"},
    T128: {0: "igemm -2", 1: "igemm -2"},
}
# ---- with a fused pre-BN operand (90-93 run on 41), with RED: id -> {fits: route}; ids not
# listed are refused either way.  pre and red together: always refused
PRE = {
    39: {0: REFUSE, 1: "halo 39"},
    41: {0: REFUSE, 1: "halo 41"},
    42: {0: REFUSE, 1: "halo 42"},
    80: {0: REFUSE, 1: "res64 80"},
    90: {0: REFUSE, 1: "halo 41"},
    91: {0: REFUSE, 1: "halo 41"},
    92: {0: REFUSE, 1: "halo 41"},
    93: {0: REFUSE, 1: "halo 41"},
}
RED = {
    42: {0: REFUSE, 1: "halo 42"},
    80: {0: REFUSE, 1: "res64 80"},
    90: {0: REFUSE, 1: "pipe 90"},
    91: {0: REFUSE, 1: "pipe 91"},
    92: {0: REFUSE, 1: "pipe 92"},
    93: {0: REFUSE, 1: "pipe 93"},
}
# ---- the parity classes of a stride-2 dgrad: id -> route of the single launch where it has one
# whatever seg2 / red say (the igemm tiles with the merged / RED variants); the pipelined tiles
# below; every other id has none: one launch per class, refused with seg2 or red
MULTI_ALWAYS = {11: "igemm 11", 12: "igemm 12", 13: "igemm 13", 14: "igemm 14", 15: "igemm 15",
                16: "igemm 16", 17: "igemm 17"}
# the pipelined tiles (90-93) and the ids without such a launch, per (fits_all, seg2,
# seg2_same_c, red); "pipe {}" = the one launch on the row's own tile
P = "pipe {}"
MULTI_PIPE = {
    (0, 0, 0, 0): LOOP, (0, 0, 0, 1): REFUSE, (0, 0, 1, 0): LOOP, (0, 0, 1, 1): REFUSE,
    (0, 1, 0, 0): REFUSE, (0, 1, 0, 1): REFUSE, (0, 1, 1, 0): REFUSE, (0, 1, 1, 1): REFUSE,
    (1, 0, 0, 0): P, (1, 0, 0, 1): P, (1, 0, 1, 0): P, (1, 0, 1, 1): P,
    (1, 1, 0, 0): REFUSE, (1, 1, 0, 1): REFUSE, (1, 1, 1, 0): P, (1, 1, 1, 1): P,
}
MULTI_NONE = {
    (0, 0, 0, 0): LOOP, (0, 0, 0, 1): REFUSE, (0, 0, 1, 0): LOOP, (0, 0, 1, 1): REFUSE,
    (0, 1, 0, 0): REFUSE, (0, 1, 0, 1): REFUSE, (0, 1, 1, 0): REFUSE, (0, 1, 1, 1): REFUSE,
    (1, 0, 0, 0): LOOP, (1, 0, 0, 1): REFUSE, (1, 0, 1, 0): LOOP, (1, 0, 1, 1): REFUSE,
    (1, 1, 0, 0): REFUSE, (1, 1, 0, 1): REFUSE, (1, 1, 1, 0): REFUSE, (1, 1, 1, 1): REFUSE,
}
# ---- weight gradient: id -> {(fits, pre): route}
WGRAD = {
    2: {(0, 0): "v2 2", (1, 0): "v2 2", (0, 1): REFUSE, (1, 1): REFUSE},
    3: {(0, 0): "v2 3", (1, 0): "v2 3", (0, 1): REFUSE, (1, 1): REFUSE},
    4: {(0, 0): ("v2 3", "v2 2"), (1, 0): "halo 4", (0, 1): REFUSE, (1, 1): "halo 4"},
    5: {(0, 0): ("v2 3", "v2 2"), (1, 0): "halo 5", (0, 1): REFUSE, (1, 1): "halo 5"},
    6: {(0, 0): "v2 6", (1, 0): "v2 6", (0, 1): REFUSE, (1, 1): REFUSE},
    7: {(0, 0): ("v2 3", "v2 2"), (1, 0): "s2 7", (0, 1): REFUSE, (1, 1): REFUSE},
    8: {(0, 0): REFUSE, (1, 0): "res64 8", (0, 1): REFUSE, (1, 1): "res64 8"},
}


def _at(route, ncols):
    return route if isinstance(route, str) else route[0 if ncols == 64 else 1]


def expected_lines():
    out = []
    bits = (0, 1)
    for cid, plain in PLAIN.items():
        for fits, add, pre, red, ncols in itertools.product(bits, bits, bits, bits, (64, 128)):
            if pre and red:
                r = REFUSE
            elif pre or red:
                r = (PRE if pre else RED).get(cid, {0: REFUSE, 1: REFUSE})[fits]
            else:
                r = _at(plain[(fits, add)] if (fits, add) in plain else plain[fits], ncols)
            out.append(f"conv {cid} fits={fits} add={add} pre={pre} red={red} ncols={ncols} : {r}")
        for fits, seg2, same, red in itertools.product(bits, bits, bits, bits):
            if cid in MULTI_ALWAYS:
                r = MULTI_ALWAYS[cid]
            elif cid in (90, 91, 92, 93):
                r = MULTI_PIPE[(fits, seg2, same, red)].format(cid)
            else:
                r = MULTI_NONE[(fits, seg2, same, red)]
            out.append(f"multi {cid} fits={fits} seg2={seg2} same={same} red={red} : {r}")
    for wid, routes in WGRAD.items():
        for fits, pre, ncols in itertools.product(bits, bits, (64, 128)):
            out.append(f"wgrad {wid} fits={fits} pre={pre} ncols={ncols} : "
                       f"{_at(routes[(fits, pre)], ncols)}")
    return out


@pytest.mark.skipif(shutil.which("g++") is None, reason="no host C++ compiler")
def test_route_tables(tmp_path):
    exe = tmp_path / "conv_route"
    subprocess.run(["g++", "-std=c++17", "-O1", str(HERE / "native" / "conv_route.cpp"), "-o",
                    str(exe)], check=True, capture_output=True, text=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stdout + r.stderr
    got = r.stdout.splitlines()
    assert got[-1] == "ok"
    want = expected_lines()
    assert len(want) == 20 * (32 + 16) + 7 * 8
    assert sorted(got[:-1]) == sorted(want), "\n".join(
        sorted(set(got[:-1]) ^ set(want))[:40])
