"""The process-wide switches (csrc/switches.hpp), without a GPU.

  * the library: each of the four setters the C ABI reaches, per value of its environment variable, in a process of its own, against
    the answers recorded before the switches moved into the header (tests/switch_pins.py PINNED);
  * the header: tests/switches_main.cpp, compiled with g++ against the very header the library includes, under the address and
    undefined-behaviour sanitizers, run once per value -- the same literals for those four rows, so the header cannot drift from the
    library, and the three rows no setter reaches (HEADER_ONLY)."""
import os
import struct
import subprocess

import pytest

import switch_pins as SP

CXX = os.environ.get("CXX", "g++")
CASES = [(n, v, want) for n, rows in SP.PINNED.items() for v, want in rows]


def test_the_table_covers_every_switch_and_value():
    for rows in list(SP.PINNED.values()) + list(SP.HEADER_ONLY.values()):
        assert [v for v, _ in rows] == SP.ENV_VALUES
    assert sorted(SP.PINNED) == sorted(SP.SETTERS) and len(CASES) == 32
    assert all(len(want) == 1 + len(SP.SEQUENCE) for _, _, want in CASES)


@pytest.mark.parametrize("name,value,want", CASES, ids=["%s-%s" % (n, "unset" if v is None else repr(v)) for n, v, _ in CASES])
def test_library_setter_answers_as_pinned(name, value, want):
    assert SP.answers(name, value) == want


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    """The program is stand-alone (its own main): linked with the sanitizers' runtimes, it needs no preload."""
    exe = str(tmp_path_factory.mktemp("switches") / "switches_san")
    subprocess.check_call([CXX, "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I", os.path.join(SP.ROOT, "gaussian-pcloud-render_amd", "csrc"),
                           os.path.join(SP.ROOT, "tests", "switches_main.cpp"), "-o", exe])
    return exe


def _f32(x):
    return struct.unpack("f", struct.pack("f", x))[0]


@pytest.mark.parametrize("i", range(len(SP.ENV_VALUES)), ids=["unset" if v is None else repr(v) for v in SP.ENV_VALUES])
def test_header_answers_as_the_library_did(program, i):
    value = SP.ENV_VALUES[i]
    e = {k: v for k, v in os.environ.items() if not k.startswith("GSR_")}
    if value is not None:
        e["GSR_TICKETS"] = value   # (read when the program is loaded: setenv in main would come too late)
    r = subprocess.run([program] + ([] if value is None else [value]), env=e, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    got = {ln.split()[0]: ln.split()[1:] for ln in r.stdout.splitlines()}
    for name, rows in SP.PINNED.items():
        assert rows[i][0] == value and [int(x) for x in got[name]] == rows[i][1], (name, value, got[name])
    only = {n: rows[i][1] for n, rows in SP.HEADER_ONLY.items()}
    t = only["block_tickets"]
    assert [int(x) for x in got["block_tickets"]] == [t]
    assert [int(x) for x in got["block_tickets_set"]] == [t, t, 0, 0, 1, 1, 1, 1, 1]   # set >= 0 stores set != 0
    assert _f32(float(got["tile_order_knee"][0])) == _f32(only["tile_order_knee"])   # (printed with 9 digits: a float32 round trip)
    assert _f32(float(got["tile_order_exp"][0])) == _f32(only["tile_order_exp"])
    assert got["tile_order_knee_again"] == got["tile_order_knee"]                       # read once
    assert [int(x) for x in got["contrib_lane_reduce"]] == [only["contrib_lane_reduce"], 1, 0]   # read at every call
    # (both arithmetic switches were left at 1 by the sequence) inference, inference channels, training, training channels
    assert got["forward_fast_math"] == ["1", "1", "1", "0"]
