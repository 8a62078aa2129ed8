"""The pin of the process-wide switches' parsing (csrc/switches.hpp): what each of the four setters the C ABI reaches answers, per value
of its environment variable, in a process of its own.  Importable without torch, the built library or a device.

  SETTERS / ENV_VALUES / SEQUENCE   the switches (name -> setter symbol, variable), the values of the variable (None: unset) and the
                                    setter calls every child makes
  answers                           runs the child: [setter(-1)] + [setter(s) for s in SEQUENCE], from a fresh load of the library
  PINNED                            name -> [[value, answers], ...]: what the library answered BEFORE the switches moved into
                                    switches.hpp (profiles/r22_native_layout.txt has the provenance); tests/test_cpu_switches.py holds
                                    the library and, through tests/switches_main.cpp, the header to it

`python tests/switch_pins.py` prints the table of the library GSR_LIB names (default: the tree's)."""
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.environ.get("GSR_LIB") or os.path.join(ROOT, "gaussian-pcloud-render_amd", "diff_gaussian_rasterization", "libgsr_hip.so")

SETTERS = {
    "forward_half_views": ("gsr_set_forward_half_views", "GSR_FWD_HALF_V"),
    "backward_subquadrant_moments": ("gsr_set_backward_moments", "GSR_BWD_SUBQ"),
    "render_math": ("gsr_set_render_math", "GSR_RENDER_MATH"),
    "train_math": ("gsr_set_train_math", "GSR_TRAIN_MATH"),
}
ENV_VALUES = [None, "", "0", "1", "2", "3", "-1", "abc"]
SEQUENCE = (-1, 0, -7, 1, 2, 3, 255, -1)

_CHILD = ("import ctypes, sys; f = getattr(ctypes.CDLL(sys.argv[1]), sys.argv[2]); "
          "print(' '.join(str(f(s)) for s in (-1,) + %r))" % (SEQUENCE,))


def answers(name, value, lib=LIB):
    symbol, var = SETTERS[name]
    e = {k: v for k, v in os.environ.items() if k not in [s[1] for s in SETTERS.values()]}
    if value is not None:
        e[var] = value
    out = subprocess.run([sys.executable, "-c", _CHILD, lib, symbol], env=e, capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr
    return [int(x) for x in out.stdout.split()]


PINNED = {
    'forward_half_views': [
        [None, [1, 1, 0, 0, 1, 2, 3, 255, 255]],
        ['', [0, 0, 0, 0, 1, 2, 3, 255, 255]],
        ['0', [0, 0, 0, 0, 1, 2, 3, 255, 255]],
        ['1', [1, 1, 0, 0, 1, 2, 3, 255, 255]],
        ['2', [2, 2, 0, 0, 1, 2, 3, 255, 255]],
        ['3', [3, 3, 0, 0, 1, 2, 3, 255, 255]],
        ['-1', [0, 0, 0, 0, 1, 2, 3, 255, 255]],
        ['abc', [0, 0, 0, 0, 1, 2, 3, 255, 255]],
    ],
    'backward_subquadrant_moments': [
        [None, [2, 2, 0, 0, 1, 2, 2, 2, 2]],
        ['', [0, 0, 0, 0, 1, 2, 2, 2, 2]],
        ['0', [0, 0, 0, 0, 1, 2, 2, 2, 2]],
        ['1', [1, 1, 0, 0, 1, 2, 2, 2, 2]],
        ['2', [2, 2, 0, 0, 1, 2, 2, 2, 2]],
        ['3', [2, 2, 0, 0, 1, 2, 2, 2, 2]],
        ['-1', [2, 2, 0, 0, 1, 2, 2, 2, 2]],
        ['abc', [0, 0, 0, 0, 1, 2, 2, 2, 2]],
    ],
    'render_math': [
        [None, [0, 0, 0, 0, 1, 1, 1, 1, 1]],
        ['', [0, 0, 0, 0, 1, 1, 1, 1, 1]],
        ['0', [0, 0, 0, 0, 1, 1, 1, 1, 1]],
        ['1', [1, 1, 0, 0, 1, 1, 1, 1, 1]],
        ['2', [0, 0, 0, 0, 1, 1, 1, 1, 1]],
        ['3', [0, 0, 0, 0, 1, 1, 1, 1, 1]],
        ['-1', [0, 0, 0, 0, 1, 1, 1, 1, 1]],
        ['abc', [0, 0, 0, 0, 1, 1, 1, 1, 1]],
    ],
    'train_math': [
        [None, [0, 0, 0, 0, 1, 1, 1, 1, 1]],
        ['', [0, 0, 0, 0, 1, 1, 1, 1, 1]],
        ['0', [0, 0, 0, 0, 1, 1, 1, 1, 1]],
        ['1', [1, 1, 0, 0, 1, 1, 1, 1, 1]],
        ['2', [0, 0, 0, 0, 1, 1, 1, 1, 1]],
        ['3', [0, 0, 0, 0, 1, 1, 1, 1, 1]],
        ['-1', [0, 0, 0, 0, 1, 1, 1, 1, 1]],
        ['abc', [0, 0, 0, 0, 1, 1, 1, 1, 1]],
    ],
}

# The three rows no setter of the C ABI reaches, as csrc/ read them before they moved (worked out from that text, not recorded from a
# run): the pair emission's numbering is 0 iff GSR_TICKETS is set and atoi gives 0; the tile order's knee and exponent are atof of the
# variable, 2048 and 0.3 unset; the contribution walk reduces by lanes iff atoi(GSR_CONTRIB_REDUCE) is 1.
HEADER_ONLY = {
    'block_tickets': [[None, 1], ['', 0], ['0', 0], ['1', 1], ['2', 1], ['3', 1], ['-1', 1], ['abc', 0]],
    'tile_order_knee': [[None, 2048.0], ['', 0.0], ['0', 0.0], ['1', 1.0], ['2', 2.0], ['3', 3.0], ['-1', -1.0], ['abc', 0.0]],
    'tile_order_exp': [[None, 0.3], ['', 0.0], ['0', 0.0], ['1', 1.0], ['2', 2.0], ['3', 3.0], ['-1', -1.0], ['abc', 0.0]],
    'contrib_lane_reduce': [[None, 0], ['', 0], ['0', 0], ['1', 1], ['2', 0], ['3', 0], ['-1', 0], ['abc', 0]],
}


if __name__ == "__main__":
    print("PINNED = {")
    for n in SETTERS:
        print("    %r: [" % n)
        for v in ENV_VALUES:
            print("        [%r, %r]," % (v, answers(n, v)))
        print("    ],")
    print("}")
