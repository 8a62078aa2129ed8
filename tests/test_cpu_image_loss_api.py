"""The photometric-loss entries (include/gsr.h gsr_image_loss_state_bytes / _forward / _backward) as far as they can be reached
without a GPU: the exported symbols, the size query, the refusals that precede any HIP call, in their order, and the Python side's
refusal of CPU tensors."""
import ctypes
import inspect
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
A, B, Cc, D, E = 0x1000, 0x2000, 0x3000, 0x4000, 0x5000   # stand-ins for device arrays (never followed)
SYMS = ("gsr_image_loss_state_bytes", "gsr_image_loss_forward", "gsr_image_loss_backward")
INVALID, CAPACITY = -1, -3


def _native():
    from diff_gaussian_rasterization import _native as N
    return N


def test_symbols_are_exported_declared_and_bound():
    N = _native()
    lib = ctypes.CDLL(N.LIB_PATH)
    text = open(os.path.join(ROOT, "include", "gsr.h")).read()
    header = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    names = {}
    for sym in SYMS:
        assert hasattr(lib, sym) and sym in N.SYMBOLS and sym in N._DECL, sym
        m = re.search(r"\b(?:int|size_t)\s+%s\s*\(([^)]*)\)" % sym, header)
        assert m, "include/gsr.h does not declare %s" % sym
        names[sym] = [a.strip().split()[-1].lstrip("*") for a in m.group(1).split(",")]
        assert len(names[sym]) == len(N._DECL[sym][1]), sym
    assert names[SYMS[0]] == ["V", "W", "H"] and N._DECL[SYMS[0]][0] is ctypes.c_size_t
    assert names[SYMS[1]] == ["V", "W", "H", "ss", "lambda_dssim", "image", "target", "loss_terms", "state", "state_bytes", "stream"]
    assert names[SYMS[2]] == ["V", "W", "H", "ss", "lambda_dssim", "image", "target", "dL_dloss", "state", "state_bytes", "dL_dimage",
                              "stream"]
    assert N._DECL[SYMS[1]][1][4] is ctypes.c_float and N._DECL[SYMS[2]][1][4] is ctypes.c_float
    # the header states the contract: whose duty the forward-before-backward order is, and what makes the outputs reproducible
    doc = text[text.index("Photometric loss of the rendered frames"):text.index("size_t gsr_image_loss_state_bytes")]
    for phrase in ("CALLER'S duty", "No float atomics", "bit-identical", "metrics only", "GSR_ERR_CAPACITY", "never approximated"):
        assert phrase in doc, phrase
    assert list(inspect.signature(N.image_loss_forward).parameters) == ["image", "target", "lambda_dssim", "super_sample", "state"]
    assert list(inspect.signature(N.image_loss_backward).parameters) == ["image", "target", "lambda_dssim", "super_sample", "state",
                                                                         "dL_dloss", "out"]
    from pcrender import losses
    assert list(inspect.signature(losses.photometric_loss).parameters) == ["image", "target", "lambda_dssim", "super_sample"]
    assert list(inspect.signature(losses.image_metrics).parameters) == ["image", "target", "super_sample"]
    assert "image_loss" in open(os.path.join(ROOT, "gaussian-pcloud-render_amd", "build.py")).read()


def test_size_query_is_a_multiple_of_256_monotone_and_zero_for_refused_sizes():
    q = _native().lib.gsr_image_loss_state_bytes
    Vs, Ws, Hs = (1, 2, 3, 12, 256), (1, 5, 31, 32, 33, 64, 100, 1920), (1, 7, 32, 33, 48, 1080)
    size = {(V, W, H): q(V, W, H) for V in Vs for W in Ws for H in Hs}
    for (V, W, H), n in size.items():
        assert n > 0 and n % 256 == 0, (V, W, H, n)
        assert n >= 36 * V * W * H                                     # the three maps of three channels
    for seq, key in ((Vs, lambda s: (s, 100, 48)), (Ws, lambda s: (12, s, 48)), (Hs, lambda s: (12, 100, s))):
        vals = [size[key(s)] for s in seq]
        assert vals == sorted(vals), vals
    for (V, W, H), n in size.items():                                  # ... and in every argument, everywhere on the grid
        for (V2, W2, H2), n2 in size.items():
            if V2 >= V and W2 >= W and H2 >= H:
                assert n2 >= n
    for bad in ((0, 8, 8), (-1, 8, 8), (257, 8, 8), (1, 0, 8), (1, 8, 0), (1, -3, 8), (1, 1 << 16, 1 << 16), (256, 4096, 1024),
                (1, 2147483647, 2147483647)):
        assert q(*bad) == 0, bad
    assert q(1, 26754, 26754) > 0 and q(1, 26755, 26755) == 0          # 3 W H on either side of 2^31


def _entries():
    N = _native()

    def fwd(V=1, W=8, H=8, ss=1, lam=0.2, image=A, target=B, terms=Cc, state=D, state_bytes=1 << 40):
        return N.lib.gsr_image_loss_forward(V, W, H, ss, lam, image, target, terms, state, state_bytes, None), N.lib.gsr_last_error()

    def bwd(V=1, W=8, H=8, ss=1, lam=0.2, image=A, target=B, terms=Cc, state=D, state_bytes=1 << 40, dL=None):
        return (N.lib.gsr_image_loss_backward(V, W, H, ss, lam, image, target, dL, state, state_bytes, terms, None),
                N.lib.gsr_last_error())

    return N, (("image_loss_forward", fwd), ("image_loss_backward", bwd))


def test_refusals_before_any_hip_call_in_their_order():
    N, entries = _entries()
    nan = float("nan")
    for who, call in entries:
        tag = who.encode()
        # 1. the view count, whatever else is wrong
        for V in (0, -1, 257):
            rc, err = call(V=V, W=0, ss=3, lam=nan, image=None, state_bytes=0)
            assert rc == INVALID and tag in err and b"view count" in err, (who, V, err)
        # 2. the sizes, before the rate, lambda and the pointers
        for kw in (dict(W=0), dict(H=0), dict(W=-5), dict(W=26755, H=26755), dict(V=256, W=4096, H=1024), dict(W=16384, H=16384, ss=2),
                   dict(W=8, H=8, ss=60000), dict(W=2147483647, H=2147483647)):
            rc, err = call(**dict(dict(ss=3 if "ss" not in kw else kw["ss"], lam=nan, image=None, state_bytes=0), **kw))
            assert rc == INVALID and b"bad sizes" in err and b"2^31" in err, (who, kw, err)
        # 3. the rate: refused, never approximated, and the message says where other rates belong
        for ss in (0, 3, 4, -1):
            rc, err = call(ss=ss, lam=nan, image=None, state_bytes=0)
            assert rc == INVALID and b"super-sample rate" in err and b"mean of every 2 x 2 block" in err and b"caller" in err, (who, ss, err)
        # 4. lambda
        for lam in (-0.001, 1.001, nan, float("inf")):
            rc, err = call(lam=lam, image=None, state_bytes=0)
            assert rc == INVALID and b"lambda_dssim" in err, (who, lam, err)
        # 5. the pointers, before the state block's size
        for kw in (dict(image=None), dict(target=None), dict(terms=None)):
            rc, err = call(state_bytes=0, **kw)
            assert rc == INVALID and b"is NULL" in err, (who, kw, err)
        # 6. the state block's size: the message carries what the query returns
        for V, W, H, ss in ((1, 8, 8, 1), (3, 100, 37, 2), (12, 1920, 1080, 1)):
            need = N.lib.gsr_image_loss_state_bytes(V, W, H)
            for lam in (0.0, 0.2, 1.0):
                rc, err = call(V=V, W=W, H=H, ss=ss, lam=lam, state_bytes=need - 1)
                assert rc == CAPACITY and b"state block too small" in err and (b"< %d " % need) in err, (who, err)
    # NULL state: the forward's metrics-only mode gets past every check (not exercised here: it would launch); the backward refuses
    rc, err = entries[1][1](state=None, state_bytes=0)
    assert rc == INVALID and b"state is NULL" in err


def test_python_wrappers_refuse_cpu_tensors():
    N = _native()
    from pcrender import losses
    img, tgt = torch.zeros(2, 3, 8, 8), torch.zeros(2, 3, 8, 8)
    with pytest.raises(RuntimeError, match="no CPU path"):
        N.image_loss_forward(img, tgt, 0.2)
    with pytest.raises(RuntimeError, match="no CPU path"):
        N.image_loss_backward(img, tgt, 0.2, 1, torch.zeros(256, dtype=torch.uint8))
    with pytest.raises(RuntimeError, match="no CPU path"):
        losses.photometric_loss(img.requires_grad_(True), tgt)
    with pytest.raises(RuntimeError, match="no CPU path"):
        losses.image_metrics(img, tgt)
