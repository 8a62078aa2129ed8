"""The child-process machinery of the refusal tables (tests/test_cpu_backward_refusals.py, test_cpu_follower_refusals.py,
test_cpu_deterministic_channels_api.py): calls on host memory posing as arenas, in a process that sees no device, so that every
refusal of the C ABI is reachable on any machine.  Importable without torch, the built library or a device.

  P / W / H / PAIRS / NX / LAYOUT            the sizes every table calls with
  PTR / ROT / ODD                            dummy addresses: nothing is read or written before a call is refused
  native_without_device                      (child) _native, after the check that no device is visible
  buf / params / arenas                      (child) host memory with an identity, a GsrParams, the arenas of V views
  follower_params                            the GsrParams of test_cpu_camera_api.py, test_cpu_view_stats_api.py, test_cpu_contrib_api.py
  forward / recolor / frame                  (child) the calls that leave a frame record on an arena; a named history of them
  child_json                                 (parent) runs a test file as the child and returns the JSON it prints
  backward_table / BACKWARD_EXPECTED         the table of the three batch backward entries and what each row is refused with: two
                                             test files hold a build to them"""
import ctypes as C
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "gaussian-pcloud-render_amd")

P, W, H, PAIRS = 10, 64, 48, 1000
NX, LAYOUT = 8, 1
PTR, ROT, ODD = 0x1000, 0x2000, 0x2004     # dummy addresses: nothing is read or written before a call is refused

_KEEP = []


def native_without_device():
    from diff_gaussian_rasterization import _native as N
    if N.lib.gsr_wall_clock_khz() != 0:
        raise SystemExit("a HIP device is visible: the forwards below would launch kernels on host memory")
    return N


def params(N, P=P, W=W, H=H, M=0, need_backward=1, **ptr):
    p = N.GsrParams()
    p.P, p.W, p.H, p.M, p.need_backward = P, W, H, M, need_backward
    for k in ("means3D", "opacities", "bg", "viewmatrix", "projmatrix", "campos", "colors_precomp", "scales", "rotations"):
        setattr(p, k, PTR)
    for k, v in ptr.items():
        setattr(p, k, v)
    return p


def follower_params(N, P=10, W=8, H=8):
    """the GsrParams of the API tests of the entries that follow a forward: every input pointer set, precomputed colours and covariance"""
    p = N.GsrParams()
    p.P, p.W, p.H = P, W, H
    for name in ("bg", "means3D", "opacities", "viewmatrix", "projmatrix", "campos", "colors_precomp", "cov3D_precomp"):
        setattr(p, name, PTR)
    return p


def buf(n):
    b = C.create_string_buffer(int(n))
    _KEEP.append(b)                    # (kept: an address is never reused for another case's arena)
    return C.addressof(b)


def arenas(N, V):
    # (a few bytes of their own give the geometry arena and the state block their identity; the sizes are only claimed)
    lib = N.lib
    return dict(geom=buf(16), geom_bytes=V * lib.gsr_geom_bytes(P), image=PTR, image_bytes=V * lib.gsr_image_bytes(W, H),
                binning=PTR, binning_bytes=V * lib.gsr_binning_bytes(PAIRS), state=buf(16),
                state_bytes=V * lib.gsr_extra_state_bytes(W, H, PAIRS, NX) + 256)


def forward(N, a, V, kind, nb):
    """leaves the frame record of a forward on a["geom"]; the call itself ends at hipGetDevice"""
    lib = N.lib
    p, n = params(N, need_backward=nb), (C.c_int64 * V)()
    head = (C.byref(p), V, a["geom"], a["geom_bytes"], a["image"], a["image_bytes"], a["binning"], a["binning_bytes"], PTR, PTR, n, 0)
    x = (NX, LAYOUT, PTR, None, PTR, PTR)
    if kind == "colour":
        rc = lib.gsr_forward_batch(*head, None)
    elif kind == "infer":
        rc = lib.gsr_forward_batch_channels(*head, *x, None)
    else:
        rc = lib.gsr_forward_batch_channels_train(*head, *x, a["state"], a["state_bytes"], None)
    assert rc == -2, (rc, lib.gsr_last_error())


def recolor(N, a, V, nb):
    p = params(N, need_backward=nb)
    rc = N.lib.gsr_forward_recolor(C.byref(p), V, 0, a["geom"], a["geom_bytes"], a["binning"], a["binning_bytes"], a["image"],
                                   a["image_bytes"], PTR, None)
    assert rc != 0, "a recolor without a device succeeded"


FRAMES = {"none": [], "fwd_nb1": [("colour", 1)], "fwd_nb0": [("colour", 0)], "chan_train": [("train", 1)],
          "chan_train_nb0": [("train", 0)], "chan_infer": [("infer", 1)], "recolor_nb0": [("colour", 1), ("recolor", 0)],
          "recolor_nb1": [("colour", 1), ("recolor", 1)], "recolor_on_fwd_nb0": [("colour", 0), ("recolor", 1)],
          "recolor_nb1_no_record": [("recolor", 1)], "recolor_on_chan_train": [("train", 1), ("recolor", 1)]}


def frame(N, name):
    """the arenas of V views after the calls of FRAMES[name]; a name that ends in _v2 / _v3: V = 2 / 3, else V = 1"""
    V = int(name[-1]) if name[-3:] in ("_v2", "_v3") else 1
    a = arenas(N, V)
    for kind, nb in FRAMES[name[:-3] if V > 1 else name]:
        recolor(N, a, V, nb) if kind == "recolor" else forward(N, a, V, kind, nb)
    return a


def child_json(path):
    """runs the test file `path` as a script in a child that sees no device, wherever the suite runs; the last line it prints is JSON"""
    e = dict(os.environ)
    e["PYTHONPATH"] = os.pathsep.join([PKG, os.path.join(ROOT, "tests"), e.get("PYTHONPATH", "")])
    e["HIP_VISIBLE_DEVICES"] = e["ROCR_VISIBLE_DEVICES"] = "-1"
    out = subprocess.run([sys.executable, os.path.abspath(path)], env=e, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout + out.stderr
    return json.loads(out.stdout.strip().splitlines()[-1])


def backward_table():
    """[(entry, case name, frame the arena holds, changes to the good call)]"""
    rows = []
    for e in ("batch", "det", "channels"):
        good = "chan_train" if e == "channels" else "fwd_nb1"
        add = lambda name, frame=good, **kw: rows.append((e, name, frame, kw))  # noqa: E731
        add("params_null", params=None)
        add("bad_sizes", P=-1)
        add("views_0", V=0)
        add("views_257", V=257)
        add("input_pointer_null", means3D=None)
        add("both_colour_sources", shs=PTR)
        add("no_covariance_source", scales=None, rotations=None)
        for k in ("radii", "dpix", "dmean2D", "dopacity", "dcolor", "dmean3D", "dcov3D"):
            add(k + "_null", **{k: None})
        add("dsh_null", shs=PTR, colors_precomp=None, M=1, dsh=None)
        add("dscale_null", dscale=None)
        add("drot_null", drot=None)
        add("drot_misaligned", drot=ODD)
        add("binning_null", binning=None)
        add("geom_too_small", geom_bytes=100)
        add("geom_null", geom=None)
        add("image_too_small", image_bytes=100)
        add("binning_too_small", binning_bytes=100)
        add("binning_without_capacity", binning_bytes=1024)
        add("binning_too_small_for_views", frame=good + "_v2", V=2, binning_bytes=600)
        # the arena's record
        add("record_fwd_nb0", frame="fwd_nb0")
        add("record_recolor_nb0", frame="recolor_nb0")
        add("record_recolor_on_fwd_nb0", frame="recolor_on_fwd_nb0")
        add("record_other_V", V=2)
        add("record_other_P", P=11)
        add("record_other_W", W=80)
        add("record_other_H", H=64)
        # two faults at once: what wins
        add("params_and_pointer", P=-1, radii=None)
        add("pointer_and_record_nb0", frame="fwd_nb0", radii=None)
        add("pointer_and_record_other_V", V=2, dcov3D=None)
        add("pointer_and_no_record", frame="none", dpix=None)
        add("binning_null_and_record_other_P", P=11, binning=None)
        add("misaligned_and_record_recolor_nb0", frame="recolor_nb0", drot=ODD)
        add("dsh_and_dscale", shs=PTR, colors_precomp=None, M=1, dsh=None, dscale=None)
        add("pointer_and_geom_too_small", radii=None, geom_bytes=100)
        add("no_record_geom_too_small", frame="none", geom_bytes=100)
        add("record_other_H_and_image_too_small", H=64, image_bytes=100)
        if e == "det":
            add("scratch_null", scratch=None, scratch_bytes=1 << 30)
            add("scratch_short", scratch_bytes=256)
            add("scratch_short_two_views", frame="fwd_nb1_v2", V=2, scratch_bytes=100000)
            add("scratch_short_after_recolor_without_record", frame="recolor_nb1_no_record", scratch_bytes=256)
            add("scratch_and_pointer", scratch=None, radii=None)
            add("scratch_and_record_nb0", frame="fwd_nb0", scratch=None)
            add("scratch_and_geom_too_small", scratch=None, geom_bytes=100)
        if e == "channels":
            add("nx_5", nx=5)
            add("layout_3", layout=3)
            add("layout_2_with_nx_4", nx=4, layout=2)
            for k in ("extra", "bg_extra", "dvalues", "dextra", "state"):
                add(k + "_null", **{k: None})
            add("nx_and_params_null", nx=5, params=None)
            add("extra_null_and_params_null", extra=None, params=None)
            add("dextra_null_and_bad_sizes", dextra=None, P=-1)
            add("state_null_and_no_record", frame="none", state=None)
            add("no_record", frame="none")
            add("no_record_and_pointer", frame="none", radii=None)
            add("record_colour_forward", frame="fwd_nb1")
            add("record_channels_inference_forward", frame="chan_infer")
            add("record_channels_train_nb0", frame="chan_train_nb0")
            add("record_recolor", frame="recolor_on_chan_train")
            add("record_other_nx", nx=4)
            add("record_other_layout", layout=0)
            add("record_other_nx_and_other_V", nx=4, V=2)
            add("record_other_state", state="other")
            add("record_state_shorter", state_bytes=256)
            add("record_other_state_and_pointer", state="other", radii=None)
            add("record_other_V_and_other_state", V=2, state="other")
            add("state_too_small_for_binning", binning_pairs=100000)
            add("state_too_small_for_binning_and_pointer", binning_pairs=100000, dmean2D=None)
            add("geom_too_small_and_state_too_small_for_binning", binning_pairs=100000, geom_bytes=100)
    return rows


# Generated by running backward_table (`python tests/test_cpu_backward_refusals.py`, GSR_LIB pointing at that build) against the
# library of the commit BEFORE the three entries were routed through one backward_impl (98511e5), and committed as literals.
BACKWARD_EXPECTED = {
    "batch/params_null": (-1, "[gsr] params is NULL"),
    "batch/bad_sizes": (-1, "[gsr] bad sizes P=-1 W=64 H=48"),
    "batch/views_0": (-1, "[gsr] view count 0 outside 1..256"),
    "batch/views_257": (-1, "[gsr] view count 257 outside 1..256"),
    "batch/input_pointer_null": (-1, "[gsr] a required input pointer is NULL"),
    "batch/both_colour_sources": (-1, "Please provide excatly one of either SHs or precomputed colors!"),
    "batch/no_covariance_source": (-1, "Please provide exactly one of either scale/rotation pair or precomputed 3D covariance!"),
    "batch/radii_null": (-1, "[gsr] a required backward pointer is NULL"),
    "batch/dpix_null": (-1, "[gsr] a required backward pointer is NULL"),
    "batch/dmean2D_null": (-1, "[gsr] a required backward pointer is NULL"),
    "batch/dopacity_null": (-1, "[gsr] a required backward pointer is NULL"),
    "batch/dcolor_null": (-1, "[gsr] a required backward pointer is NULL"),
    "batch/dmean3D_null": (-1, "[gsr] a required backward pointer is NULL"),
    "batch/dcov3D_null": (-1, "[gsr] a required backward pointer is NULL"),
    "batch/dsh_null": (-1, "[gsr] dL_dsh is NULL"),
    "batch/dscale_null": (-1, "[gsr] dL_dscale/dL_drot is NULL"),
    "batch/drot_null": (-1, "[gsr] dL_dscale/dL_drot is NULL"),
    "batch/drot_misaligned": (-1, "[gsr] dL_drot must be 16-byte aligned (it is written one float4 per Gaussian)"),
    "batch/binning_null": (-1, "[gsr] binning arena is NULL"),
    "batch/geom_too_small": (-3, "[gsr] geom arena too small (100 < 21760, need_backward)"),
    "batch/geom_null": (-3, "[gsr] geom arena too small (21760 < 21760, need_backward)"),
    "batch/image_too_small": (-3, "[gsr] image arena too small (100 < 64256)"),
    "batch/binning_too_small": (-3, "[gsr] binning arena too small"),
    "batch/binning_without_capacity": (-3, "[gsr] binning arena too small (1024 bytes for 1 views)"),
    "batch/binning_too_small_for_views": (-3, "[gsr] binning arena too small"),
    "batch/record_fwd_nb0": (-1,
        "[gsr] backward: the last forward on this geometry arena had need_backward = 0 and saved nothing for "
        "it"),
    "batch/record_recolor_nb0": (-1,
        "[gsr] backward: the last gsr_forward_recolor on this geometry arena had need_backward = 0 and saved "
        "nothing for it"),
    "batch/record_recolor_on_fwd_nb0": (-1,
        "[gsr] backward: the recolor's forward on this geometry arena had need_backward = 0 (a need_backward "
        "recolor needs the arenas of a need_backward forward)"),
    "batch/record_other_V": (-1,
        "[gsr] backward: V = 2, P = 10, 64 x 48, but the last forward or recolor on this geometry arena had V"
        " = 1, P = 10, 64 x 48"),
    "batch/record_other_P": (-1,
        "[gsr] backward: V = 1, P = 11, 64 x 48, but the last forward or recolor on this geometry arena had V"
        " = 1, P = 10, 64 x 48"),
    "batch/record_other_W": (-1,
        "[gsr] backward: V = 1, P = 10, 80 x 48, but the last forward or recolor on this geometry arena had V"
        " = 1, P = 10, 64 x 48"),
    "batch/record_other_H": (-1,
        "[gsr] backward: V = 1, P = 10, 64 x 64, but the last forward or recolor on this geometry arena had V"
        " = 1, P = 10, 64 x 48"),
    "batch/params_and_pointer": (-1, "[gsr] bad sizes P=-1 W=64 H=48"),
    "batch/pointer_and_record_nb0": (-1, "[gsr] a required backward pointer is NULL"),
    "batch/pointer_and_record_other_V": (-1, "[gsr] a required backward pointer is NULL"),
    "batch/pointer_and_no_record": (-1, "[gsr] a required backward pointer is NULL"),
    "batch/binning_null_and_record_other_P": (-1, "[gsr] binning arena is NULL"),
    "batch/misaligned_and_record_recolor_nb0": (-1,
        "[gsr] dL_drot must be 16-byte aligned (it is written one float4 per Gaussian)"),
    "batch/dsh_and_dscale": (-1, "[gsr] dL_dsh is NULL"),
    "batch/pointer_and_geom_too_small": (-1, "[gsr] a required backward pointer is NULL"),
    "batch/no_record_geom_too_small": (-3, "[gsr] geom arena too small (100 < 21760, need_backward)"),
    "batch/record_other_H_and_image_too_small": (-1,
        "[gsr] backward: V = 1, P = 10, 64 x 64, but the last forward or recolor on this geometry arena had V"
        " = 1, P = 10, 64 x 48"),
    "det/params_null": (-1, "[gsr] params is NULL"),
    "det/bad_sizes": (-1, "[gsr] bad sizes P=-1 W=64 H=48"),
    "det/views_0": (-1, "[gsr] view count 0 outside 1..256"),
    "det/views_257": (-1, "[gsr] view count 257 outside 1..256"),
    "det/input_pointer_null": (-1, "[gsr] a required input pointer is NULL"),
    "det/both_colour_sources": (-1, "Please provide excatly one of either SHs or precomputed colors!"),
    "det/no_covariance_source": (-1, "Please provide exactly one of either scale/rotation pair or precomputed 3D covariance!"),
    "det/radii_null": (-1, "[gsr] a required backward pointer is NULL"),
    "det/dpix_null": (-1, "[gsr] a required backward pointer is NULL"),
    "det/dmean2D_null": (-1, "[gsr] a required backward pointer is NULL"),
    "det/dopacity_null": (-1, "[gsr] a required backward pointer is NULL"),
    "det/dcolor_null": (-1, "[gsr] a required backward pointer is NULL"),
    "det/dmean3D_null": (-1, "[gsr] a required backward pointer is NULL"),
    "det/dcov3D_null": (-1, "[gsr] a required backward pointer is NULL"),
    "det/dsh_null": (-1, "[gsr] dL_dsh is NULL"),
    "det/dscale_null": (-1, "[gsr] dL_dscale/dL_drot is NULL"),
    "det/drot_null": (-1, "[gsr] dL_dscale/dL_drot is NULL"),
    "det/drot_misaligned": (-1, "[gsr] dL_drot must be 16-byte aligned (it is written one float4 per Gaussian)"),
    "det/binning_null": (-1, "[gsr] binning arena is NULL"),
    "det/geom_too_small": (-3, "[gsr] geom arena too small (100 < 21760, need_backward)"),
    "det/geom_null": (-3, "[gsr] geom arena too small (21760 < 21760, need_backward)"),
    "det/image_too_small": (-3, "[gsr] image arena too small (100 < 64256)"),
    "det/binning_too_small": (-3, "[gsr] binning arena too small"),
    "det/binning_without_capacity": (-3, "[gsr] binning arena too small (1024 bytes for 1 views)"),
    "det/binning_too_small_for_views": (-3, "[gsr] binning arena too small"),
    "det/record_fwd_nb0": (-1,
        "[gsr] backward: the last forward on this geometry arena had need_backward = 0 and saved nothing for "
        "it"),
    "det/record_recolor_nb0": (-1,
        "[gsr] backward: the last gsr_forward_recolor on this geometry arena had need_backward = 0 and saved "
        "nothing for it"),
    "det/record_recolor_on_fwd_nb0": (-1,
        "[gsr] backward: the recolor's forward on this geometry arena had need_backward = 0 (a need_backward "
        "recolor needs the arenas of a need_backward forward)"),
    "det/record_other_V": (-1,
        "[gsr] backward: V = 2, P = 10, 64 x 48, but the last forward or recolor on this geometry arena had V"
        " = 1, P = 10, 64 x 48"),
    "det/record_other_P": (-1,
        "[gsr] backward: V = 1, P = 11, 64 x 48, but the last forward or recolor on this geometry arena had V"
        " = 1, P = 10, 64 x 48"),
    "det/record_other_W": (-1,
        "[gsr] backward: V = 1, P = 10, 80 x 48, but the last forward or recolor on this geometry arena had V"
        " = 1, P = 10, 64 x 48"),
    "det/record_other_H": (-1,
        "[gsr] backward: V = 1, P = 10, 64 x 64, but the last forward or recolor on this geometry arena had V"
        " = 1, P = 10, 64 x 48"),
    "det/params_and_pointer": (-1, "[gsr] bad sizes P=-1 W=64 H=48"),
    "det/pointer_and_record_nb0": (-1, "[gsr] a required backward pointer is NULL"),
    "det/pointer_and_record_other_V": (-1, "[gsr] a required backward pointer is NULL"),
    "det/pointer_and_no_record": (-1, "[gsr] a required backward pointer is NULL"),
    "det/binning_null_and_record_other_P": (-1, "[gsr] binning arena is NULL"),
    "det/misaligned_and_record_recolor_nb0": (-1, "[gsr] dL_drot must be 16-byte aligned (it is written one float4 per Gaussian)"),
    "det/dsh_and_dscale": (-1, "[gsr] dL_dsh is NULL"),
    "det/pointer_and_geom_too_small": (-1, "[gsr] a required backward pointer is NULL"),
    "det/no_record_geom_too_small": (-3, "[gsr] geom arena too small (100 < 21760, need_backward)"),
    "det/record_other_H_and_image_too_small": (-1,
        "[gsr] backward: V = 1, P = 10, 64 x 64, but the last forward or recolor on this geometry arena had V"
        " = 1, P = 10, 64 x 48"),
    "det/scratch_null": (-3,
        "[gsr] backward_det: scratch block too small (1073741824 < 300544 = gsr_backward_det_bytes(1, 10, 64,"
        " 48, 1023): the forward's lists hold up to 1023 pairs per view)"),
    "det/scratch_short": (-3,
        "[gsr] backward_det: scratch block too small (256 < 300544 = gsr_backward_det_bytes(1, 10, 64, 48, "
        "1023): the forward's lists hold up to 1023 pairs per view)"),
    "det/scratch_short_two_views": (-3,
        "[gsr] backward_det: scratch block too small (100000 < 600832 = gsr_backward_det_bytes(2, 10, 64, 48,"
        " 1023): the forward's lists hold up to 1023 pairs per view)"),
    "det/scratch_short_after_recolor_without_record": (-3,
        "[gsr] backward_det: scratch block too small (256 < 300544 = gsr_backward_det_bytes(1, 10, 64, 48, "
        "1023): the forward's lists hold up to 1023 pairs per view)"),
    "det/scratch_and_pointer": (-1, "[gsr] a required backward pointer is NULL"),
    "det/scratch_and_record_nb0": (-1,
        "[gsr] backward: the last forward on this geometry arena had need_backward = 0 and saved nothing for "
        "it"),
    "det/scratch_and_geom_too_small": (-3, "[gsr] geom arena too small (100 < 21760, need_backward)"),
    "channels/params_null": (-1, "[gsr] params is NULL"),
    "channels/bad_sizes": (-1, "[gsr] bad sizes P=-1 W=64 H=48"),
    "channels/views_0": (-1, "[gsr] view count 0 outside 1..256"),
    "channels/views_257": (-1, "[gsr] view count 257 outside 1..256"),
    "channels/input_pointer_null": (-1, "[gsr] a required input pointer is NULL"),
    "channels/both_colour_sources": (-1, "Please provide excatly one of either SHs or precomputed colors!"),
    "channels/no_covariance_source": (-1, "Please provide exactly one of either scale/rotation pair or precomputed 3D covariance!"),
    "channels/radii_null": (-1, "[gsr] a required backward pointer is NULL"),
    "channels/dpix_null": (-1, "[gsr] a required backward pointer is NULL"),
    "channels/dmean2D_null": (-1, "[gsr] a required backward pointer is NULL"),
    "channels/dopacity_null": (-1, "[gsr] a required backward pointer is NULL"),
    "channels/dcolor_null": (-1, "[gsr] a required backward pointer is NULL"),
    "channels/dmean3D_null": (-1, "[gsr] a required backward pointer is NULL"),
    "channels/dcov3D_null": (-1, "[gsr] a required backward pointer is NULL"),
    "channels/dsh_null": (-1, "[gsr] dL_dsh is NULL"),
    "channels/dscale_null": (-1, "[gsr] dL_dscale/dL_drot is NULL"),
    "channels/drot_null": (-1, "[gsr] dL_dscale/dL_drot is NULL"),
    "channels/drot_misaligned": (-1, "[gsr] dL_drot must be 16-byte aligned (it is written one float4 per Gaussian)"),
    "channels/binning_null": (-1, "[gsr] binning arena is NULL"),
    "channels/geom_too_small": (-3, "[gsr] geom arena too small (100 < 21760, need_backward)"),
    "channels/geom_null": (-1,
        "[gsr] backward_channels: no forward on this geometry arena (run gsr_forward_batch_channels_train "
        "first)"),
    "channels/image_too_small": (-3, "[gsr] image arena too small (100 < 64256)"),
    "channels/binning_too_small": (-3, "[gsr] binning arena too small"),
    "channels/binning_without_capacity": (-3, "[gsr] binning arena too small (1024 bytes for 1 views)"),
    "channels/binning_too_small_for_views": (-3, "[gsr] binning arena too small"),
    "channels/record_fwd_nb0": (-1,
        "[gsr] backward_channels: the forward on this arena saved no extra channels (it needs "
        "gsr_forward_batch_channels_train with need_backward = 1)"),
    "channels/record_recolor_nb0": (-1,
        "[gsr] backward_channels after gsr_forward_recolor is not supported: the recolor replaced the saves "
        "of the channels forward (run gsr_forward_batch_channels_train again)"),
    "channels/record_recolor_on_fwd_nb0": (-1,
        "[gsr] backward_channels after gsr_forward_recolor is not supported: the recolor replaced the saves "
        "of the channels forward (run gsr_forward_batch_channels_train again)"),
    "channels/record_other_V": (-1, "[gsr] backward_channels: views / sizes differ from the forward's"),
    "channels/record_other_P": (-1, "[gsr] backward_channels: views / sizes differ from the forward's"),
    "channels/record_other_W": (-1, "[gsr] backward_channels: views / sizes differ from the forward's"),
    "channels/record_other_H": (-1, "[gsr] backward_channels: views / sizes differ from the forward's"),
    "channels/params_and_pointer": (-1, "[gsr] bad sizes P=-1 W=64 H=48"),
    "channels/pointer_and_record_nb0": (-1,
        "[gsr] backward_channels: the forward on this arena saved no extra channels (it needs "
        "gsr_forward_batch_channels_train with need_backward = 1)"),
    "channels/pointer_and_record_other_V": (-1, "[gsr] backward_channels: views / sizes differ from the forward's"),
    "channels/pointer_and_no_record": (-1,
        "[gsr] backward_channels: no forward on this geometry arena (run gsr_forward_batch_channels_train "
        "first)"),
    "channels/binning_null_and_record_other_P": (-1, "[gsr] backward_channels: views / sizes differ from the forward's"),
    "channels/misaligned_and_record_recolor_nb0": (-1,
        "[gsr] backward_channels after gsr_forward_recolor is not supported: the recolor replaced the saves "
        "of the channels forward (run gsr_forward_batch_channels_train again)"),
    "channels/dsh_and_dscale": (-1, "[gsr] dL_dsh is NULL"),
    "channels/pointer_and_geom_too_small": (-1, "[gsr] a required backward pointer is NULL"),
    "channels/no_record_geom_too_small": (-1,
        "[gsr] backward_channels: no forward on this geometry arena (run gsr_forward_batch_channels_train "
        "first)"),
    "channels/record_other_H_and_image_too_small": (-1, "[gsr] backward_channels: views / sizes differ from the forward's"),
    "channels/nx_5": (-1, "[gsr] extra channels come in 4 or 8 (got 5): pad with zeros"),
    "channels/layout_3": (-1, "[gsr] extra_per_view is 0, 1 or (with 8 channels) 2"),
    "channels/layout_2_with_nx_4": (-1, "[gsr] extra_per_view is 0, 1 or (with 8 channels) 2"),
    "channels/extra_null": (-1, "[gsr] an extra-channel pointer is NULL"),
    "channels/bg_extra_null": (-1, "[gsr] an extra-channel pointer is NULL"),
    "channels/dvalues_null": (-1, "[gsr] an extra-channel pointer is NULL"),
    "channels/dextra_null": (-1, "[gsr] dL_dextra / extra_state is NULL"),
    "channels/state_null": (-1, "[gsr] dL_dextra / extra_state is NULL"),
    "channels/nx_and_params_null": (-1, "[gsr] params is NULL"),
    "channels/extra_null_and_params_null": (-1, "[gsr] params is NULL"),
    "channels/dextra_null_and_bad_sizes": (-1, "[gsr] dL_dextra / extra_state is NULL"),
    "channels/state_null_and_no_record": (-1, "[gsr] dL_dextra / extra_state is NULL"),
    "channels/no_record": (-1,
        "[gsr] backward_channels: no forward on this geometry arena (run gsr_forward_batch_channels_train "
        "first)"),
    "channels/no_record_and_pointer": (-1,
        "[gsr] backward_channels: no forward on this geometry arena (run gsr_forward_batch_channels_train "
        "first)"),
    "channels/record_colour_forward": (-1,
        "[gsr] backward_channels: the forward on this arena saved no extra channels (it needs "
        "gsr_forward_batch_channels_train with need_backward = 1)"),
    "channels/record_channels_inference_forward": (-1,
        "[gsr] backward_channels: the forward on this arena saved no extra channels (it needs "
        "gsr_forward_batch_channels_train with need_backward = 1)"),
    "channels/record_channels_train_nb0": (-1,
        "[gsr] backward_channels: the forward on this arena saved no extra channels (it needs "
        "gsr_forward_batch_channels_train with need_backward = 1)"),
    "channels/record_recolor": (-1,
        "[gsr] backward_channels after gsr_forward_recolor is not supported: the recolor replaced the saves "
        "of the channels forward (run gsr_forward_batch_channels_train again)"),
    "channels/record_other_nx": (-1,
        "[gsr] backward_channels: nx = 4, extra_per_view = 1, but the forward had nx = 8, extra_per_view = 1"),
    "channels/record_other_layout": (-1,
        "[gsr] backward_channels: nx = 8, extra_per_view = 0, but the forward had nx = 8, extra_per_view = 1"),
    "channels/record_other_nx_and_other_V": (-1,
        "[gsr] backward_channels: nx = 4, extra_per_view = 1, but the forward had nx = 8, extra_per_view = 1"),
    "channels/record_other_state": (-1, "[gsr] backward_channels: extra_state is not the block the forward saved into"),
    "channels/record_state_shorter": (-1, "[gsr] backward_channels: extra_state is not the block the forward saved into"),
    "channels/record_other_state_and_pointer": (-1, "[gsr] backward_channels: extra_state is not the block the forward saved into"),
    "channels/record_other_V_and_other_state": (-1, "[gsr] backward_channels: views / sizes differ from the forward's"),
    "channels/state_too_small_for_binning": (-3, "[gsr] extra-state block too small for this binning arena"),
    "channels/state_too_small_for_binning_and_pointer": (-1, "[gsr] a required backward pointer is NULL"),
    "channels/geom_too_small_and_state_too_small_for_binning": (-3, "[gsr] geom arena too small (100 < 21760, need_backward)"),
}
