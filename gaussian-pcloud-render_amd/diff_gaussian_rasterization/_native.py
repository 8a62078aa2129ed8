"""ctypes binding of libgsr_hip.so (include/gsr.h).

Plays the role of the reference's pybind module ``diff_gaussian_rasterization._C`` (ext.cpp:15-19):
three entry points taking torch tensors.  Tensors are only used for device memory and the
stream; what crosses the boundary are raw pointers and sizes.

There is NO fallback: if the shared library is missing or a tensor is not on a HIP device the
call raises.
"""
import ctypes as C
import os
import threading
import weakref as _weakref

import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("GSR_LIB") or os.path.join(_HERE, "libgsr_hip.so")   # (GSR_LIB: another build of the same ABI, for A/B runs)

_fp = C.c_void_p


class GsrParams(C.Structure):
    _fields_ = [
        ("P", C.c_int), ("D", C.c_int), ("M", C.c_int), ("W", C.c_int), ("H", C.c_int),
        ("tanfovx", C.c_float), ("tanfovy", C.c_float), ("scale_modifier", C.c_float),
        ("prefiltered", C.c_int), ("debug", C.c_int), ("need_backward", C.c_int), ("reference_lists", C.c_int),
        ("bg", _fp), ("means3D", _fp), ("shs", _fp), ("colors_precomp", _fp), ("opacities", _fp),
        ("scales", _fp), ("rotations", _fp), ("cov3D_precomp", _fp),
        ("viewmatrix", _fp), ("projmatrix", _fp), ("campos", _fp),
    ]


GSR_RETRY = 1

Q = dict(DEPTHS=1, MEANS2D=2, CONIC_OPACITY=3, RGB=4, TILES_TOUCHED=5, POINT_LIST=6, POINT_LIST_KEYS=7, RANGES=8,
         FINAL_T=9, N_CONTRIB=10, CLAMPED=11, TILE_NEED=12, DEPTH_SORT=13, LIST_PAIRS=14)

_int, _i64, _size, _pp = C.c_int, C.c_int64, C.c_size_t, C.POINTER(GsrParams)
_ARENAS = [_fp, _size, _fp, _size, _fp, _size]
# the 12 leading arguments of the batch forwards: params, V, three arenas, radii, out_color, num_rendered, resume
_FWD = [_pp, _int] + _ARENAS + [_fp, _fp, C.POINTER(_i64), _int]
_FWD_X = _FWD + [_int, _int, _fp, _fp, _fp, _fp]          # + nx, extra_per_view, extra, extra_view_scale, bg_extra, out_extra
# the 18 leading arguments of the batch backwards: params, V, radii, three arenas, dL_dpix and the eight gradient outputs
_BWD = [_pp, _int, _fp] + _ARENAS + [_fp] * 9
# symbol -> (restype, argtypes) of everything include/gsr.h declares with arguments
_DECL = {
    "gsr_geom_bytes": (_size, [_int]),
    "gsr_geom_bytes_inference": (_size, [_int]),
    "gsr_image_bytes": (_size, [_int, _int]),
    "gsr_binning_bytes": (_size, [_i64]),
    "gsr_extra_state_bytes": (_size, [_int, _int, _i64, _int]),
    "gsr_backward_det_bytes": (_size, [_int, _int, _int, _int, _i64]),
    "gsr_backward_det_channels_bytes": (_size, [_int, _int, _int, _int, _i64, _int, _int]),
    "gsr_forward_batch": (_int, _FWD + [_fp]),
    "gsr_forward_batch_channels": (_int, _FWD_X + [_fp]),
    "gsr_forward_batch_channels_train": (_int, _FWD_X + [_fp, _size, _fp]),
    "gsr_forward_stage1": (_int, [_pp, _fp, _size, _fp, _size, _fp, C.POINTER(_i64), _fp]),
    "gsr_forward_stage2": (_int, [_pp] + _ARENAS + [_i64, _fp, _fp]),
    "gsr_forward_recolor": (_int, [_pp, _int, _int] + _ARENAS + [_fp, _fp]),
    "gsr_backward_batch": (_int, _BWD + [_fp]),
    "gsr_backward_batch_det": (_int, _BWD + [_fp, _size, _fp]),
    "gsr_backward_batch_channels": (_int, _BWD + [_int, _int, _fp, _fp, _fp, _fp, _size, _fp, _fp, _fp]),
    "gsr_backward_batch_channels_det": (_int, _BWD + [_int, _int, _fp, _fp, _fp, _fp, _size, _fp, _fp, _fp, _size, _fp]),
    "gsr_backward": (_int, [_pp, _fp, _i64] + _ARENAS + [_fp] * 9 + [_fp]),
    "gsr_camera_grad_bytes": (_size, [_int, _int]),
    "gsr_backward_cameras": (_int, [_pp, _int, _fp, _fp, _size, _fp, _fp, _fp, _fp, _size, _fp]),
    "gsr_backward_view_stats": (_int, [_pp, _int, _fp, _fp, _size, _int, _fp, _fp, _fp, _fp, _fp, _fp, _fp]),
    "gsr_contrib_stats": (_int, [_pp, _int, _fp] + _ARENAS + [_fp, _int, _fp, _fp, _fp, _fp, _fp]),
    "gsr_image_loss_state_bytes": (_size, [_int, _int, _int]),
    "gsr_image_loss_forward": (_int, [_int, _int, _int, _int, C.c_float, _fp, _fp, _fp, _fp, _size, _fp]),
    "gsr_image_loss_backward": (_int, [_int, _int, _int, _int, C.c_float, _fp, _fp, _fp, _fp, _size, _fp, _fp]),
    "gsr_visible_from_radii": (_int, [_int, _int, _fp, _fp, _fp]),
    "gsr_adam_step": (_int, [_int, _int, _fp, _i64, C.c_float, C.c_float, C.c_float, _fp, _int, _fp]),
    "gsr_density_scratch_bytes": (_size, [_int]),
    "gsr_density_plan": (_int, [_int, _fp, _fp, _fp, _fp, _fp, _fp, _fp, _fp, _fp, _fp, _fp, _size, _fp]),
    "gsr_density_apply": (_int, [_int, _int, _fp, _fp, _fp, _fp, _fp, _fp, _fp, _fp, _i64, _fp]),
    "gsr_knn_scratch_bytes": (_size, [_int, _int]),
    "gsr_knn": (_int, [_int, _fp, _int, _fp, _fp, _fp, _size, _fp]),
    "gsr_cloud_geometry": (_int, [_int, _fp, _int, _fp, _int, _int, _fp, _fp, _fp, _fp, _fp, _fp, _fp]),
    "gsr_mark_visible": (_int, [_int, _fp, _fp, _fp, _fp, _fp]),
    "gsr_query": (_int, [_pp, _int, _fp, _fp, _size, _fp, _i64, _fp, _size, _fp]),
    "gsr_set_profiling": (None, [_int]),
    "gsr_set_forward_half_views": (_int, [_int]),
    "gsr_set_backward_moments": (_int, [_int]),
    "gsr_set_render_math": (_int, [_int]),
    "gsr_set_train_math": (_int, [_int]),
    "gsr_get_profile": (_int, [C.POINTER(C.c_char_p), C.POINTER(C.c_float), _int]),
    "gsr_selftest": (_int, [_fp]),
    "gsr_sort_probe": (_int, [_fp, _fp, _size, _fp, _size, _int, _i64, _int, _int, _fp, _fp, _fp, _fp]),
    "gsr_tile_ranges_probe": (_int, [_fp, _size, _fp, _size, _int, _i64, _int, _int, _fp, _fp]),
    "gsr_d2h_count": (C.c_longlong, []),
    "gsr_clock_probe_launch": (_int, [_fp, _int, _fp]),
    "gsr_wall_clock_khz": (_int, []),
    "gsr_last_list_pairs": (_int, [C.POINTER(_i64), _int]),
}
_RESTYPE_ONLY = {"gsr_last_error": C.c_char_p, "gsr_version": C.c_char_p}
# every symbol include/gsr.h declares (tests check the library exports all of them)
SYMBOLS = tuple(_DECL) + tuple(_RESTYPE_ONLY)


def _load():
    if not os.path.exists(LIB_PATH):
        raise ImportError(
            "diff_gaussian_rasterization: %s not found - build it with "
            "`python gaussian-pcloud-render_amd/build.py` (hipcc, gfx950). There is no CPU fallback." % LIB_PATH)
    lib = C.CDLL(LIB_PATH)
    for name, (restype, argtypes) in _DECL.items():
        getattr(lib, name).restype, getattr(lib, name).argtypes = restype, argtypes
    for name, restype in _RESTYPE_ONLY.items():
        getattr(lib, name).restype = restype
    return lib


lib = _load()


def _ptr(t):
    """NULL for absent optionals: the reference passes empty tensors whose data_ptr is nullptr
    (rasterize_points.cu:94-111 -> rasterizer_impl.cu:321,389,411)."""
    if t is None or t.numel() == 0:
        return None
    return t.data_ptr()


def _check(rc):
    if rc != 0:
        raise RuntimeError(lib.gsr_last_error().decode("utf-8", "replace"))


_F32 = torch.float32


def _f32c(t, device, name):
    if t.numel() == 0:
        return t
    if t.dtype != torch.float32:
        raise RuntimeError("expected scalar type Float but found %s for %s" % (t.dtype, name))
    if t.device == device and t.is_contiguous():     # the usual case: nothing to dispatch
        return t
    return t.to(device).contiguous()


# the current stream's handle and "is `device` the current device" without building torch.cuda.Stream / device objects: this
# module's code runs between the caller's last host->device copy and the first kernel launch, i.e. while the GPU idles whenever
# the caller's loop drains the stream once per frame (the reference's does: simple_raw_render.py:260-263 builds the settings
# tensors from host arrays for every call)
_raw_stream = getattr(torch._C, "_cuda_getCurrentRawStream", None)


def _stream_handle(device):
    if _raw_stream is not None and device.index is not None:
        return _raw_stream(device.index)
    return torch.cuda.current_stream(device).cuda_stream


class _NoContext:
    def __enter__(self):
        return self

    def __exit__(self, *exc):
        return False

    @staticmethod
    def give(*tensors):
        return tensors[0] if len(tensors) == 1 else tensors


_NO_CONTEXT = _NoContext()


def _on_device(device):
    """context that makes `device` the current HIP device (nothing to do when it already is)"""
    if device.index is None or device.index == torch.cuda.current_device():
        return _NO_CONTEXT
    return torch.cuda.device(device)


def _require_hip(device):
    if device.type != "cuda":
        raise RuntimeError(
            "diff_gaussian_rasterization (MI355X build) needs tensors on a HIP device (torch device 'cuda'); got %s. "
            "There is no CPU path." % device)


# the tensors behind GsrParams' eleven pointer fields, in the fields' order, as error messages name them
_POINTER_FIELDS = ("bg", "means3D", "sh", "colors_precomp", "opacities", "scales", "rotations", "cov3D_precomp", "viewmatrix",
                   "projmatrix", "campos")


def _params(bg, means3D, colors, opacity, scales, rotations, scale_modifier, cov3D_precomp, viewmatrix, projmatrix,
            tan_fovx, tan_fovy, H, W, sh, degree, campos, prefiltered, debug, need_backward):
    """The only place where the eleven input tensors become a GsrParams (p.M: the SH coefficients per Gaussian, rasterize_points.cu:
    83-87).  The tensors are taken as they come: only one that is not float32, on the device and contiguous is converted, and those
    are returned beside the params so that they outlive the enqueued kernels' use of their pointers.  Absent optionals (empty
    tensors) give NULL, as the reference's do (rasterize_points.cu:94-111 -> rasterizer_impl.cu:321,389,411).  The per-view short
    path comes through here while the GPU idles: in the usual case no tensor costs a function call of this module."""
    device = means3D.device
    keep, ptrs = [], []
    for t in (bg, means3D, sh, colors, opacity, scales, rotations, cov3D_precomp, viewmatrix, projmatrix, campos):
        if t.numel() == 0:
            ptrs.append(None)
            continue
        if t.dtype is not _F32 or t.device != device or not t.is_contiguous():
            t = _f32c(t, device, _POINTER_FIELDS[len(ptrs)])
            keep.append(t)
        ptrs.append(t.data_ptr())
    # field order of GsrParams / gsr_params (include/gsr.h)
    p = GsrParams(means3D.shape[0], int(degree), int(sh.shape[1]) if ptrs[2] is not None else 0, int(W), int(H), float(tan_fovx),
                  float(tan_fovy), float(scale_modifier), int(bool(prefiltered)), int(bool(debug)), int(bool(need_backward)),
                  int(reference_lists()), *ptrs)
    return p, keep


def _follower_params(background, means3D, colors, scales, rotations, scale_modifier, cov3D_precomp, viewmatrices, projmatrices,
                     tan_fovx, tan_fovy, H, W, sh, degree, camposs, debug, need_backward=True):
    """_params of a call that follows a forward on its arenas (the backwards, the readers of the gradient records, the contribution
    statistics): opacity lives in the geometry arena and the pointer only has to be non-NULL, so means3D stands in; prefiltered
    plays no part after the forward."""
    return _params(background, means3D, colors, means3D, scales, rotations, scale_modifier, cov3D_precomp, viewmatrices,
                   projmatrices, tan_fovx, tan_fovy, H, W, sh, degree, camposs, False, debug, need_backward)


def _size_fault(P, V, bg, sh, colors, opacity, scales, rotations, cov3D_precomp, viewmatrices, projmatrices, camposs):
    """"<name> must have ..." for the first input of a forward whose size does not fit P Gaussians and V views, else None.  The C ABI
    sees raw pointers, so this is the one place where a tensor with the wrong number of rows can be caught before a kernel reads
    past its end.  Shapes only: no device work, no host copy.  Absent optionals (empty tensors) fit."""
    for name, t, per in (("opacities", opacity, 1), ("scales", scales, 3), ("rotations", rotations, 4),
                         ("cov3D_precomp", cov3D_precomp, 6), ("colors_precomp", colors, 3)):
        n = t.numel()
        if n != per * P and n != 0:
            return "%s must have %d x num_points = %d elements (got %d)" % (name, per, per * P, n)
    if sh.numel() != 0:
        shape = sh.shape
        if len(shape) != 3 or shape[0] != P or shape[2] != 3:
            return "sh must have shape (num_points = %d, coefficients, 3) (got %s)" % (P, tuple(shape))
    if 0 < bg.numel() < 3:   # (the kernels read three values; none at all: the library's NULL check)
        return "bg must have at least 3 elements (got %d)" % bg.numel()
    for name, t, per in (("viewmatrices", viewmatrices, 16), ("projmatrices", projmatrices, 16), ("camposs", camposs, 3)):
        if V < 1 or t.numel() != per * V:
            return "%s must have %d x num_views = %d elements for num_views >= 1 (got %d)" % (name, per, per * V, t.numel())
    return None


# ---- footprint clipping (include/gsr.h, gsr_params.reference_lists) ---------------------------------------------------
# Default: a Gaussian emits pairs only for the tiles of the reference's rectangle in which it can reach alpha >= 1/255; every
# API-visible result is unchanged.  set_reference_lists(True) / GSR_REFERENCE_LISTS=1 keeps the reference's full rectangles, so
# that the private lists, ranges and n_contrib can be compared with the reference's element by element (parity tests).
_REFERENCE_LISTS = [os.environ.get("GSR_REFERENCE_LISTS", "0") not in ("", "0")]   # process default
_TLS = threading.local()                                                              # per-thread override (tests render from several threads)


def reference_lists():
    return getattr(_TLS, "reference_lists", _REFERENCE_LISTS[0])


def set_reference_lists(on):
    """Setting of the CALLING THREAD (None: back to the process default).  Returns the thread's previous override (or None)."""
    old = getattr(_TLS, "reference_lists", None)
    if on is None:
        if hasattr(_TLS, "reference_lists"):
            del _TLS.reference_lists
    else:
        _TLS.reference_lists = bool(on)
    return old


# ---- deterministic backward (include/gsr.h gsr_backward_batch_det) ---------------------------------------------------------
# None (default): follow torch.are_deterministic_algorithms_enabled(); True / False force the path on / off.  GSR_DETERMINISTIC
# (0 / 1) in the environment sets the initial value.  With the path on, the colour backwards go through gsr_backward_batch_det:
# bit-identical gradients from call to call and from process to process for the same inputs and call shape (not across different
# numbers of views per call), for a scratch block per backward and the time of a sort and an ordered reduction.
_DETERMINISTIC = [{"0": False, "1": True}.get(os.environ.get("GSR_DETERMINISTIC", "").strip())]
# backwards issued through each entry (tests): the colour ones, the deterministic channels backward, the camera gradients and the
# view statistics; and the contribution statistics, which follow a forward
CALLS = dict(backward=0, backward_det=0, backward_channels_det=0, backward_cameras=0, backward_view_stats=0, contrib_stats=0)


def set_deterministic(flag):
    """True / False: force the deterministic colour backward on / off; None: follow torch's deterministic-algorithms switch."""
    _DETERMINISTIC[0] = None if flag is None else bool(flag)


def get_deterministic():
    """The value set_deterministic was last given (None, True or False)."""
    return _DETERMINISTIC[0]


def deterministic_active():
    f = _DETERMINISTIC[0]
    return bool(torch.are_deterministic_algorithms_enabled()) if f is None else f


# The deterministic CHANNELS backward (include/gsr.h gsr_backward_batch_channels_det) has a switch of its own: set_deterministic and
# torch's switch keep refusing rasterize_views_channels, as they always did.  With this switch on, rasterize_views_channels (and
# pcrender.raster_passes.train_passes through it) runs whatever the other switch says, and its backward -- colour and extra
# channels through one storing kernel -- is bit-identical from call to call.  GSR_DETERMINISTIC_CHANNELS=1 sets the initial value.
_DETERMINISTIC_CHANNELS = [os.environ.get("GSR_DETERMINISTIC_CHANNELS", "").strip() == "1"]


def set_deterministic_channels(flag):
    """True: rasterize_views_channels differentiates through the deterministic channels backward; False (default): the atomic one."""
    _DETERMINISTIC_CHANNELS[0] = bool(flag)


def get_deterministic_channels():
    """The value set_deterministic_channels was last given (initially GSR_DETERMINISTIC_CHANNELS=1 in the environment, else False)."""
    return _DETERMINISTIC_CHANNELS[0]


def last_list_pairs(V):
    """largest per-view pair count of the lists of the calling thread's last forward (gsr_last_list_pairs)"""
    pairs = (C.c_int64 * V)()
    _check(lib.gsr_last_list_pairs(pairs, V))
    return int(max(pairs))


def det_scratch(V, P, W, H, pairs, binning_bytes, device, nx=0, extra_per_view=0):
    """the scratch block of one deterministic backward; nx != 0: of the channels backward (gsr_backward_det_channels_bytes).
    pairs None: the lists' extent is not known here; (bytes of a view's binning arena) / 16 is an upper bound of what the arena
    holds (the library checks the size against the lists it remembers)"""
    if pairs is None:
        pairs = max(1, int(binning_bytes) // max(1, V) // 16)
    n = (lib.gsr_backward_det_channels_bytes(V, P, W, H, int(pairs), nx, extra_per_view) if nx
         else lib.gsr_backward_det_bytes(V, P, W, H, int(pairs)))
    return torch.empty((int(n),), dtype=torch.uint8, device=device)


# ---- binning-arena capacity -----------------------------------------------------------------------------------------
# The pair count of a frame (num_rendered) is only known on the device while the frame is being enqueued, so the binning
# arena is allocated by CAPACITY: the largest count this (device, P, W, H) configuration produced recently, plus slack.
# A frame that needs more gets GSR_RETRY and repeats its binning half with an exact-size arena; the first frame of a
# configuration counts first (stage 1) and then binds (stage 2), like the reference's synchronous flow.
_CAP_HINT = {}
CAP_SLACK = 1.25


def _cap_key(device, P, W, H):
    return (device.index if device.index is not None else torch.cuda.current_device(), int(P), int(W), int(H))


def _note_counts(key, counts):
    old = _CAP_HINT.get(key, 0)
    _CAP_HINT[key] = max(max(counts), int(old * 0.98))   # shrinks slowly when the frames get lighter


def reset_capacity_hints():
    _CAP_HINT.clear()


# arena sizes are functions of (P, need_backward) resp. (W, H) alone: asked of the library once per configuration
_ARENA_BYTES, _IMAGE_BYTES = {}, {}


def _arena_bytes(P, need_backward):
    k = (P, bool(need_backward))
    b = _ARENA_BYTES.get(k)
    if b is None:
        if len(_ARENA_BYTES) > 256:
            _ARENA_BYTES.clear()
        b = _ARENA_BYTES[k] = int(lib.gsr_geom_bytes(P) if need_backward else lib.gsr_geom_bytes_inference(P))
    return b


def _image_bytes(W, H):
    k = (W, H)
    b = _IMAGE_BYTES.get(k)
    if b is None:
        if len(_IMAGE_BYTES) > 256:
            _IMAGE_BYTES.clear()
        b = _IMAGE_BYTES[k] = int(lib.gsr_image_bytes(W, H))
    return b



# ---- consecutive calls overlap on the device (no caller threads) ---------------------------------------------------------
# A per-view caller issues forward(j), backward(j), forward(j+1), ... on ONE stream, so the device runs them back to back: the
# tail of a single view's render kernels (a handful of deep list walks on an otherwise idle chip) and the bandwidth-bound front
# end of the next view never share the GPU.  Four caller threads on four streams get 1.5x out of that overlap (bench.py,
# drop_in_api.four_streams); the same overlap is available to ONE caller when the library can prove that the next forward does
# not depend on the work still in flight:
#   * every forward runs on one of a few internal side streams (rotating), the caller's stream waits (on the device) for it at
#     the end of the call, so everything the caller enqueues afterwards is ordered behind the results as before;
#   * the side stream has to wait for the INPUTS only.  An input tensor seen before -- the same Python tensor object with the
#     same torch version counter, i.e. not written through torch since -- was complete when the call that first saw it
#     began; if that holds for every input, the side stream waits for the event recorded then, not for the caller stream's
#     tail: forward(j+1)'s front end runs beside backward(j).  A new tensor, a bumped version counter (optimizer step, any
#     in-place op), a tensor without a counter (inference mode): the side stream waits for the caller's stream as it is
#     now -- exactly the unoverlapped order.
# Tensors are remembered by weak reference (no lifetime is extended; a recycled address can not impersonate an old tensor).
# What the version counter does not see -- `t.data.copy_(...)`, a foreign kernel writing through `data_ptr()` -- is not seen here
# either: autograd's own in-place checks have the same blind spot (a swapped storage, `t.data = other`, IS seen: the record
# holds data_ptr / offset / shape / strides).  Off by default (below); when on, set_overlap(False) restores plain in-stream execution.  All outputs and arenas are allocated on the side stream and handed to the caller's stream with
# record_stream, so torch's caching allocator never recycles them under a kernel that still runs.
# OPT-IN since round 5 (GSR_OVERLAP=1 or set_overlap(True)): what the overlap is worth depends on which hardware queues the runtime
# binds the side streams to at their first launch -- 1 250-1 360 frames/s in most processes, 1 010-1 160 in some, in-order 985 --
# which a process can neither see nor choose, and the reference's literal caller (fresh settings tensors per call,
# simple_raw_render.py:260-263) never qualifies for it anyway: the default is plain stream order, the same in every process.
# Each side stream wants a hardware queue of its own (the ROCm runtime maps HIP streams onto GPU_MAX_HW_QUEUES queues, default 4,
# and streams that share a queue serialise); the variable is read when HIP starts and changes the stream-to-queue mapping of the
# whole process, so the library only touches it when asked to (GSR_SET_HW_QUEUES=1, before the process first uses the GPU).
if os.environ.get("GSR_SET_HW_QUEUES", "0") == "1" and not torch.cuda.is_initialized():
    os.environ.setdefault("GPU_MAX_HW_QUEUES", "8")

_OVERLAP_ON = os.environ.get("GSR_OVERLAP", "0") == "1"
_OVERLAP_STREAMS = int(os.environ.get("GSR_OVERLAP_STREAMS", "3"))
_OVERLAP_PRIORITY = int(os.environ.get("GSR_OVERLAP_PRIORITY", "-1"))    # -1: side streams above the caller's stream
OVERLAP_MAX_VIEWS = 3
_OVERLAP = {}            # (device index, caller stream) -> _OverlapState
OVERLAP_STATS = dict(calls=0, overlapped=0)


def set_overlap(on):
    """Switch the device-side overlap of consecutive forward calls on or off (off: every kernel on the caller's stream)."""
    global _OVERLAP_ON
    _OVERLAP_ON = bool(on)      # (the side streams are kept: the runtime maps streams to hardware queues in creation order, and a
                                # later set of streams may land on the caller's queue -- 1 150 instead of 1 290 frames/s,
                                # scripts/debug/overlap_warm.py)


class _OverlapState:
    def __init__(self, device, cur):
        # side streams above the caller's priority: a view's front end is short and on the critical path of the next frame, the
        # previous view's backward is not.  What the overlap is worth depends on which hardware queues / dispatch pipes the
        # runtime binds these streams to at their first launch, which a process can neither see nor choose: 1 250-1 360 frames/s
        # in most processes, 1 010-1 060 in some (in-order: 985), stable for the life of a process (gpurun_out/r4q*).  Choosing
        # streams with a concurrency test of small spin kernels made it WORSE (1 000-1 140 in every process: the binding seems
        # to follow what is in flight at the first launch), so the streams are taken as they come.
        self.streams = [torch.cuda.Stream(device=device, priority=_OVERLAP_PRIORITY) for _ in range(_OVERLAP_STREAMS)]
        self.turn = 0
        self.seen = {}       # id(tensor) -> (weakref, version, event, sequence number, storage key)
        self.seq = 0

    @staticmethod
    def _where(t):
        """What the tensor object points at: `param.data = other` (weight clamping, checkpoint loading, densification code) swaps
        the storage under the same Python object WITHOUT bumping the version counter, so object identity + version is not enough."""
        return (t.data_ptr(), t.storage_offset(), tuple(t.shape), tuple(t.stride()), t.dtype)

    def input_event(self, tensors, cur):
        """The event the side stream has to wait for: the newest `first seen` event when every input is a known, unmodified
        tensor, else an event recorded on the caller's stream now (under which the unknown inputs are registered)."""
        self.seq += 1
        newest, missing = None, []
        for t in tensors:
            try:
                ver = t._version
            except RuntimeError:      # inference tensor: no version counter, never assumed unchanged
                return self._now(cur, []), False
            rec = self.seen.get(id(t))
            if rec is not None and rec[0]() is t and rec[1] == ver and rec[4] == self._where(t):
                if newest is None or rec[3] > newest[3]:
                    newest = rec
            else:
                missing.append((t, ver))
        if missing or newest is None:
            return self._now(cur, missing), False
        return newest[2], True

    def _now(self, cur, missing):
        ev = torch.cuda.Event()
        ev.record(cur)
        if len(self.seen) > 512:
            self.seen = {k: r for k, r in self.seen.items() if r[0]() is not None}
            if len(self.seen) > 512:
                self.seen.clear()
        for t, ver in missing:
            self.seen[id(t)] = (_weakref.ref(t), ver, ev, self.seq, self._where(t))
        return ev

    def next_stream(self):
        self.turn = (self.turn + 1) % len(self.streams)
        return self.streams[self.turn]


class _OnSideStream:
    """Context of one forward call: inside, torch's current stream is a side stream that waits only for the call's inputs;
    leaving it, the caller's stream is ordered behind the side stream and takes over the outputs handed to `give`."""

    def __init__(self, device, tensors):
        self.device, self.active, self.out = device, False, []
        if device.type != "cuda":
            return
        self.cur = torch.cuda.current_stream(device)
        key = (device.index if device.index is not None else torch.cuda.current_device(), self.cur.cuda_stream)
        st = _OVERLAP.get(key)
        if st is None:
            st = _OVERLAP[key] = _OverlapState(device, self.cur)
        live = [t for t in tensors if isinstance(t, torch.Tensor) and t.numel() != 0 and t.device.type == "cuda"]
        ev, early = st.input_event(live, self.cur)
        OVERLAP_STATS["calls"] += 1
        OVERLAP_STATS["overlapped"] += int(early)
        self.side = st.next_stream()
        self.side.wait_event(ev)
        self.active = True

    def give(self, *tensors):
        self.out += [t for t in tensors if isinstance(t, torch.Tensor) and t.numel() != 0]
        return tensors[0] if len(tensors) == 1 else tensors

    def __enter__(self):
        if self.active:
            self.ctx = torch.cuda.stream(self.side)
            self.ctx.__enter__()
        return self

    def __exit__(self, *exc):
        if self.active:
            self.ctx.__exit__(*exc)
            done = torch.cuda.Event()
            done.record(self.side)
            self.cur.wait_event(done)
            for t in self.out:
                t.record_stream(self.cur)
        return False


def _extra_layout(extra, P, V, device):
    """The `extra` triple (values, view_scale or None, bg) of a channels forward or backward, checked against P points and V views:
    (nx, extra_per_view of gsr.h, values -- the split pair as one flat tensor --, view_scale, bg)."""
    xv, xs, xb = extra
    if isinstance(xv, (tuple, list)):
        # split layout (gsr.h extra_per_view = 2): channels 0..3 shared by the views [P,4], channels 4..7 per view [V,P,4]
        lo, hi = xv
        if tuple(lo.shape) != (P, 4) or tuple(hi.shape) != (V, P, 4):
            raise RuntimeError("split extra channels must have shapes (num_points, 4) and (num_views, num_points, 4)")
        xv = torch.cat([_f32c(lo, device, "extra").reshape(-1), _f32c(hi, device, "extra").reshape(-1)])
        x_per_view, nx = 2, 8
    else:
        x_per_view = int(xv.dim() == 3)
        nx = int(xv.shape[-1]) if xv.dim() in (2, 3) else -1
        if nx not in (4, 8) or xv.shape[-2] != P or (x_per_view and xv.shape[0] != V):
            raise RuntimeError("extra channels must have shape (num_points, 4 or 8) or (num_views, num_points, 4 or 8)")
    if xb.numel() != nx or (xs is not None and tuple(xs.shape) != (V, nx)):
        raise RuntimeError("bg_extra must have nx entries and view_scale shape (V, nx)")
    return nx, x_per_view, xv, xs, xb


def _extra_f32(xv, xs, xb, device):
    return (_f32c(xv, device, "extra"), None if xs is None else _f32c(xs, device, "extra_view_scale"),
            _f32c(xb.reshape(-1), device, "bg_extra"))


def _grad_tensors(P, M, device, has_sr, alloc=None):
    """The eight outputs of a backward in the reference's order (dL_dmeans2D, dL_dcolors, dL_dopacity, dL_dmeans3D, dL_dcov3D, dL_dsh,
    dL_dscales, dL_drotations).  Nothing is cleared: the per-Gaussian backward kernel writes every output for every Gaussian (the
    reference zero-fills nine tensors, rasterize_points.cu:151-159), and the accumulation records live in the geometry arena --
    except where no kernel writes: P = 0, and scales / rotations that were not given.  alloc: see rasterize_gaussians_backward_batch."""
    new = (alloc or torch.empty) if P != 0 else torch.zeros
    sr = new if has_sr else torch.zeros
    return (new((P, 3), dtype=_F32, device=device), new((P, 3), dtype=_F32, device=device), new((P, 1), dtype=_F32, device=device),
            new((P, 3), dtype=_F32, device=device), new((P, 6), dtype=_F32, device=device), new((P, M, 3), dtype=_F32, device=device),
            sr((P, 3), dtype=_F32, device=device), sr((P, 4), dtype=_F32, device=device))


def _arena_args(geom, binning, image):
    return (geom.data_ptr(), geom.numel(), binning.data_ptr(), binning.numel(), image.data_ptr(), image.numel())


def _bwd_inputs(background, means3D, radii, colors, scales, rotations, scale_modifier, cov3D_precomp, viewmatrices, projmatrices,
                tan_fovx, tan_fovy, dL_dout_color, sh, degree, camposs, debug):
    """(params, tensors to keep, radii, dL_dout_color) of a general-path backward, converted"""
    p, keep = _follower_params(background, means3D, colors, scales, rotations, scale_modifier, cov3D_precomp, viewmatrices,
                               projmatrices, tan_fovx, tan_fovy, int(dL_dout_color.shape[2]), int(dL_dout_color.shape[3]), sh, degree,
                               camposs, debug)
    return p, keep, radii.contiguous(), _f32c(dL_dout_color, means3D.device, "dL_dout_color")


def _bwd_head(p, V, radii, arenas, dpix, g):
    """The 18 leading arguments of the three batch backwards.  arenas: (geom, bytes, binning, bytes, image, bytes); g: _grad_tensors
    (the C ABI takes opacity before colour)."""
    return (C.byref(p), V, radii.data_ptr()) + arenas + (
        dpix.data_ptr(), g[0].data_ptr(), g[2].data_ptr(), g[1].data_ptr(), g[3].data_ptr(), g[4].data_ptr(), _ptr(g[5]), g[6].data_ptr(),
        g[7].data_ptr())


def _colour_backward(p, V, radii, arenas, dpix, grads, W, H, device, deterministic, pairs):
    """One colour backward into `grads`, through gsr_backward_batch or (deterministic) gsr_backward_batch_det with a scratch block
    for lists of `pairs` pairs per view."""
    head = _bwd_head(p, V, radii, arenas, dpix, grads)
    stream = _stream_handle(device)
    if deterministic:
        CALLS["backward_det"] += 1
        scratch = det_scratch(V, p.P, W, H, pairs, arenas[3], device)
        _check(lib.gsr_backward_batch_det(*head, scratch.data_ptr(), scratch.numel(), stream))
    else:
        CALLS["backward"] += 1
        _check(lib.gsr_backward_batch(*head, stream))


def rasterize_gaussians_batch(background, means3D, colors, opacity, scales, rotations, scale_modifier, cov3D_precomp,
                              viewmatrices, projmatrices, tan_fovx, tan_fovy, image_height, image_width, sh, degree,
                              camposs, prefiltered, debug, need_backward=True, capacity=None, extra=None):
    """V views of one cloud in one submission (C ABI gsr_forward_batch): viewmatrices / projmatrices [V,4,4] (transposed like
    the reference's settings), camposs [V,3].  Returns (num_rendered list[V], out_color [V,3,H,W], radii [V,P],
    geomBuffer, binningBuffer, imgBuffer).  `capacity` (pairs per view) overrides the remembered arena capacity.
    extra = (values [P,nx] shared by the views or [V,P,nx] per view -- or the pair ([P,4] shared, [V,P,4] per view) for eight channels
    of which only the last four depend on the view --, view_scale [V,nx] or None, bg [nx]) with nx in (4, 8): the
    render also composites those channels with the colour's alphas (gsr_forward_batch_channels) and the result gains a 7th
    element, out_extra [V,nx,H,W].  With need_backward the call also saves what rasterize_gaussians_backward_channels_batch needs
    (gsr_forward_batch_channels_train): a caller-owned extra-state block, kept with the geometry arena (extra_state(geomBuffer))."""
    if means3D.dim() != 2 or means3D.shape[1] != 3:
        raise RuntimeError("means3D must have dimensions (num_points, 3)")
    P, V = means3D.shape[0], viewmatrices.numel() // 16
    fault = _size_fault(P, V, background, sh, colors, opacity, scales, rotations, cov3D_precomp, viewmatrices, projmatrices, camposs)
    if fault is not None:
        raise RuntimeError(fault)
    device = means3D.device
    _require_hip(device)
    H, W = int(image_height), int(image_width)
    byte = dict(dtype=torch.uint8, device=device)
    nx, x_per_view, xv, xs, xb = (0, 0, None, None, None) if extra is None else _extra_layout(extra, P, V, device)
    if P == 0:  # rasterize_points.cu:81: the zero image (not the background) is returned
        e = torch.empty((0,), **byte)
        r0 = ([0] * V, torch.zeros((V, 3, H, W), dtype=torch.float32, device=device),
              torch.zeros((V, 0), dtype=torch.int32, device=device), e, e.clone(), e.clone())
        return r0 if extra is None else r0 + (torch.zeros((V, nx, H, W), dtype=torch.float32, device=device),)
    key = _cap_key(device, P, W, H)
    # everything below -- layout conversions of the inputs, the allocation of outputs and arenas, every kernel -- happens on a side
    # stream that waits for the inputs only (see _OnSideStream); the caller's stream takes the results over when the block ends
    # (only calls of up to OVERLAP_MAX_VIEWS views: a 12-view batch has no tail for the next call's front end to hide behind, and
    # running the two side by side costs 2.5 % on short bursts -- gpurun_out/r4k: 1 754 vs 1 711 frames/s at 20 frames per block)
    if _OVERLAP_ON and V <= OVERLAP_MAX_VIEWS:
        ov = _OnSideStream(device, [background, means3D, colors, opacity, scales, rotations, cov3D_precomp, viewmatrices, projmatrices,
                                    sh, camposs, xv, xs, xb])
    else:
        ov = _NO_CONTEXT
    with _on_device(device), ov:
        if nx:
            xv, xs, xb = _extra_f32(xv, xs, xb, device)
        f32 = dict(dtype=torch.float32, device=device)
        out_extra = torch.empty((V, nx, H, W), **f32) if nx else None
        # every pixel and every radius is written by the kernels (the reference fills both with zeros first)
        out_color = torch.empty((V, 3, H, W), **f32)
        radii = torch.empty((V, P), dtype=torch.int32, device=device)
        stream = _stream_handle(device)
        # (the matrices go over as pointers: [V,4,4] / [V,16] / [4,4] are the same 16 V floats once contiguous)
        p, keep = _params(background, means3D, colors, opacity, scales, rotations, scale_modifier, cov3D_precomp,
                          viewmatrices, projmatrices, tan_fovx, tan_fovy, H, W, sh, degree, camposs, prefiltered, debug,
                          need_backward)
        # the 64-B per-Gaussian gradient records are only carved for calls a backward may follow
        geom = torch.empty((V * _arena_bytes(P, need_backward),), **byte)
        img = torch.empty((V * _image_bytes(W, H),), **byte)
        counts = (C.c_int64 * V)()
        if capacity is None:
            hint = _CAP_HINT.get(key)
            capacity = None if hint is None else int(hint * CAP_SLACK) + 4096
        xstate = [None]
        if capacity is None and V == 1 and not nx:
            # first frame of this configuration: count, then bind (one host round trip, like the reference)
            _check(lib.gsr_forward_stage1(C.byref(p), geom.data_ptr(), geom.numel(), img.data_ptr(), img.numel(),
                                          radii.data_ptr(), counts, stream))
            binning = torch.empty((lib.gsr_binning_bytes(int(counts[0] * CAP_SLACK) + 4096),), **byte)
            _check(lib.gsr_forward_stage2(C.byref(p), geom.data_ptr(), geom.numel(), binning.data_ptr(), binning.numel(),
                                          img.data_ptr(), img.numel(), counts[0], out_color.data_ptr(), stream))
        else:
            if capacity is None:
                capacity = 16 * P      # first batch of this configuration: a guess, corrected by the retry below
            def submit(binning, resume):
                head = (C.byref(p), V, geom.data_ptr(), geom.numel(), img.data_ptr(), img.numel(), binning.data_ptr(), binning.numel(),
                        radii.data_ptr(), out_color.data_ptr(), counts, resume)
                if not nx:
                    return lib.gsr_forward_batch(*head, stream)
                x = (nx, x_per_view, xv.data_ptr(), _ptr(xs), xb.data_ptr(), out_extra.data_ptr())
                if not need_backward:
                    return lib.gsr_forward_batch_channels(*head, *x, stream)
                # the extra-state block is sized with the binning arena (both grow on a retry)
                n = int(capacity) if not resume else need_pairs[0]
                xstate[0] = torch.empty((V * lib.gsr_extra_state_bytes(W, H, n, nx) + 256,), **byte)
                return lib.gsr_forward_batch_channels_train(*head, *x, xstate[0].data_ptr(), xstate[0].numel(), stream)

            need_pairs = [0]
            binning = torch.empty((V * lib.gsr_binning_bytes(int(capacity)),), **byte)
            rc = submit(binning, 0)
            if rc == GSR_RETRY:
                need = need_pairs[0] = int(last_list_pairs(V) * CAP_SLACK) + 4096
                binning = torch.empty((V * lib.gsr_binning_bytes(need),), **byte)
                rc = submit(binning, 1)
            _check(rc)
            if xstate[0] is not None:
                geom._gsr_extra_state = (xstate[0], nx, x_per_view)
        ov.give(out_color, radii, geom, binning, img, out_extra, xstate[0])
        pairs = last_list_pairs(V)   # (same host thread as the forward call: the count is kept per thread)
    del keep
    counts = [int(c) for c in counts]
    _note_counts(key, (pairs,))      # the arena holds the lists: sized by their pairs, not by num_rendered
    if nx:
        return counts, out_color, radii, geom, binning, img, out_extra
    return counts, out_color, radii, geom, binning, img


# ---- the per-view call's short path ----------------------------------------------------------------------------------------
# The reference's caller builds its settings with blocking host->device copies (simple_raw_render.py:79-112), which drain the
# stream once per frame: everything the host does between the last copy and this call's first kernel is time the GPU idles in.
# forward_view / backward_view are rasterize_gaussians_batch / _backward_batch cut down to what ONE view in steady state needs
# before the launch: inline argument checks, the three scratch arenas as ONE allocation (they live and die together: saved for
# the backward as one tensor), outputs in their final shape (no views), sizes from dictionaries.  Anything unusual -- first frame
# of a configuration, debug, P == 0, the overlap mode -- returns None and the caller takes the general path.
_BIN_BYTES = {}
_CAP_QUANTUM = 1 << 16
_TLS_FAST = threading.local()


def _slab_layout(P, W, H, need_backward, capacity):
    g = (_arena_bytes(P, need_backward) + 255) & ~255
    i = (_image_bytes(W, H) + 255) & ~255
    b = _BIN_BYTES.get(capacity)
    if b is None:
        if len(_BIN_BYTES) > 1024:
            _BIN_BYTES.clear()
        b = _BIN_BYTES[capacity] = int(lib.gsr_binning_bytes(capacity))
    return g, i, b


def forward_view(rs, means3D, sh, colors, opacity, scales, rotations, cov3D_precomp, need_backward):
    """One view through gsr_forward_batch.  Returns (num_rendered, color [3,H,W], radii [P], arenas, layout) -- arenas: ONE uint8
    tensor holding the geometry, image and binning arenas at the byte offsets 0, layout[0], layout[0] + layout[1] -- or None when
    the call has to take the general path."""
    device = means3D.device
    P = means3D.shape[0]
    if _OVERLAP_ON or device.type != "cuda" or means3D.dim() != 2 or means3D.shape[1] != 3 or P == 0:
        return None
    H, W = int(rs.image_height), int(rs.image_width)
    hint = _CAP_HINT.get((device.index, P, W, H))
    if hint is None or device.index is None or device.index != torch.cuda.current_device():
        return None
    if _size_fault(P, 1, rs.bg, sh, colors, opacity, scales, rotations, cov3D_precomp, rs.viewmatrix, rs.projmatrix, rs.campos):
        return None     # (the general path raises, naming the tensor)
    p, keep = _params(rs.bg, means3D, colors, opacity, scales, rotations, rs.scale_modifier, cov3D_precomp, rs.viewmatrix,
                      rs.projmatrix, rs.tanfovx, rs.tanfovy, H, W, sh, rs.sh_degree, rs.campos, rs.prefiltered, False, need_backward)
    capacity = (int(hint * CAP_SLACK) + 4096 + _CAP_QUANTUM - 1) // _CAP_QUANTUM * _CAP_QUANTUM
    g, i, b = _slab_layout(P, W, H, need_backward, capacity)
    arenas = torch.empty((g + i + b,), dtype=torch.uint8, device=device)
    color = torch.empty((3, H, W), dtype=_F32, device=device)
    radii = torch.empty((P,), dtype=torch.int32, device=device)
    counts = getattr(_TLS_FAST, "counts", None)
    if counts is None:
        counts = _TLS_FAST.counts = (C.c_int64 * 1)()
        _TLS_FAST.pairs = (C.c_int64 * 1)()
    base = arenas.data_ptr()
    stream = _stream_handle(device)
    rc = lib.gsr_forward_batch(C.byref(p), 1, base, g, base + g, i, base + g + i, b, radii.data_ptr(), color.data_ptr(), counts, 0, stream)
    pairs = _TLS_FAST.pairs
    if rc == GSR_RETRY:
        _check(lib.gsr_last_list_pairs(pairs, 1))
        capacity = (int(pairs[0] * CAP_SLACK) + 4096 + _CAP_QUANTUM - 1) // _CAP_QUANTUM * _CAP_QUANTUM
        g2, i2, b2 = _slab_layout(P, W, H, need_backward, capacity)
        grown = torch.empty((g + i + b2,), dtype=torch.uint8, device=device)
        # the geometry / image halves of the frame are kept: device copy in stream order, then only the binning half is repeated
        grown[:g + i].copy_(arenas[:g + i])
        arenas, b, base = grown, b2, grown.data_ptr()
        rc = lib.gsr_forward_batch(C.byref(p), 1, base, g, base + g, i, base + g + i, b, radii.data_ptr(), color.data_ptr(), counts, 1, stream)
    _check(rc)
    _check(lib.gsr_last_list_pairs(pairs, 1))
    _note_counts((device.index, P, W, H), (int(pairs[0]),))
    return int(counts[0]), color, radii, arenas, (g, i, b)


def backward_view(rs, means3D, radii, colors, scales, rotations, cov3D_precomp, grad_color, sh, arenas, layout, deterministic=False,
                  pairs=None):
    """Backward of forward_view (gsr_backward_batch, V = 1): the reference's 8-tuple.  deterministic: gsr_backward_batch_det with a
    scratch block for lists of `pairs` pairs (None: bounded from the binning arena's size)."""
    device = means3D.device
    H, W = int(grad_color.shape[-2]), int(grad_color.shape[-1])
    p, keep = _follower_params(rs.bg, means3D, colors, scales, rotations, rs.scale_modifier, cov3D_precomp, rs.viewmatrix,
                               rs.projmatrix, rs.tanfovx, rs.tanfovy, H, W, sh, rs.sh_degree, rs.campos, False)
    if grad_color.dtype is not _F32 or grad_color.device != device or not grad_color.is_contiguous():
        grad_color = _f32c(grad_color, device, "dL_dout_color")
    grads = _grad_tensors(p.P, p.M, device, scales.numel() != 0)
    g, i, b = layout
    base = arenas.data_ptr()
    with _on_device(device):
        _colour_backward(p, 1, radii, (base, g, base + g + i, b, base + g, i), grad_color, grads, W, H, device, deterministic, pairs)
    return grads


def rasterize_gaussians(background, means3D, colors, opacity, scales, rotations, scale_modifier, cov3D_precomp,
                        viewmatrix, projmatrix, tan_fovx, tan_fovy, image_height, image_width, sh, degree, campos,
                        prefiltered, debug, need_backward=True):
    """Counterpart of RasterizeGaussiansCUDA (rasterize_points.cu:35-115); same argument order, same
    6-tuple result (num_rendered, out_color, radii, geomBuffer, binningBuffer, imgBuffer)."""
    counts, out_color, radii, geom, binning, img = rasterize_gaussians_batch(
        background, means3D, colors, opacity, scales, rotations, scale_modifier, cov3D_precomp, viewmatrix, projmatrix,
        tan_fovx, tan_fovy, image_height, image_width, sh, degree, campos, prefiltered, debug, need_backward=need_backward)
    return counts[0], out_color[0], radii[0], geom, binning, img


def recolor(background, means3D, colors, sh, degree, campos, image_height, image_width, num_rendered, geomBuffer,
            binningBuffer, imgBuffer, debug=False, need_backward=False):
    """Re-render a finished forward's view(s) with other per-Gaussian colours (exactly one of `colors` / `sh` [P,M,3]
    non-empty), reusing its geometry, sorted lists and ranges (gsr_forward_recolor).  campos [3] -> color [3,H,W];
    campos [V,3] (a batch forward's arenas) -> [V,3,H,W], with `colors` [P,3] shared by the views or [V,P,3] per view.
    need_backward (arenas of a need_backward forward): also rewrite the saves, so that a backward afterwards -- with these
    colours / SH and campos -- differentiates this render (include/gsr.h)."""
    device = means3D.device
    _require_hip(device)
    P, H, W = means3D.shape[0], int(image_height), int(image_width)
    single = campos.numel() == 3
    V = 1 if single else campos.reshape(-1, 3).shape[0]
    out_color = (torch.empty if P != 0 else torch.zeros)((V, 3, H, W), dtype=torch.float32, device=device)   # every pixel is written
    if P != 0:
        with torch.cuda.device(device):
            e = torch.empty(0)
            p, keep = _params(background, means3D, colors, torch.empty((1,), device=device), e, e, 1.0, e,
                              torch.empty((1,), device=device), torch.empty((1,), device=device), 1.0, 1.0, H, W, sh, degree,
                              campos, False, debug, need_backward)
            per_view = int(colors.numel() != 0 and colors.dim() == 3)
            if per_view and tuple(colors.shape) != (V, P, 3):
                raise RuntimeError("recolor: per-view colours must have shape (V, P, 3)")
            _check(lib.gsr_forward_recolor(C.byref(p), V, per_view, geomBuffer.data_ptr(), geomBuffer.numel(), binningBuffer.data_ptr(),
                                           binningBuffer.numel(), imgBuffer.data_ptr(), imgBuffer.numel(),
                                           out_color.data_ptr(), _stream_handle(device)))
            del keep
    return out_color[0] if single else out_color


def rasterize_gaussians_backward_batch(background, means3D, radii, colors, scales, rotations, scale_modifier, cov3D_precomp,
                                       viewmatrices, projmatrices, tan_fovx, tan_fovy, dL_dout_color, sh, degree, camposs,
                                       geomBuffer, binningBuffer, imageBuffer, debug, _alloc=None, deterministic=None, pairs=None):
    """Backward of rasterize_gaussians_batch: dL_dout_color [V,3,H,W], radii [V,P]; gradients summed over the views.
    deterministic (None: the package switch, deterministic_active()): through gsr_backward_batch_det (bit-identical from call to
    call), with a scratch block for lists of `pairs` pairs per view (None: bounded from the binning arena's size).
    Returns the reference's 8-tuple (dL_dmeans2D, dL_dcolors, dL_dopacity, dL_dmeans3D, dL_dcov3D, dL_dsh, dL_dscales,
    dL_drotations).  _alloc(shape, dtype=, device=): allocator of the outputs (tests hand over float-aligned views to
    exercise the C ABI's alignment fallback; default torch.empty)."""
    device = means3D.device
    _require_hip(device)
    P = means3D.shape[0]
    V, H, W = int(dL_dout_color.shape[0]), int(dL_dout_color.shape[2]), int(dL_dout_color.shape[3])
    M = int(sh.shape[1]) if sh.numel() != 0 and sh.shape[0] != 0 else 0
    grads = _grad_tensors(P, M, device, scales.numel() != 0, _alloc)
    if deterministic is None:
        deterministic = deterministic_active()
    if P != 0:
        with _on_device(device):
            p, keep, radii_c, dpix = _bwd_inputs(background, means3D, radii, colors, scales, rotations, scale_modifier, cov3D_precomp,
                                                 viewmatrices, projmatrices, tan_fovx, tan_fovy, dL_dout_color, sh, degree, camposs, debug)
            _colour_backward(p, V, radii_c, _arena_args(geomBuffer, binningBuffer, imageBuffer), dpix, grads, W, H, device,
                             deterministic, pairs)
            del keep
    return grads


def extra_state(geomBuffer):
    """(extra-state block, nx, extra_per_view) a channels forward with need_backward kept with its geometry arena, or None."""
    return getattr(geomBuffer, "_gsr_extra_state", None)


def rasterize_gaussians_backward_channels_batch(background, means3D, radii, colors, scales, rotations, scale_modifier, cov3D_precomp,
                                                viewmatrices, projmatrices, tan_fovx, tan_fovy, dL_dout_color, sh, degree, camposs,
                                                geomBuffer, binningBuffer, imageBuffer, debug, extra, dL_dout_extra, state=None,
                                                deterministic=False, pairs=None, _alloc=None):
    """Backward of rasterize_gaussians_batch(..., extra=(values, view_scale, bg), need_backward=True) (C ABI
    gsr_backward_batch_channels): `extra` is the forward's triple, dL_dout_extra [V,nx,H,W].  Returns the 8-tuple of
    rasterize_gaussians_backward_batch + dL/d values in the layout of the values ([P,nx], [V,P,nx], or the pair ([P,4], [V,P,4])).
    state: the forward's extra_state(geomBuffer) (default: looked up on geomBuffer).
    deterministic: through gsr_backward_batch_channels_det (every output bit-identical from call to call), with a scratch block for
    lists of `pairs` pairs per view (None: bounded from the binning arena's size).  _alloc: allocator of the outputs, as in
    rasterize_gaussians_backward_batch."""
    device = means3D.device
    _require_hip(device)
    P = means3D.shape[0]
    V, H, W = int(dL_dout_color.shape[0]), int(dL_dout_color.shape[2]), int(dL_dout_color.shape[3])
    M = int(sh.shape[1]) if sh.numel() != 0 and sh.shape[0] != 0 else 0
    nx, x_per_view, xv, xs, xb = _extra_layout(extra, P, V, device)
    grads = _grad_tensors(P, M, device, scales.numel() != 0, _alloc)
    n_out = P * 4 * (1 + V) if x_per_view == 2 else P * nx * (V if x_per_view else 1)
    gx = ((_alloc or torch.empty) if P != 0 else torch.zeros)((n_out,), dtype=_F32, device=device)
    if P != 0:
        st = state if state is not None else extra_state(geomBuffer)
        if st is None:
            raise RuntimeError("backward_channels: the forward kept no extra-channel state (a channels forward with need_backward=True)")
        with _on_device(device):
            p, keep, radii_c, dpix = _bwd_inputs(background, means3D, radii, colors, scales, rotations, scale_modifier, cov3D_precomp,
                                                 viewmatrices, projmatrices, tan_fovx, tan_fovy, dL_dout_color, sh, degree, camposs, debug)
            xv, xs, xb = _extra_f32(xv, xs, xb, device)
            dx = _f32c(dL_dout_extra, device, "dL_dout_extra")
            arenas = _arena_args(geomBuffer, binningBuffer, imageBuffer)
            args = _bwd_head(p, V, radii_c, arenas, dpix, grads) + (
                nx, x_per_view, xv.data_ptr(), _ptr(xs), xb.data_ptr(), st[0].data_ptr(), st[0].numel(), dx.data_ptr(), gx.data_ptr())
            if deterministic:
                CALLS["backward_channels_det"] += 1
                scratch = det_scratch(V, P, W, H, pairs, arenas[3], device, nx, x_per_view)
                _check(lib.gsr_backward_batch_channels_det(*args, scratch.data_ptr(), scratch.numel(), _stream_handle(device)))
            else:
                _check(lib.gsr_backward_batch_channels(*args, _stream_handle(device)))
            del keep
    if x_per_view == 2:
        gx = (gx[:P * 4].reshape(P, 4), gx[P * 4:].reshape(V, P, 4))
    else:
        gx = gx.reshape((V, P, nx) if x_per_view else (P, nx))
    return grads + (gx,)


def camera_scratch(V, P, device):
    """the scratch block of one backward_cameras call (gsr_camera_grad_bytes)"""
    return torch.empty((int(lib.gsr_camera_grad_bytes(V, P)),), dtype=torch.uint8, device=device)


def backward_cameras(background, means3D, radii, colors, scales, rotations, scale_modifier, cov3D_precomp, viewmatrices, projmatrices,
                     tan_fovx, tan_fovy, image_height, image_width, sh, degree, camposs, geomBuffer, debug=False, _out=None,
                     _scratch=None):
    """Camera gradients of the last backward on `geomBuffer` (C ABI gsr_backward_cameras): the arguments of that backward, radii
    [V,P].  Returns (dL_dviewmatrices [V,4,4], dL_dprojmatrices [V,4,4], dL_dcamposs [V,3]), the gradients of the matrices as
    stored.  _out / _scratch: the three outputs and the scratch block (tests hand over prefilled ones; default: fresh tensors)."""
    device = means3D.device
    _require_hip(device)
    P, V = means3D.shape[0], viewmatrices.numel() // 16
    new = torch.empty if P != 0 else torch.zeros
    out = _out if _out is not None else (new((V, 4, 4), dtype=_F32, device=device), new((V, 4, 4), dtype=_F32, device=device),
                                         new((V, 3), dtype=_F32, device=device))
    if P != 0:
        CALLS["backward_cameras"] += 1
        with _on_device(device):
            p, keep = _follower_params(background, means3D, colors, scales, rotations, scale_modifier, cov3D_precomp, viewmatrices,
                                       projmatrices, tan_fovx, tan_fovy, image_height, image_width, sh, degree, camposs, debug)
            scratch = _scratch if _scratch is not None else camera_scratch(V, P, device)
            radii_c = radii.contiguous()
            _check(lib.gsr_backward_cameras(C.byref(p), V, radii_c.data_ptr(), geomBuffer.data_ptr(), geomBuffer.numel(),
                                            out[0].data_ptr(), out[1].data_ptr(), out[2].data_ptr(), scratch.data_ptr(),
                                            scratch.numel(), _stream_handle(device)))
            del keep
    return out


def _stats_out(who, t, shape, dtype, device, name):
    """an output of backward_view_stats or contrib_stats (`who`) handed over by the caller: the library writes into it in place"""
    if t is None:
        return None
    if tuple(t.shape) != shape or t.dtype != dtype or t.device != device or not t.is_contiguous():
        raise RuntimeError("%s: %s must be a contiguous %s tensor of shape %s on %s (got %s %s on %s)"
                           % (who, name, dtype, shape, device, t.dtype, tuple(t.shape), t.device))
    return t


def backward_view_stats(background, means3D, radii, colors, scales, rotations, scale_modifier, cov3D_precomp, viewmatrices,
                        projmatrices, tan_fovx, tan_fovy, image_height, image_width, sh, degree, camposs, geomBuffer, debug=False,
                        accumulate=True, grad_norm_sum=None, visible_views=None, max_radius=None, view_grads=False, _out=None):
    """Density-control statistics and per-view gradients of the last backward on `geomBuffer` (C ABI gsr_backward_view_stats): the
    arguments of that backward, radii [V,P].  grad_norm_sum (float32 [P]), visible_views, max_radius (int32 [P]): the caller's
    tensors, updated in place (accumulate) or overwritten; None: not computed.  view_grads: also return the per-view shares
    (dL_dmean2D [V,P,2], dL_dcolor [V,P,3], dL_dopacity [V,P]), else None.  _out: the three share tensors, any of them None (tests
    hand over prefilled ones and subsets; default with view_grads: three fresh tensors)."""
    device = means3D.device
    _require_hip(device)
    P, V = means3D.shape[0], viewmatrices.numel() // 16
    who, i32 = "backward_view_stats", torch.int32
    stats = (_stats_out(who, grad_norm_sum, (P,), _F32, device, "grad_norm_sum"),
             _stats_out(who, visible_views, (P,), i32, device, "visible_views"), _stats_out(who, max_radius, (P,), i32, device, "max_radius"))
    shapes = ((V, P, 2), (V, P, 3), (V, P))
    if _out is not None:
        shares = tuple(_stats_out(who, t, s, _F32, device, n)
                       for t, s, n in zip(_out, shapes, ("dL_dmean2D_views", "dL_dcolor_views", "dL_dopacity_views")))
    elif view_grads:
        new = torch.empty if P != 0 else torch.zeros
        shares = tuple(new(s, dtype=_F32, device=device) for s in shapes)
    else:
        shares = (None, None, None)
    if P != 0:
        CALLS["backward_view_stats"] += 1
        with _on_device(device):
            p, keep = _follower_params(background, means3D, colors, scales, rotations, scale_modifier, cov3D_precomp, viewmatrices,
                                       projmatrices, tan_fovx, tan_fovy, image_height, image_width, sh, degree, camposs, debug)
            radii_c = radii.contiguous()
            _check(lib.gsr_backward_view_stats(C.byref(p), V, radii_c.data_ptr(), geomBuffer.data_ptr(), geomBuffer.numel(),
                                               int(bool(accumulate)), *[None if t is None else t.data_ptr() for t in stats + shares],
                                               _stream_handle(device)))
            del keep
    return shares if (view_grads or _out is not None) else None


def contrib_stats(background, means3D, radii, colors, scales, rotations, scale_modifier, cov3D_precomp, viewmatrices, projmatrices,
                  tan_fovx, tan_fovy, image_height, image_width, sh, degree, camposs, geomBuffer, binningBuffer, imageBuffer,
                  debug=False, accumulate=True, pixel_weights=None, weight_sum=None, weight_max=None, pixel_count=None,
                  dominant_count=None):
    """Per-Gaussian contribution statistics of the last forward or recolor on the three arenas (C ABI gsr_contrib_stats): the
    arguments of that forward, radii [V,P] or None.  weight_sum, weight_max (float32 [P]), pixel_count, dominant_count (int32 [P]):
    the caller's tensors, updated in place (accumulate) or overwritten; None: not computed.  pixel_weights: float32 [V,H,W] on the
    device or None."""
    device = means3D.device
    _require_hip(device)
    P, V = means3D.shape[0], viewmatrices.numel() // 16
    H, W = int(image_height), int(image_width)
    outs = tuple(_stats_out("contrib_stats", t, (P,), dtype, device, name)
                 for t, dtype, name in ((weight_sum, _F32, "weight_sum"), (weight_max, _F32, "weight_max"),
                                        (pixel_count, torch.int32, "pixel_count"), (dominant_count, torch.int32, "dominant_count")))
    if pixel_weights is not None and (tuple(pixel_weights.shape) != (V, H, W) or pixel_weights.dtype != _F32
                                      or pixel_weights.device != device):
        raise RuntimeError("contrib_stats: pixel_weights must be a %s tensor of shape %s on %s (got %s %s on %s)"
                           % (_F32, (V, H, W), device, pixel_weights.dtype, tuple(pixel_weights.shape), pixel_weights.device))
    if P != 0:
        CALLS["contrib_stats"] += 1
        with _on_device(device):
            p, keep = _follower_params(background, means3D, colors, scales, rotations, scale_modifier, cov3D_precomp, viewmatrices,
                                       projmatrices, tan_fovx, tan_fovy, H, W, sh, degree, camposs, debug, need_backward=False)
            radii_c = None if radii is None else radii.contiguous()
            pw = None if pixel_weights is None else pixel_weights.contiguous()
            _check(lib.gsr_contrib_stats(C.byref(p), V, _ptr(radii_c), geomBuffer.data_ptr(), geomBuffer.numel(),
                                         binningBuffer.data_ptr(), binningBuffer.numel(), imageBuffer.data_ptr(), imageBuffer.numel(),
                                         _ptr(pw), int(bool(accumulate)), *[None if t is None else t.data_ptr() for t in outs],
                                         _stream_handle(device)))
            del keep, pw
    return None


def _loss_frames(who, image, target, super_sample):
    """(device, V, W, H, ss) of an image-loss call: float32 contiguous HIP tensors, image [V,3,H ss,W ss] and target [V,3,H,W]"""
    device = image.device
    _require_hip(device)
    ss = int(super_sample)
    for t, name in ((image, "image"), (target, "target")):
        if t.dtype != _F32 or t.dim() != 4 or t.shape[1] != 3 or t.device != device or not t.is_contiguous():
            raise RuntimeError("%s: %s must be a contiguous float32 [V,3,H,W] tensor on %s (got %s %s on %s)"
                               % (who, name, device, t.dtype, tuple(t.shape), t.device))
    V, _, H, W = target.shape
    if tuple(image.shape) != (V, 3, H * ss, W * ss):
        raise RuntimeError("%s: image is %s, the target %s at super_sample = %d needs %s"
                           % (who, tuple(image.shape), tuple(target.shape), ss, (V, 3, H * ss, W * ss)))
    return device, V, W, H, ss


def image_loss_state(V, W, H, device):
    """a state block for image_loss_forward / image_loss_backward (C ABI gsr_image_loss_state_bytes)"""
    return torch.empty(int(lib.gsr_image_loss_state_bytes(V, W, H)), dtype=torch.uint8, device=device)


def image_loss_forward(image, target, lambda_dssim, super_sample=1, state=None):
    """C ABI gsr_image_loss_forward: the [V,4] loss terms (L1, SSIM, MSE, (1 - lambda) L1 + lambda (1 - SSIM)) of the frames `image`
    against `target`.  state: a block of image_loss_state the backward reads afterwards, or None (metrics only)."""
    device, V, W, H, ss = _loss_frames("image_loss_forward", image, target, super_sample)
    terms = torch.empty((V, 4), dtype=_F32, device=device)
    with _on_device(device):
        _check(lib.gsr_image_loss_forward(V, W, H, ss, float(lambda_dssim), image.data_ptr(), target.data_ptr(), terms.data_ptr(),
                                          None if state is None else state.data_ptr(), 0 if state is None else state.numel(),
                                          _stream_handle(device)))
    return terms


def image_loss_backward(image, target, lambda_dssim, super_sample, state, dL_dloss=None, out=None):
    """C ABI gsr_image_loss_backward after image_loss_forward with the same arguments and state: dL/d image, shaped like image.
    dL_dloss: float32 [V] on the device, or None for 1 per view.  out: the tensor to write into (every element is written)."""
    device, V, W, H, ss = _loss_frames("image_loss_backward", image, target, super_sample)
    if dL_dloss is not None:
        if dL_dloss.dtype != _F32 or tuple(dL_dloss.shape) != (V,) or dL_dloss.device != device:
            raise RuntimeError("image_loss_backward: dL_dloss must be a float32 [%d] tensor on %s (got %s %s on %s)"
                               % (V, device, dL_dloss.dtype, tuple(dL_dloss.shape), dL_dloss.device))
        dL_dloss = dL_dloss.contiguous()
    if out is None:
        out = torch.empty_like(image)
    elif out.dtype != _F32 or out.shape != image.shape or out.device != device or not out.is_contiguous():
        raise RuntimeError("image_loss_backward: out must be a contiguous float32 tensor shaped like image on %s" % device)
    with _on_device(device):
        _check(lib.gsr_image_loss_backward(V, W, H, ss, float(lambda_dssim), image.data_ptr(), target.data_ptr(), _ptr(dL_dloss),
                                           None if state is None else state.data_ptr(), 0 if state is None else state.numel(),
                                           out.data_ptr(), _stream_handle(device)))
    return out


class AdamGroup(C.Structure):
    """gsr_adam_group of include/gsr.h"""
    _fields_ = [("param", _fp), ("grad", _fp), ("exp_avg", _fp), ("exp_avg_sq", _fp), ("width", C.c_int), ("lr", C.c_float)]


ADAM_MAX_GROUPS = 8


def visible_from_radii(radii, out=None):
    """C ABI gsr_visible_from_radii: the uint8 [P] mask any_v(radii[v] > 0) of the int32 radii [V,P] (or [P]) a rasterize call returned.
    out: the tensor to write into (every element is written)."""
    if radii.dtype != torch.int32 or radii.dim() not in (1, 2) or not radii.is_contiguous():
        raise ValueError("visible_from_radii: radii must be a contiguous int32 [V,P] or [P] tensor (got %s %s)"
                         % (radii.dtype, tuple(radii.shape)))
    V, P = (1, radii.shape[0]) if radii.dim() == 1 else radii.shape
    if out is not None and (out.dtype != torch.uint8 or tuple(out.shape) != (P,) or not out.is_contiguous() or out.device != radii.device):
        raise ValueError("visible_from_radii: out must be a contiguous uint8 [%d] tensor on %s (got %s %s on %s)"
                         % (P, radii.device, out.dtype, tuple(out.shape), out.device))
    device = radii.device
    _require_hip(device)
    if out is None:
        out = torch.empty((P,), dtype=torch.uint8, device=device)
    with _on_device(device):
        _check(lib.gsr_visible_from_radii(V, P, radii.data_ptr(), out.data_ptr(), _stream_handle(device)))
    return out


def adam_step(groups, t, beta1, beta2, eps, visible=None, zero_grads=False):
    """C ABI gsr_adam_step: one Adam step, number t (1 for the first), of every group in ONE launch, in place.  groups: a list of 1..8
    (param, grad, exp_avg, exp_avg_sq, lr), the four of them contiguous float32 tensors of one shape [P, ...] on one HIP device, P common
    to all groups.  visible: a uint8 [P] mask (rows with 0 keep the bits of param and both moments) or None for a dense step.
    zero_grads: every grad is written to 0 after it has been consumed, masked rows included."""
    groups = list(groups)
    if not 1 <= len(groups) <= ADAM_MAX_GROUPS:
        raise ValueError("adam_step: %d groups, the call takes 1..%d" % (len(groups), ADAM_MAX_GROUPS))
    table = (AdamGroup * len(groups))()
    P = None
    for k, (param, grad, exp_avg, exp_avg_sq, lr) in enumerate(groups):
        for t_, name in ((param, "param"), (grad, "grad"), (exp_avg, "exp_avg"), (exp_avg_sq, "exp_avg_sq")):
            if t_.dtype != _F32 or not t_.is_contiguous():
                raise ValueError("adam_step: %s of group %d must be a contiguous float32 tensor (got %s, contiguous: %s)"
                                 % (name, k, t_.dtype, t_.is_contiguous()))
            if t_.shape != param.shape:
                raise ValueError("adam_step: %s of group %d is %s, its param %s" % (name, k, tuple(t_.shape), tuple(param.shape)))
        if param.dim() < 1 or param.shape[0] < 1 or param.numel() < 1:
            raise ValueError("adam_step: param of group %d is %s: [P, ...] with P >= 1 and at least one element per row" % (k, tuple(param.shape)))
        P = param.shape[0] if P is None else P
        if param.shape[0] != P:
            raise ValueError("adam_step: group %d has %d rows, group 0 has %d: the groups of a call belong to one cloud" % (k, param.shape[0], P))
        table[k] = AdamGroup(param.data_ptr(), grad.data_ptr(), exp_avg.data_ptr(), exp_avg_sq.data_ptr(), param.numel() // P, float(lr))
    if visible is not None and (visible.dtype != torch.uint8 or tuple(visible.shape) != (P,) or not visible.is_contiguous()):
        raise ValueError("adam_step: visible must be a contiguous uint8 [%d] tensor (got %s %s)" % (P, visible.dtype, tuple(visible.shape)))
    device = groups[0][0].device
    _require_hip(device)
    for k, g in enumerate(groups):
        for t_ in g[:4]:
            if t_.device != device:
                raise ValueError("adam_step: a tensor of group %d is on %s, group 0 on %s" % (k, t_.device, device))
    if visible is not None and visible.device != device:
        raise ValueError("adam_step: visible is on %s, the groups on %s" % (visible.device, device))
    with _on_device(device):
        _check(lib.gsr_adam_step(P, len(groups), table, int(t), float(beta1), float(beta2), float(eps),
                                 None if visible is None else visible.data_ptr(), 1 if zero_grads else 0, _stream_handle(device)))


class DensityRuleStruct(C.Structure):
    """gsr_density_rule of include/gsr.h"""
    _fields_ = [("grad_threshold", C.c_float), ("dense_size", C.c_float), ("min_opacity", C.c_float), ("max_screen_radius", C.c_int),
                ("max_world_size", C.c_float), ("log_scales", C.c_int), ("normalize_rotations", C.c_int), ("seed", C.c_uint64)]


class DensityGroup(C.Structure):
    """gsr_density_group of include/gsr.h"""
    _fields_ = [("src", _fp), ("dst", _fp), ("width", C.c_int), ("role", C.c_int)]


DENSITY_MAX_GROUPS = 8
DENSITY_PRUNED, DENSITY_KEPT, DENSITY_CLONED, DENSITY_CLONED_COPY, DENSITY_SPLIT = range(5)        # GSR_DENSITY_* action codes
DENSITY_COPY, DENSITY_MEANS, DENSITY_SCALES, DENSITY_MOMENT = range(4)                             # GSR_DENSITY_* roles


def _density_input(t, dtype, shape, device, name, who):
    if t.dtype != dtype or tuple(t.shape) != tuple(shape) or not t.is_contiguous():
        raise ValueError("%s: %s must be a contiguous %s %s tensor (got %s %s, contiguous: %s)"
                         % (who, name, dtype, list(shape), t.dtype, tuple(t.shape), t.is_contiguous()))
    if device is not None and t.device != device:
        raise ValueError("%s: %s is on %s, scales on %s" % (who, name, t.device, device))


def density_plan(rule, scales, opacities, grad_norm_sum, visible_views, max_radius, prune_mask=None):
    """C ABI gsr_density_plan: the decision of adaptive density control for a cloud of P Gaussians.  rule: a DensityRuleStruct;
    scales float32 [P,3]; opacities float32 [P] or [P,1]; grad_norm_sum float32 [P], visible_views and max_radius int32 [P] as
    DensityStats holds them; prune_mask uint8 [P] or None.  Returns (offsets uint32-as-int32 [P+1], action uint8 [P], totals int64 [5]),
    all on the device: nothing is read back."""
    who = "density_plan"
    if scales.dim() != 2 or scales.shape[0] < 1:
        raise ValueError("%s: scales must be [P, 3] with P >= 1 (got %s)" % (who, tuple(scales.shape)))
    P = scales.shape[0]
    _density_input(scales, _F32, (P, 3), None, "scales", who)
    device = scales.device
    if opacities.dim() == 2 and opacities.shape[1] == 1:
        opacities = opacities.view(-1) if opacities.is_contiguous() else opacities
    _density_input(opacities, _F32, (P,), device, "opacities", who)
    _density_input(grad_norm_sum, _F32, (P,), device, "grad_norm_sum", who)
    _density_input(visible_views, torch.int32, (P,), device, "visible_views", who)
    _density_input(max_radius, torch.int32, (P,), device, "max_radius", who)
    if prune_mask is not None:
        _density_input(prune_mask, torch.uint8, (P,), device, "prune_mask", who)
    _require_hip(device)
    offsets = torch.empty((P + 1,), dtype=torch.int32, device=device)
    action = torch.empty((P,), dtype=torch.uint8, device=device)
    totals = torch.empty((5,), dtype=torch.int64, device=device)
    nbytes = lib.gsr_density_scratch_bytes(P)
    scratch = torch.empty((max(nbytes, 256),), dtype=torch.uint8, device=device)
    with _on_device(device):
        _check(lib.gsr_density_plan(P, C.addressof(rule), scales.data_ptr(), opacities.data_ptr(), grad_norm_sum.data_ptr(),
                                    visible_views.data_ptr(), max_radius.data_ptr(), None if prune_mask is None else prune_mask.data_ptr(),
                                    offsets.data_ptr(), action.data_ptr(), totals.data_ptr(), scratch.data_ptr(), nbytes,
                                    _stream_handle(device)))
    return offsets, action, totals


def density_apply(groups, rule, offsets, action, P_out, scales=None, rotations=None, noise=None, index=None):
    """C ABI gsr_density_apply: the output rows of 1..8 groups from a plan, in ONE gather launch.  groups: a list of (src, dst, role),
    src a contiguous float32 [P, ...] tensor, dst a contiguous float32 [P_out, ...] tensor with the same row shape, role one of
    DENSITY_COPY / MEANS / SCALES / MOMENT.  offsets, action: what density_plan returned.  P_out: the host's copy of offsets[P].
    scales [P,3] and rotations [P,4]: needed with a MEANS group.  noise: float32 [P,2,3] or None for the generator of rule.seed.
    index: an int32 [P_out] tensor that receives the output-row -> source map, or None."""
    who = "density_apply"
    groups = list(groups)
    if not 1 <= len(groups) <= DENSITY_MAX_GROUPS:
        raise ValueError("%s: %d groups, the call takes 1..%d" % (who, len(groups), DENSITY_MAX_GROUPS))
    P_out = int(P_out)
    if action.dtype != torch.uint8 or action.dim() != 1 or action.shape[0] < 1 or not action.is_contiguous():
        raise ValueError("%s: action must be a contiguous uint8 [P] tensor (got %s %s)" % (who, action.dtype, tuple(action.shape)))
    P, device = action.shape[0], action.device
    _density_input(offsets, torch.int32, (P + 1,), device, "offsets", who)
    if not 0 <= P_out <= 2 * P:
        raise ValueError("%s: P_out = %d outside 0..2 P = %d" % (who, P_out, 2 * P))
    table = (DensityGroup * len(groups))()
    for k, (src, dst, role) in enumerate(groups):
        for t_, name, rows in ((src, "src", P), (dst, "dst", P_out)):
            if t_.dtype != _F32 or not t_.is_contiguous() or t_.dim() < 1 or t_.shape[0] != rows or t_.device != device:
                raise ValueError("%s: %s of group %d must be a contiguous float32 tensor of %d rows on %s (got %s %s on %s, contiguous: %s)"
                                 % (who, name, k, rows, device, t_.dtype, tuple(t_.shape), t_.device, t_.is_contiguous()))
        if src.shape[1:] != dst.shape[1:] or src.numel() < 1:
            raise ValueError("%s: group %d has source rows of %s and destination rows of %s" % (who, k, tuple(src.shape[1:]), tuple(dst.shape[1:])))
        if role not in (DENSITY_COPY, DENSITY_MEANS, DENSITY_SCALES, DENSITY_MOMENT):
            raise ValueError("%s: role %r of group %d is none of DENSITY_COPY, MEANS, SCALES, MOMENT" % (who, role, k))
        table[k] = DensityGroup(src.data_ptr(), dst.data_ptr(), src.numel() // P, role)
    if scales is not None:
        _density_input(scales, _F32, (P, 3), device, "scales", who)
    if rotations is not None:
        _density_input(rotations, _F32, (P, 4), device, "rotations", who)
    if noise is not None:
        _density_input(noise, _F32, (P, 2, 3), device, "noise", who)
    if index is not None:
        _density_input(index, torch.int32, (P_out,), device, "index", who)
    _require_hip(device)
    if P_out == 0:       # nothing to write (and an empty destination has no address to pass)
        return
    with _on_device(device):
        _check(lib.gsr_density_apply(P, len(groups), table, C.addressof(rule), offsets.data_ptr(), action.data_ptr(), _ptr(scales),
                                     _ptr(rotations), _ptr(noise), _ptr(index), P_out, _stream_handle(device)))


CLOUD_MAX_K = 32
CLOUD_OUTPUTS = ("spacing", "cov6", "eigenvalues", "normals", "rotations")      # gsr_cloud_geometry's outputs, in its argument order
_CLOUD_WIDTH = dict(spacing=(), cov6=(6,), eigenvalues=(3,), normals=(3,), rotations=(4,))


def _cloud_points(points, who):
    if points.dim() != 2 or points.shape[0] < 1 or points.shape[1] != 3:
        raise ValueError("%s: points must be [P, 3] with P >= 1 (got %s)" % (who, tuple(points.shape)))
    if points.dtype != _F32 or not points.is_contiguous():
        raise ValueError("%s: points must be a contiguous torch.float32 tensor (got %s, contiguous: %s)"
                         % (who, points.dtype, points.is_contiguous()))
    return points.shape[0]


def knn(points, K, want_d2=True):
    """C ABI gsr_knn: the exact K nearest neighbours of every point of a contiguous float32 [P, 3] cloud, ties to the lower index.
    Returns (idx int32 [P, K], d2 float32 [P, K] or None), ascending, padded with -1 / +inf; on the device, nothing is read back."""
    who = "knn"
    P = _cloud_points(points, who)
    K = int(K)
    if not 1 <= K <= CLOUD_MAX_K:
        raise ValueError("%s: K = %d outside 1..%d" % (who, K, CLOUD_MAX_K))
    device = points.device
    _require_hip(device)
    idx = torch.empty((P, K), dtype=torch.int32, device=device)
    d2 = torch.empty((P, K), dtype=_F32, device=device) if want_d2 else None
    nbytes = lib.gsr_knn_scratch_bytes(P, K)
    scratch = torch.empty((max(nbytes, 256),), dtype=torch.uint8, device=device)
    with _on_device(device):
        _check(lib.gsr_knn(P, points.data_ptr(), K, idx.data_ptr(), _ptr(d2), scratch.data_ptr(), scratch.numel(), _stream_handle(device)))
    return idx, d2


def cloud_geometry(points, knn_idx, k_s=3, k_n=None, orient_to=None, want=CLOUD_OUTPUTS):
    """C ABI gsr_cloud_geometry: per-point geometry from neighbour lists.  points float32 [P, 3], knn_idx int32 [P, K] (as knn returns
    it).  k_s: neighbours of the spacing (3: 3DGS's initial scale), clipped to K; k_n: neighbours of the covariance (None: K).
    orient_to: three numbers the normals are turned away from, or None.  want: the outputs to compute, names of CLOUD_OUTPUTS.
    Returns a dict name -> tensor (spacing [P], cov6 [P, 6], eigenvalues [P, 3] ascending, normals [P, 3], rotations [P, 4])."""
    who = "cloud_geometry"
    P = _cloud_points(points, who)
    device = points.device
    if knn_idx.dtype != torch.int32 or knn_idx.dim() != 2 or knn_idx.shape[0] != P or not knn_idx.is_contiguous() or \
            not 1 <= knn_idx.shape[1] <= CLOUD_MAX_K:
        raise ValueError("%s: knn_idx must be a contiguous torch.int32 [P = %d, K in 1..%d] tensor (got %s %s, contiguous: %s)"
                         % (who, P, CLOUD_MAX_K, knn_idx.dtype, tuple(knn_idx.shape), knn_idx.is_contiguous()))
    if knn_idx.device != device:
        raise ValueError("%s: knn_idx is on %s, points on %s" % (who, knn_idx.device, device))
    K = knn_idx.shape[1]
    k_s, k_n = min(int(k_s), K), K if k_n is None else int(k_n)
    if k_s < 1 or not 1 <= k_n <= K:
        raise ValueError("%s: k_s = %d (at least 1), k_n = %d (1..K = %d)" % (who, k_s, k_n, K))
    want = tuple(want)
    if not want or any(w not in CLOUD_OUTPUTS for w in want):
        raise ValueError("%s: want = %r: one or more of %s" % (who, want, ", ".join(CLOUD_OUTPUTS)))
    o = None
    if orient_to is not None:
        o = [float(v) for v in (orient_to.tolist() if hasattr(orient_to, "tolist") else orient_to)]
        if len(o) != 3:
            raise ValueError("%s: orient_to takes three numbers (got %d)" % (who, len(o)))
        o = (C.c_float * 3)(*o)
    _require_hip(device)
    out = {w: torch.empty((P,) + _CLOUD_WIDTH[w], dtype=_F32, device=device) for w in CLOUD_OUTPUTS if w in want}
    with _on_device(device):
        _check(lib.gsr_cloud_geometry(P, points.data_ptr(), K, knn_idx.data_ptr(), k_s, k_n, None if o is None else C.addressof(o),
                                      *[_ptr(out.get(w)) for w in CLOUD_OUTPUTS], _stream_handle(device)))
    return out


def rasterize_gaussians_backward(background, means3D, radii, colors, scales, rotations, scale_modifier, cov3D_precomp,
                                 viewmatrix, projmatrix, tan_fovx, tan_fovy, dL_dout_color, sh, degree, campos,
                                 geomBuffer, R, binningBuffer, imageBuffer, debug, deterministic=None, pairs=None):
    """Counterpart of RasterizeGaussiansBackwardCUDA (rasterize_points.cu:117-196); same argument order,
    same 8-tuple (dL_dmeans2D, dL_dcolors, dL_dopacity, dL_dmeans3D, dL_dcov3D, dL_dsh, dL_dscales, dL_drotations)."""
    return rasterize_gaussians_backward_batch(
        background, means3D, radii.reshape(1, -1), colors, scales, rotations, scale_modifier, cov3D_precomp, viewmatrix,
        projmatrix, tan_fovx, tan_fovy, dL_dout_color.reshape((1,) + tuple(dL_dout_color.shape[-3:])), sh, degree, campos,
        geomBuffer, binningBuffer, imageBuffer, debug, deterministic=deterministic, pairs=pairs)


def mark_visible(means3D, viewmatrix, projmatrix):
    """Counterpart of markVisible (rasterize_points.cu:198-217)."""
    device = means3D.device
    _require_hip(device)
    P = means3D.shape[0]
    present = torch.zeros((P,), dtype=torch.bool, device=device)
    if P != 0:
        with torch.cuda.device(device):
            m = _f32c(means3D, device, "means3D")
            v = _f32c(viewmatrix, device, "viewmatrix")
            pr = _f32c(projmatrix, device, "projmatrix")
            _check(lib.gsr_mark_visible(P, m.data_ptr(), v.data_ptr(), pr.data_ptr(), present.data_ptr(),
                                        _stream_handle(device)))
    return present


# ---- inspection helpers for tests / bench (not part of the reference API) -------------------------------
_QSPEC = {
    "DEPTHS": (torch.float32, lambda P, R, T, N: (P,)), "MEANS2D": (torch.float32, lambda P, R, T, N: (P, 2)),
    "CONIC_OPACITY": (torch.float32, lambda P, R, T, N: (P, 4)), "RGB": (torch.float32, lambda P, R, T, N: (P, 3)),
    "TILES_TOUCHED": (torch.int32, lambda P, R, T, N: (P,)), "POINT_LIST": (torch.int32, lambda P, R, T, N: (R,)),
    "POINT_LIST_KEYS": (torch.int64, lambda P, R, T, N: (R,)), "RANGES": (torch.int32, lambda P, R, T, N: (T, 2)),
    "FINAL_T": (torch.float32, lambda P, R, T, N: (N,)), "N_CONTRIB": (torch.int32, lambda P, R, T, N: (N,)),
    "CLAMPED": (torch.uint8, lambda P, R, T, N: (P, 3)), "TILE_NEED": (torch.int32, lambda P, R, T, N: (T,)),
    "DEPTH_SORT": (torch.int32, lambda P, R, T, N: (4,)), "LIST_PAIRS": (torch.int64, lambda P, R, T, N: (2,)),
}


def query(name, P, W, H, R, geom, binning, img, view=0, n_views=1):
    """Copy one private arena array of `view` out of the arenas of an `n_views` batch (device tensor).  Unsigned data come
    back in same-width signed dtypes."""
    if name in ("POINT_LIST", "POINT_LIST_KEYS"):
        # the lists hold LIST_PAIRS[0] pairs: R (the reference's num_rendered) with reference_lists, fewer with footprint clipping
        R = int(query("LIST_PAIRS", P, W, H, R, geom, binning, img, view=view, n_views=n_views)[0])
    dtype, shp = _QSPEC[name]
    T = ((W + 15) // 16) * ((H + 15) // 16)
    out = torch.zeros(shp(P, R, T, W * H), dtype=dtype, device=geom.device)
    if out.numel() == 0:
        return out
    p = GsrParams()
    p.P, p.W, p.H = P, W, H
    # view v's arenas start v strides into the allocations (include/gsr.h: V identically laid out single-view arenas)
    g_stride, i_stride = lib.gsr_geom_bytes_inference(P) - 256, lib.gsr_image_bytes(W, H) - 256
    b_stride = ((binning.numel() - 256) // n_views) // 256 * 256 if binning.numel() else 0
    if geom.data_ptr() % 256 or img.data_ptr() % 256 or (binning.numel() and binning.data_ptr() % 256):
        raise RuntimeError("query: arena base pointers are expected to be 256-byte aligned")
    with torch.cuda.device(geom.device):
        _check(lib.gsr_query(C.byref(p), Q[name], geom.data_ptr() + view * g_stride,
                             (binning.data_ptr() + view * b_stride) if binning.numel() else None, b_stride + 256,
                             img.data_ptr() + view * i_stride, int(R), out.data_ptr(), out.numel() * out.element_size(),
                             _stream_handle(geom.device)))
    return out


def grad_records(geom, P, view=0, n_views=1):
    """The [P, 16] render-level gradient records of `view` (mean2D.xy, conic.xyw, colour rgb, opacity, 7 unused words) as the
    last backward on these arenas left them: the counterpart of the reference's internal dL_dconic / dL_dmean2D / dL_dcolors /
    dL_dopacity accumulators (rasterize_points.cu:151-159), for tests that pin the render backward on its own.  The records
    follow the n_views per-view geometry arenas inside a need_backward geometry allocation (include/gsr.h)."""
    g_stride = lib.gsr_geom_bytes_inference(P) - 256
    gr_stride = lib.gsr_geom_bytes(P) - lib.gsr_geom_bytes_inference(P)
    if geom.data_ptr() % 256:
        raise RuntimeError("grad_records: arena base pointers are expected to be 256-byte aligned")
    if geom.numel() < n_views * (g_stride + gr_stride):
        raise RuntimeError("grad_records: not a need_backward geometry arena of %d views" % n_views)
    off = n_views * g_stride + view * gr_stride
    return geom[off:off + P * 64].view(torch.float32).view(P, 16).clone()


class ClockProbe:
    """Shader-clock readings under load (bench / profiles): launch() enqueues the library's one-wave probe kernel on a side
    stream of its own, next to whatever the device is running; mhz() waits for the probes and returns one effective shader
    clock per launch, in MHz (include/gsr.h gsr_clock_probe_launch)."""

    def __init__(self, device, capacity=256, iters=256):
        self.device, self.iters, self.n, self._mu = device, int(iters), 0, threading.Lock()
        with torch.cuda.device(device):
            self.buf = torch.zeros((capacity, 2), dtype=torch.int64, device=device)
            self.stream = torch.cuda.Stream(device=device)
            self.khz = int(lib.gsr_wall_clock_khz())
        torch.cuda.synchronize(device)

    def launch(self):
        with self._mu:
            if self.n >= self.buf.shape[0]:
                return
            slot = self.n
            self.n += 1
        with torch.cuda.device(self.device):
            _check(lib.gsr_clock_probe_launch(self.buf.data_ptr() + 16 * slot, self.iters, self.stream.cuda_stream))

    def mhz(self, first=0):
        """effective shader clock of probes first .. n-1 (MHz); [] when the wall clock rate is unknown"""
        self.stream.synchronize()
        rows = self.buf[first:self.n].cpu().numpy()
        if self.khz <= 0:
            return []
        return [float(s) / float(w) * self.khz / 1e3 for s, w in rows if w > 0]


def selftest(device):
    with torch.cuda.device(device):
        _check(lib.gsr_selftest(_stream_handle(device)))


SORT_KEY16, SORT_SMALL_BLOCKS, SORT_DEPTH_CTL = 1, 2, 4


def sort_probe(keys, vals, cap, end_bit, V=1, stride=0, counts=None, small_blocks=False, depth_ctl=False):
    """The library's radix sort on device arrays (tests; include/gsr.h gsr_sort_probe).  keys: contiguous int32 or int16 tensor
    (the bit patterns of uint32_t / uint16_t keys) holding V views `stride` bytes apart; vals: int32 tensor laid out the same way,
    or None for index values; counts: int64 tensor [V, k] whose column 0 holds the views' element counts, or None (cap each).
    Returns (keys_out like keys, vals_out int32 with a view every `stride` bytes, ctl int32 [V, 4] or None)."""
    _require_hip(keys.device)
    if keys.dtype not in (torch.int32, torch.int16) or not keys.is_contiguous():
        raise RuntimeError("sort_probe: keys are a contiguous int32 or int16 tensor")
    flags = ((SORT_KEY16 if keys.dtype == torch.int16 else 0) | (SORT_SMALL_BLOCKS if small_blocks else 0)
             | (SORT_DEPTH_CTL if depth_ctl else 0))
    nbytes = (V - 1) * int(stride) + int(cap) * 4
    if keys.numel() * keys.element_size() < (V - 1) * int(stride) + int(cap) * keys.element_size() or \
            (vals is not None and (vals.dtype != torch.int32 or not vals.is_contiguous() or vals.numel() * 4 < nbytes)):
        raise RuntimeError("sort_probe: arrays shorter than V views of cap elements")
    if counts is not None and (counts.dtype != torch.int64 or counts.dim() != 2 or counts.shape[0] != V or not counts.is_contiguous()):
        raise RuntimeError("sort_probe: counts are a contiguous int64 tensor [V, k]")
    keys_out = torch.zeros_like(keys)
    vals_out = torch.zeros(max(1, (nbytes + 3) // 4), dtype=torch.int32, device=keys.device)
    ctl = torch.zeros((V, 4), dtype=torch.int32, device=keys.device) if depth_ctl else None
    with torch.cuda.device(keys.device):
        _check(lib.gsr_sort_probe(keys.data_ptr(), _ptr(vals), int(stride), _ptr(counts),
                                  counts.shape[1] * 8 if counts is not None else 0, V, int(cap), int(end_bit), flags,
                                  keys_out.data_ptr(), vals_out.data_ptr(), _ptr(ctl), _stream_handle(keys.device)))
    return keys_out, vals_out, ctl


def tile_ranges_probe(keys, counts, cap, T, V=1, stride=0):
    """The tile-range search on sorted device keys (tests; include/gsr.h gsr_tile_ranges_probe).  keys: contiguous int32 or int16
    tensor, V views `stride` bytes apart; counts: int64 tensor [V, k], column 0 = the views' key counts.  Returns int32 [V, T, 2]."""
    _require_hip(keys.device)
    if keys.dtype not in (torch.int32, torch.int16) or not keys.is_contiguous():
        raise RuntimeError("tile_ranges_probe: keys are a contiguous int32 or int16 tensor")
    if keys.numel() < ((V - 1) * int(stride)) // keys.element_size() + int(cap):
        raise RuntimeError("tile_ranges_probe: keys shorter than V views of cap elements")
    if counts.dtype != torch.int64 or counts.dim() != 2 or counts.shape[0] != V or not counts.is_contiguous():
        raise RuntimeError("tile_ranges_probe: counts are a contiguous int64 tensor [V, k]")
    ranges = torch.full((V, max(1, int(T)), 2), -1, dtype=torch.int32, device=keys.device)
    with torch.cuda.device(keys.device):
        _check(lib.gsr_tile_ranges_probe(keys.data_ptr() if keys.numel() else None, int(stride), counts.data_ptr(), counts.shape[1] * 8,
                                         V, int(cap), int(T), int(keys.dtype == torch.int16), ranges.data_ptr(),
                                         _stream_handle(keys.device)))
    return ranges


def set_backward_moments(mode):
    """How the render backward's pixel contraction takes its second moments: 0 about the quadrant centre, 1 about the four
    sub-quadrant centres (mean2D / conic sums 1.25x / 2.0x the reference build's rounding error instead of 1.85x / 4.3x, +8 % of
    that kernel's time), 2 (default) per batch of eight entries, the sub-quadrant way only where a splat lies far from the quadrant
    centre in its own sigmas (1.33x / 2.1x, +0.8 %); include/gsr.h gsr_set_backward_moments, GSR_BWD_SUBQ.  Returns the mode in force."""
    return int(lib.gsr_set_backward_moments(int(mode)))


_RENDER_MATH = {"exact": 0, "fast": 1}


def _math_mode(mode, what):
    if isinstance(mode, str):
        if mode not in _RENDER_MATH:
            raise ValueError("%s is 'exact' or 'fast' (0 or 1), not %r" % (what, mode))
        return _RENDER_MATH[mode]
    m = int(mode)
    if isinstance(mode, bool) or m not in (0, 1):
        raise ValueError("%s is 'exact' or 'fast' (0 or 1), not %r" % (what, mode))
    return m


def set_render_math(mode):
    """Arithmetic of the inference forwards (need_backward = False): "exact" / 0 (default) bit-identical to the reference build,
    "fast" / 1 fewer instructions per (pixel, entry), within the 1e-4 contract of the exact mode except at threshold decisions,
    deterministic, not bit-identical to the reference; training forwards ignore it (include/gsr.h gsr_set_render_math,
    GSR_RENDER_MATH).  Process-wide.  Returns the name of the mode in force."""
    lib.gsr_set_render_math(_math_mode(mode, "render math"))
    return get_render_math()


def get_render_math():
    """"exact" or "fast": the arithmetic mode of the inference forwards in force"""
    return "fast" if int(lib.gsr_set_render_math(-1)) == 1 else "exact"


def set_train_math(mode):
    """Arithmetic of training calls (need_backward = True): "exact" / 0 (default), or "fast" / 1: the colour forwards run the fast
    kernels of set_render_math("fast") and save from them, and the render backward that follows re-evaluates alpha with the same
    functions -- it follows the forward that wrote the saves, not the switch at backward time.  Deterministic with itself, images
    and gradients within the contract, not bit-identical to the reference; the extra-channel passes stay exact (include/gsr.h
    gsr_set_train_math, GSR_TRAIN_MATH).  Independent of set_render_math.  Process-wide.  Returns the name of the mode in force."""
    lib.gsr_set_train_math(_math_mode(mode, "train math"))
    return get_train_math()


def get_train_math():
    """"exact" or "fast": the arithmetic mode of the training calls in force"""
    return "fast" if int(lib.gsr_set_train_math(-1)) == 1 else "exact"


def set_profiling(on):
    """False / 0: off; True / 1: hipEvents around every stage; 2: around the two render kernels only"""
    lib.gsr_set_profiling(int(on))


def get_profile():
    names = (C.c_char_p * 8192)()
    ms = (C.c_float * 8192)()
    n = lib.gsr_get_profile(names, ms, 8192)
    return [(names[i].decode(), float(ms[i])) for i in range(n)]
