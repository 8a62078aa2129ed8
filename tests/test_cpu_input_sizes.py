"""The size check of a forward's input tensors (_native._size_fault), on CPU tensors: the C ABI sees raw pointers, so a tensor with
the wrong number of rows has to be caught where tensors become pointers, before a kernel reads past its end."""
import pytest
import torch

P, V = 5, 2
NAMES = ("bg", "sh", "colors_precomp", "opacities", "scales", "rotations", "cov3D_precomp", "viewmatrices", "projmatrices", "camposs")


def _inputs(colour="sh", M=16, cov="scale_rotation", opacity_shape=(P, 1)):
    """a well-formed input set in _size_fault's argument order, absent optionals as empty tensors"""
    e = torch.Tensor([])
    return dict(bg=torch.zeros(3), sh=torch.zeros(P, M, 3) if colour == "sh" else e,
                colors_precomp=torch.zeros(P, 3) if colour == "precomp" else e, opacities=torch.zeros(opacity_shape),
                scales=torch.zeros(P, 3) if cov == "scale_rotation" else e, rotations=torch.zeros(P, 4) if cov == "scale_rotation" else e,
                cov3D_precomp=torch.zeros(P, 6) if cov == "precomp" else e, viewmatrices=torch.zeros(V, 4, 4),
                projmatrices=torch.zeros(V, 4, 4), camposs=torch.zeros(V, 3))


def _fault(t):
    from diff_gaussian_rasterization import _native as N
    assert tuple(t) == NAMES
    return N._size_fault(P, V, *t.values())


WELL_FORMED = [dict(colour="sh", M=1), dict(colour="sh", M=16), dict(colour="precomp"), dict(cov="precomp"),
               dict(colour="precomp", cov="precomp"), dict(opacity_shape=(P,)), dict(opacity_shape=(P, 1))]


@pytest.mark.parametrize("kw", WELL_FORMED, ids=lambda kw: "-".join("%s=%s" % i for i in kw.items()))
def test_well_formed_inputs_fit(kw):
    assert _fault(_inputs(**kw)) is None


def _rows(t, n):
    """t with n rows more (n < 0: fewer) along its first dimension"""
    return t[:n] if n < 0 else torch.cat([t, t[:n]], 0)


# what each message states as expected, at P = 5 and V = 2
EXPECTED = {"sh": "shape (num_points = 5, coefficients, 3)", "colors_precomp": "3 x num_points = 15 elements",
            "opacities": "1 x num_points = 5 elements", "scales": "3 x num_points = 15 elements",
            "rotations": "4 x num_points = 20 elements", "cov3D_precomp": "6 x num_points = 30 elements",
            "viewmatrices": "16 x num_views = 32 elements", "projmatrices": "16 x num_views = 32 elements",
            "camposs": "3 x num_views = 6 elements"}
# every input in the set in which it is present: spherical harmonics with scales and rotations, then the two precomputed sources
CASES = [(dict(), n) for n in NAMES if n not in ("bg", "colors_precomp", "cov3D_precomp")] + \
        [(dict(colour="precomp", cov="precomp"), n) for n in ("colors_precomp", "cov3D_precomp", "opacities")]


@pytest.mark.parametrize("delta", [-1, 1], ids=["one_row_too_few", "one_row_too_many"])
@pytest.mark.parametrize("kw,name", CASES, ids=["%s-%s" % (n, "precomp" if kw else "sh") for kw, n in CASES])
def test_each_input_with_a_wrong_row_count_is_named(kw, name, delta):
    t = _inputs(**kw)
    t[name] = _rows(t[name], delta)
    fault = _fault(t)
    assert fault is not None and fault.startswith("%s must have %s" % (name, EXPECTED[name])), fault
    assert fault.endswith("(got %s)" % str(tuple(t[name].shape) if name == "sh" else t[name].numel())), fault


def test_other_misfits():
    t = _inputs()
    for bad in (torch.zeros(2), torch.zeros(1)):                 # the kernels read three background values
        assert _fault(dict(t, bg=bad)).startswith("bg must have at least 3")
    assert _fault(dict(t, bg=torch.zeros(4))) is None
    assert _fault(dict(t, sh=torch.zeros(P, 16, 4))).startswith("sh must have shape")      # same rows, wrong last dimension
    assert _fault(dict(t, sh=torch.zeros(P, 48))).startswith("sh must have shape")         # same size, not [P, M, 3]
    assert _fault(dict(t, opacities=torch.zeros(P, 2))).startswith("opacities must have")
    # the first misfit in the order opacities, scales, rotations, cov3D_precomp, colors_precomp, sh, bg, views is the one reported
    assert _fault(dict(t, rotations=torch.zeros(P, 5), scales=torch.zeros(P, 4), camposs=torch.zeros(3))).startswith("scales must have")
    # no views at all
    from diff_gaussian_rasterization import _native as N
    e = torch.Tensor([])
    assert N._size_fault(P, 0, *dict(t, viewmatrices=e, projmatrices=e, camposs=e).values()).startswith("viewmatrices must have")


def test_the_batch_forward_raises_the_named_fault_before_it_asks_for_a_device():
    from diff_gaussian_rasterization import _native as N

    def call(t):
        return N.rasterize_gaussians_batch(t["bg"], torch.zeros(P, 3), t["colors_precomp"], t["opacities"], t["scales"], t["rotations"], 1.0,
                                           t["cov3D_precomp"], t["viewmatrices"], t["projmatrices"], 1.0, 1.0, 8, 8, t["sh"], 3,
                                           t["camposs"], False, False, need_backward=False)

    t = _inputs()
    with pytest.raises(RuntimeError, match=r"^opacities must have 1 x num_points = 5 elements \(got 4\)$"):
        call(dict(t, opacities=torch.zeros(P - 1, 1)))
    with pytest.raises(RuntimeError, match=r"^projmatrices must have 16 x num_views = 32 elements"):
        call(dict(t, projmatrices=torch.zeros(3, 4, 4)))
    with pytest.raises(RuntimeError, match=r"means3D must have dimensions \(num_points, 3\)"):      # (still the first check)
        N.rasterize_gaussians_batch(t["bg"], torch.zeros(P, 4), t["colors_precomp"], t["opacities"][:-1], t["scales"], t["rotations"], 1.0,
                                    t["cov3D_precomp"], t["viewmatrices"], t["projmatrices"], 1.0, 1.0, 8, 8, t["sh"], 3, t["camposs"],
                                    False, False)
    with pytest.raises(RuntimeError, match="no CPU path"):
        call(t)
