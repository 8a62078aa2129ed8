"""The density-control entries (include/gsr.h gsr_density_scratch_bytes / gsr_density_plan / gsr_density_apply) and pcrender.density as
far as they can be reached without a GPU: the exported symbols and their arguments, the header's contract, the refusals that precede
any HIP call, in their order (stand-in pointers that are never followed), the size query, the Python side's refusals, DensityRule and
the default roles, and GaussianAdam.adopt on CPU tensors."""
import ctypes
import inspect
import math
import os
import re

import pytest
import torch

import density_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
A, B, Cc, D, E, Fp, G, Hh, I, J = (0x1000 * k for k in range(1, 11))   # stand-ins for device arrays (never followed)
SYMS = ("gsr_density_scratch_bytes", "gsr_density_plan", "gsr_density_apply")
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
    assert names[SYMS[0]] == ["P"] and N._DECL[SYMS[0]][0] is ctypes.c_size_t
    assert names[SYMS[1]] == ["P", "rule", "scales", "opacities", "grad_norm_sum", "visible_views", "max_radius", "prune_mask", "offsets",
                              "action", "totals", "scratch", "scratch_bytes", "stream"]
    assert names[SYMS[2]] == ["P", "G", "groups", "rule", "offsets", "action", "scales", "rotations", "noise", "index", "P_out", "stream"]
    assert N._DECL[SYMS[1]][1][12] is ctypes.c_size_t and N._DECL[SYMS[2]][1][10] is ctypes.c_int64
    fields = lambda name: [f.strip().split()[-1].lstrip("*") for f in  # noqa: E731
                           re.search(r"typedef struct \{([^}]*)\} %s;" % name, header).group(1).split(";") if f.strip()]
    assert fields("gsr_density_rule") == [f[0] for f in N.DensityRuleStruct._fields_] == list(R.Rule._fields)
    assert fields("gsr_density_group") == [f[0] for f in N.DensityGroup._fields_] == ["src", "dst", "width", "role"]
    assert ctypes.sizeof(N.DensityRuleStruct) == 40 and N.DensityRuleStruct.seed.offset == 32 and ctypes.sizeof(N.DensityGroup) == 24
    assert R.header_codes() == dict(PRUNED=0, KEPT=1, CLONED=2, CLONED_COPY=3, SPLIT=4, COPY=0, MEANS=1, SCALES=2, MOMENT=3)
    assert (N.DENSITY_PRUNED, N.DENSITY_KEPT, N.DENSITY_CLONED, N.DENSITY_CLONED_COPY, N.DENSITY_SPLIT) == (0, 1, 2, 3, 4)
    assert (N.DENSITY_COPY, N.DENSITY_MEANS, N.DENSITY_SCALES, N.DENSITY_MOMENT) == (0, 1, 2, 3) and N.DENSITY_MAX_GROUPS == 8
    # the header states the definition formula by formula, and the contract
    doc = text[text.index("Adaptive density control: clone, split and prune in one pass"):text.index("#define GSR_DENSITY_PRUNED")]
    for phrase in ("sigma = expf(scales)", "g     = grad_norm_sum / (float)max(visible_views, 1)", "hot  = g >= grad_threshold",
                   "dead = opacities[i] < min_opacity || (prune_mask && prune_mask[i])", "smax / 1.6f > max_world_size",
                   "A NaN compares false everywhere", "ascending source index", "offsets[P] = P'", "sigma' = sigma / 1.6f",
                   "s' = s - 0x1.e148a2p-2f", "n = sqrtf(((r r + x x) + y y) + z z)", "d_r = (R[r][0] t0 + R[r][1] t1) + R[r][2] t2",
                   "mu'_r = mu_r + d_r", "Philox4x32-10", "0xD2511F53", "0xCD9E8D57", "0x9E3779B9", "0xBB67AE85", "(i, k, 0, 0)",
                   "u_j = ((float)(x_j >> 8) + 0.5f) * 0x1p-24f", "r01 = sqrtf(-2.0f * logf(u0))", "eps0 = r01 * cosf(6.2831855f * u1)",
                   "eps1 = r01 * sinf(6.2831855f * u1)", "eps2 = sqrtf(-2.0f * logf(u2)) * cosf(6.2831855f * u3)",
                   "counter is the CALL's i", "-1 - i for a new row", "never write past dst", "src and dst must not overlap",
                   "Nothing is read back from the device, no host wait is made, nothing is allocated", "There are no atomics",
                   "bit-identical", "does not depend on which other groups share the call", "HOST array", "GSR_ERR_CAPACITY"):
        assert phrase in doc, phrase
    assert list(inspect.signature(N.density_plan).parameters) == ["rule", "scales", "opacities", "grad_norm_sum", "visible_views",
                                                                  "max_radius", "prune_mask"]
    assert list(inspect.signature(N.density_apply).parameters) == ["groups", "rule", "offsets", "action", "P_out", "scales", "rotations",
                                                                   "noise", "index"]
    build = open(os.path.join(ROOT, "gaussian-pcloud-render_amd", "build.py")).read()
    assert '"density_control"' in build[build.index("UNITS ="):build.index("FLAGS =")]
    for f in ("density_control.hip", "density_control.hpp"):
        assert os.path.exists(os.path.join(ROOT, "gaussian-pcloud-render_amd", "csrc", f))


def _rule(N, **kw):
    v = dict(grad_threshold=2e-4, dense_size=0.05, min_opacity=0.005, max_screen_radius=20, max_world_size=0.5, log_scales=0,
             normalize_rotations=1, seed=7)
    v.update(kw)
    return N.DensityRuleStruct(*[v[f[0]] for f in N.DensityRuleStruct._fields_])


NAN, INF = float("nan"), float("inf")
BAD_RULES = (dict(grad_threshold=-1e-9), dict(grad_threshold=NAN), dict(grad_threshold=INF), dict(dense_size=-0.1), dict(dense_size=NAN),
             dict(dense_size=INF), dict(max_world_size=-1.0), dict(max_world_size=INF), dict(max_world_size=NAN),
             dict(max_screen_radius=-1), dict(min_opacity=NAN))


def test_size_query_is_monotone_a_multiple_of_256_and_zero_for_a_refused_P():
    f = _native().lib.gsr_density_scratch_bytes
    prev = 0
    for P in (1, 2, 255, 256, 257, 1025, R.TWO_ROUNDS_P, 70001, 800_000, 2_000_000, (1 << 30) - 1):
        n = f(P)
        assert n >= prev and n > 0 and n % 256 == 0 and n >= 4 * 4 * -(-P // R.THREADS), (P, n)
        prev = n
    for P in (0, -1, 1 << 30, 2147483647, -2147483648):
        assert f(P) == 0, P


def test_plan_refusals_before_any_hip_call_in_their_order():
    N = _native()
    lib = N.lib
    names = ("rule", "scales", "opacities", "grad_norm_sum", "visible_views", "max_radius", "prune_mask", "offsets", "action", "totals",
             "scratch")

    def call(P=1000, rule="good", scratch_bytes=None, **null):
        r = _rule(N) if rule == "good" else rule
        ptr = dict(zip(names, (None if r is None else ctypes.addressof(r), A, B, Cc, D, E, Fp, G, Hh, I, J)))
        ptr.update({k: None for k in null})
        nbytes = lib.gsr_density_scratch_bytes(P) if scratch_bytes is None else scratch_bytes
        rc = lib.gsr_density_plan(P, *[ptr[k] for k in names], nbytes, None)
        return rc, lib.gsr_last_error()

    # 1. the sizes, whatever else is wrong
    for P in (0, -5, 1 << 30, 2147483647):
        rc, err = call(P=P, rule=_rule(N, dense_size=NAN), scratch_bytes=0, scales=1)
        assert rc == INVALID and b"density_plan" in err and b"bad sizes" in err, (P, err)
    # 2. the rule, before the pointers and the scratch
    for kw in BAD_RULES:
        rc, err = call(rule=_rule(N, **kw), scratch_bytes=0, offsets=1)
        assert rc == INVALID and b"density_plan" in err and b"bad rule" in err, (kw, err)
    # 3. the pointers (a NULL prune_mask is "no mask", never refused), before the scratch size
    for k in names:
        if k == "prune_mask":
            continue
        rc, err = call(scratch_bytes=0, **({k: 1} if k != "rule" else {}), **({"rule": None} if k == "rule" else {}))
        assert rc == INVALID and b"density_plan" in err and b"is NULL" in err, (k, err)
    # 4. the scratch, with the size needed
    need = lib.gsr_density_scratch_bytes(1000)
    rc, err = call(scratch_bytes=need - 1)
    assert rc == CAPACITY and b"density_plan" in err and str(need).encode() in err, err
    # (min_opacity may be negative or infinite -- logits -- and thresholds of 0 are values: not refused; not exercised, they would launch)


def _table(N, *specs):
    """a HOST array of gsr_density_group from (width, role) or (width, role, dict of pointer overrides)"""
    arr = (N.DensityGroup * max(len(specs), 1))()
    for k, s in enumerate(specs):
        ptr = dict(src=A, dst=B)
        ptr.update(s[2] if len(s) > 2 else {})
        arr[k] = N.DensityGroup(ptr["src"], ptr["dst"], s[0], s[1])
    return arr


def test_apply_refusals_before_any_hip_call_in_their_order():
    N = _native()
    lib = N.lib
    COPY, MEANS, SCALES, MOMENT = R.COPY, R.MEANS, R.SCALES, R.MOMENT

    def call(P=1000, G=None, specs=((3, COPY),), rule="good", groups="table", offsets=Cc, action=D, scales=E, rotations=Fp, noise=None,
             index=None, P_out=10):
        r = _rule(N) if rule == "good" else rule
        table = _table(N, *specs) if groups == "table" else groups
        rc = lib.gsr_density_apply(P, len(specs) if G is None else G, table, None if r is None else ctypes.addressof(r), offsets, action,
                                   scales, rotations, noise, index, P_out, None)
        return rc, lib.gsr_last_error()

    bad_rule, null_src = _rule(N, dense_size=NAN), dict(src=None)
    # 1. P
    for P in (0, -5, 1 << 30):
        rc, err = call(P=P, G=0, rule=bad_rule, P_out=-1)
        assert rc == INVALID and b"density_apply" in err and b"bad sizes P=" in err, (P, err)
    # 2. the group count, the widths, the roles
    for Gn in (0, -1, 9):
        rc, err = call(G=Gn, rule=bad_rule, specs=((0, 7, null_src),), P_out=-1)
        assert rc == INVALID and b"density_apply" in err and b"group count" in err, (Gn, err)
    for P, specs in ((1000, ((0, COPY),)), (1000, ((3, COPY), (-2, COPY))), (1 << 29, ((2, COPY),)), (800_000, ((3, MEANS), (1343, COPY))),
                     (1000, ((4, 4),)), (1000, ((3, COPY), (3, -1)))):
        rc, err = call(P=P, specs=tuple(s + (null_src,) for s in specs) + ((4, MEANS),), rule=bad_rule, P_out=-1)
        assert rc == INVALID and b"density_apply" in err and b"bad sizes in group" in err, (P, specs, err)
    assert b"NULL" in call(P=800_000, specs=((1342, COPY, null_src),))[1]                 # 2 x 800000 x 1342 < 2^31: past the size check
    # 3. MEANS and SCALES take width 3
    for specs in (((4, MEANS),), ((3, COPY), (1, SCALES)), ((48, SCALES), (3, MEANS), (3, MEANS))):
        rc, err = call(specs=tuple(s + (null_src,) for s in specs), rule=bad_rule, P_out=-1)
        assert rc == INVALID and b"density_apply" in err and b"takes width 3" in err, (specs, err)
    # 4. at most one of each
    for specs in (((3, MEANS), (3, MEANS)), ((3, SCALES), (3, COPY), (3, SCALES)), ((3, MEANS), (3, SCALES), (3, MEANS), (3, SCALES))):
        rc, err = call(specs=tuple(s + (null_src,) for s in specs), rule=bad_rule, P_out=-1)
        assert rc == INVALID and b"density_apply" in err and b"at most one of each" in err, (specs, err)
    # 5. the rule
    for kw in BAD_RULES:
        rc, err = call(rule=_rule(N, **kw), specs=((3, MEANS, null_src),), offsets=None, P_out=-1)
        assert rc == INVALID and b"density_apply" in err and b"bad rule" in err, (kw, err)
    # 6. the pointers: scales and rotations only with a MEANS group
    for kw in (dict(groups=None), dict(rule=None), dict(offsets=None), dict(action=None)):
        rc, err = call(P_out=-1, **kw)
        assert rc == INVALID and b"density_apply" in err and b"is NULL" in err, (kw, err)
    for field in ("src", "dst"):
        rc, err = call(specs=((3, COPY), (48, MOMENT, {field: None})), P_out=-1)
        assert rc == INVALID and b"density_apply" in err and b"NULL" in err and b"group 1" in err, (field, err)
    for kw in (dict(scales=None), dict(rotations=None)):
        rc, err = call(specs=((3, SCALES), (3, MEANS)), P_out=-1, **kw)
        assert rc == INVALID and b"density_apply" in err and b"MEANS group is present" in err, (kw, err)
    # 7. P_out; without a MEANS group NULL scales and rotations are fine, and P_out = 0 is GSR_OK before any device call
    for P_out in (-1, 2001, 1 << 40):
        rc, err = call(P_out=P_out, scales=None, rotations=None, specs=((3, SCALES), (4, COPY)))
        assert rc == INVALID and b"density_apply" in err and b"P_out" in err, (P_out, err)
    assert call(P_out=0, scales=None, rotations=None, specs=((3, SCALES), (4, COPY)))[0] == 0
    assert call(P_out=0, specs=((3, MEANS), (48, MOMENT)), index=G)[0] == 0


def _cpu_plan_inputs(P=6):
    return (torch.rand(P, 3), torch.rand(P, 1), torch.rand(P), torch.ones(P, dtype=torch.int32), torch.ones(P, dtype=torch.int32))


def test_python_wrappers_refuse_cpu_tensors_and_malformed_arguments():
    N = _native()
    rule = _rule(N)
    s, o, g, v, r = _cpu_plan_inputs()
    with pytest.raises(RuntimeError, match="no CPU path"):
        N.density_plan(rule, s, o, g, v, r)
    with pytest.raises(RuntimeError, match="no CPU path"):
        N.density_plan(rule, s, o.view(-1), g, v, r, prune_mask=torch.zeros(6, dtype=torch.uint8))
    for bad in ((s.double(), o, g, v, r), (torch.rand(6, 4), o, g, v, r), (torch.rand(3, 6).t(), o, g, v, r), (s, torch.rand(5), g, v, r),
                (s, o, g.half(), v, r), (s, o, g, v.long(), r), (s, o, g, v, torch.ones(7, dtype=torch.int32)), (torch.rand(0, 3), o, g, v, r)):
        with pytest.raises(ValueError):
            N.density_plan(rule, *bad)
    with pytest.raises(ValueError):
        N.density_plan(rule, s, o, g, v, r, prune_mask=torch.zeros(6, dtype=torch.bool))
    offsets, action = torch.zeros(7, dtype=torch.int32), torch.ones(6, dtype=torch.uint8)
    src, dst = torch.rand(6, 16, 3), torch.rand(9, 16, 3)
    with pytest.raises(RuntimeError, match="no CPU path"):
        N.density_apply([(src, dst, N.DENSITY_COPY)], rule, offsets, action, 9)
    for groups in ([], [(src, dst, N.DENSITY_COPY)] * 9, [(src.double(), dst, 0)], [(src, torch.rand(8, 16, 3), 0)], [(src, torch.rand(9, 48), 0)],
                   [(torch.rand(5, 16, 3), dst, 0)], [(src, dst, 4)], [(src, torch.rand(16, 3, 9).permute(2, 0, 1), 0)]):
        with pytest.raises(ValueError):
            N.density_apply(groups, rule, offsets, action, 9)
    for kw in (dict(P_out=13), dict(P_out=-1), dict(scales=torch.rand(6, 4)), dict(rotations=torch.rand(6, 3)), dict(noise=torch.rand(6, 3, 2)),
               dict(index=torch.zeros(9, dtype=torch.int64)), dict(index=torch.zeros(8, dtype=torch.int32))):
        args = dict(P_out=9)
        args.update(kw)
        with pytest.raises(ValueError):
            N.density_apply([(src, dst, 0)], rule, offsets, action, **args)
    with pytest.raises(ValueError):
        N.density_apply([(src, dst, 0)], rule, torch.zeros(6, dtype=torch.int32), action, 9)


def test_density_rule_defaults_and_default_roles():
    from pcrender import density
    sig = inspect.signature(density.densify_and_prune)
    assert list(sig.parameters) == ["params", "stats", "rule", "opt", "prune_mask", "noise", "roles"]
    assert all(sig.parameters[k].default is None for k in ("opt", "prune_mask", "noise", "roles"))
    assert list(inspect.signature(density.plan).parameters) == ["params", "stats", "rule", "prune_mask"]
    r = density.DensityRule(extent=5.0)
    assert (r.grad_threshold, r.percent_dense, r.min_opacity) == (2e-4, 0.01, 0.005)             # 3DGS's
    assert r.dense_size == 0.01 * 5.0 and r.max_world_size == 0.1 * 5.0 and r.max_screen_radius == 0
    r = density.DensityRule(dense_size=0.2, seed=(1 << 63) + 5, log_scales=True, min_opacity=math.log(0.005 / 0.995))
    assert r.dense_size == 0.2 and r.max_world_size == 0.0
    s = r.struct()
    assert s.seed == (1 << 63) + 5 and s.log_scales == 1 and s.normalize_rotations == 1 and s.min_opacity < -5 and s.max_world_size == 0.0
    assert density.DensityRule(extent=2.0, percent_dense=0.05, max_world_size=0.3).struct().dense_size == pytest.approx(0.1, rel=1e-6)
    with pytest.raises(ValueError):
        density.DensityRule()
    names = ["means3D", "shs", "opacities", "scales", "rotations", "anything"]
    assert density.default_roles(names) == dict(means3D="means", shs="copy", opacities="copy", scales="scales", rotations="copy",
                                                anything="copy")
    assert {k: density.ROLES[v] for k, v in density.default_roles(names).items()}["means3D"] == R.MEANS
    assert density.ROLES == dict(copy=R.COPY, means=R.MEANS, scales=R.SCALES, moment=R.MOMENT)
    # refusals that come before any device call
    params = {k: torch.zeros(4, 3) for k in ("means3D", "scales")}
    with pytest.raises(ValueError, match="roles"):
        density.densify_and_prune(params, None, r, roles=dict(means3D="moment"))
    with pytest.raises(ValueError, match="roles"):
        density.densify_and_prune(params, None, r, roles=dict(nothing="copy"))


def _cloud(P=6):
    g = torch.Generator().manual_seed(P)
    params = {"means3D": torch.randn((P, 3), generator=g).requires_grad_(True), "shs": torch.randn((P, 16, 3), generator=g).requires_grad_(True),
              "opacities": torch.randn((P, 1), generator=g).requires_grad_(True)}
    return params, {"means3D": 1.6e-4, "shs": 2.5e-3, "opacities": 5e-2}


def test_gaussian_adam_adopt_on_the_host():
    from pcrender import optim
    assert list(inspect.signature(optim.GaussianAdam.adopt).parameters) == ["self", "new_params", "exp_avg", "exp_avg_sq"]
    params, lrs = _cloud()
    opt = optim.GaussianAdam(params, lrs)
    opt.t = 11
    new_params, _ = _cloud(P=9)
    m = {k: torch.randn_like(p).detach() for k, p in new_params.items()}
    v = {k: torch.rand_like(p).detach() for k, p in new_params.items()}
    opt.adopt(new_params, m, v)
    assert opt.P == 9 and opt.t == 11 and tuple(opt._visible.shape) == (9,) and list(opt.params) == list(params)
    assert all(opt.params[k] is new_params[k] and opt.exp_avg[k] is m[k] and opt.exp_avg_sq[k] is v[k] for k in params)
    assert opt.lrs == lrs
    # what reindex refuses, adopt refuses: names, row shapes; and moments that do not fit their parameters
    other, _ = _cloud(P=4)
    fit = lambda ps: ({k: torch.zeros_like(p).detach() for k, p in ps.items()}, {k: torch.zeros_like(p).detach() for k, p in ps.items()})  # noqa: E731
    for bad in ((dict(means3D=other["means3D"]),) + fit(other),                                    # names
                (other,) + tuple({k: x for k, x in part.items() if k != "shs"} for part in fit(other)),
                (dict(other, shs=torch.zeros(4, 9, 3, requires_grad=True)),) + fit(other),         # rows of another shape
                (other, fit(other)[0], fit(new_params)[1]),                                        # moments of another cloud
                (other, {k: x.double() for k, x in fit(other)[0].items()}, fit(other)[1]),
                (other, fit(other)[0], {k: x.expand(2, *x.shape)[1].transpose(0, -1) for k, x in fit(other)[1].items()}),
                (dict(other, means3D=torch.zeros(5, 3, requires_grad=True)),) + fit(other)):       # not one cloud
        with pytest.raises(ValueError):
            opt.adopt(*bad)
    assert opt.P == 9 and opt.params["shs"] is new_params["shs"] and opt.exp_avg["shs"] is m["shs"]   # refused calls change nothing
    # adopt with the moments reindex would make is reindex
    index = torch.tensor([0, 2, -3, -1, 5, 1, -1, 3, 0])
    a, b = optim.GaussianAdam(*_cloud()), optim.GaussianAdam(*_cloud())
    for o in (a, b):
        gen = torch.Generator().manual_seed(3)
        for k in o.params:
            o.exp_avg[k].copy_(torch.randn(o.params[k].shape, generator=gen))
            o.exp_avg_sq[k].copy_(torch.rand(o.params[k].shape, generator=gen))
    a.reindex(index, new_params)
    pick = lambda t: torch.where((index >= 0).view((-1,) + (1,) * (t.dim() - 1)), t[index.clamp_min(0)], torch.zeros(()))  # noqa: E731
    b.adopt(new_params, {k: pick(x).contiguous() for k, x in b.exp_avg.items()}, {k: pick(x).contiguous() for k, x in b.exp_avg_sq.items()})
    assert all(torch.equal(a.exp_avg[k], b.exp_avg[k]) and torch.equal(a.exp_avg_sq[k], b.exp_avg_sq[k]) for k in a.params)
