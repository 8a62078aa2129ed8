"""Adaptive density control, applied by the library (C ABI gsr_density_plan / gsr_density_apply):

    rule = DensityRule(extent=scene_extent, seed=step)
    new_params, index = densify_and_prune(params, stats, rule, opt=opt)     # clone, split and prune; the optimizer follows
    stats = DensityStats(index.shape[0], index.device)

`params` is the dict of float32 [P, ...] leaves of one cloud (the one GaussianAdam holds), `stats` the DensityStats that
rasterize_views_stats fed.  The decision is 3DGS's densify_and_prune (include/gsr.h states it), evaluated in one pass on the device;
the new cloud is in ascending source order, a Gaussian's rows adjacent.  `index[j]` is the source row of new row j, or -1 - source for a
new Gaussian (a copy or a child): GaussianAdam.reindex takes it as it is.

There is no CPU path: the tensors are float32 on a HIP device.
"""
import dataclasses

import torch

from diff_gaussian_rasterization import _native

ROLES = {"copy": _native.DENSITY_COPY, "means": _native.DENSITY_MEANS, "scales": _native.DENSITY_SCALES, "moment": _native.DENSITY_MOMENT}


@dataclasses.dataclass
class DensityRule:
    """The thresholds of a densification step; the defaults are 3DGS's.  With `extent` (the scene's radius) given, dense_size and
    max_world_size default to percent_dense * extent and 0.1 * extent; without it dense_size has to be given and the world-size test
    is off unless max_world_size is.  min_opacity is compared in the domain the opacities are STORED in: pass logit(0.005) for logits.
    max_screen_radius = 0 and max_world_size = 0 switch their tests off.  log_scales: `scales` holds logarithms; normalize_rotations:
    a child is displaced along the normalised quaternion's axes (3DGS), not the raw one's (what the rasterizer renders)."""
    grad_threshold: float = 2e-4
    percent_dense: float = 0.01
    min_opacity: float = 0.005
    extent: float = None
    dense_size: float = None
    max_screen_radius: int = 0
    max_world_size: float = None
    log_scales: bool = False
    normalize_rotations: bool = True
    seed: int = 0

    def __post_init__(self):
        if self.dense_size is None:
            if self.extent is None:
                raise ValueError("DensityRule: give extent (dense_size = percent_dense * extent) or dense_size")
            self.dense_size = self.percent_dense * self.extent
        if self.max_world_size is None:
            self.max_world_size = 0.0 if self.extent is None else 0.1 * self.extent

    def struct(self):
        """the gsr_density_rule of this rule"""
        return _native.DensityRuleStruct(float(self.grad_threshold), float(self.dense_size), float(self.min_opacity),
                                         int(self.max_screen_radius), float(self.max_world_size), 1 if self.log_scales else 0,
                                         1 if self.normalize_rotations else 0, int(self.seed) & 0xFFFFFFFFFFFFFFFF)


class DensityPlan:
    """What gsr_density_plan left on the device: offsets [P+1] (the exclusive prefix of the rows per Gaussian), action [P] (the
    GSR_DENSITY_* codes), totals [5] = (P', carried rows, copies, children, vanished Gaussians).  `counts` reads the totals: the one
    device-to-host read of a densification step, 40 bytes, made once and kept."""

    def __init__(self, rule, offsets, action, totals):
        self.rule, self.offsets, self.action, self.totals = rule, offsets, action, totals
        self.P, self._counts = action.shape[0], None

    @property
    def counts(self):
        if self._counts is None:
            self._counts = tuple(int(v) for v in self.totals.tolist())
        return self._counts

    @property
    def P_out(self):
        return self.counts[0]


def default_roles(names):
    """the role of every group by its name: means3D is displaced, scales shrunk, everything else copied"""
    return {k: "means" if k == "means3D" else "scales" if k == "scales" else "copy" for k in names}


def plan(params, stats, rule, prune_mask=None):
    """The decision for the cloud `params` (needs "scales" and "opacities") from `stats` under `rule`; prune_mask: a uint8 or bool [P]
    tensor of Gaussians to remove whatever else holds (importance pruning).  Everything stays on the device."""
    if prune_mask is not None and prune_mask.dtype == torch.bool:
        prune_mask = prune_mask.to(torch.uint8)
    struct = rule.struct()
    offsets, action, totals = _native.density_plan(struct, params["scales"].detach(), params["opacities"].detach(), stats.grad_norm_sum,
                                                   stats.visible_views, stats.max_radius, prune_mask)
    return DensityPlan(struct, offsets, action, totals)


def _apply(p, groups, index, **kw):
    """the groups (src, dst, role) in calls of at most DENSITY_MAX_GROUPS.  Every call gets the index: a call writes it (the same
    values each time) and its gather then reads a row's source from it, where a call without one bisects the offsets for every row"""
    for at in range(0, len(groups), _native.DENSITY_MAX_GROUPS):
        _native.density_apply(groups[at:at + _native.DENSITY_MAX_GROUPS], p.rule, p.offsets, p.action, p.P_out, index=index, **kw)


def densify_and_prune(params, stats, rule, opt=None, prune_mask=None, noise=None, roles=None):
    """Clone, split and prune the cloud `params` (a dict of float32 [P, ...] leaves with "means3D", "scales", "rotations" and
    "opacities" among them).  Returns (new_params, index): new leaves of P' rows with requires_grad as the old ones had, and the int32
    [P'] map described above.  opt: a GaussianAdam over the same names, which takes the new leaves and moments built by two more
    gathers (a carried row keeps its moments, a new one starts at zero -- the bits reindex(index, new_params) gives).  noise: float32
    [P,2,3] standard-normal draws per (source, child), or None for the library's generator on rule.seed.  roles: {name: "copy" |
    "means" | "scales"}; by default by name (default_roles).
    The plan is enqueued first and then P' is read: the one unavoidable device-to-host read of the step (the new leaves have to be
    allocated), after everything before it has been enqueued."""
    names = list(params)
    roles = dict(default_roles(names), **(roles or {}))
    if set(roles) != set(names) or any(r not in ("copy", "means", "scales") for r in roles.values()):
        raise ValueError("densify_and_prune: roles %s for the parameters %s: one of copy, means, scales each" % (roles, names))
    if opt is not None and set(opt.params) != set(names):
        raise ValueError("densify_and_prune: parameters %s, the optimizer has %s" % (sorted(names), sorted(opt.params)))
    p = plan(params, stats, rule, prune_mask)
    n = p.P_out                                                   # the read
    device = p.action.device
    new_params = {k: torch.empty((n,) + tuple(v.shape[1:]), dtype=torch.float32, device=device) for k, v in params.items()}
    index = torch.empty((n,), dtype=torch.int32, device=device)
    if n > 0:
        geometry = dict(scales=params["scales"].detach(), rotations=params["rotations"].detach(), noise=noise)
        _apply(p, [(params[k].detach(), new_params[k], ROLES[roles[k]]) for k in names], index, **geometry)
    for k, v in params.items():
        new_params[k].requires_grad_(v.requires_grad)
    if opt is not None:
        moments = []
        for part in (opt.exp_avg, opt.exp_avg_sq):
            new = {k: torch.empty_like(new_params[k], requires_grad=False) for k in opt.params}
            if n > 0:
                _apply(p, [(part[k], new[k], ROLES["moment"]) for k in opt.params], index)
            moments.append(new)
        opt.adopt(new_params, *moments)
    return new_params, index
