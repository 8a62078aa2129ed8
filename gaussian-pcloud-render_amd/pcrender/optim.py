"""The optimizer step of a training loop, applied by the library (C ABI gsr_adam_step / gsr_visible_from_radii):

    opt = GaussianAdam({"means3D": means3D, "shs": shs, ...}, {"means3D": 1.6e-4, "shs": 2.5e-3, ...})
    frames, radii = rasterize_views(...)
    photometric_loss(frames, target).sum().backward()
    opt.step(radii=radii, zero_grads=True)      # one launch for every group; Gaussians no view saw keep parameters and moments

`GaussianAdam` is torch.optim.Adam (no amsgrad, no weight decay) over the parameter groups of ONE cloud -- every tensor is [P, ...] --
with the visibility mask of splat trainers' "sparse Adam": a row that no view of the batch saw is left alone, moments included, where
dense Adam would keep moving it on stale momentum.  Moments and the mask buffer are allocated at construction; a step allocates
nothing and waits for nothing.  `reindex` carries the moments through densification and pruning; `expon_lr` is the log-linear
schedule trainers use for the positions.

There is no CPU path for `step`: the tensors are float32 on a HIP device.
"""
import math

import torch

from diff_gaussian_rasterization import _native


def expon_lr(step, lr_init, lr_final, delay_steps=0, delay_mult=1.0, max_steps=30000):
    """The log-linear schedule: lr_init at step 0, lr_final from max_steps on, and exp of the linear interpolation of the logarithms in
    between (the geometric mean at the midpoint).  With delay_steps > 0 the rate is scaled by a factor that rises from delay_mult at
    step 0 to 1 at delay_steps along a quarter sine.  0 before step 0 and where both end points are 0."""
    if step < 0 or (lr_init == 0.0 and lr_final == 0.0):
        return 0.0
    scale = 1.0
    if delay_steps > 0:
        scale = delay_mult + (1.0 - delay_mult) * math.sin(0.5 * math.pi * min(max(step / delay_steps, 0.0), 1.0))
    u = min(max(step / max_steps, 0.0), 1.0)
    return scale * math.exp((1.0 - u) * math.log(lr_init) + u * math.log(lr_final))


class GaussianAdam:
    """Adam over the named float32 [P, ...] leaf tensors `params` of one cloud, with the learning rates `lrs` (same names)."""

    def __init__(self, params, lrs, betas=(0.9, 0.999), eps=1e-15):
        self.betas, self.eps, self.t = (float(betas[0]), float(betas[1])), float(eps), 0
        self.lrs = {}
        self._adopt(dict(params))
        if set(lrs) != set(self.params):
            raise ValueError("GaussianAdam: learning rates for %s, parameters %s" % (sorted(lrs), sorted(self.params)))
        for name in self.params:
            self.set_lr(name, lrs[name])
        self.exp_avg = {k: torch.zeros_like(p, memory_format=torch.contiguous_format) for k, p in self.params.items()}
        self.exp_avg_sq = {k: torch.zeros_like(p, memory_format=torch.contiguous_format) for k, p in self.params.items()}

    def _adopt(self, params):
        """take `params` as the cloud: checks, P, the mask buffer"""
        if not 1 <= len(params) <= _native.ADAM_MAX_GROUPS:
            raise ValueError("GaussianAdam: %d parameter groups, one step takes 1..%d" % (len(params), _native.ADAM_MAX_GROUPS))
        first = next(iter(params.values()))
        for name, p in params.items():
            if p.dtype != torch.float32 or p.dim() < 1 or not p.is_contiguous() or not p.is_leaf:
                raise ValueError("GaussianAdam: %s must be a contiguous float32 leaf tensor [P, ...] (got %s %s)" % (name, p.dtype, tuple(p.shape)))
            if p.shape[0] != first.shape[0] or p.shape[0] < 1 or p.device != first.device:
                raise ValueError("GaussianAdam: %s is %s on %s, the first group has %d rows on %s: one cloud, one device"
                                 % (name, tuple(p.shape), p.device, first.shape[0], first.device))
        self.params, self.P = params, first.shape[0]
        self._visible = torch.empty((self.P,), dtype=torch.uint8, device=first.device)

    def set_lr(self, name, lr):
        if name not in self.params:
            raise KeyError(name)
        self.lrs[name] = float(lr)

    def step(self, radii=None, visible=None, zero_grads=False):
        """One step of every parameter that has a gradient, in one launch.  radii: the int32 [V,P] (or [P]) radii of the rasterize call
        that made the gradients -- Gaussians with no positive radius are left alone; or visible: a uint8 [P] mask; neither: a dense
        step.  zero_grads: the gradients are zeroed in the same pass (they stay allocated, so backward() accumulates into zeros)."""
        if radii is not None and visible is not None:
            raise ValueError("GaussianAdam.step: radii and visible are two ways to say the same thing: pass at most one")
        named = [(k, p) for k, p in self.params.items() if p.grad is not None]
        if not named:
            raise RuntimeError("GaussianAdam.step: no parameter has a gradient")
        if radii is not None:
            visible = _native.visible_from_radii(radii, out=self._visible)
        groups = [(p, p.grad, self.exp_avg[k], self.exp_avg_sq[k], self.lrs[k]) for k, p in named]
        _native.adam_step(groups, self.t + 1, self.betas[0], self.betas[1], self.eps, visible=visible, zero_grads=zero_grads)
        self.t += 1

    def state_dict(self):
        return {"step": self.t, "betas": self.betas, "eps": self.eps, "lrs": dict(self.lrs),
                "exp_avg": {k: v.clone() for k, v in self.exp_avg.items()},
                "exp_avg_sq": {k: v.clone() for k, v in self.exp_avg_sq.items()}}

    def load_state_dict(self, state):
        for part in ("exp_avg", "exp_avg_sq"):
            if set(state[part]) != set(self.params):
                raise ValueError("GaussianAdam.load_state_dict: %s of %s, parameters %s" % (part, sorted(state[part]), sorted(self.params)))
            for k, v in state[part].items():
                if v.shape != self.params[k].shape:
                    raise ValueError("GaussianAdam.load_state_dict: %s[%s] is %s, the parameter %s"
                                     % (part, k, tuple(v.shape), tuple(self.params[k].shape)))
        for part in ("exp_avg", "exp_avg_sq"):
            for k, v in state[part].items():
                getattr(self, part)[k].copy_(v)
        self.t, self.betas, self.eps = int(state["step"]), (float(state["betas"][0]), float(state["betas"][1])), float(state["eps"])
        for k, lr in state["lrs"].items():
            self.set_lr(k, lr)

    def adopt(self, new_params, exp_avg, exp_avg_sq):
        """The checked hand-over after densification or pruning for a caller that has built the new moments itself (pcrender.density
        does, in HIP): `new_params` (same names, P' rows each) replace the parameters, `exp_avg` and `exp_avg_sq` (same names, each
        tensor contiguous float32 with its parameter's shape, on its device) replace the moments.  The step count stays."""
        new_params, moments = dict(new_params), (dict(exp_avg), dict(exp_avg_sq))
        for part, name in zip((new_params,) + moments, ("parameters", "exp_avg", "exp_avg_sq")):
            if set(part) != set(self.params):
                raise ValueError("GaussianAdam.adopt: %s %s, the optimizer has %s" % (name, sorted(part), sorted(self.params)))
        new_params = {k: new_params[k] for k in self.params}      # the groups keep their order
        for k, p in new_params.items():
            if p.shape[1:] != self.params[k].shape[1:]:
                raise ValueError("GaussianAdam.adopt: %s has rows of %s, they were %s" % (k, tuple(p.shape[1:]), tuple(self.params[k].shape[1:])))
            for part, name in zip(moments, ("exp_avg", "exp_avg_sq")):
                m = part[k]
                if m.shape != p.shape or m.dtype != torch.float32 or not m.is_contiguous() or m.device != p.device:
                    raise ValueError("GaussianAdam.adopt: %s[%s] must be a contiguous float32 %s tensor on %s (got %s %s on %s)"
                                     % (name, k, tuple(p.shape), p.device, m.dtype, tuple(m.shape), m.device))
        self._adopt(new_params)
        self.exp_avg = {k: moments[0][k] for k in self.params}
        self.exp_avg_sq = {k: moments[1][k] for k in self.params}

    def reindex(self, index, new_params):
        """After densification or pruning: `new_params` (same names, P' rows each) replace the parameters; the moment row of new
        Gaussian i is the old row index[i], or zero where index[i] < 0.  index: an integer [P'] tensor.  The step count stays."""
        new_params = dict(new_params)
        if set(new_params) != set(self.params):
            raise ValueError("GaussianAdam.reindex: parameters %s, the optimizer has %s" % (sorted(new_params), sorted(self.params)))
        new_params = {k: new_params[k] for k in self.params}      # the groups keep their order
        index = torch.as_tensor(index)
        if index.dim() != 1 or index.dtype not in (torch.int32, torch.int64) or int(index.shape[0]) != next(iter(new_params.values())).shape[0]:
            raise ValueError("GaussianAdam.reindex: index must be an integer [P'] tensor, one entry per new row")
        for k, p in new_params.items():
            if p.shape[1:] != self.params[k].shape[1:]:
                raise ValueError("GaussianAdam.reindex: %s has rows of %s, they were %s" % (k, tuple(p.shape[1:]), tuple(self.params[k].shape[1:])))
        if int(index.max()) >= self.P:
            raise ValueError("GaussianAdam.reindex: index reaches row %d, there were %d" % (int(index.max()), self.P))
        self._adopt(new_params)
        index = index.to(device=self._visible.device, dtype=torch.int64)
        kept, source = index >= 0, index.clamp_min(0)
        for part in (self.exp_avg, self.exp_avg_sq):
            for k, p in self.params.items():
                rows = part[k].index_select(0, source)
                part[k] = torch.where(kept.view((-1,) + (1,) * (rows.dim() - 1)), rows, torch.zeros_like(rows)).contiguous()
