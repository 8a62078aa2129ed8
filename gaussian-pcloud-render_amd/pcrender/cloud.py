"""From a raw point cloud to Gaussians on the device: exact k nearest neighbours, the point spacing, PCA normals and oriented discs
(C ABI gsr_knn / gsr_cloud_geometry).

The reference's caller does this on the CPU with Open3D (simple_benchmark.py:263-277): a Python loop of KD-tree queries for the mean
nearest-neighbour distance, then estimate_normals().  Here

    nn = cloud.knn(points, 16)
    geo = cloud.cloud_geometry(points, nn.idx, k_s=1)
    avg_dist = cloud.mean_spacing(geo.spacing)            # the reference's avg_dist
    g = cloud.gaussians_from_points(points, colors, mode="surfel")
    images = raster_passes.render_passes(**g, H_c2w=..., ...)

There is no CPU path: the tensors live on a HIP device."""
import collections

import torch

from diff_gaussian_rasterization import _native

from .raster_passes import pcgc_rescale

Neighbours = collections.namedtuple("Neighbours", "idx d2")
CloudGeometry = collections.namedtuple("CloudGeometry", _native.CLOUD_OUTPUTS)
MODES = ("isotropic", "surfel")


def knn(points, K, want_d2=True):
    """The exact K nearest neighbours of every point of a float32 [P, 3] cloud: Neighbours(idx int32 [P, K], d2 float32 [P, K] or
    None), ascending by (squared distance, index), padded with -1 / +inf.  Points with a non-finite coordinate are absent."""
    return Neighbours(*_native.knn(points, K, want_d2))


def cloud_geometry(points, knn_idx, k_s=3, k_n=None, orient_to=None, want=_native.CLOUD_OUTPUTS):
    """CloudGeometry(spacing, cov6, eigenvalues, normals, rotations) from neighbour lists; outputs not in `want` are None.
    spacing: sqrt of the mean squared distance to the first k_s neighbours (k_s = 3: 3DGS's initial scale; k_s = 1: the nearest
    neighbour's distance).  normals: the unit eigenvector of the smallest eigenvalue of the covariance of a point and its first k_n
    neighbours (None: all of them), turned away from orient_to when that is given.  rotations: the quaternion (r, x, y, z) whose
    axes are (largest-eigenvalue direction, normal x that, normal); the matching scales are sqrt(eigenvalues) reversed."""
    out = _native.cloud_geometry(points, knn_idx, k_s=k_s, k_n=k_n, orient_to=orient_to, want=want)
    return CloudGeometry(*[out.get(k) for k in _native.CLOUD_OUTPUTS])


def mean_spacing(spacing):
    """The mean of the spacing over the points that have a neighbour, as a 0-dim tensor on the device (with k_s = 1: the reference
    caller's avg_dist).  Nothing is read back; float(...) of the result is the caller's choice."""
    has = spacing > 0
    return (spacing * has).sum() / has.sum().clamp_min(1)


def gaussians_from_points(points, colors, mode="isotropic", K=16, k_s=3, scale_factor=1., voxelized=False, log_scales=False,
                          thickness=0.1, offset=512, orient_to=None):
    """Gaussians from positions [P, 3] and colours in [0, 1] [P, 3]: the dict render_passes / train_passes take (means3D, opacities,
    scales, rotations, shs, normals), contiguous float32 tensors ready to become the leaves of GaussianAdam.

    means3D, shs and opacities are simple_primitives': pcgc_rescale(points) for voxelised input, SH = [RGB2SH(colour) | 12 zero rows],
    opacity 1.  The neighbourhoods are taken in the units of means3D, so the scales are world sizes.
      mode "isotropic"   scales = spacing on all three axes, identity quaternions
      mode "surfel"      rotations from the neighbourhood's principal axes; scales (sqrt(l2), sqrt(l1), sqrt(l0)) with the two in-plane
                         axes floored at spacing and the normal axis clamped to thickness x spacing: a disc that closes the surface
    log_scales: the scales are returned as logarithms, as 3DGS stores them (DensityRule(log_scales=True)); the renderer takes exp().
    A point without a neighbour gets the cloud's mean spacing."""
    if mode not in MODES:
        raise ValueError("gaussians_from_points: mode %r is none of %s" % (mode, ", ".join(MODES)))
    if points.dim() != 2 or points.shape[1] != 3 or colors.dim() != 2 or colors.shape[1] != 3 or colors.shape[0] != points.shape[0]:
        raise ValueError("gaussians_from_points: points [P, 3] and colors [P, 3] (got %s and %s)" % (tuple(points.shape), tuple(colors.shape)))
    if not thickness > 0:
        raise ValueError("gaussians_from_points: thickness = %r, a positive fraction of the spacing" % (thickness,))
    P = points.shape[0]
    K = max(1, min(int(K), _native.CLOUD_MAX_K))
    means = (pcgc_rescale(points.float(), offset, scale_factor) if voxelized else points.float()).contiguous()
    nn = knn(means, K, want_d2=False)
    want = ("spacing", "normals") if mode == "isotropic" else ("spacing", "eigenvalues", "normals", "rotations")
    geo = cloud_geometry(means, nn.idx, k_s=k_s, orient_to=orient_to, want=want)
    spacing = torch.where(geo.spacing > 0, geo.spacing, mean_spacing(geo.spacing)).unsqueeze(1)
    if mode == "isotropic":
        scales = spacing.expand(P, 3).contiguous()
        rotations = torch.tensor([1, 0, 0, 0], dtype=torch.float32, device=means.device).expand(P, 4).contiguous()
    else:
        axes = geo.eigenvalues.clamp_min(0).sqrt().flip(1)                                   # (sqrt l2, sqrt l1, sqrt l0)
        scales = torch.cat([torch.maximum(axes[:, 0:2], spacing), (thickness * spacing).expand(P, 1)], dim=1).contiguous()
        rotations = geo.rotations
    dc = ((colors.float() - 0.5) / 0.28209479177387814).unsqueeze(-2)                        # models/sh_utils.py:114-115
    shs = torch.cat([dc, torch.zeros((P, 12, 3), dtype=torch.float32, device=means.device)], dim=1).contiguous()
    return dict(means3D=means, opacities=torch.ones((P, 1), dtype=torch.float32, device=means.device),
                scales=scales.log() if log_scales else scales, rotations=rotations, shs=shs, normals=geo.normals)
