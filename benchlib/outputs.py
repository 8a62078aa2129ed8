"""`--dump-outputs DIR` of bench.py: what the timed path handed its caller in its last step, written as DIR/<name>.npy in float32 so
that two builds of the project can be compared output for output on the same seeded inputs.

  image            the frame of the last timed step, [3, H, W]; a frame of more than MAX_PIXELS pixels is a fixed seeded sample
                   of its pixels, [3, MAX_PIXELS]
  radii            that view's radii, one row per Gaussian
  grad_<leaf>      the gradients the caller's leaf tensors hold after the last timed submission (summed over the views of that
                   submission, as autograd hands them over), one row per Gaussian

Per-Gaussian arrays are a fixed seeded sample of the same rows (at most MAX_ROWS, fewer if the 64 MB would not hold them)."""
import os

import numpy as np

MAX_BYTES = 64 << 20
MAX_PIXELS = 1 << 21          # a 1920x1080 frame (2 073 600 pixels) is written whole
MAX_ROWS = 1 << 17


def sample(n, k, seed):
    """Sorted indices of a fixed, seeded sample of k of n items; all n when k >= n."""
    if k >= n:
        return np.arange(n)
    return np.sort(np.random.default_rng(seed).choice(n, k, replace=False))


def select(frame, radii, grads):
    """frame [3,H,W], radii [P], grads {leaf name: [P, ...]} (torch tensors or arrays) -> {file name: float32 array} within
    MAX_BYTES."""
    f32 = lambda a: np.asarray(a.detach().float().cpu() if hasattr(a, "detach") else a, dtype=np.float32)  # noqa: E731
    img = f32(frame)
    C, H, W = img.shape
    px = sample(H * W, MAX_PIXELS, 0)
    out = {"image": img if px.size == H * W else img.reshape(C, H * W)[:, px]}
    per_row = {"radii": f32(radii)}
    per_row.update(("grad_" + k, f32(v)) for k, v in sorted(grads.items()))
    P = per_row["radii"].shape[0]
    row_bytes = 4 * sum(int(np.prod(a.shape[1:])) for a in per_row.values())
    rows = sample(P, min(MAX_ROWS, (MAX_BYTES - out["image"].nbytes) // row_bytes), 1)
    out.update((k, a if rows.size == P else a[rows]) for k, a in per_row.items())
    assert sum(a.nbytes for a in out.values()) <= MAX_BYTES
    return {k: np.ascontiguousarray(a) for k, a in out.items()}


def write(out_dir, frame, radii, grads):
    """Writes select(...) to out_dir/<name>.npy; returns {name: shape}."""
    os.makedirs(out_dir, exist_ok=True)
    arrays = select(frame, radii, grads)
    for k, a in arrays.items():
        np.save(os.path.join(out_dir, k + ".npy"), a)
    return {k: list(a.shape) for k, a in arrays.items()}
