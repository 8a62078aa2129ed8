"""Adaptive density control (include/gsr.h gsr_density_plan / gsr_density_apply) restated in numpy, and the seeded cases the CPU and GPU
tests share.  Importable without the built library or a device.

  kernel_constants / THREADS / SCAN_ROUND / VEC / MAX_BLOCKS   as csrc/density_control.hpp defines them
  apply_split                                     the gather's rounds and workgroups per group (the split rule adam_ref restates)
  header_codes / PRUNED ... SPLIT / COPY ... MOMENT   the GSR_DENSITY_* codes as include/gsr.h defines them
  Rule / make_rule                                the fields of gsr_density_rule (thresholds held as the float32 values the ABI takes)
  actions / plan_of                               the decision op by op in float32; offsets, index and totals from the action codes
  philox / philox_scalar / uniforms / noise64     Philox4x32-10 through two code paths, the float32 uniforms, Box-Muller in float64
  rotation / child_means / child_scales           a child's geometry op by op in float32, or in float64 (dtype)
  child_mean_bar                                  the bar between the two, by counting roundings
  apply_ref                                       the output rows of a group table
  near_threshold                                  the rows a log_scales case may leave out of the exact comparison
  CASES / case / case_inputs / census             the case table, its seeded inputs, and what occurs in them"""
import os
import re
from collections import namedtuple

import numpy as np

import adam_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32
U = 2.0 ** -24            # the unit round-off of float32
LOG_SHRINK = F(float.fromhex("0x1.e148a2p-2"))   # the float32 nearest log(1.6)
TWO_PI = F(6.2831855)
M0, M1, W0, W1 = 0xD2511F53, 0xCD9E8D57, 0x9E3779B9, 0xBB67AE85
MASK32 = 0xFFFFFFFF


def kernel_constants():
    text = open(os.path.join(ROOT, "gaussian-pcloud-render_amd", "csrc", "density_control.hpp")).read()
    get = lambda name: int(re.search(r"constexpr int %s = (\d+);" % name, text).group(1))  # noqa: E731
    return get("DENSITY_THREADS"), get("DENSITY_SCAN_ROUND"), get("DENSITY_VEC"), get("DENSITY_MAX_BLOCKS")


def header_codes():
    text = open(os.path.join(ROOT, "include", "gsr.h")).read()
    return {m.group(1): int(m.group(2)) for m in re.finditer(r"#define GSR_DENSITY_([A-Z_]+) (\d+)", text)}


THREADS, SCAN_ROUND, VEC, MAX_BLOCKS = kernel_constants()
BLOCK = VEC * THREADS     # output elements of a group one gather workgroup covers per grid-stride round
_CODES = header_codes()
PRUNED, KEPT, CLONED, CLONED_COPY, SPLIT = (_CODES[k] for k in ("PRUNED", "KEPT", "CLONED", "CLONED_COPY", "SPLIT"))
COPY, MEANS, SCALES, MOMENT = (_CODES[k] for k in ("COPY", "MEANS", "SCALES", "MOMENT"))
ROWS = np.zeros(5, np.int64)
ROWS[[KEPT, CLONED_COPY]] = 1
ROWS[[CLONED, SPLIT]] = 2

Rule = namedtuple("Rule", "grad_threshold dense_size min_opacity max_screen_radius max_world_size log_scales normalize_rotations seed")


def make_rule(grad_threshold=2e-4, dense_size=0.05, min_opacity=0.005, max_screen_radius=20, max_world_size=0.5, log_scales=0,
              normalize_rotations=1, seed=0x0123456789ABCDEF):
    return Rule(F(grad_threshold), F(dense_size), F(min_opacity), int(max_screen_radius), F(max_world_size), int(log_scales),
                int(normalize_rotations), int(seed))


def _max3(s):
    """max(max(x, y), z) with a > b ? a : b, as the kernel writes it"""
    m = np.where(s[:, 0] > s[:, 1], s[:, 0], s[:, 1])
    return np.where(m > s[:, 2], m, s[:, 2])


def sigma(rule, scales, dtype=F):
    s = np.asarray(scales, dtype)
    return np.exp(s) if rule.log_scales else s


def actions(rule, scales, opacities, grad_sum, views, radius, prune_mask=None):
    """the action code of every Gaussian: the definition in its order, float32, one rounding per written operation"""
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        smax = _max3(sigma(rule, scales))
        g = np.asarray(grad_sum, F) / np.maximum(np.asarray(views, np.int32), 1).astype(F)
        assert smax.dtype == F and g.dtype == F
        hot = g >= rule.grad_threshold
        dead = np.asarray(opacities, F).reshape(-1) < rule.min_opacity
        if prune_mask is not None:
            dead = dead | (np.asarray(prune_mask) != 0)
        big = np.zeros(len(smax), bool)
        if rule.max_screen_radius > 0:
            big |= np.asarray(radius, np.int32) > rule.max_screen_radius
        if rule.max_world_size > 0:
            big |= smax > rule.max_world_size
        clone = hot & (smax <= rule.dense_size)
        split = hot & (smax > rule.dense_size)
        small = (smax / F(1.6) > rule.max_world_size) if rule.max_world_size > 0 else np.zeros(len(smax), bool)
    out = np.where(dead | big, PRUNED, KEPT)
    out = np.where(split, np.where(dead | small, PRUNED, SPLIT), out)
    out = np.where(clone, np.where(dead, PRUNED, np.where(big, CLONED_COPY, CLONED)), out)
    return out.astype(np.uint8)


def plan_of(action):
    """(offsets uint32 [P+1], index int32 [P'], totals int64 [5]) of the action codes"""
    action = np.asarray(action)
    rows = ROWS[action]
    offsets = np.concatenate([[0], np.cumsum(rows)])
    src = np.repeat(np.arange(len(action)), rows)
    k = np.arange(offsets[-1]) - offsets[src]
    carried = (action[src] == KEPT) | ((action[src] == CLONED) & (k == 0))
    index = np.where(carried, src, -1 - src).astype(np.int32)
    n_carried, n_copies = int(carried.sum()), int(np.isin(action, (CLONED, CLONED_COPY)).sum())
    totals = np.array([offsets[-1], n_carried, n_copies, 2 * int((action == SPLIT).sum()), int((action == PRUNED).sum())], np.int64)
    assert totals[0] == totals[1] + totals[2] + totals[3]
    return offsets.astype(np.uint32), index, totals


# ---- the generator ----------------------------------------------------------------------------------------------------------------
def philox(counter, key):
    """Philox4x32-10, vectorised: counter a tuple of four integer arrays (or scalars), key (k0, k1); returns uint32 [..., 4]"""
    c = [np.asarray(x, np.uint64) & np.uint64(MASK32) for x in np.broadcast_arrays(*counter)]
    k0, k1 = int(key[0]) & MASK32, int(key[1]) & MASK32
    for _ in range(10):
        p0, p1 = np.uint64(M0) * c[0], np.uint64(M1) * c[2]
        c = [(p1 >> np.uint64(32)) ^ c[1] ^ np.uint64(k0), p1 & np.uint64(MASK32), (p0 >> np.uint64(32)) ^ c[3] ^ np.uint64(k1),
             p0 & np.uint64(MASK32)]
        k0, k1 = (k0 + W0) & MASK32, (k1 + W1) & MASK32
    return np.stack(c, -1).astype(np.uint32)


def philox_scalar(counter, key):
    """the same on Python integers, one counter"""
    c0, c1, c2, c3 = (int(x) & MASK32 for x in counter)
    k0, k1 = int(key[0]) & MASK32, int(key[1]) & MASK32
    for _ in range(10):
        hi0, lo0 = divmod(M0 * c0, 1 << 32)
        hi1, lo1 = divmod(M1 * c2, 1 << 32)
        c0, c1, c2, c3 = hi1 ^ c1 ^ k0, lo1, hi0 ^ c3 ^ k1, lo0
        k0, k1 = (k0 + W0) % (1 << 32), (k1 + W1) % (1 << 32)
    return c0, c1, c2, c3


def seed_key(seed):
    return int(seed) & MASK32, (int(seed) >> 32) & MASK32


def uniforms(words):
    """u = ((float)(x >> 8) + 0.5f) * 2^-24 in float32 (the sum rounds to even from x >> 8 = 2^23 on: u lies in (0, 1])"""
    u = ((np.asarray(words, np.uint32) >> np.uint32(8)).astype(F) + F(0.5)) * F(U)
    assert u.dtype == F
    return u


def noise64(seed, P):
    """(eps, radius) float64 [P][2][3]: Box-Muller in float64 from the float32 uniforms of counter (i, k, 0, 0); radius is the
    Box-Muller radius of each component (r01, r01, r2)"""
    i, k = np.meshgrid(np.arange(P), np.arange(2), indexing="ij")
    u = uniforms(philox((i, k, 0, 0), seed_key(seed))).astype(np.float64)
    r01, r2 = np.sqrt(-2.0 * np.log(u[..., 0])), np.sqrt(-2.0 * np.log(u[..., 2]))
    a1, a3 = float(TWO_PI) * u[..., 1], float(TWO_PI) * u[..., 3]
    return np.stack([r01 * np.cos(a1), r01 * np.sin(a1), r2 * np.cos(a3)], -1), np.stack([r01, r01, r2], -1)


# ---- a child's geometry -------------------------------------------------------------------------------------------------------------
def rotation(rule, rotations, dtype=F):
    """R [P][3][3] of the stored quaternions (r, x, y, z), every operation in dtype"""
    q = np.asarray(rotations, dtype)
    r, x, y, z = (q[:, k] for k in range(4))
    if rule.normalize_rotations:
        n = np.sqrt(((r * r + x * x) + y * y) + z * z)
        r, x, y, z = r / n, x / n, y / n, z / n
    one, two = dtype(1), dtype(2)
    R = np.stack([np.stack([one - two * (y * y + z * z), two * (x * y - r * z), two * (x * z + r * y)], -1),
                  np.stack([two * (x * y + r * z), one - two * (x * x + z * z), two * (y * z - r * x)], -1),
                  np.stack([two * (x * z - r * y), two * (y * z + r * x), one - two * (x * x + y * y)], -1)], 1)
    assert R.dtype == dtype
    return R


def displacement(R, sig, eps):
    """d [P][2][3]: t = sigma * eps; d_r = (R[r][0] t0 + R[r][1] t1) + R[r][2] t2, in the arrays' dtype"""
    t = sig[:, None, :] * eps
    return (R[:, None, :, 0] * t[..., None, 0] + R[:, None, :, 1] * t[..., None, 1]) + R[:, None, :, 2] * t[..., None, 2]


def child_means(rule, means, scales, rotations, eps, dtype=F):
    """[P][2][3]: the means of both children of EVERY Gaussian, as if each were split"""
    d = displacement(rotation(rule, rotations, dtype), sigma(rule, scales, dtype), np.asarray(eps, dtype))
    out = np.asarray(means, dtype)[:, None, :] + d
    assert out.dtype == dtype
    return out


def child_mean_bar(rule, means64, scales, rotations, eps):
    """The bar on |child_means float32 - float64| by counting roundings (U = 2^-24 per operation).  A normalised quaternion component
    carries 4 U (sum of squares, sqrt, division), a product of two 9 U, an entry of R at most 21 U in absolute terms (the pairs of
    products sum to at most 1); a raw quaternion of norm N carries 4 U N^2.  The products sigma * eps, R * t and the two sums add 3 U
    per term, exp of a log scale (its float32 result against float64) 2 U more, and the final sum one rounding of the result."""
    q = np.asarray(rotations, np.float64)
    n2 = np.ones(len(q)) if rule.normalize_rotations else np.maximum((q * q).sum(1), 1.0)
    R = np.abs(rotation(rule, rotations, np.float64))
    t = np.abs(sigma(rule, scales, np.float64)[:, None, :] * np.asarray(eps, np.float64))      # [P][2][3]
    per_term = (21 * U * n2)[:, None, None, None] + (3 + (2 if rule.log_scales else 0)) * U * R[:, None, :, :]
    return (per_term * t[:, :, None, :]).sum(-1) + U * np.abs(means64)


def child_scales(rule, scales):
    s = np.asarray(scales, F)
    out = s - LOG_SHRINK if rule.log_scales else s / F(1.6)
    assert out.dtype == F
    return out


def apply_ref(rule, action, groups, scales=None, rotations=None, noise=None, dtype=F):
    """the output rows [P'][width] of every (src [P][width], role) of `groups`, and the index"""
    offsets, index, _ = plan_of(action)
    src = np.where(index >= 0, index, -1 - index)
    fresh, split = index < 0, np.asarray(action)[src] == SPLIT
    k = np.arange(len(index)) - offsets[src].astype(np.int64)
    out = []
    for data, role in groups:
        rows = np.array(np.asarray(data)[src])
        if role == MOMENT:
            rows[fresh] = 0
        elif role == SCALES:
            rows[split] = child_scales(rule, data)[src[split]]
        elif role == MEANS:
            rows = rows.astype(dtype)
            rows[split] = child_means(rule, data, scales, rotations, noise, dtype)[src[split], k[split]]
        out.append(rows)
    return out, index


def near_threshold(rule, scales, ulps=4):
    """rows whose float64 smax lies within `ulps` float32 ulp of a threshold it is compared with: the rows a log_scales case may leave
    out of the exact comparison (the kernel's expf and numpy's may differ there)"""
    smax = sigma(rule, scales, np.float64).max(1)
    near = np.zeros(len(smax), bool)
    for T in (float(rule.dense_size), float(rule.max_world_size), float(F(1.6)) * float(rule.max_world_size)):
        if T > 0:
            near |= np.abs(smax - T) <= ulps * float(np.spacing(F(T)))
    return near


# ---- the case table -----------------------------------------------------------------------------------------------------------------
# kind: how the decision inputs are drawn; log / norm: the rule's log_scales and normalize_rotations; mask: with a prune_mask
Case = namedtuple("Case", "name P kind log norm mask")
TWO_ROUNDS_P = THREADS * SCAN_ROUND + 1        # the smallest P whose workgroup counts need a second round of the scan's loop
assert -(-TWO_ROUNDS_P // THREADS) > SCAN_ROUND >= -(-(TWO_ROUNDS_P - 1) // THREADS)
THREE_ROUNDS_P = 2 * THREADS * SCAN_ROUND + 1  # ... and a third
SMALL_P = (1, 2, 255, 256, 257, 1023, 1024, 1025)
CASES = tuple(Case("mixed,P=%d" % P, P, "mixed", n % 2, (n // 2) % 2, (n // 4) % 2) for n, P in enumerate(SMALL_P)) + (
    Case("mixed,P=%d" % TWO_ROUNDS_P, TWO_ROUNDS_P, "mixed", 0, 1, 1),
    Case("mixed,P=70001", 70001, "mixed", 0, 0, 1),
    Case("mixed,log,P=70001", 70001, "mixed", 1, 1, 0),
    Case("all_pruned,P=1025", 1025, "all_pruned", 0, 1, 0),
    Case("all_split,P=1025", 1025, "all_split", 0, 1, 0),
    Case("all_kept,P=1025", 1025, "all_kept", 0, 1, 0),
    Case("thresholds", 0, "thresholds", 0, 1, 1),      # P follows from the table of on-threshold rows
    Case("mixed,P=%d" % THREE_ROUNDS_P, THREE_ROUNDS_P, "mixed", 0, 1, 1),     # (appended: a case's seed is its place in the table)
)
WIDTHS = (1, 3, 4, 45, 48)
# the groups of an apply call beside means3D, scales and rotations: name, width, role
EXTRA_GROUPS = (("opacities", 1, COPY), ("sh_rest", 45, COPY), ("shs", 48, COPY), ("m48", 48, MOMENT), ("m3", 3, MOMENT))


def case(name):
    """the case of that name"""
    return {c.name: c for c in CASES}[name]


def case_rule(c):
    return make_rule(log_scales=c.log, normalize_rotations=c.norm, max_screen_radius=0 if c.kind == "all_split" else 20)


def _threshold_rows(rule):
    """every combination of {one ulp below, on, one ulp above} the four thresholds, and the world-size threshold's three sides"""
    side = lambda t: [np.nextafter(F(t), F(-np.inf)), F(t), np.nextafter(F(t), F(np.inf))]  # noqa: E731
    rows = [(g, s, o, r) for g in side(rule.grad_threshold) for s in side(rule.dense_size) for o in side(rule.min_opacity)
            for r in (rule.max_screen_radius - 1, rule.max_screen_radius, rule.max_screen_radius + 1)]
    rows += [(g, s, F(0.5), 3) for g in (F(0), F(1)) for s in side(rule.max_world_size) + side(F(1.6) * rule.max_world_size)]
    return rows


def case_inputs(c):
    """the seeded inputs of a case: a dict of numpy arrays (scales in the stored domain), the rule under "rule" """
    rule = case_rule(c)
    rng = np.random.default_rng(1000 + CASES.index(c))
    table = _threshold_rows(rule) if c.kind == "thresholds" else None
    P = len(table) if table else c.P
    sig = np.exp(rng.uniform(np.log(0.004), np.log(0.3), (P, 3))).astype(F)
    grad = (2e-4 * np.exp(rng.normal(0.0, 1.5, P))).astype(F)
    views = rng.integers(0, 13, P).astype(np.int32)
    radius = rng.integers(0, 31, P).astype(np.int32)
    opac = np.where(rng.random(P) < 0.1, rng.uniform(0.0, 0.005, P), rng.uniform(0.005, 1.0, P)).astype(F)
    if c.kind == "mixed":
        big = rng.random(P) < 0.05                              # some beyond the world size, with and without children that fit
        sig[big, 0] = rng.uniform(0.45, 1.2, int(big.sum())).astype(F)
        grad = grad * np.maximum(views, 1).astype(F)            # the sum over the views that saw it
        grad[views == 0] = 0
        if P >= 255:
            grad[rng.integers(0, P, 4)] = np.nan
            grad[rng.integers(0, P, 4)] = np.inf
    elif c.kind == "all_pruned":
        opac[:] = 0
    elif c.kind == "all_split":
        sig[:, 1] = rng.uniform(0.06, 0.4, P).astype(F)
        grad[:], views[:], opac[:] = 1.0, 1, 0.9
    elif c.kind == "all_kept":
        grad[:], radius[:], opac[:] = 0, 5, 0.9
    elif c.kind == "thresholds":
        t = np.array(table, np.float64)
        grad, views = t[:, 0].astype(F), np.ones(P, np.int32)
        sig = np.stack([t[:, 1].astype(F), t[:, 1].astype(F) * F(0.5), t[:, 1].astype(F) * F(0.25)], 1)
        opac, radius = t[:, 2].astype(F), t[:, 3].astype(np.int32)
    scales = np.log(sig).astype(F) if c.log else sig
    rot = rng.normal(0.0, 1.0, (P, 4)).astype(F) * rng.uniform(0.5, 2.0, (P, 1)).astype(F)      # deliberately unnormalised
    mask = (rng.random(P) < 0.07).astype(np.uint8) if c.mask and c.kind != "thresholds" else None
    out = dict(rule=rule, P=P, scales=scales, opacities=opac, grad_norm_sum=grad, visible_views=views, max_radius=radius, prune_mask=mask,
               rotations=rot, means3D=rng.normal(0.0, 2.0, (P, 3)).astype(F), noise=rng.normal(0.0, 1.0, (P, 2, 3)).astype(F))
    for name, width, _ in EXTRA_GROUPS[1:]:
        out[name] = rng.normal(0.0, 1.0, (P, width)).astype(F)
    return out


def case_actions(inp):
    return actions(inp["rule"], inp["scales"], inp["opacities"], inp["grad_norm_sum"], inp["visible_views"], inp["max_radius"],
                   inp["prune_mask"])


def case_groups(inp):
    """the eight (name, src, role) groups of a case's apply call: widths 3, 3, 4, 1, 45, 48 and two moment groups"""
    return [("means3D", inp["means3D"], MEANS), ("scales", inp["scales"], SCALES), ("rotations", inp["rotations"], COPY)] + [
        (name, inp["opacities"].reshape(-1, 1) if name == "opacities" else inp[name], role) for name, _, role in EXTRA_GROUPS]


def apply_split(P_out, widths):
    """(units, workgroups per group, rounds per group) of a gsr_density_apply call of P_out output rows: density_group_blocks and the
    entry's loop are adam_step.hpp's rule with this header's constants"""
    units, blocks = adam_ref.work_split(P_out, widths, BLOCK, MAX_BLOCKS)
    return units, blocks, [adam_ref.div_up(P_out * w, BLOCK) for w in widths]


def census(inputs):
    """over the inputs of several cases: how often every action code occurs, and every side (-1 below, 0 on, 1 above) of the four
    thresholds of the issue's list"""
    codes, sides = np.zeros(5, np.int64), {k: set() for k in ("grad", "dense", "opacity", "radius")}
    for inp in inputs:
        rule = inp["rule"]
        codes += np.bincount(case_actions(inp), minlength=5)
        with np.errstate(invalid="ignore", divide="ignore"):
            g = inp["grad_norm_sum"] / np.maximum(inp["visible_views"], 1).astype(F)
        for name, value, t in (("grad", g, rule.grad_threshold), ("dense", _max3(sigma(rule, inp["scales"])), rule.dense_size),
                               ("opacity", inp["opacities"], rule.min_opacity), ("radius", inp["max_radius"], rule.max_screen_radius)):
            sides[name] |= set(np.sign(value[np.isfinite(value)].astype(np.float64) - float(t)).astype(int).tolist())
    return codes, sides
