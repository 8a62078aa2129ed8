"""The Adam step of include/gsr.h (gsr_adam_step) restated on the CPU, the seeded cases the CPU and GPU tests share, and the bars a
single step is held to.  Importable without the built library or a device.

  kernel_constants / VEC / WAVE / BLOCK     ADAM_VEC, ADAM_THREADS, ADAM_MAX_BLOCKS (MAX_BLOCKS) as csrc/adam_step.hpp defines them; the
                                            elements of one block round
  group_blocks / work_split / rounds_taken  the entry's split of a call's rounds over a capped grid and a workgroup's grid-stride walk,
                                            restated (density_control.hpp has the same rule: density_ref calls these with its constants)
  host_constants                            step_g and rsq2 as the entry forms them: in double, rounded once to float32
  adam64 / adam32                           the definition in float64 (unrounded constants: what torch.optim.Adam computes in float64)
                                            and op by op in numpy float32 (the arithmetic the kernel is specified to perform)
  CASES / MASKS / TS / case_inputs / mask   the case table (sizes named with the kernel's constants), the mask kinds, the step counts
  CAP_CASES / CAP_CLAIMS / BENCH_SHAPE      the cases above the grid cap (8 M elements each: a table of their own, walked by one test
                                            each), what each is there to reach, and the benchmark cloud's shape
  EPS / check_step / check_step_in_ranges   the single-step bars, derived by counting roundings (see check_step); the same over row ranges
  Quadratic / trajectory_error              the seeded quadratic of the trajectory test and its error metric"""
import os
import re
from collections import namedtuple

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EPS = 2.0 ** -24          # the unit round-off of float32
TINY = 2.0 ** -150        # ... and the absolute error of one rounding into its subnormal range
BETA1, BETA2, ADAM_EPS = 0.9, 0.999, 1e-15
F = np.float32


def kernel_constants():
    text = open(os.path.join(ROOT, "gaussian-pcloud-render_amd", "csrc", "adam_step.hpp")).read()
    get = lambda name: int(re.search(r"constexpr int %s = (\d+);" % name, text).group(1))  # noqa: E731
    return get("ADAM_VEC"), get("ADAM_THREADS"), get("ADAM_MAX_BLOCKS")


VEC, THREADS, MAX_BLOCKS = kernel_constants()
WAVE = 64
BLOCK = VEC * THREADS     # elements of a group one workgroup covers per grid-stride round


# ---- the work split ---------------------------------------------------------------------------------------------------------------
def div_up(a, b):
    return -(-a // b)


def group_blocks(n, units, block=None, cap=None):
    """adam_group_blocks (and density_group_blocks, with that header's constants): the workgroups of a group of n elements when the
    call's groups hold `units` rounds of `block` elements -- a round each up to `cap` rounds, above it the floor of the proportional
    share of `cap`, at least one"""
    block, cap = BLOCK if block is None else block, MAX_BLOCKS if cap is None else cap
    mine = div_up(n, block)
    if units <= cap:
        return mine
    share = mine * cap // units
    return 1 if share < 1 else share


def work_split(P, widths, block=None, cap=None):
    """(units, workgroups per group) as the entry fills block_end: units the rounds of all groups of the call, P rows each"""
    block = BLOCK if block is None else block
    units = sum(div_up(P * w, block) for w in widths)
    return units, [group_blocks(P * w, units, block, cap) for w in widths]


def rounds_taken(n, nblocks, vec, block=None):
    """How often each round of `block` elements of a group of n elements is taken when `nblocks` workgroups walk it as k_adam_step
    does -- the scalar loop (base = block index x BLOCK; base < n; base += nblocks x BLOCK) or, with vec, the 16-B loop over
    n / VEC slots and one more for the tail (i = block index x THREADS + lane; i < slots; i += nblocks x THREADS), followed for a
    workgroup's lane 0.  int [rounds]"""
    block = BLOCK if block is None else block
    lanes = block // VEC
    taken = np.zeros(div_up(n, block), np.int64)
    slots = n // VEC + (1 if n % VEC else 0)
    for b in range(nblocks):
        if not vec:
            base = b * block
            while base < n:
                taken[base // block] += 1
                base += nblocks * block
        else:
            first = b * lanes                  # lane 0; a round is taken when its first slot exists
            while first < slots:
                taken[first // lanes] += 1
                first += nblocks * lanes
    return taken


def host_constants(lr, t, b1=BETA1, b2=BETA2):
    """(step_g, rsq2) as float32: lr / (1 - b1^t) and 1 / sqrt(1 - b2^t) of the float32 values lr, b1, b2, in double, rounded once"""
    lr, b1, b2 = float(F(lr)), float(F(b1)), float(F(b2))
    return F(lr / (1.0 - b1 ** t)), F(1.0 / np.sqrt(1.0 - b2 ** t))


def _rows(visible, width, shape):
    """the elementwise update mask of a [P, width] group from the [P] row mask (None: everything)"""
    if visible is None:
        return np.ones(shape, bool)
    return np.broadcast_to((np.asarray(visible) != 0)[:, None], shape)


def adam64(p, g, m, v, lr, t, visible=None, b1=BETA1, b2=BETA2, eps=ADAM_EPS):
    """One step in float64 on [P, width] arrays: (p', m', v').  lr, b1, b2, eps enter as the float32 values the C ABI takes, everything
    after that is double, the two bias corrections included.  Rows with visible == 0 are returned as they came."""
    p, g, m, v = (np.asarray(a, np.float64) for a in (p, g, m, v))
    lr, b1, b2, eps = float(F(lr)), float(F(b1)), float(F(b2)), float(F(eps))
    m2 = b1 * m + (1.0 - b1) * g
    v2 = b2 * v + (1.0 - b2) * (g * g)
    p2 = p - (lr / (1.0 - b1 ** t)) * (m2 / (np.sqrt(v2) * (1.0 / np.sqrt(1.0 - b2 ** t)) + eps))
    on = _rows(visible, p.shape[1], p.shape)
    return np.where(on, p2, p), np.where(on, m2, m), np.where(on, v2, v)


def adam32(p, g, m, v, lr, t, visible=None, b1=BETA1, b2=BETA2, eps=ADAM_EPS):
    """One step op by op in numpy float32, one rounding per written operation, with the host's float32 constants"""
    p, g, m, v = (np.asarray(a, F) for a in (p, g, m, v))
    step, rsq2 = host_constants(lr, t, b1, b2)
    b1, b2, eps = F(b1), F(b2), F(eps)
    c1, c2 = F(1.0) - b1, F(1.0) - b2
    m2 = b1 * m + c1 * g
    v2 = b2 * v + c2 * (g * g)
    p2 = p - step * (m2 / (np.sqrt(v2) * rsq2 + eps))
    assert p2.dtype == F and m2.dtype == F and v2.dtype == F
    on = _rows(visible, p.shape[1], p.shape)
    return np.where(on, p2, p), np.where(on, m2, m), np.where(on, v2, v)


# ---- the case table ---------------------------------------------------------------------------------------------------------------
# name, P, widths and learning rates of the groups, rows by which every pointer of the call is offset into its allocation
Case = namedtuple("Case", "name P widths lrs offset_rows")
WIDTHS = (1, 3, 4, 45, 48)
LRS = (1.6e-4, 2.5e-3, 5e-2, 5e-3, 1e-3, 1.25e-4, 2e-2, 1e-2)


def rows_of_a_block(width):
    return BLOCK // width


def _single(width):
    Ps = [1, 5, WAVE - 1, WAVE, WAVE + 1, 257] + [r for r in (rows_of_a_block(width) - 1, rows_of_a_block(width) + 1) if r >= 1]
    return [Case("w%d,P=%d" % (width, P), P, (width,), (LRS[WIDTHS.index(width)],), 0) for P in sorted(set(Ps))]


CASES = tuple(c for w in WIDTHS for c in _single(w)) + (
    Case("w3,P=342", 342, (3,), (2.5e-3,), 0),                                      # P width % 4 = 2, just past one block round
    Case("8groups,P=257", 257, (3, 48, 1, 3, 4, 45, 2, 7), LRS, 0),                 # mixed widths: vector and scalar groups in one call
    Case("8groups,P=%d" % (BLOCK + 1), BLOCK + 1, (3, 48, 1, 3, 4, 45, 2, 7), LRS, 0),   # several workgroups in every group
    Case("offset1,P=65", 65, (3, 45, 4, 48), LRS[:4], 1),                           # widths 3 and 45 lose their 16-byte alignment
    Case("offset1,P=%d" % (rows_of_a_block(3) + 1), rows_of_a_block(3) + 1, (3, 45, 1), LRS[:3], 1),
)


def cap_cases(cap, block):
    """The cases above a grid cap of `cap` workgroups of `block` elements per round, each just past cap x block elements:
      cap,w48      one 16-B group of cap + 1 rounds on cap workgroups: workgroup 0 takes a second round, a partial one
      cap,offset1  two scalar groups (pointers one row off), second rounds in both, block_end a prefix of floor-divided shares
      cap,floor    a width-1 group whose share floors to 0 and gets one workgroup, beside a group of odd width cap + 1
      cap,cloud    the five groups of a training cloud in one call, P x 3 and P x 1 no multiples of 4"""
    P48 = cap * block // 48 + 1
    return (Case("cap,w48", P48, (48,), (1e-3,), 0),
            Case("cap,offset1", P48, (3, 45), LRS[:2], 1),
            Case("cap,floor", block, (1, cap + 1), (5e-2, 5e-3), 0),
            Case("cap,cloud", 150001 * (cap * block) // (8192 * 1024) | 1, (3, 48, 1, 3, 4), LRS[:5], 0))   # 150001 today


CAP_CASES = cap_cases(MAX_BLOCKS, BLOCK)
# per case: the groups with a workgroup that takes a second round, and the groups whose share floors to 0
CAP_CLAIMS = {"cap,w48": ((0,), ()), "cap,offset1": ((0, 1), ()), "cap,floor": ((1,), (0,)), "cap,cloud": ((0, 1, 2, 3, 4), ())}
CAP_CLOUD_HALVES = ((0, CAP_CASES[3].P // 2 + 1), (CAP_CASES[3].P // 2 + 1, CAP_CASES[3].P))   # each below the cap; the cut is odd
VISIBLE_CAP_P = MAX_BLOCKS * THREADS + 1      # the smallest P at which k_visible_from_radii's capped grid walks a second round
BENCH_SHAPE = Case("bench", 800000, (3, 48, 1, 3, 4), LRS[:5], 0)                               # the benchmark cloud
MASKS = ("zeros", "ones", "alternating", "one_row", "random30")
TS = (1, 2, 1000, 10 ** 6)


def case(name):
    return next(c for c in CASES + CAP_CASES if c.name == name)


def on_vector_path(c, width):
    """whether a group of the case starts 16-B aligned (allocations are; offset_rows rows of `width` floats come before it)"""
    return (c.offset_rows * width) % VEC == 0


def mask(kind, P, seed=0):
    """uint8 [P]"""
    if kind == "zeros":
        return np.zeros(P, np.uint8)
    if kind == "ones":
        return np.ones(P, np.uint8)
    if kind == "alternating":
        return (np.arange(P) % 2).astype(np.uint8)
    if kind == "one_row":
        out = np.zeros(P, np.uint8)
        out[(2 * P) // 3] = 1
        return out
    assert kind == "random30"
    return (np.random.default_rng(77 + seed).random(P) < 0.3).astype(np.uint8)


def _log_uniform(rng, lo, hi, shape):
    return np.exp(rng.uniform(np.log(lo), np.log(hi), shape))


def case_inputs(c, seed=0):
    """per group (p, g, m, v), float32 [P, width]: |g| and |m| log-uniform in [1e-6, 1e2] with random signs, v log-uniform in
    [1e-12, 1e4], p normal -- no intermediate of the step is subnormal"""
    if c in CAP_CASES and _CAP_INPUTS.get("key") == (c, seed):
        return _CAP_INPUTS["inputs"]
    rng = np.random.default_rng(sum(map(ord, c.name)) * 31 + seed)
    out = []
    for w in c.widths:
        shape = (c.P, w)
        sign = lambda: rng.choice([-1.0, 1.0], shape)  # noqa: E731
        out.append(tuple(a.astype(F) for a in (rng.standard_normal(shape), sign() * _log_uniform(rng, 1e-6, 1e2, shape),
                                               sign() * _log_uniform(rng, 1e-6, 1e2, shape), _log_uniform(rng, 1e-12, 1e4, shape))))
    if c in CAP_CASES:       # 140 MB and 0.7 s: the last one is kept for the next call with it (nothing writes to a case's inputs)
        _CAP_INPUTS.update(key=(c, seed), inputs=out)
    return out


_CAP_INPUTS = {}


# ---- the single-step bars ---------------------------------------------------------------------------------------------------------
def check_step(got, inputs, lr, t, visible=None, b1=BETA1, b2=BETA2, eps=ADAM_EPS, what=""):
    """Hold one group's (p', m', v') = got (float32 [P, width]) to the definition; inputs = (p, g, m, v) float32.  With EPS = 2^-24:
        |m' - m64| <= 4 EPS (|b1 m| + |c1 g|)      c1's rounding, two products, one sum
        |v' - v64| <= 5 EPS v64                    c2's rounding, g g, two products, one sum
        |p' - (p - u64)| <= EPS |p - u64| + 8 EPS |u64|     u64: the float64 update formed from the RETURNED float32 m', v' and the
                                                   float32 constants -- square root, product, sum, quotient, product: 5 roundings, and
                                                   the final subtraction's own
    Each rounding's relative bound holds for normal results only; where a result is subnormal (the gradients of a real render reach
    1e-30: c2 g g underflows) IEEE gradual underflow bounds its error by TINY = 2^-150 instead, so every bar carries that term once
    per rounding it counts.  On the case table, whose inputs keep every intermediate normal, the term is 45 orders below the bars.
    Rows with visible == 0: the bits of the inputs.  Returns the three largest ratios error / bar (for printing)."""
    p, g, m, v = (np.asarray(a, F) for a in inputs)
    p2, m2, v2 = (np.asarray(a) for a in got)
    assert p2.dtype == F and m2.dtype == F and v2.dtype == F and p2.shape == p.shape, what
    on = _rows(visible, p.shape[1], p.shape)
    for new, old, name in ((p2, p, "param"), (m2, m, "exp_avg"), (v2, v, "exp_avg_sq")):
        assert (new.view(np.uint32)[~on] == old.view(np.uint32)[~on]).all(), "%s: masked rows of %s changed" % (what, name)
    if not on.any():
        return 0.0, 0.0, 0.0
    _, m64, v64 = adam64(p, g, m, v, lr, t, None, b1, b2, eps)
    b1d, b2d = float(F(b1)), float(F(b2))
    d = lambda a: np.asarray(a, np.float64)  # noqa: E731
    m_bar = 4 * EPS * (np.abs(b1d * d(m)) + np.abs((1 - b1d) * d(g))) + 4 * TINY
    v_bar = 5 * EPS * v64 + 5 * TINY
    step, rsq2 = host_constants(lr, t, b1, b2)
    u64 = float(step) * (d(m2) / (np.sqrt(d(v2)) * float(rsq2) + float(F(eps))))
    want = d(p) - u64
    p_bar = EPS * np.abs(want) + 8 * EPS * np.abs(u64) + 8 * TINY
    ratios = []
    for err, bar, name in ((np.abs(d(m2) - m64), m_bar, "exp_avg"), (np.abs(d(v2) - v64), v_bar, "exp_avg_sq"),
                           (np.abs(d(p2) - want), p_bar, "param")):
        assert np.isfinite(err[on]).all(), "%s: %s is not finite" % (what, name)
        bad = on & (err > bar)
        worst = float((err[on] / bar[on]).max()) if (bar[on] > 0).all() else float("inf") if (err[on] > bar[on]).any() else 0.0
        ratios.append(worst)
        assert not bad.any(), "%s: %s misses its bar at %d elements, worst error / bar = %.3g" % (what, name, int(bad.sum()), worst)
    return tuple(ratios)


def check_step_in_ranges(got, inputs, lr, t, visible=None, what="", elems=1 << 20):
    """check_step over every element, about `elems` of them at a time (it is elementwise: the float64 temporaries of 8 M elements at
    once are 1 GB).  Returns the largest ratios over the ranges."""
    P, width = inputs[0].shape
    step = max(1, elems // width)
    worst = np.zeros(3)
    for a in range(0, P, step):
        b = min(P, a + step)
        worst = np.maximum(worst, check_step(tuple(x[a:b] for x in got), tuple(x[a:b] for x in inputs), lr, t,
                                             None if visible is None else visible[a:b], what="%s rows [%d, %d)" % (what, a, b)))
    return worst


# ---- a case through the library ---------------------------------------------------------------------------------------------------
_GUARD = 0x7FC0BEEF     # a NaN pattern around every array: guard rows in front (the case's offset, at least one) and behind


def device_rows(a, offset_rows, dev):
    """a float32 [P, width] host array as rows [offset_rows, offset_rows + P) of a device allocation of offset_rows + P + 1 rows (with
    offset_rows = 0 the array starts where the allocation does, which is what keeps it 16-byte aligned); every other row holds the
    guard pattern.  Returns (view of the P rows, the whole allocation)."""
    import torch
    P, width = a.shape
    whole = torch.full((offset_rows + P + 1, width), _GUARD, dtype=torch.int32, device=dev).view(torch.float32)
    rows = whole[offset_rows:offset_rows + P]
    rows.copy_(torch.from_numpy(np.ascontiguousarray(a)))
    return rows, whole


def guards_intact(whole, offset_rows, P):
    import torch
    bits = whole.view(torch.int32)
    return bool((bits[:offset_rows] == _GUARD).all()) and bool((bits[offset_rows + P:] == _GUARD).all())


def run_library(N, c, dev, kind=None, t=1, zero_grads=False, seed=0, only=None, rows=None):
    """One gsr_adam_step of case c on the device.  kind: a mask kind or None (dense); only: the indices of the groups to submit (default
    all); rows = (a, b): submit rows [a, b) alone, with offset pointers and P = b - a.  Returns (out, inputs, visible): out[k] =
    (p', m', v', grad after the call) of group k as float32 numpy [P, width] -- the whole arrays, also where only rows of them were
    submitted --, inputs the host arrays they started from, visible the uint8 mask or None.  Asserts that no guard row was written."""
    import torch
    inputs = case_inputs(c, seed)
    vis = None if kind is None else mask(kind, c.P)
    a, b = (0, c.P) if rows is None else rows
    held, groups = [], []
    for k, (inp, lr) in enumerate(zip(inputs, c.lrs)):
        pairs = [device_rows(x, c.offset_rows, dev) for x in inp]      # p, g, m, v
        held.append(pairs)
        if only is None or k in only:
            p, g, m, v = (r[a:b] for r, _ in pairs)
            groups.append((p, g, m, v, lr))
    vis_dev = None if vis is None else torch.from_numpy(vis[a:b].copy()).to(dev)
    N.adam_step(groups, t, BETA1, BETA2, ADAM_EPS, visible=vis_dev, zero_grads=zero_grads)
    out = []
    for pairs in held:
        for _, whole in pairs:
            assert guards_intact(whole, c.offset_rows, c.P), "%s: a row outside the arrays was written" % c.name
        (p, _), (g, _), (m, _), (v, _) = pairs
        out.append(tuple(x.cpu().numpy() for x in (p, m, v, g)))
    return out, inputs, vis


def same_bits(a, b):
    return a.shape == b.shape and bool((np.ascontiguousarray(a).view(np.uint32) == np.ascontiguousarray(b).view(np.uint32)).all())


# ---- the trajectory ---------------------------------------------------------------------------------------------------------------
TRAJ_P, TRAJ_WIDTHS, TRAJ_LRS, TRAJ_STEPS, TRAJ_SEEDS = 257, (3, 48, 1, 3, 4), (1e-2, 2e-2, 5e-2, 5e-3, 1e-2), 100, tuple(range(8))


class Quadratic:
    """The seeded loss sum_k k (p - c)^2 / 2 of every group: its gradient k (p - c) is one subtraction and one product in the
    precision of p, so a float32 path and the float32 restatement see the same roundings."""

    def __init__(self, seed):
        rng = np.random.default_rng(4242 + seed)
        self.p0 = [rng.standard_normal((TRAJ_P, w)).astype(F) for w in TRAJ_WIDTHS]
        self.k = [rng.uniform(0.5, 2.0, (TRAJ_P, w)).astype(F) for w in TRAJ_WIDTHS]
        self.c = [rng.standard_normal((TRAJ_P, w)).astype(F) for w in TRAJ_WIDTHS]
        self.masks = (np.random.default_rng(999 + seed).random((TRAJ_STEPS, TRAJ_P)) < 0.3).astype(np.uint8)

    def grad(self, i, p):
        return self.k[i].astype(p.dtype) * (p - self.c[i].astype(p.dtype))

    def run(self, step_fn, dtype, masked):
        """TRAJ_STEPS steps of step_fn (adam64 or adam32) from p0 with zero moments: the final parameters per group"""
        out = []
        for i in range(len(TRAJ_WIDTHS)):
            p = self.p0[i].astype(dtype)
            m, v = np.zeros_like(p), np.zeros_like(p)
            for t in range(1, TRAJ_STEPS + 1):
                p, m, v = step_fn(p, self.grad(i, p), m, v, TRAJ_LRS[i], t, self.masks[t - 1] if masked else None)
            out.append(p)
        return out


def trajectory_error(p, p64, p0):
    """e = max|p - p64| / max|p64 - p0|"""
    p, p64, p0 = (np.asarray(a, np.float64) for a in (p, p64, p0))
    return float(np.abs(p - p64).max() / np.abs(p64 - p0).max())
