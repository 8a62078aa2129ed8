"""For one fuzz case: the rows of dL_dmean3D where the library is furthest from the float64 chain, with the reference build's
distance, the distance of the same chain evaluated in float32 (numpy) and the spread under 1e-6 input noise.
usage: python scripts/diag_row_conditioning.py <case>"""
import os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "gaussian-pcloud-render_amd")]
import numpy as np, torch
import util, sweep_support as F
from oracle.oracle import Oracle, Reference
from fp64_backward import gaussian_backward_fp64
i = int(sys.argv[1])
s, mode = F.random_case(i)
dL = util.seeded_dL(s, seed=77 + i)
r, gr = Reference("strict").forward_backward(s, dL)
of, og = Oracle().forward_backward(s, dL)
p, gp = util.run_product(s, torch.device("cuda:0"), dL_dpix=dL)
ex = gaussian_backward_fp64(s, of["radii"], of["clamped"], og["dL_dmean2D"], og["dL_dconic"], og["dL_dcolor"])
for k in ("dL_dmean3D", "dL_dscale", "dL_drot"):
    if not gp[k].size:
        continue
    e = np.asarray(ex[k], np.float64).reshape(gp[k].shape[0], -1)
    a, b = gp[k].astype(np.float64).reshape(e.shape), gr[k].astype(np.float64).reshape(e.shape)
    rl, rb = np.linalg.norm(a - e, axis=1), np.linalg.norm(b - e, axis=1)
    rows = np.argsort(-rl)[:5]
    f32 = gaussian_backward_fp64(s, of["radii"], of["clamped"], og["dL_dmean2D"], og["dL_dconic"], og["dL_dcolor"], rows=rows, dtype=np.float32)[k]
    base = gaussian_backward_fp64(s, of["radii"], of["clamped"], og["dL_dmean2D"], og["dL_dconic"], og["dL_dcolor"], rows=rows)[k]
    rf = np.linalg.norm((f32.astype(np.float64) - base).reshape(rows.size, -1), axis=1)
    # library fed with ITS OWN render-level sums through the float64 chain: isolates the chain from the sums
    own = gaussian_backward_fp64(s, p["radii"], of["clamped"], gp["dL_dmean2D"], None, gp["dL_dcolor"], rows=rows) if False else None
    print(k, "max|g| %.3g" % np.abs(e).max())
    for j, row in enumerate(rows):
        print("  row %5d |exact| %.4g  lib-exact %.3g  ref-exact %.3g  f32chain-exact %.3g   conic %s opacity %.3g radius %d" % (
            row, np.linalg.norm(e[row]), rl[row], rb[row], rf[j], p["conic_opacity"][row][:3], p["conic_opacity"][row][3], p["radii"][row]))
