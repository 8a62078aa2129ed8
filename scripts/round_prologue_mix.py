"""Static size of the render kernels' ROUND PROLOGUE: what a wave executes once per round of 64 list entries outside the
pair / group loops -- gather addresses, footprint test, staging, rotation of the prefetched records.
usage: python scripts/round_prologue_mix.py [build dir = gaussian-pcloud-render_amd/build]   (needs `build.py --save-temps`)

For every render kernel in the two assembly files the round loop is the smallest loop that holds both a record gather
(global_load_dwordx4) and the alpha evaluation (v_exp_f32); the instructions of the loops nested in it are left out.  Printed per
kernel: vector instructions of the prologue (all / v_mov), scalar and LDS instructions, and the kernel's registers, scratch and
occupancy from its .amdhsa / comment lines."""
import os, re, sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BUILD = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "gaussian-pcloud-render_amd", "build")


def kernels(lines):
    """(symbol, body lines, trailer lines) of every kernel of the file"""
    starts = [i for i, l in enumerate(lines) if re.match(r"^_Z\w*k_render_\w+:", l)]
    for st in starts:
        end = next(i for i in range(st, len(lines)) if "s_endpgm" in lines[i])
        sym = lines[st].split(":")[0]
        trailer = lines[end:end + 400]
        yield sym, [l.strip() for l in lines[st:end + 1]], trailer


def loops_of(body):
    lab = {}
    for i, l in enumerate(body):
        m = re.match(r"^(\.LBB\d+_\d+):", l)
        if m:
            lab[m.group(1)] = i
    out = {}
    for i, l in enumerate(body):
        m = re.match(r"^s_c?branch\S*\s+(\.LBB\d+_\d+)", l)
        if m and lab.get(m.group(1), 1 << 30) < i:
            out[m.group(1)] = (lab[m.group(1)], max(i, out.get(m.group(1), (0, 0))[1]))
    return sorted(out.values())


def ops(seg):
    for l in seg:
        t = l.split(";")[0].strip()
        if t and not t.startswith((".", "//")) and not t.endswith(":"):
            yield t.split(None, 1)[0]


def figure(trailer, key):
    for l in trailer:
        m = re.search(r";\s*%s:\s*(\d+)" % key, l)
        if m:
            return int(m.group(1))
    return -1


def demangle(sym):
    m = re.search(r"k_render_forward_half", sym)
    if m:
        return "k_render_forward_half"
    m = re.search(r"k_render_(forward|backward)ILi(\d+)E?(?:Li(\d+)E)?(.*)", sym)
    if not m:
        return sym
    if m.group(1) == "forward":
        return "k_render_forward<%s>" % m.group(2)
    tail = ", det" if "RenderBwdDet" in sym else ""
    return "k_render_backward<%s, %s%s>" % (m.group(2), m.group(3) if m.group(3) else "0", tail)


print("%-36s %6s %6s %6s %6s | %5s %5s %7s %4s" % ("kernel", "valu", "v_mov", "salu", "lds", "vgpr", "agpr", "scratch", "occ"))
for fn in ("render_fwd-hip-amdgcn-amd-amdhsa-gfx950.s", "render_bwd-hip-amdgcn-amd-amdhsa-gfx950.s"):
    lines = open(os.path.join(BUILD, fn)).read().splitlines()
    for sym, body, trailer in kernels(lines):
        lp = loops_of(body)
        has = lambda a, b, pat: any(o.startswith(pat) for o in ops(body[a:b + 1]))  # noqa: E731
        rounds = [(a, b) for a, b in lp if has(a, b, "global_load_dwordx4") and has(a, b, "v_exp_f32")]
        if not rounds:
            continue
        a, b = min(rounds, key=lambda ab: ab[1] - ab[0])
        inner = [(x, y) for x, y in lp if x >= a and y <= b and (x, y) != (a, b)]
        keep = [i for i in range(a, b + 1) if not any(x <= i <= y for x, y in inner)]
        o = list(ops(body[i] for i in keep))
        valu = sum(1 for x in o if x.startswith("v_"))
        mov = sum(1 for x in o if x.startswith("v_mov"))
        salu = sum(1 for x in o if x.startswith("s_") and not x.startswith(("s_cbranch", "s_branch", "s_waitcnt", "s_nop")))
        lds = sum(1 for x in o if x.startswith("ds_"))
        print("%-36s %6d %6d %6d %6d | %5d %5d %7d %4d" % (demangle(sym), valu, mov, salu, lds, figure(trailer, "NumVgprs"),
                                                          figure(trailer, "NumAgprs"), figure(trailer, "ScratchSize"), figure(trailer, "Occupancy")))
