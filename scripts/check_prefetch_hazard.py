"""The render kernels issue their prefetch loads from inline asm and retire them by hand (render_walk.hpp), so the compiler does
not know that a destination register is still in flight between the load and the `s_waitcnt vmcnt(0)` of the retire asm.  If
register pressure makes it SPILL or COPY such a register in between, it saves a value that has not arrived.  This script reads
the assembly of a `build.py --save-temps` build and reports every instruction that names a destination register of an
asm-issued global_load before the next s_waitcnt vmcnt(0).
usage: python scripts/check_prefetch_hazard.py [build dir]      exit status 1 if anything is found"""
import os, re, sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BUILD = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "gaussian-pcloud-render_amd", "build")


def regs(tok):
    m = re.fullmatch(r"v\[(\d+):(\d+)\]", tok)
    if m:
        return set(range(int(m.group(1)), int(m.group(2)) + 1))
    m = re.fullmatch(r"v(\d+)", tok)
    return {int(m.group(1))} if m else set()


bad = 0
for fn in ("render_fwd-hip-amdgcn-amd-amdhsa-gfx950.s", "render_bwd-hip-amdgcn-amd-amdhsa-gfx950.s"):
    kernel, in_asm, flying = "?", False, set()
    for n, raw in enumerate(open(os.path.join(BUILD, fn)), 1):
        l = raw.split(";")[0].strip() if not raw.strip().startswith(";;#") else raw.strip()
        if re.match(r"^_Z\w+:", l):
            kernel, flying = l[:-1], set()
        if l.startswith(";;#ASMSTART"):
            in_asm = True
            continue
        if l.startswith(";;#ASMEND"):
            in_asm = False
            continue
        if not l or l.startswith(".") or l.endswith(":"):
            continue
        toks = re.findall(r"v\[\d+:\d+\]|v\d+", l)
        arriving = set()
        if in_asm and l.startswith("global_load"):
            arriving = regs(toks[0])   # (a load may take its address from its own destination)
            used = set().union(*[regs(t) for t in toks[1:]]) if len(toks) > 1 else set()
        elif re.match(r"s_waitcnt .*vmcnt\(0\)", l):   # the retire asm, or a wait of the compiler's own
            flying = set()
            continue
        else:
            used = set().union(*[regs(t) for t in toks]) if toks else set()
        if l.startswith("s_endpgm"):
            flying = set()
        hit = used & flying
        flying |= arriving
        if hit:
            bad += 1
            print("%s:%d %s: `%s` touches v%s while its load is in flight" % (fn, n, kernel[:60], l, sorted(hit)))
print("prefetch hazards: %d" % bad)
sys.exit(1 if bad else 0)
