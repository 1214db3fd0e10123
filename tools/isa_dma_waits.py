"""LDS-DMA loops of hipcc's --save-temps assembly and the vmcnt waits inside them.

For every kernel of a .s file, every loop (a backward branch) whose body holds a
`buffer_load ... lds` / `global_load_lds` is listed with its `s_waitcnt vmcnt(N)` instructions,
hand-placed ones (between ;;#ASMSTART and ;;#ASMEND) told from compiler-inserted ones.  A
compiler-inserted vmcnt(0) in such a loop drains the DMA ring in the middle of the loop body (the
compiler cannot tell the ring stage being read from the one being filled, and waits for all of
them before the first transposed LDS read it issues itself): the kernel still computes the right
thing but fill and MFMA no longer overlap.  Exit status 1 if any such wait is found.

Usage: python tools/isa_dma_waits.py <file.s> [<file.s> ...] [--only SUBSTRING] [--quiet]
(--quiet: only the kernels with such a wait.  The .s files: make EXTRA=-save-temps=obj OBJDIR=<dir>.)
"""
import re
import subprocess
import sys
from collections import Counter

DMA = re.compile(r"^(buffer_load_\w+\s.*\blds\b|global_load_lds_\w+)")
VMCNT = re.compile(r"\bvmcnt\((\d+)\)")
BRANCH = re.compile(r"^s_c?branch\w*\s+(\.LBB\w+)")
VMEM = re.compile(r"^(buffer_|global_|flat_|scratch_)")
MEMOP = re.compile(r"^(ds_|buffer_|global_|flat_|scratch_)")


def demangle(names):
    for tool in ("/opt/rocm/llvm/bin/llvm-cxxfilt", "llvm-cxxfilt", "c++filt"):
        try:
            out = subprocess.run([tool], input="\n".join(names), capture_output=True, text=True, check=True).stdout
            return dict(zip(names, out.split("\n")))
        except (OSError, subprocess.CalledProcessError):
            continue
    return {n: n for n in names}


def kernels(text):
    """[(mangled name, body lines)] of the device functions, and {name: (vgprs, spills)}"""
    lines = text.split("\n")
    out, i = [], 0
    while i < len(lines):
        m = re.match(r"^(_Z\w+):", lines[i])
        if m:
            j = i + 1
            while j < len(lines) and not re.match(r"^\.Lfunc_end", lines[j]):
                j += 1
            out.append((m.group(1), lines[i + 1:j]))
            i = j
        i += 1
    regs, name = {}, None
    for l in lines:  # amdhsa.kernels metadata: .name precedes the counts of its kernel
        m = re.match(r"^\s+\.name:\s+(\S+)", l)
        if m:
            name = m.group(1)
            regs.setdefault(name, [None, None])
        m = re.match(r"^\s+\.vgpr_count:\s+(\d+)", l)
        if m and name:
            regs[name][0] = int(m.group(1))
        m = re.match(r"^\s+\.vgpr_spill_count:\s+(\d+)", l)
        if m and name:
            regs[name][1] = int(m.group(1))
    return out, regs


def instructions(body):
    """[(line index, text, in_asm)] for the instructions (a label: text None); {label: index into that list}"""
    ins, labels, in_asm = [], {}, False
    for n, raw in enumerate(body):
        l = raw.strip()
        if l.startswith(";;#ASMSTART"):
            in_asm = True
        elif l.startswith(";;#ASMEND"):
            in_asm = False
        m = re.match(r"^(\.LBB\w+):", l)
        if m:
            labels[m.group(1)] = len(ins)
            ins.append((n, None, False))
            continue
        if not l or l[0] in ".;" or l.endswith(":"):
            continue
        ins.append((n, l.split(";")[0].strip(), in_asm))
    return ins, labels


def dma_loops(body):
    """per loop with LDS-DMA (widest extent per header label): dict(label, lines, dma, tr, waits);
    waits = [(line, count, hand-placed, what memory instruction follows)].  A compiler vmcnt(0)
    with no vector-memory instruction (and no label) since the previous vmcnt(0) waits for nothing
    (hipcc adds one to the fence of a __syncthreads() right behind a hand-placed one): not listed."""
    ins, labels = instructions(body)
    loops = {}
    for k, (n, l, _) in enumerate(ins):
        m = BRANCH.match(l) if l else None
        if not m or m.group(1) not in labels or labels[m.group(1)] > k:
            continue
        if m.group(1) in loops and loops[m.group(1)][1] > k:
            continue
        loops[m.group(1)] = (labels[m.group(1)], k)
    out = []
    for label, (a, k) in loops.items():
        seg = ins[a:k + 1]
        ndma = sum(1 for s in seg if s[1] and DMA.match(s[1]))
        if not ndma:
            continue
        waits, drained = [], False
        for q, (n, t, hand) in enumerate(seg):
            if t is None or VMEM.match(t):
                drained = False
                continue
            w = VMCNT.search(t) if t.startswith("s_waitcnt") else None
            if not w:
                continue
            c = int(w.group(1))
            if not (c == 0 and drained and not hand):
                nxt = next((u[1].split()[0] for u in seg[q + 1:] if u[1] and MEMOP.match(u[1])), "-")
                waits.append((n, c, hand, nxt))
            drained = drained or c == 0
        out.append(dict(label=label, lines=(seg[0][0], seg[-1][0]), dma=ndma, waits=waits,
                        tr=sum(1 for s in seg if s[1] and s[1].startswith("ds_read_b64_tr"))))
    return out


def scan(path, only=None):
    """[dict(kernel, vgprs, spills, sites, tr_sites, loops)] for the kernels with LDS-DMA loops;
    sites = compiler-inserted vmcnt(0) waits inside such loops (tr_sites: those directly in front
    of a transposed read)"""
    ks, regs = kernels(open(path).read())
    names = demangle([k[0] for k in ks])
    out = []
    for mangled, body in ks:
        if only and only not in mangled and only not in names[mangled]:
            continue
        loops = dma_loops(body)
        if not loops:
            continue
        vg, sp = regs.get(mangled, (None, None))
        sites = {n for lp in loops for n, c, hand, _ in lp["waits"] if c == 0 and not hand}
        trsites = {n for lp in loops for n, c, hand, nxt in lp["waits"]
                   if c == 0 and not hand and nxt.startswith("ds_read_b64_tr")}
        short = re.sub(r"\(.*", "", names[mangled]).replace("void ", "")
        out.append(dict(kernel=short, vgprs=vg, spills=sp, sites=len(sites), tr_sites=len(trsites), loops=loops))
    return out


def report(path, only=None, quiet=False):
    bad = 0
    for k in scan(path, only):
        bad += k["sites"]
        if quiet and not k["sites"]:
            continue
        print(f"{k['kernel']}: vgprs {k['vgprs']} spills {k['spills']}; compiler vmcnt(0) in LDS-DMA loops "
              f"{k['sites']} ({k['tr_sites']} before a transposed read)")
        for lp in k["loops"]:
            cnt = Counter((c, hand, nxt) for _, c, hand, nxt in lp["waits"])
            w = ", ".join(f"{n}x vmcnt({c}) {'hand' if hand else 'COMPILER'} before {nxt}"
                          for (c, hand, nxt), n in sorted(cnt.items(), key=lambda x: (x[0][1], x[0][0])))
            print(f"  loop {lp['label']} lines {lp['lines'][0]}-{lp['lines'][1]}: {lp['dma']} lds-dma, "
                  f"{lp['tr']} tr-reads; {w or 'no vmcnt wait'}")
    return bad


def main(argv):
    only, quiet, files = None, False, []
    it = iter(argv)
    for a in it:
        if a == "--only":
            only = next(it)
        elif a == "--quiet":
            quiet = True
        else:
            files.append(a)
    if not files:
        print(__doc__)
        return 2
    bad = 0
    for f in files:
        print(f"== {f.split('/')[-1]}")
        bad += report(f, only, quiet)
    print(f"compiler-inserted vmcnt(0) in LDS-DMA loops: {bad}")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
