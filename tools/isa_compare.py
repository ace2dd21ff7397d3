#!/usr/bin/env python
"""Two builds of the library kernel by kernel, from their gfx950 code objects (no GPU needed):

    python tools/isa_compare.py PARENT/libpycllp_hip.so BRANCH/libpycllp_hip.so OUTDIR TAG

OUTDIR/isa_identity_TAG.txt: every kernel's disassembly (llvm-objdump -d --no-show-raw-insn, address comments and the padding
mark behind a code object's last kernel and the s_nop fill behind a kernel's last instruction removed, split at the <symbol>: lines) -- identical, changed, gone or new, and in how
many code objects it sits.  OUTDIR/kernel_resources_parent_branch_TAG.txt: for the wave kernels the figures of
tools/kernel_resources.py side by side and the instruction counts per opcode of f64 arithmetic, MFMA, LDS and memory
instructions compared (a changed f64 count means an operation was contracted or split differently)."""
import sys, re, os, subprocess, tempfile, collections
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import kernel_resources as kr
LLVM = kr.LLVM
def dem(names):
    out = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True).stdout.split("\n")
    return [re.sub(r"\(anonymous namespace\)::", "", o).split("(")[0].replace("void ", "") for o in out[:len(names)]]
def load(lib):
    ks = {}     # demangled name -> list of (text, rec)
    with tempfile.TemporaryDirectory() as tmp:
        for co in kr.code_objects(lib, tmp):
            recs = {r["name"]: r for r in kr.kernels_of(co)}
            dis = subprocess.run([os.path.join(LLVM, "llvm-objdump"), "-d", "--no-show-raw-insn", co], capture_output=True, text=True).stdout
            cur, body = None, {}
            for line in dis.split("\n"):
                mm = re.match(r"^[0-9a-f]+ <(\S+)>:", line)
                if mm: cur = mm.group(1); body[cur] = []; continue
                if cur is None or not line.strip(): continue
                t = re.sub(r"\s*//.*$", "", line).strip()
                if t != "...": body[cur].append(t)   # "...": objdump's mark for the zero padding behind a code object's last kernel
            for b in body.values():                  # ... and the s_nop fill behind a kernel's last instruction: alignment of the next
                while b and b[-1] == "s_nop 0": b.pop()   # function or, behind a code object's last kernel, its 256-byte tail
            syms = [s for s in body if s in recs]
            for s, d in zip(syms, dem(syms)):
                ks.setdefault(d, []).append((body[s], recs[s]))
    return ks
def cls(op):
    if op.startswith("v_mfma"): return "mfma"
    if op.endswith("_f64") or "_f64_" in op: return "f64"
    if op.startswith("ds_"): return "lds"
    if op.startswith(("buffer_", "global_", "flat_")): return "mem"
    if op.startswith("scratch_"): return "scratch"
    return None
def counts(text):
    c = collections.Counter()
    for l in text:
        op = re.sub(r"_e(32|64)$", "", l.split()[0])      # the encoding of an opcode (VOP2/VOPC against VOP3) is not counted as another opcode
        k = cls(op)
        if k: c[(k, op)] += 1
    return c
P, B = load(sys.argv[1]), load(sys.argv[2])
out, tag = sys.argv[3], sys.argv[4]
os.makedirs(out, exist_ok=True)
wave = lambda n: "wreg" in n
with open(os.path.join(out, "isa_identity_%s.txt" % tag), "w") as f:
    same = diff = 0
    for n in sorted(set(P) | set(B)):
        p, b = P.get(n, []), B.get(n, [])
        if not b: st = "gone"
        elif not p: st = "new"
        else:
            st = "identical" if p[0][0] == b[0][0] else "changed"
            if any(x[0] != p[0][0] for x in p) or any(x[0] != b[0][0] for x in b): st += " (copies differ among themselves)"
        same += st == "identical"; diff += st != "identical"
        f.write("%-100s %s   copies %d -> %d\n" % (n, st, len(p), len(b)))
    f.write("# identical %d, other %d\n" % (same, diff))
    print("identical", same, "other", diff)
with open(os.path.join(out, "kernel_resources_parent_branch_%s.txt" % tag), "w") as f:
    f.write("# %-58s | parent: VGPR AGPR SGPR vspill sspill scratchB ld/st | branch: same | f64/MFMA/LDS/mem opcode counts\n" % "kernel")
    bad = 0
    for n in sorted(set(P) & set(B)):
        if not wave(n): continue
        (pt, pr), (bt, br) = P[n][0], B[n][0]
        pc, bc = counts(pt), counts(bt)
        ps = sum(v for (k, o), v in pc.items() if k == "scratch"); bs = sum(v for (k, o), v in bc.items() if k == "scratch")
        d = {k: (pc.get(k, 0), bc.get(k, 0)) for k in set(pc) | set(bc) if k[0] != "scratch" and pc.get(k, 0) != bc.get(k, 0)}
        worse = br["vspill"] > pr["vspill"] or br["scratch"] > pr["scratch"] or bs > ps
        verdict = "opcode counts equal" if not d else "OPCODES DIFFER " + " ".join("%s %d->%d" % (k[1], a, b) for k, (a, b) in sorted(d.items()))
        if worse: verdict += "  MORE SPILL/SCRATCH"
        bad += bool(d) or worse
        fmt = lambda r, s: "%3d %3d %3d %3d %3d %4d %3d" % (r["vgpr"], r["agpr"], r["sgpr"], r["vspill"], r["sspill"], r["scratch"], s)
        f.write("%-60s | %s | %s | n_instr %d -> %d | %s\n" % (n[:60], fmt(pr, ps), fmt(br, bs), len(pt), len(bt), verdict))
    f.write("# wave kernels with differing f64/MFMA/LDS/memory opcode counts or more spill/scratch: %d\n" % bad)
    print("wave kernels flagged", bad)
