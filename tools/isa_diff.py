"""Dev tool: did a refactor change the kernels?  Compares two directories written by `make asm` (csrc/build/asm of two
checkouts) kernel by kernel: the ordered mnemonic sequence with the operands dropped (register renumbering does not show)
and the VGPR / SGPR / scratch / LDS / occupancy figures of the *.usage.txt remarks.  Kernels are matched by symbol, so one
may move to another file.  Exit status 1 when a kernel that matches none of the --allow substrings (of the demangled
name) differs or exists on one side only.
usage: python tools/isa_diff.py parent/build/asm branch/build/asm [--allow lanczos_fused_kernel ...] [--all]"""
import argparse, glob, os, re, subprocess, sys

FIGS = [("VGPR", "VGPRs"), ("SGPR", "SGPRs"), ("scratch", r"ScratchSize \[bytes/lane\]"), ("LDS", r"LDS Size \[bytes/block\]"),
        ("occ", r"Occupancy \[waves/SIMD\]")]


def kernels(d):
    """symbol -> (tuple of mnemonics, tuple of figures)"""
    figs, out = {}, {}
    for f in glob.glob(os.path.join(d, "*.usage.txt")):
        for b in re.split(r"remark: [^\n]*Function Name: ", open(f).read())[1:]:
            figs[b.split()[0]] = tuple(int(re.search(k + r": (\d+)", b).group(1)) for _, k in FIGS)
    for f in glob.glob(os.path.join(d, "*-hip-amdgcn-amd-amdhsa-gfx950.s")):
        txt = open(f).read()
        for name in re.findall(r"^\s*\.amdhsa_kernel (\S+)", txt, re.M):
            body = re.search(r"^%s:[^\n]*\n(.*?)\.Lfunc_end" % re.escape(name), txt, re.S | re.M).group(1)
            ins = tuple(l.split()[0] for l in body.split("\n") if l.startswith("\t") and not l.strip().startswith((".", ";")))
            out[name] = (ins, figs.get(name))
    return out


ap = argparse.ArgumentParser()
ap.add_argument("parent"), ap.add_argument("branch")
ap.add_argument("--allow", nargs="*", default=[], help="substrings of demangled kernel names that may differ")
ap.add_argument("--all", action="store_true", help="print identical kernels too")
a = ap.parse_args()
A, B = kernels(a.parent), kernels(a.branch)
names = sorted(set(A) | set(B))
dem = dict(zip(names, subprocess.run(["c++filt"] + names, capture_output=True, text=True).stdout.split("\n")))
bad = same = 0
print("| kernel | instructions | " + " | ".join(n for n, _ in FIGS) + " | verdict |\n|---|---|" + "---|" * len(FIGS) + "---|")
for n in names:
    (ia, fa), (ib, fb) = A.get(n, (None, None)), B.get(n, (None, None))
    verdict = ("only in parent" if ib is None else "only in branch" if ia is None else
               "same" if ia == ib and fa == fb else "same mnemonics, other figures" if ia == ib else "differs")
    same += verdict == "same"
    if verdict == "same" and not a.all:
        continue
    allowed = any(s in dem[n] for s in a.allow)
    bad += not allowed and verdict != "same"
    cell = lambda x, y: "%s" % x if x == y else "%s -> %s" % (x, y)
    fa, fb = fa or ("-",) * len(FIGS), fb or ("-",) * len(FIGS)
    print("| `%s` | %s | %s | %s%s |" % (re.sub(r"^(void )?attwarp::", "", dem[n])[:90], cell(ia and len(ia), ib and len(ib)),
          " | ".join(cell(x, y) for x, y in zip(fa, fb)), verdict, " (allowed)" if allowed and verdict != "same" else ""))
print("\n%d kernels, %d identical, %d outside the allow-list differ" % (len(names), same, bad))
sys.exit(1 if bad else 0)
