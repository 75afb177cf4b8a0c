#!/usr/bin/env python3
"""Same instructions, kernel for kernel: asm_same.py PARENT_OBJDIR TREE_OBJDIR

Compares the device assembly (*gfx950.s, as seervideoldm_amd.build keeps it under lib/obj) of the GEMM tile kernel and the
split-K reduce kernels between a build whose gemm.hip holds them all and a build that spreads them over gemm_tiles_*.hip and
gemm_reduce.hip.  Per kernel symbol (.amdhsa_kernel): the instruction text between the symbol's label and its .Lfunc_end, with
comments stripped and the function number of the .LBB<n>_<m> labels normalised, and the .amdhsa_* lines of the kernel descriptor.
Fails on any difference, on a symbol missing on either side, and on a symbol that two files of the tree hold.  Every other
*gfx950.s must be the same file on both sides, but for the compilation-unit id (__hip_cuid_<hash>) that hipcc derives from the
source's path, which differs between two checkouts.  The script diffs text; it looks for no particular instruction.
"""
import re
import sys
from pathlib import Path

GEMM = re.compile(r"^(gemm|gemm_tiles_\w+|gemm_reduce)-hip-")
LABEL = re.compile(r"\.L(BB|tmp|func_end|func_begin)(\d+)")
CUID = re.compile(rb"__hip_cuid_[0-9a-f]+")


def kernels(path: Path) -> dict:
    """symbol -> (body lines, descriptor lines) of every kernel of one assembly file"""
    lines = path.read_text().splitlines()
    names = {l.split()[1] for l in lines if l.strip().startswith(".amdhsa_kernel")}
    out, cur, body, desc, in_desc = {}, None, [], {}, None
    for l in lines:
        t = l.split(";")[0].rstrip()
        s = t.strip()
        if in_desc is not None:
            if s == ".end_amdhsa_kernel":
                desc[in_desc] = dl
                in_desc = None
            elif s:
                dl.append(s)
            continue
        if s.startswith(".amdhsa_kernel"):
            in_desc, dl = s.split()[1], []
            continue
        if cur is None:
            if s.endswith(":") and s[:-1] in names:
                cur, body = s[:-1], []
            continue
        if s.startswith(".Lfunc_end"):
            out[cur] = body
            cur = None
            continue
        if s:
            body.append(LABEL.sub(lambda m: ".L" + m.group(1) + "#", s))
    assert cur is None and set(out) == set(desc) == names, f"{path}: labels, bodies and descriptors do not pair up"
    return {k: (out[k], desc[k]) for k in names}


def main(parent: Path, tree: Path) -> int:
    bad = []
    pk, tk, where = {}, {}, {}
    for f in sorted(parent.glob("*gfx950.s")):
        if GEMM.match(f.name):
            pk.update(kernels(f))
    per_file = {}
    for f in sorted(tree.glob("*gfx950.s")):
        if not GEMM.match(f.name) or f.name.startswith("gemm_tiles_all-"):
            continue
        ks = kernels(f)
        per_file[f.name.split("-hip-")[0]] = len(ks)
        for k, v in ks.items():
            if k in tk:
                bad.append(f"in two files of the tree ({where[k]}, {f.name}): {k}")
            tk[k], where[k] = v, f.name
    for k in sorted(set(pk) - set(tk)):
        bad.append(f"missing in the tree: {k}")
    for k in sorted(set(tk) - set(pk)):
        bad.append(f"missing in the parent: {k}")
    same = 0
    for k in sorted(set(pk) & set(tk)):
        (pb, pd), (tb, td) = pk[k], tk[k]
        if pd != td:
            bad.append(f"kernel descriptor differs ({where[k]}): {k}")
        elif pb != tb:
            at = next((i for i, (a, b) in enumerate(zip(pb, tb)) if a != b), min(len(pb), len(tb)))
            bad.append(f"instructions differ from line {at} of {len(pb)} / {len(tb)} ({where[k]}): {k}")
        else:
            same += 1
    others = 0
    for f in sorted(parent.glob("*gfx950.s")):
        if GEMM.match(f.name):
            continue
        g = tree / f.name
        others += 1
        if not g.exists():
            bad.append(f"missing in the tree: {f.name}")
        elif CUID.sub(b"__hip_cuid", g.read_bytes()) != CUID.sub(b"__hip_cuid", f.read_bytes()):
            bad.append(f"file differs: {f.name}")
    tiles = sum(1 for k in tk if "seer_gemm_kernel" in k)
    print(f"parent: {len(pk)} kernel symbols; tree: {len(tk)} ({tiles} tile kernels, {len(tk) - tiles} reduce kernels)")
    print("tree, kernels per unit: " + ", ".join(f"{n} {c}" for n, c in sorted(per_file.items())))
    print(f"equal (instructions and descriptor): {same} of {len(pk)}")
    print(f"other sources' assembly, as files: {others - sum(1 for b in bad if b.endswith('.s'))} of {others} equal")
    for b in bad:
        print("DIFF " + b)
    print("OK" if not bad else f"FAILED: {len(bad)} difference(s)")
    return 1 if bad else 0


if __name__ == "__main__":
    if len(sys.argv) != 3:
        sys.exit(__doc__)
    sys.exit(main(Path(sys.argv[1]), Path(sys.argv[2])))
