#!/usr/bin/env python3
"""Same instructions, kernel for kernel: asm_same.py PARENT_OBJDIR TREE_OBJDIR
                                     or: asm_same.py --units UNIT[,UNIT...] [--reorder-ok UNIT[,UNIT...]] PARENT_OBJDIR TREE_OBJDIR

Compares the device assembly (*gfx950.s, as seervideoldm_amd.build keeps it under lib/obj) of the GEMM tile kernel and the
split-K reduce kernels between a build whose gemm.hip holds them all and a build that spreads them over gemm_tiles_*.hip and
gemm_reduce.hip.  Per kernel symbol (.amdhsa_kernel): the instruction text between the symbol's label and its .Lfunc_end, with
comments stripped and the function number of the .LBB<n>_<m> labels normalised, and the .amdhsa_* lines of the kernel descriptor.
Fails on any difference, on a symbol missing on either side, and on a symbol that two files of the tree hold.  Every other
*gfx950.s must be the same file on both sides, but for the compilation-unit id (__hip_cuid_<hash>) that hipcc derives from the
source's path, which differs between two checkouts.  The script diffs text; it looks for no particular instruction.

--units: the same comparison for named sources that keep their names on both sides (attention, attention40, attention_bwd, gemm_tn,
...).  Per kernel symbol it reports (i) the symbol on both sides, (ii) equal descriptor lines, and (iii) identical instruction text or
(iv) different text with the same multiset of mnemonics (the first word of every instruction line): what a scheduler that moved
instructions and renumbered registers leaves behind.  (i) and (ii) are required of every kernel, (iii) of every kernel of a unit
that --reorder-ok does not name, (iii) or (iv) of the others.  Every source outside --units must be the same file, as above.
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


def compare_units(parent: Path, tree: Path, units: list, reorder_ok: set) -> int:
    from collections import Counter
    bad, named = [], set()
    for u in units:
        name = f"{u}-hip-amdgcn-amd-amdhsa-gfx950.s"
        named.add(name)
        if not (parent / name).exists() or not (tree / name).exists():
            bad.append(f"{u}: no {name} on one side")
            continue
        pk, tk = kernels(parent / name), kernels(tree / name)
        for k in sorted(set(pk) ^ set(tk)):
            bad.append(f"{u}: (i) missing in the {'tree' if k in pk else 'parent'}: {k}")
        count = Counter()
        for k in sorted(set(pk) & set(tk)):
            (pb, pd), (tb, td) = pk[k], tk[k]
            words = lambda body: Counter(l.split()[0] for l in body if not l.endswith(":"))
            how = "(iii) identical" if pb == tb else "(iv) same mnemonics" if words(pb) == words(tb) else "instructions differ"
            moved = sum(1 for a, b in zip(pb, tb) if a != b) + abs(len(pb) - len(tb))
            print(f"{u}: {'(ii) descriptor equal' if pd == td else 'DESCRIPTOR DIFFERS'}, {how}"
                  + (f" ({moved} of {len(pb)} lines differ)" if pb != tb else f" ({len(pb)} lines)") + f": {k}")
            count[how] += 1
            if pd != td:
                bad.append(f"{u}: (ii) kernel descriptor differs: {k}")
            if how.startswith("instr") or (how.startswith("(iv)") and u not in reorder_ok):
                bad.append(f"{u}: {how}: {k}")
        print(f"{u}: {len(pk)} kernel symbols in the parent, {len(tk)} in the tree; " + ", ".join(f"{c} {h}" for h, c in sorted(count.items())))
    others = [f for f in sorted(parent.glob("*gfx950.s")) if f.name not in named]
    for f in others:
        g = tree / f.name
        if not g.exists():
            bad.append(f"missing in the tree: {f.name}")
        elif CUID.sub(b"__hip_cuid", g.read_bytes()) != CUID.sub(b"__hip_cuid", f.read_bytes()):
            bad.append(f"file differs: {f.name}")
    for f in sorted(tree.glob("*gfx950.s")):
        if not (parent / f.name).exists():
            bad.append(f"missing in the parent: {f.name}")
    print(f"other sources' assembly, as files: {len(others) - sum(1 for b in bad if b.endswith('.s'))} of {len(others)} equal")
    for b in bad:
        print("DIFF " + b)
    print("OK" if not bad else f"FAILED: {len(bad)} difference(s)")
    return 1 if bad else 0


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
    args, opts = sys.argv[1:], {"--units": [], "--reorder-ok": []}
    while args and args[0] in opts and len(args) > 1:
        opts[args[0]] = args[1].split(",")
        args = args[2:]
    if len(args) != 2 or (opts["--reorder-ok"] and not opts["--units"]):
        sys.exit(__doc__)
    if opts["--units"]:
        sys.exit(compare_units(Path(args[0]), Path(args[1]), opts["--units"], set(opts["--reorder-ok"])))
    sys.exit(main(Path(args[0]), Path(args[1])))
