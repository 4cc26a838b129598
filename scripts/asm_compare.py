#!/usr/bin/env python3
"""Compare two builds of the HIP sources function by function, at the assembly level.

    python scripts/asm_compare.py DIR_A DIR_B        # dirs of <tu>.dev.s / <tu>.host.s files
    python scripts/asm_compare.py DIR_A DIR_B --rename-b REGEX REPL [--rename-b ...]

Made with `hipcc <the Makefile's flags> --cuda-device-only -S` (and --cuda-host-only) per source
file.  Each function's body (device: kernel code + its .amdhsa_kernel descriptor; host: the x86
text) is normalised for label numbering and compared; prints the functions that differ, exist in
one build only, and a summary.  Under a function that differs: the opcodes whose counts differ and
the .amdhsa_* descriptor and code object metadata lines that differ (registers, spills, scratch,
LDS), A -> B.  A kernel with MFMA loops is reported in parts: with labels renamed by order of
appearance and register numbers masked, every outermost backward branch whose span holds v_mfma
instructions is a loop (the one with the most is the main loop); for each, the opcode counts that
differ inside it (s_waitcnt per operand) and whether its masked instruction sequence is the same,
then the counts that differ outside the loops.  --rename-b applies re.sub(REGEX, REPL) to B's
assembly text first: a kernel whose template or argument list lost a parameter has another mangled
name, and is compared under the old one (else it shows as "only in A" and "only in B").  Used to show that a
source clean-up leaves every kept kernel's and host function's code unchanged, and what moved in a
kernel whose source was refactored.  A translation unit split in two is compared by concatenating
the two .s files of that build under the old name.
"""
import collections
import os
import re
import sys

META = (".agpr_count", ".vgpr_count", ".sgpr_count", ".vgpr_spill_count", ".sgpr_spill_count",
        ".private_segment_fixed_size", ".group_segment_fixed_size")
FUNC = re.compile(r"^([A-Za-z_.$][\w.$]*):\s*(?:;.*|#.*|//.*)?$")


def split(path, renames=()):
    out, cur, name = {}, [], None
    text = open(path).read()
    for pat, repl in renames:
        text = re.sub(pat, repl, text)
    lines = text.splitlines()
    for ln in lines:
        m = re.match(r"^\s*\.type\s+([\w.$]+),\s*@function", ln)
        if m:
            name, cur = m.group(1), []
            continue
        if name is not None:
            if re.match(r"^\.Lfunc_end\d+:", ln):
                out[name] = cur
                name = None
                continue
            cur.append(ln)
    # device kernel descriptors
    desc, dname = {}, None
    for ln in lines:
        m = re.match(r"^\s*\.amdhsa_kernel\s+(\S+)", ln)
        if m:
            dname, desc[m.group(1)] = m.group(1), []
            continue
        if dname is not None:
            if ".end_amdhsa_kernel" in ln:
                dname = None
                continue
            desc[dname].append(ln)
    # code object metadata: one record per kernel, "- .agpr_count:" first, keys in alphabetical
    # order, so .name sits in the middle: the counts after it go to the kernel's list through `rec`
    rec = []
    for ln in lines:
        m = re.match(r"^\s*(-\s+)?(\.\w+):\s*(\S+)\s*$", ln)
        if not m:
            continue
        if m.group(1) and m.group(2) == ".agpr_count":
            rec = []
        if m.group(2) in META:
            rec.append(f"    .meta{m.group(2)} {m.group(3)}")
        elif m.group(2) == ".name" and m.group(3) in desc:
            desc[m.group(3)] += rec
            rec = desc[m.group(3)]
    for k, v in desc.items():
        out.setdefault(k, []).extend(["#desc"] + v)
    return out


def norm(body):
    res = []
    for ln in body:
        if not ln.strip().startswith("#desc"):
            ln = re.sub(r"\s+#.*$", "", ln.split(";")[0].split("//")[0]).rstrip()  # device ; / host # comments
            if ln.lstrip().startswith("#"):
                continue
        if not ln.strip() or ln.strip().startswith(("; %bb", ".loc", ".file", ".cfi")):
            continue
        ln = re.sub(r"\.LBB\d+_(\d+)", r".LBB_\1", ln)
        ln = re.sub(r"\.Ltmp\d+", ".Ltmp", ln)
        ln = re.sub(r"\.Lfunc_end\d+", ".Lfunc_end", ln)
        ln = re.sub(r"\.LJTI\d+_(\d+)", r".LJTI_\1", ln)
        ln = re.sub(r"\.LCPI\d+_(\d+)", r".LCPI_\1", ln)
        ln = re.sub(r"\.L\.str(\.\d+)?", ".L.str", ln)
        ln = re.sub(r"__hip_cuid_\w+", "__hip_cuid", ln)
        ln = re.sub(r"__hip_gpubin_handle_\w+", "__hip_gpubin_handle", ln)
        res.append(ln)
    return res


LABEL = re.compile(r"\.LBB_\d+")
REG = re.compile(r"\b([vsa])(?:\d+\b|\[\d+:\d+\])")


def masked(code):
    """The code lines with labels renamed by order of appearance and register numbers masked
    (v12 -> v, s[4:5] -> s[], a3 -> a)."""
    names = {}
    out = []
    for ln in code:
        ln = LABEL.sub(lambda m: names.setdefault(m.group(0), f".L{len(names)}"), ln)
        out.append(REG.sub(lambda m: m.group(1) + ("[]" if "[" in m.group(0) else ""), ln).strip())
    return out


def mfma_loops(code):
    """[(first, last)] line indices of the outermost loops that hold v_mfma instructions, in order of
    appearance: every backward branch whose span, from its target label to the branch, holds one;
    spans inside another are dropped, overlapping ones joined.  (A kernel that branches to one of
    several time loops -- the wavefront forward's layer 0 and layers 1-2 -- has one entry per loop.)"""
    at = {ln[:-1]: i for i, ln in enumerate(code) if ln.endswith(":")}
    mf = [0]
    for ln in code:
        mf.append(mf[-1] + ln.startswith("v_mfma"))
    spans = []
    for i, ln in enumerate(code):
        w = ln.split()
        if len(w) == 2 and w[0].startswith(("s_cbranch", "s_branch")) and at.get(w[1], i) < i:
            if mf[i + 1] - mf[at[w[1]]] > 0:
                spans.append((at[w[1]], i))
    out = []
    for lo, hi in sorted(spans):
        if out and lo <= out[-1][1]:
            out[-1] = (out[-1][0], max(out[-1][1], hi))
        else:
            out.append((lo, hi))
    return out


def opcodes(code):
    """Opcode counts of code lines; s_waitcnt keyed by its operand text."""
    return collections.Counter(ln if ln.startswith("s_waitcnt") else ln.split()[0] for ln in code
                               if not ln.endswith(":") and not ln.startswith("."))


def count_diff(oa, ob, indent="    "):
    for op in sorted(set(oa) | set(ob)):
        if oa[op] != ob[op]:
            print(f"{indent}{op:<28} {oa[op]:>5} -> {ob[op]:<5}")


def report(na, nb):
    """What differs between two normalised bodies of one function: the opcodes whose counts differ
    (count in A -> count in B) and the .amdhsa_* descriptor lines that differ.  Where both bodies
    have the same number of MFMA loops (mfma_loops), the counts are given inside each loop -- the one
    with the most v_mfma is called the main loop -- and outside them, and whether each loop's masked
    instruction sequence is the same."""
    def parts(body):
        cut = body.index("#desc") if "#desc" in body else len(body)
        desc = dict(ln.split(None, 1) for ln in body[cut + 1:] if ln.lstrip().startswith((".amdhsa_", ".meta.")))
        return [ln.strip() for ln in body[:cut]], desc
    (ra, da), (rb, db) = parts(na), parts(nb)
    ca, cb = masked(ra), masked(rb)
    la, lb = mfma_loops(ca), mfma_loops(cb)
    if la and len(la) == len(lb):
        main = max(range(len(la)), key=lambda k: sum(ln.startswith("v_mfma") for ln in ca[la[k][0]:la[k][1] + 1]))
        for k, ((a0, a1), (b0, b1)) in enumerate(zip(la, lb)):
            # (the loop's labels renamed from its own first line on: the code before it may differ)
            ina, inb = masked(ra[a0:a1 + 1]), masked(rb[b0:b1 + 1])
            name = "main loop" if k == main else f"MFMA loop {k + 1} of {len(la)}"
            print(f"    {name}: {sum(ln.startswith('v_mfma') for ln in ina)} -> "
                  f"{sum(ln.startswith('v_mfma') for ln in inb)} v_mfma, {len(ina)} -> {len(inb)} lines; "
                  f"masked sequence {'identical' if ina == inb else 'differs'}")
            count_diff(opcodes(ina), opcodes(inb), "      ")

        def rest(code, loops):
            keep, pos = [], 0
            for lo, hi in loops:
                keep += code[pos:lo]
                pos = hi + 1
            return keep + code[pos:]
        oa, ob = rest(ca, la), rest(cb, lb)
        print("    outside the MFMA loops:" + (" masked sequence identical" if oa == ob else ""))
        count_diff(opcodes(oa), opcodes(ob), "      ")
    else:
        oa, ob = (collections.Counter(ln.split()[0] for ln in r if not ln.endswith(":") and not ln.startswith("."))
                  for r in (ra, rb))
        count_diff(oa, ob)
        if oa == ob:
            print("    (the same opcode counts: registers, order or operands differ)")
    for k in sorted(set(da) | set(db)):
        if da.get(k) != db.get(k):
            print(f"    {k:<52} {da.get(k, '-')} -> {db.get(k, '-')}")


def main(a, b, renames=()):
    same = diff = only_a = only_b = 0
    for fn in sorted(os.listdir(a)):
        if not fn.endswith(".s"):
            continue
        fa = split(os.path.join(a, fn))
        fb = split(os.path.join(b, fn), renames) if os.path.exists(os.path.join(b, fn)) else {}
        for k in sorted(set(fa) | set(fb)):
            if k not in fb:
                only_a += 1
                print(f"only in A  {fn}: {k}")
            elif k not in fa:
                only_b += 1
                print(f"only in B  {fn}: {k}")
            elif norm(fa[k]) != norm(fb[k]):
                diff += 1
                print(f"DIFFERENT  {fn}: {k}")
                report(norm(fa[k]), norm(fb[k]))
            else:
                same += 1
    print(f"identical {same}, different {diff}, only in A {only_a}, only in B {only_b}")
    return 1 if diff else 0


if __name__ == "__main__":
    args = sys.argv[1:]
    ren = []
    while "--rename-b" in args:
        i = args.index("--rename-b")
        ren.append((args[i + 1], args[i + 2]))
        del args[i:i + 3]
    sys.exit(main(args[0], args[1], ren))
