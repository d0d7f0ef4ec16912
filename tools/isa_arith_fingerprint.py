"""A CPU pre-check for contraction drift: do two compilations of one kernel do the same floating-point arithmetic in the same order?

    python tools/isa_arith_fingerprint.py PARENT.s CANDIDATE.s KERNEL [--show N]

PARENT.s and CANDIDATE.s are the device assembly of ONE family object built from two trees (the Makefile's flags for the object plus
`--cuda-device-only -S -o FILE.s`, e.g. `-DLM_FAMILY=0 -DLM_PART=0`); KERNEL is a substring of the kernel's (mangled) symbol, or a
regular expression matched against it.

The kernel's instruction stream is cut at its loop back-edges (a branch to a label that stands above it: the loop's first instruction
and the instruction behind the branch both start a region), and of every region the tool keeps the ordered list of floating-point
arithmetic opcodes — fma, fmac, mul, add, sub, their packed forms, rcp, rsq, sqrt, min, max, with the negation and magnitude modifiers
of their operands. Registers, encodings (_e32 / _e64 / _dpp / _sdwa) and every other instruction are ignored. With -ffp-contract=fast a
source change near floating-point code can make the compiler fuse other products (a v_mul + v_fma where there was a packed multiply and
an unfused subtract): that shows as a first region whose lists differ, printed with its neighbourhood. Per region the tool also counts
the instructions by class, so that "fewer moves / LDS instructions / waits" can be read off before a GPU run.

Equal fingerprints are no proof of equal results (the operands could differ); different ones are no proof of different results either
(the scheduler may reorder independent operations: the tool says for how many regions the operations themselves differ, not only their order). It is a pre-check: the bitwise tests on the GPU decide. Exit status: 0 equal,
1 different, 2 the kernel was not found.
"""
import argparse
import re
import sys

FP_OP = re.compile(r"^v_(pk_)?(fma|fmac|fmaak|fmamk|mad|mac|madak|madmk|mul|mul_legacy|add|sub|subrev|rcp|rcp_iflag|rsq|sqrt|min|max|min3|max3|med3|minimum|maximum|minimum3|maximum3)"
                   r"_(f16|f32|f64|bf16)(_e32|_e64)?(_dpp|_sdwa|_e64_dpp)?$")
LABEL = re.compile(r"^([A-Za-z_.$][\w.$]*):")
CLASSES = ("fp_arith", "valu_other", "move", "lds", "lds_permute", "vmem", "salu", "wait", "branch", "other")


def kernel_lines(path, pattern):
    """(symbol, the lines between the kernel's label and its end) of the first symbol matching `pattern`."""
    rx = re.compile(pattern if any(ch in pattern for ch in "^$*+?[]()|\\") else re.escape(pattern))
    out, name = None, None
    with open(path) as fh:
        for raw in fh:
            line = raw.split(";")[0].split("//")[0].rstrip()
            m = LABEL.match(line)
            if out is None:
                if m and not m.group(1).startswith(".L") and rx.search(m.group(1)):
                    name, out = m.group(1), []
                continue
            if line.strip().startswith((".Lfunc_end", ".size")) or line.strip().startswith(".end_amdhsa_kernel"):
                break
            if m and not m.group(1).startswith(".L"):          # the next function
                break
            out.append(line)
    return name, out


def parse(lines):
    """[(kind, text)]: kind 'label' (text = the label) or 'inst' (text = mnemonic, operands)."""
    items = []
    for line in lines:
        s = line.strip()
        if not s or (s.startswith(".") and not LABEL.match(s)):
            continue
        m = LABEL.match(s)
        if m:
            items.append(("label", m.group(1), ""))
            s = s[m.end():].strip()
            if not s:
                continue
        if s.startswith("."):
            continue
        parts = s.split(None, 1)
        items.append(("inst", parts[0], parts[1] if len(parts) > 1 else ""))
    return items


def classify(mn):
    if FP_OP.match(mn):
        return "fp_arith"
    if mn.startswith(("v_mov_", "v_accvgpr_", "v_readlane", "v_readfirstlane", "v_writelane", "v_swap_", "v_permlane")):
        return "move"
    if mn.startswith("ds_"):
        return "lds_permute" if "permute" in mn or "swizzle" in mn else "lds"
    if mn.startswith(("global_", "buffer_", "flat_", "scratch_")):
        return "vmem"
    if mn.startswith("s_waitcnt") or mn.startswith("s_wait_"):
        return "wait"
    if mn.startswith(("s_cbranch", "s_branch", "s_endpgm", "s_setpc", "s_swappc", "s_call")):
        return "branch"
    if mn.startswith("s_"):
        return "salu"
    if mn.startswith("v_"):
        return "valu_other"
    return "other"


def fp_signature(mn, ops):
    """The opcode without its encoding suffix, a sign per source operand ('-' negated, 'a' magnitude taken) and the packed modifiers."""
    base = re.sub(r"(_e32|_e64)?(_dpp|_sdwa)?$", "", mn)
    ops = ops.split("//")[0]
    mods = " ".join(re.findall(r"\b(?:neg_lo|neg_hi|op_sel|op_sel_hi|clamp|mul:\d|div:\d)\b(?::\[[^\]]*\])?", ops))
    fields = [f.strip() for f in re.split(r",(?![^\[]*\])", ops)]
    srcs = [f for f in fields[1:] if f and not re.match(r"^(neg_lo|neg_hi|op_sel|op_sel_hi|clamp|mul|div|quad_perm|row_|wave_|bank_mask|bound_ctrl|dst_sel|dst_unused|src0_sel|src1_sel|fi)\b", f.split(" ")[0])]
    signs = "".join(("-" if f.startswith("-") else "+") + ("a" if "|" in f or "abs(" in f else "") for f in (re.split(r"\s", f)[0] for f in srcs))
    return base + "(" + signs + ")" + ((" " + mods) if mods else "")


def regions(items):
    """The instruction list cut at the loop back-edges: [(first label or '', [instructions])]."""
    pos, insts, label_at = {}, [], {}
    for kind, a, b in items:
        if kind == "label":
            pos[a] = len(insts)
            label_at.setdefault(len(insts), a)
        else:
            insts.append((a, b))
    cuts = {0}
    for i, (mn, ops) in enumerate(insts):
        if mn.startswith(("s_cbranch", "s_branch")):
            tgt = ops.split()[0] if ops else ""
            if tgt in pos and pos[tgt] <= i:
                cuts.add(pos[tgt])
                cuts.add(i + 1)
    cuts = sorted(c for c in cuts if c < len(insts)) + [len(insts)]
    return [(label_at.get(a, ""), insts[a:b]) for a, b in zip(cuts[:-1], cuts[1:])]


def fingerprint(path, pattern):
    name, lines = kernel_lines(path, pattern)
    if name is None:
        return None, []
    out = []
    for label, insts in regions(parse(lines)):
        counts = dict.fromkeys(CLASSES, 0)
        fp = []
        for mn, ops in insts:
            c = classify(mn)
            counts[c] += 1
            if c == "fp_arith":
                fp.append(fp_signature(mn, ops))
        out.append(dict(label=label, n=len(insts), counts=counts, fp=fp))
    return name, out


def totals(regs):
    t = dict.fromkeys(CLASSES, 0)
    for r in regs:
        for k, v in r["counts"].items():
            t[k] += v
    return t


def report(name_a, a, name_b, b, show=6, out=sys.stdout):
    """Prints the comparison; returns True when every region's floating-point list is the same."""
    w = out.write
    w("kernel A: %s\nkernel B: %s\n" % (name_a, name_b))
    w("regions: %d / %d, instructions: %d / %d\n" % (len(a), len(b), sum(r["n"] for r in a), sum(r["n"] for r in b)))
    ta, tb = totals(a), totals(b)
    w("class           A        B    B - A\n")
    for k in CLASSES:
        w("%-12s %6d   %6d   %+6d\n" % (k, ta[k], tb[k], tb[k] - ta[k]))
    same = True
    if len(a) != len(b):
        w("the loop structure differs (%d and %d regions): comparing the whole kernel's list instead of region by region\n" % (len(a), len(b)))
        la, lb = [x for r in a for x in r["fp"]], [x for r in b for x in r["fp"]]
        pairs = [(-1, la, lb)]
    else:
        pairs = [(i, ra["fp"], rb["fp"]) for i, (ra, rb) in enumerate(zip(a, b))]
    for i, la, lb in pairs:
        if la == lb:
            continue
        same = False
        k = next((j for j, (x, y) in enumerate(zip(la, lb)) if x != y), min(len(la), len(lb)))
        where = "whole kernel" if i < 0 else "region %d (label %s / %s, %d / %d instructions)" % (i, a[i]["label"] or "-", b[i]["label"] or "-", a[i]["n"], b[i]["n"])
        w("FIRST DIFFERENCE: %s, floating-point operation %d of %d / %d\n" % (where, k, len(la), len(lb)))
        for j in range(max(0, k - show), min(max(len(la), len(lb)), k + show + 1)):
            x, y = (la[j] if j < len(la) else "-"), (lb[j] if j < len(lb) else "-")
            w("  %5d  %-44s %-44s %s\n" % (j, x, y, "" if x == y else "<--"))
        if i >= 0:
            w("  region classes A: %s\n  region classes B: %s\n" % (a[i]["counts"], b[i]["counts"]))
        break
    if not same:
        # a region with the same operations in another ORDER is the scheduler's doing; other operations are the contraction's
        other = [(i, la, lb) for i, la, lb in pairs if sorted(la) != sorted(lb)]
        w("regions whose lists differ: %d, of which with OTHER operations (not only another order): %d\n" % (sum(1 for _, la, lb in pairs if la != lb), len(other)))
        for i, la, lb in other[:8]:
            ca, cb = {}, {}
            for x in la:
                ca[x] = ca.get(x, 0) + 1
            for x in lb:
                cb[x] = cb.get(x, 0) + 1
            d = {k: cb.get(k, 0) - ca.get(k, 0) for k in sorted(set(ca) | set(cb)) if cb.get(k, 0) != ca.get(k, 0)}
            w("  %s: B - A %s\n" % ("whole kernel" if i < 0 else "region %d (%s)" % (i, a[i]["label"] or "-"), d))
    if same:
        w("floating-point arithmetic: the same %d operations in the same order in every region\n" % sum(len(r["fp"]) for r in a))
        for i, (ra, rb) in enumerate(zip(a, b)):
            if ra["counts"] != rb["counts"]:
                d = {k: rb["counts"][k] - ra["counts"][k] for k in CLASSES if rb["counts"][k] != ra["counts"][k]}
                w("  region %d (%s, %d fp operations): B - A %s\n" % (i, ra["label"] or "-", len(ra["fp"]), d))
    return same


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("parent")
    ap.add_argument("candidate")
    ap.add_argument("kernel")
    ap.add_argument("--show", type=int, default=6, help="operations printed on either side of the first difference")
    args = ap.parse_args(argv)
    na, a = fingerprint(args.parent, args.kernel)
    nb, b = fingerprint(args.candidate, args.kernel)
    if na is None or nb is None:
        print("kernel %r not found in %s" % (args.kernel, args.parent if na is None else args.candidate))
        return 2
    return 0 if report(na, a, nb, b, args.show) else 1


if __name__ == "__main__":
    sys.exit(main())
