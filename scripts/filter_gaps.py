"""Dev: the MFMA gaps of a filter kernel's steady round in a hipcc -S listing, priced by the issue costs of one wave per SIMD.
usage: python scripts/filter_gaps.py build/isa/knn.s <kernel-name-substring, e.g. knn_filter_q4_kernelILi0E> [marker, default "; steady round"] [-v: every gap's opcodes]
       a marker of the form loop=<mfma opcode> takes the innermost loop with the most such MFMAs instead (bodies without a marker comment)

The loop is the one whose last block holds the marker comment (asm volatile("; steady round")).  Its instructions are walked in
EXECUTION order for the steady state: a conditional branch to a label inside the loop is taken (the back edge, and the skips
over code a steady round never runs), one that leaves the loop is not.  Every executed instruction that is not an MFMA is a
filler of the gap it sits in; the gap across the back edge is printed last.  Costs: an MFMA holds vector issue for 8 cycles, a
transcendental costs 8, everything else (s_nop 0, scalar ALU, waits, loads, branches) 4; a gap runs max(32, 8 + its fillers' sum)."""
import re
import sys

TRANS = ("v_exp_", "v_log_", "v_rcp_", "v_rsq_", "v_sqrt_", "v_sin_", "v_cos_")


def kernel_lines(lines, kern):
    start = [i for i, l in enumerate(lines) if re.match(r"^_Z\w*" + re.escape(kern) + r"\w*:", l)][0]
    end = start
    while not lines[end].startswith(".Lfunc_end"):
        end += 1
    return start, end


def is_insn(l):
    return l.startswith("\t") and not l.startswith("\t.") and not l.startswith("\t;") and l.strip() != ""


def walk_opcode_loop(lines, kern, opcode):
    """For bodies without a marker: the innermost loop (a branch back to a label above it) that holds the most instructions
    `opcode`, walked from its header to its back edge."""
    start, end = kernel_lines(lines, kern)
    label_at = {m.group(1): i for i in range(start, end) if (m := re.match(r"^(\.LBB\d+_\d+):", lines[i]))}
    loops = []
    for i in range(start, end):
        if is_insn(lines[i]) and lines[i].split()[0].startswith(("s_cbranch", "s_branch")):
            t = label_at.get(lines[i].split()[1], end)
            if t < i:
                loops.append((sum(1 for k in range(t, i) if is_insn(lines[k]) and lines[k].split()[0] == opcode), -(i - t), t, i))
    loops = [l for l in loops if not any(l[2] <= o[2] and o[3] <= l[3] and o is not l for o in loops)]      # innermost only
    if not loops or max(loops)[0] == 0:
        raise SystemExit(f"no loop with {opcode} in {kern}")
    n = max(loops)[0]
    _, _, lo, hi = max(l for l in loops if l[0] == n)          # the shortest of those with the most
    seq, i = [], lo
    while i <= hi:
        l = lines[i]
        if not is_insn(l):
            i += 1
            continue
        op = l.split()[0]
        seq.append((i, op, l.strip()))
        if i == hi:
            seq[-1] = (i, op + " (taken)", l.strip())
            break
        if op == "s_branch" or op.startswith("s_cbranch"):
            t = label_at[l.split()[1]]
            if i < t <= hi:
                seq[-1] = (i, op + " (taken)", l.strip())
                i = t
                continue
        i += 1
    return seq, (lo, hi)


def walk(lines, kern, marker):
    if marker.startswith("loop="):
        return walk_opcode_loop(lines, kern, marker[5:])
    start, end = kernel_lines(lines, kern)
    mark = [i for i in range(start, end) if lines[i].strip() == marker]
    if len(mark) != 1:
        raise SystemExit(f"{len(mark)} lines '{marker}' in {kern}")
    mark = mark[0]
    label_at = {m.group(1): i for i in range(start, end) if (m := re.match(r"^(\.LBB\d+_\d+):", lines[i]))}
    # the loop: from the label of the marker's block (rotated loop: the latch) or the target of the branch after the marker
    # (unrotated: the header) to the last branch back to it
    branches = [i for i in range(start, end) if is_insn(lines[i]) and lines[i].split()[0].startswith(("s_cbranch", "s_branch"))]
    latch = max(i for i in label_at.values() if i < mark)
    nxt = next(i for i in branches if i > mark)
    lo = min(latch, label_at[lines[nxt].split()[1]]) if label_at[lines[nxt].split()[1]] < mark else latch
    hi = max([i for i in branches if label_at.get(lines[i].split()[1], -1) in (lo, latch)] + [nxt])
    seq, i, steps = [], mark + 1, 0
    while True:
        steps += 1
        if steps > 200000:
            raise SystemExit("no way back to the marker")
        if i > hi:
            raise SystemExit(f"fell out of the loop at line {i + 1}")
        l = lines[i]
        if l.strip() == marker:
            break
        if not is_insn(l):
            i += 1
            continue
        op = l.split()[0]
        seq.append((i, op, l.strip()))
        if op == "s_branch" or op.startswith("s_cbranch"):
            t = label_at[l.split()[1]]
            if op == "s_branch" or lo <= t <= hi:
                seq[-1] = (i, op + " (taken)", l.strip())
                i = t
                continue
        i += 1
    return seq, (lo, hi)


def cost(op):
    return 8 if op.startswith(TRANS) else 4


def main():
    args = [a for a in sys.argv[1:] if a != "-v"]
    path, kern = args[:2]
    marker = args[2] if len(args) > 2 else "; steady round"
    lines = open(path).read().split("\n")
    seq, (lo, hi) = walk(lines, kern, marker)
    waits = [re.search(r"vmcnt\((\d+)\)", t) for _, op, t in seq if op == "s_waitcnt"]       # (from the loop's first instruction on)
    first = next(k for k, (_, op, _) in enumerate(seq) if "mfma" in op)
    seq = seq[first:] + seq[:first]                      # start at an MFMA: the fillers before the first one belong to the last gap
    gaps, census = [], {}
    for _, op, _ in seq:
        if "mfma" in op:
            gaps.append([])
        else:
            gaps[-1].append(op)
            kind = ("s_nop" if op == "s_nop" else "s_waitcnt" if op == "s_waitcnt" else "taken branch" if "taken" in op else
                    "branch not taken" if op.startswith("s_cbranch") else "scalar ALU" if op.startswith("s_") else
                    "v_cndmask" if op.startswith("v_cndmask") else "other VALU" if op.startswith("v_") else "memory")
            census[kind] = census.get(kind, 0) + 1
    n = len(gaps)
    fill = [len(g) for g in gaps]
    cyc = [max(32, 8 + sum(cost(op) for op in g)) for g in gaps]
    print(f"{kern}, loop of '{marker}': lines {lo + 1}..{hi + 1}, {n} MFMAs, {sum(fill)} fillers executed per round ({sum(fill) / n:.2f} per MFMA)")
    print("census:", ", ".join(f"{k} {v}" for k, v in sorted(census.items(), key=lambda kv: -kv[1])))
    skipped = sum(1 for i in range(lo, hi + 1) if is_insn(lines[i])) - len(seq)
    print(f"instructions in the loop's lines that a steady round skips: {skipped}")
    print("fillers per gap (the last gap crosses the back edge):")
    for k in range(0, n, 17):
        print("   ", " ".join(f"{f:2d}" for f in fill[k:k + 17]))
    if "-v" in sys.argv:
        for k, g in enumerate(gaps):
            print(f"    gap {k:2d}:", " ".join(g))
    over = [k for k, f in enumerate(fill) if f > 6]
    print(f"gaps with more than 6 fillers: {len(over)}" + (f" (gap: fillers) " + ", ".join(f"{k}: {fill[k]}" for k in over) if over else ""))
    print(f"modelled cycles per round: {sum(cyc)} against {32 * n} MFMA-paced (+{100.0 * (sum(cyc) - 32 * n) / (32 * n):.1f} %)")
    print("s_waitcnt vmcnt immediates in order:", " ".join(m.group(1) for m in waits if m))


if __name__ == "__main__":
    main()
