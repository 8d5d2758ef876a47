#!/usr/bin/env python3
"""Per-block instruction statistics of a pwg_layer_split16_kernel instantiation, read from the
assembly of csrc/pwg_split16.hip (hipcc -S --cuda-device-only with the library's flags):

  python tools/split16_loop_stats.py pwg_split16.s ILb0ELi1ELb0ELb1ELb1ELi2E

The block loop is the innermost loop (label .. backward branch to it) that encloses the most
MFMAs. Printed: the opcode histogram DESIGN.md 3.0 keeps (MFMA, ds_read_b128, global loads and
stores, s_nop, s_waitcnt, VALU, transcendentals), the registers of the kernel, and for every
ds_read_b128 the number of MFMAs issued between it and the first instruction that reads a
register it writes ("cover"): cover 0 means the read's latency stands in front of its MFMA.
It also checks the read-ahead form's contract: nothing reads or writes a fragment register
between an inline ds_read_b128 and the first wait after it that can release it.
"""
import collections
import re
import sys


def regs(tok):
    """VGPR numbers named by one operand token (v12, v[4:7]); AGPRs and SGPRs are ignored."""
    m = re.fullmatch(r"v(\d+)", tok)
    if m:
        return {int(m.group(1))}
    m = re.fullmatch(r"v\[(\d+):(\d+)\]", tok)
    if m:
        return set(range(int(m.group(1)), int(m.group(2)) + 1))
    return set()


def parse(line):
    line = line.split(";")[0].strip()
    if not line or line.startswith(".") or line.endswith(":"):
        return None
    parts = line.split(None, 1)
    op = parts[0]
    ops = [t.strip() for t in parts[1].split(",")] if len(parts) > 1 else []
    ops = [t.split()[0] if t else t for t in ops]
    return op, ops


def main():
    path, key = sys.argv[1], sys.argv[2]
    lines = open(path).read().split("\n")
    start = next(i for i, l in enumerate(lines) if re.match(r"_ZN3pwg24pwg_layer_split16_kernel%s\w*:" % key, l))
    end = next(i for i in range(start, len(lines)) if lines[i].startswith(".Lfunc_end"))
    body = lines[start:end]
    labels = {m.group(1): i for i, l in enumerate(body) for m in [re.match(r"(\.LBB\w+):", l)] if m}
    best = None
    for i, l in enumerate(body):
        p = parse(l)
        if p and p[0].startswith("s_cbranch") and p[1] and p[1][0] in labels and labels[p[1][0]] < i:
            lo = labels[p[1][0]]
            n = sum(1 for x in body[lo:i] if "v_mfma" in x.split(";")[0])
            if best is None or n > best[0] or (n == best[0] and i - lo < best[2] - best[1]):
                best = (n, lo, i)
    n_mfma, lo, hi = best
    ins = [p for p in (parse(l) for l in body[lo:hi + 1]) if p]
    hist = collections.Counter()
    for op, _ in ins:
        if op.startswith("v_mfma"):
            hist["MFMA"] += 1
        elif op == "ds_read_b128":
            hist["ds_read_b128"] += 1
        elif op.startswith("ds_"):
            hist["other LDS"] += 1
        elif op.startswith("global_load") or op.startswith("buffer_load"):
            hist["global ld"] += 1
        elif op.startswith("global_store") or op.startswith("buffer_store"):
            hist["global st"] += 1
        elif op == "s_nop":
            hist["s_nop"] += 1
        elif op == "s_waitcnt":
            hist["s_waitcnt"] += 1
        elif op.startswith("v_"):
            hist["VALU"] += 1
            if re.match(r"v_(exp|rcp|log|sqrt|rsq)_", op):
                hist["transcendental"] += 1
    print("block loop: %d instructions" % len(ins))
    for k in ("MFMA", "ds_read_b128", "other LDS", "global ld", "global st", "s_nop", "s_waitcnt", "VALU",
              "transcendental"):
        print("  %-16s %d" % (k, hist[k]))
    cover = collections.Counter()
    touched = 0
    for i, (op, ops) in enumerate(ins):
        if op != "ds_read_b128":
            continue
        dst = regs(ops[0])
        n = 0
        waited = False
        for op2, ops2 in ins[i + 1:]:
            if op2 == "s_waitcnt":
                waited = True
            uses = set().union(*[regs(t) for t in ops2]) if ops2 else set()
            if op2 == "ds_read_b128":
                uses = regs(ops2[1]) if len(ops2) > 1 else set()
                if regs(ops2[0]) & dst and not waited:
                    touched += 1
            if uses & dst:
                if not waited:
                    touched += 1
                break
            if op2.startswith("v_mfma"):
                n += 1
        cover[n] += 1
        if n == 0:
            print("  cover 0: ds_read_b128 %s" % ", ".join(ops))
    print("ds_read_b128 by MFMAs between the read and its first consumer:")
    for k in sorted(cover):
        print("  cover %2d: %d" % (k, cover[k]))
    print("fragment registers touched before any wait: %d" % touched)
    meta = "\n".join(lines)
    blk = meta[meta.index(".amdhsa_kernel _ZN3pwg24pwg_layer_split16_kernel" + key):]
    blk = blk[:blk.index(".end_amdhsa_kernel")]
    for k in ("next_free_vgpr", "accum_offset", "next_free_sgpr", "private_segment_fixed_size"):
        m = re.search(r"\.amdhsa_%s (\d+)" % k, blk)
        if m:
            print("  %s %s" % (k, m.group(1)))


if __name__ == "__main__":
    main()
