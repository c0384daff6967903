#!/usr/bin/env python3
"""Per basic block of one kernel in a `hipcc -S --cuda-device-only` listing: vector instructions, v_readlane_b32, register
moves (v_mov_b32 / v_pk_mov_b32 / v_accvgpr_*), packed fp32 (v_pk_fma/mul/add_f32) and s_nop. A report tool for
profiles/r07_a_gicp_align_kernel_resources_parent_and_new.txt: the blocks of the certified path of a point are picked by
hand from its output (the loop head up to the certificate's branch, and the arithmetic tail).

usage: isa_block_counts.py listing.s SUBSTRING_OF_MANGLED_KERNEL_NAME [min_vector_instructions] [path=135,136,bb137,...]
Blocks are named by their label number (.LBB<f>_<n> -> n) or, where the compiler only left a comment, bb<n> (; %bb.<n>:);
path=... adds a line with the sum over those blocks: the instructions one point executes on that path."""
import re
import sys


def main():
    listing, key = sys.argv[1], sys.argv[2]
    least = int(sys.argv[3]) if len(sys.argv) > 3 else 8
    path = [a[5:].split(",") for a in sys.argv[4:] if a.startswith("path=")]
    lines = open(listing).read().split("\n")
    start = next(i for i, l in enumerate(lines) if l.startswith("_Z") and ":" in l and key in l.split(":")[0])
    end = next(i for i in range(start, len(lines)) if lines[i].strip().startswith("s_endpgm"))
    print(lines[start])
    blocks, cur = [], ["entry", []]
    for l in lines[start + 1:end + 1]:
        t = l.strip()
        if not t or t.startswith(";") or t.startswith("."):
            m = re.match(r"\.LBB\d+_(\d+):", t) or re.match(r"; %bb\.(\d+):", t)
            if m:
                blocks.append(cur)
                cur = [("bb" if t.startswith(";") else "") + m.group(1), []]
            continue
        cur[1].append(t.split()[0])
    blocks.append(cur)
    tot = [0] * 6
    sums = [[0] * 6]
    print("%-12s %7s %9s %6s %7s %6s %7s" % ("block", "vector", "readlane", "moves", "packed", "s_nop", "v_mem"))
    for name, ops in blocks:
        vec = [o for o in ops if o.startswith("v_")]
        row = [len(vec), sum(o.startswith("v_readlane") for o in ops),
               sum(o.startswith(("v_mov_b32", "v_pk_mov_b32", "v_accvgpr")) for o in ops),
               sum(o.startswith(("v_pk_fma_f32", "v_pk_mul_f32", "v_pk_add_f32")) for o in ops),
               sum(o.startswith("s_nop") for o in ops), sum(o.startswith(("global_", "buffer_", "scratch_", "flat_")) for o in ops)]
        tot = [a + b for a, b in zip(tot, row)]
        for pth in path:
            if name in pth:
                sums[0] = [a + b for a, b in zip(sums[0], row)]
        if row[0] >= least:
            print("%-12s %7d %9d %6d %7d %6d %7d" % (name, *row))
    print("%-12s %7d %9d %6d %7d %6d %7d" % ("kernel", *tot))
    if path:
        print("%-12s %7d %9d %6d %7d %6d %7d" % ("path", *sums[0]))


if __name__ == "__main__":
    main()
