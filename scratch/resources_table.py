#!/usr/bin/env python3
"""gicp_align_kernel rows of two registration.resources.txt files side by side (parent | new):
usage resources_table.py PARENT.resources.txt NEW.resources.txt"""
import re
import sys


def load(path):
    out = {}
    for l in open(path):
        m = re.search(r"gicp_align_kernelILi(\d)ELb(\d)ELb(\d)ELb(\d)E.*VGPRs: (\d+).*ScratchSize \[bytes/lane\]: (\d+).*VGPRs Spill: (\d+)", l)
        if m:
            out[tuple(map(int, m.groups()[:4]))] = tuple(map(int, m.groups()[4:]))
    return out


a, b = load(sys.argv[1]), load(sys.argv[2])
print("LOSS FAST_NN P2D SHARDED |  parent: VGPRs scratch spills |  new: VGPRs scratch spills")
for key in sorted(a, key=lambda k: (k[2], k[3], k[1], k[0])):
    pa, pb = a[key], b[key]
    print("  %d     %d     %d     %d     |            %3d     %3d    %3d |         %3d     %3d    %3d%s" %
          (*key, *pa, *pb, "   <- benchmarked" if key == (0, 1, 0, 0) else ""))
for p2d, name in ((0, "GICP (P2D = 0"), (1, "POINT_TO_DISTRIBUTION (")):
    ks = [k for k in a if k[2] == p2d]
    print("%s, %d instantiations): parent spills max %d, scratch max %d; new spills max %d, scratch max %d, VGPRs max %d; "
          "no instantiation worse than the parent: %s" %
          (name, len(ks), max(a[k][2] for k in ks), max(a[k][1] for k in ks), max(b[k][2] for k in ks), max(b[k][1] for k in ks),
           max(b[k][0] for k in ks), all(b[k][2] <= a[k][2] and b[k][1] <= a[k][1] for k in ks)))
