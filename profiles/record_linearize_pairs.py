#!/usr/bin/env python3
"""Record tests/golden/linearize_pairs_parent.npz: what tests/test_gpu_linearize_pairs.py compares a build with.

Run it on a GPU with the library of the commit to compare AGAINST (the parent of the change under test):

    SP_AMD_LIB=/path/to/parent/libsycl_points_amd.so python3 profiles/record_linearize_pairs.py PARENT_COMMIT_HASH [OUT.npz]

It runs the test file's own functions (same inputs, same calls) with the correspondence reuse as shipped and writes, a row per
(reg_type, loss, n) in the test's case_index order: the fan-in row of one sp_gicp_align_step at the fixed pose, and pose / linear system / last update of a
5-iteration sp_gicp_align_fused; beside them the pose, the sizes, the checksums of the inputs and the commit hash.
"""
import importlib.util
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    commit = sys.argv[1]
    assert len(commit) == 40, "the full hash of the commit whose library is loaded"
    out = sys.argv[2] if len(sys.argv) > 2 else os.path.join(ROOT, "tests", "golden", "linearize_pairs_parent.npz")
    spec = importlib.util.spec_from_file_location("t", os.path.join(ROOT, "tests", "test_gpu_linearize_pairs.py"))
    t = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(t)
    import sycl_points_amd.api as sp

    print("library:", sp._lib.LIB_PATH)
    scene, sums = t.make_scene(sp)
    T0 = t.fixed_pose()
    data = dict(parent_commit=np.array(commit), ns=np.array(t.NS), T0=T0, input_crc32=sums)
    cases = {}
    for reg_type in t.REGS:
        for loss in t.LOSSES:
            for n in t.NS:
                assert t.case_index(reg_type, loss, n) == len(cases.get("row", []))
                got = t.compute_case(sp, scene, reg_type, loss, n, T0, None)
                for what, v in got.items():
                    cases.setdefault(what, []).append(v)
                row = got["row"]
                print(reg_type, loss, n, "inliers", int(row[29]) * 4096 + int(row[28]), "searched", row[30], "error", row[27])
    data.update({what: np.stack(v) for what, v in cases.items()})  # one array per kind, a row per case (test: case_index)
    np.savez_compressed(out, **data)
    print("wrote", out, os.path.getsize(out), "bytes,", len(data), "arrays")


if __name__ == "__main__":
    main()
