"""The lean level pass's loops around its barrier have only wave-uniform exits (CPU: compiles only).

`bfs_ell_kernel` keeps a workgroup's waves in step with one `lds_barrier()` per wide level
and one per narrow run (levels of at most 64 nodes, which wave 0 expands alone while the
other waves wait at that barrier). Every loop around that barrier (the unit loop, the level
loop and the narrow-run loop) exits on block- or wave-uniform values: counts taken with
readfirstlane, ballot popcounts. If LLVM's uniformity analysis saw one of those exits as
divergent, the loop would be compiled with per-lane exit masks around a barrier, which is
how the what-if repair kernel came to hang ("The hang";
tests/test_uniformity.py).

Only the leaf loops with a per-lane trip count (init, level 0, row write-out: a lane per
word or edge) may have a divergent exit; they are at most 9 basic blocks. The bound is the
leaf bound of tests/test_uniformity.py.
"""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "scripts"))

import uniformity_check as uc  # noqa: E402

pytestmark = pytest.mark.skipif(not (os.path.exists(uc.HIPCC) and os.path.exists(uc.OPT)),
                                reason="needs hipcc and the ROCm LLVM opt")

MAX_LEAF_BLOCKS = 12


def test_lean_pass_loops_have_uniform_exits():
    res = uc.divergent_exit_cycles(os.path.join(ROOT, "openr_amd", "csrc", "spf_bfs_lvl.hip"), "bfs_ell_kernel",
                                   [os.path.join(ROOT, "include")])
    # {nibble, byte, half, word next-hop fields} x {128, 256 threads} x {profiling} x {delta rows}
    assert len(res) == 32, sorted(res)
    for name, cycles in res.items():
        big = [c for c in cycles if c[1] > MAX_LEAF_BLOCKS]
        assert not big, f"{name}: loops with divergent exits {big}"
