"""The lean pass's level-row variant keeps wave-uniform loop exits (CPU: compiles only).

`bfs_ell_rows_kernel` is `bfs_ell_kernel`'s body plus one leaf loop that stores the unit's
u8 level row for `nh_derive_kernel` (spf_derive.hip). The loops around its barrier must exit
on block- or wave-uniform values exactly as the plain kernel's do
(tests/test_lean_uniformity.py has the reasoning and the bound).
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


def test_level_row_variant_loops_have_uniform_exits():
    res = uc.divergent_exit_cycles(os.path.join(ROOT, "openr_amd", "csrc", "spf_bfs_lvl.hip"), "bfs_ell_rows_kernel",
                                   [os.path.join(ROOT, "include")])
    # {nibble, byte, half, word next-hop fields} x {128, 256 threads} x {delta rows}
    assert len(res) == 16, sorted(res)
    for name, cycles in res.items():
        big = [c for c in cycles if c[1] > MAX_LEAF_BLOCKS]
        assert not big, f"{name}: loops with divergent exits {big}"
