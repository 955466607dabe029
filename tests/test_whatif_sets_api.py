"""Link-set what-if sweep (openr_spf_whatif_sets*): the public surface, without a GPU.

The C-ABI symbols, the Python helpers that build node-failure and shared-risk-group
sets, and the wave-uniformity of the set filter kernel (compiles only).
"""
import os
import re
import subprocess
import sys

import pytest

from openr_amd import engine
from openr_amd import topology as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "openr_spf.h")
SET_CALLS = ("openr_spf_whatif_sets", "openr_spf_whatif_sets_device", "openr_spf_whatif_sets_delta",
             "openr_spf_whatif_sets_delta_device")


def test_set_calls_declared_bound_and_exported():
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    declared = set(re.findall(r"\b(openr_spf_[a-z_0-9]+)\s*\(", text))
    lib = engine.load_library()
    out = subprocess.run(["nm", "-D", "--defined-only", engine.LIB_PATH], capture_output=True, text=True, check=True)
    exported = set(re.findall(r"\bT (openr_spf_\w+)", out.stdout))
    for name in SET_CALLS:
        assert name in declared, name
        assert name in engine.EXPORTS, name
        assert name in exported, name
        assert hasattr(lib, name)
    for m in ("whatif_sets", "whatif_sets_device", "whatif_sets_delta", "whatif_sets_delta_device"):
        assert callable(getattr(engine.SpfEngine, m))
    assert lib.openr_spf_abi_version() == 1  # additive: the ABI version stays


def test_node_failure_sets_grid():
    g = T.grid(3)  # nodes r * 3 + c; link ids in the order the rows first list them
    want = [[0, 1], [0, 2, 3], [2, 4], [1, 5, 6], [3, 5, 7, 8], [4, 7, 9], [6, 10], [8, 10, 11], [9, 11]]
    assert T.node_failure_sets(g) == want
    assert T.node_failure_sets(g, [4, 0]) == [want[4], want[0]]
    assert T.node_failure_sets(g, []) == []
    with pytest.raises(ValueError):
        T.node_failure_sets(g, [9])
    # every link belongs to the sets of exactly its two end nodes
    count = [0] * g.num_links
    for s in want:
        for l in s:
            count[l] += 1
    assert count == [2] * g.num_links


def test_node_failure_sets_parallel_links_once_per_set():
    g = T.from_adj_map({0: [1, 1, 2], 1: [0, 0, 2], 2: [0, 1]})  # two parallel links 0 - 1
    assert g.num_links == 4
    sets = T.node_failure_sets(g)
    assert sets == [[0, 1, 2], [0, 1, 3], [2, 3]]
    for u, s in enumerate(sets):
        assert s == sorted(set(s))
        assert set(s) == set(g.link_id[g.row_ptr[u] : g.row_ptr[u + 1]].tolist())


def test_srlg_sets_validates_and_sorts():
    g = T.grid(3)
    assert T.srlg_sets(g, [[3, 1, 3], [], (11,)]) == [[1, 3], [], [11]]
    with pytest.raises(ValueError):
        T.srlg_sets(g, [[0, 1], [g.num_links]])
    with pytest.raises(ValueError):
        T.srlg_sets(g, [[-1]])


def test_set_filter_collectives_outside_the_link_loop():
    """whatif_set_filter's loop over a set's links has a per-lane trip count (a wave can
    straddle sets of different sizes), so it is the one loop that may have a divergent exit;
    the grid-stride unit loop around the ballot / shuffle append may not (the failure mode
    tests/test_uniformity.py records for the repair kernel)."""
    sys.path.insert(0, os.path.join(ROOT, "scripts"))
    import uniformity_check as uc

    if not (os.path.exists(uc.HIPCC) and os.path.exists(uc.OPT)):
        pytest.skip("needs hipcc and the ROCm LLVM opt")
    res = uc.divergent_exit_cycles(os.path.join(ROOT, "openr_amd", "csrc", "spf_sweep.hip"), "whatif_set_filter",
                                   [os.path.join(ROOT, "include")])
    assert len(res) == 1, sorted(res)
    (cycles,) = res.values()
    # at most the leaf loop, nested in the unit loop (depth 2), a handful of basic blocks
    assert len(cycles) <= 1, cycles
    for depth, blocks in cycles:
        assert depth >= 2 and blocks <= 12, cycles
