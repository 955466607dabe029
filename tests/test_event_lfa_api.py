"""Loop-free alternates under drain, metric and restore events (openr_spf_whatif_drain_lfa*,
_metric_lfa*, _restore_lfa*): the public surface, without a GPU.

The C-ABI symbols and Python bindings, and the wave-uniformity of every kernel in
spf_elfa.hip (compiles only), analysed as tests/test_whatif_lfa_api.py analyses spf_wlfa.hip.
"""
import os
import re
import subprocess

import pytest

from openr_amd import engine
from uniformity_ir import COLLECTIVE, analyse, kernel, no_collective_in

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "openr_spf.h")
SRC = os.path.join(ROOT, "openr_amd", "csrc", "spf_elfa.hip")
FAMILIES = ("drain", "metric", "restore")
CALLS = tuple("openr_spf_whatif_%s_lfa%s" % (f, d) for f in FAMILIES for d in ("", "_device"))


def test_event_lfa_calls_declared_bound_and_exported():
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    declared = set(re.findall(r"\b(openr_spf_[a-z_0-9]+)\s*\(", text))
    lib = engine.load_library()
    out = subprocess.run(["nm", "-D", "--defined-only", engine.LIB_PATH], capture_output=True, text=True, check=True)
    exported = set(re.findall(r"\bT (openr_spf_\w+)", out.stdout))
    assert len(CALLS) == 6
    for name in CALLS:
        assert name in declared, name
        assert name in engine.EXPORTS, name
        assert name in exported, name
        assert hasattr(lib, name)
        assert callable(getattr(engine.SpfEngine, name[len("openr_spf_"):]))
    assert lib.openr_spf_abi_version() == 1  # additive: the ABI version stays
    build_id = lib.openr_spf_build_id().decode()
    assert "spf_elfa.hip" in build_id and "spf_restore_event.h" in build_id  # the build id covers the new files


def test_header_no_longer_lists_the_gap():
    text = open(HEADER).read()
    assert not re.search(r"Not covered:\s+loop-free\s+alternates\s+under", text)
    for fam in FAMILIES:
        assert "openr_spf_whatif_%s_lfa below" % fam in re.sub(r"\s+", " ", text)


def test_new_kernels_do_not_reuse_the_wlfa_name():
    src = open(SRC).read()
    assert not re.search(r"__global__[^;{]*\bwlfa", src)


# --- wave uniformity of the kernels ---------------------------------------------------------
@pytest.fixture(scope="module")
def analysis():
    """The kernels of spf_elfa.hip (tests/uniformity_ir.py)."""
    return analyse(SRC, "elfa")


def names_of(analysis):
    """elfa_kernel<family,emit>, elfa_mark<family> and the plain names, from the mangled ones."""
    out = []
    for k in analysis:
        base = re.search(r"\d+(elfa_[a-z_]+)", k).group(1)
        t = re.search(r"elfa_(?:kernel|mark)ILi(\d)E(?:Lb([01])E)?", k)
        out.append(base + ("<%s>" % ",".join(x for x in t.groups() if x is not None) if t else ""))
    return sorted(out)


def test_every_kernel_is_analysed(analysis):
    want = ["elfa_base"] + ["elfa_kernel<%d,%d>" % (f, e) for f in range(3) for e in range(2)] + \
        ["elfa_mark<%d>" % f for f in range(3)] + ["elfa_nbr_table", "elfa_rows_compact", "elfa_rows_count",
                                                   "elfa_rows_mark"]
    assert names_of(analysis) == sorted(want), names_of(analysis)


# divergent-exit loops of elfa_kernel<family, emit>, as the final build shows them
# (drain: wlfa_kernel's 23, the set scan in three places; metric: no set scan; restore: the
# link-slice scan and the binary search of restore::Slices in their place)
KERNEL_LOOPS = {(0, 0): 23, (0, 1): 23, (1, 0): 20, (1, 1): 20, (2, 0): 27, (2, 1): 27}


@pytest.mark.parametrize("fam", [0, 1, 2], ids=list(FAMILIES))
@pytest.mark.parametrize("emit", [0, 1], ids=["count", "emit"])
def test_elfa_kernel_barriers_outside_divergent_loops(analysis, fam, emit):
    """elfa_kernel has no wave collective. Its barriers sit in the work-list loop, the
    candidate-chunk loop and the slice loop, all workgroup-uniform. The loops with per-lane
    trip counts are the staging loops, the scans of a drain's link slice or a restore's link
    and edge slices (the binary search of a lowered metric among them), the hash probes, the
    delta scans and the member loops of a lane's group."""
    blocks, cycles = kernel(analysis, "elfa_kernelILi%dELb%dE" % (fam, emit))
    assert len(cycles) == KERNEL_LOOPS[(fam, emit)], len(cycles)
    no_collective_in(blocks, cycles)
    barrier_blocks = [lb for lb, b in blocks.items() if "s.barrier" in b]
    assert barrier_blocks  # the barriers exist, outside every divergent-exit loop
    in_cycles = {lb for _, labels in cycles for lb in labels}
    assert not in_cycles & set(barrier_blocks)
    assert all(depth >= 2 for depth, _ in cycles), cycles  # never the work-list loop (1)
    others = [m.group(0) for b in blocks.values() for m in COLLECTIVE.finditer(b) if "s.barrier" not in m.group(0)]
    assert not others, others


MARK_LOOPS = {0: 2, 1: 1, 2: 4}  # a source's edges, and the event's slice scans


@pytest.mark.parametrize("fam", [0, 1, 2], ids=list(FAMILIES))
def test_elfa_mark_barriers_in_the_uniform_round_loop(analysis, fam):
    """elfa_mark: the barriers around the workgroup's LDS count sit in the round loop, whose
    trip count is a function of the launch alone; a source's edges and an event's slices are
    per-thread loops without a barrier or a wave collective."""
    blocks, cycles = kernel(analysis, "elfa_markILi%dE" % fam)
    assert len(cycles) == MARK_LOOPS[fam], len(cycles)
    no_collective_in(blocks, cycles)
    barrier_blocks = [lb for lb, b in blocks.items() if "s.barrier" in b]
    assert barrier_blocks
    in_cycles = {lb for _, labels in cycles for lb in labels}
    assert not in_cycles & set(barrier_blocks)
    others = [m.group(0) for b in blocks.values() for m in COLLECTIVE.finditer(b) if "s.barrier" not in m.group(0)]
    assert not others, others


def test_elfa_base_barriers_in_the_uniform_source_loop(analysis):
    blocks, cycles = kernel(analysis, "elfa_base")
    assert len(cycles) == 1, cycles
    no_collective_in(blocks, cycles)
    assert any("s.barrier" in b for b in blocks.values())
    assert all(depth >= 2 for depth, _ in cycles), cycles


@pytest.mark.parametrize("name", ["elfa_rows_mark", "elfa_rows_count", "elfa_rows_compact", "elfa_nbr_table"])
def test_closure_and_table_kernels_have_no_collective(analysis, name):
    blocks, _ = kernel(analysis, name)
    assert not any(COLLECTIVE.search(b) for b in blocks.values())
