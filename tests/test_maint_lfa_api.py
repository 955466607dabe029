"""Loop-free alternates under maintenance events (openr_spf_whatif_maint_lfa*): the public
surface, without a GPU.

The C-ABI symbols and Python bindings, and the documents: the maintenance sweep no longer
lists its loop-free-alternate form as not covered. The pass adds no kernel (the drain
instantiations of spf_elfa.hip serve it), which tests/test_event_lfa_api.py pins.
"""
import inspect
import os
import re
import subprocess

from openr_amd import engine

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "openr_spf.h")
CSRC = os.path.join(ROOT, "openr_amd", "csrc")
CALLS = ("openr_spf_whatif_maint_lfa", "openr_spf_whatif_maint_lfa_device")


def test_maint_lfa_calls_declared_bound_and_exported():
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    declared = set(re.findall(r"\b(openr_spf_[a-z_0-9]+)\s*\(", text))
    lib = engine.load_library()
    out = subprocess.run(["nm", "-D", "--defined-only", engine.LIB_PATH], capture_output=True, text=True, check=True)
    exported = set(re.findall(r"\bT (openr_spf_\w+)", out.stdout))
    for name in CALLS:
        assert name in declared, name
        assert name in engine.EXPORTS, name
        assert name in exported, name
        assert hasattr(lib, name)
        assert callable(getattr(engine.SpfEngine, name[len("openr_spf_"):]))
        # the argument list of the restore call of the same form, the events struct apart
        twin = getattr(lib, name.replace("maint", "restore")).argtypes
        assert len(getattr(lib, name).argtypes) == len(twin)
    assert lib.openr_spf_whatif_maint_lfa.argtypes[1]._type_ is engine.MaintEvents
    assert lib.openr_spf_abi_version() == 1  # additive: the ABI version stays


def test_python_signatures_mirror_the_restore_forms():
    for name in ("whatif_maint_lfa", "whatif_maint_lfa_device"):
        mine = inspect.signature(getattr(engine.SpfEngine, name))
        twin = inspect.signature(getattr(engine.SpfEngine, name.replace("maint", "restore")))
        assert list(mine.parameters) == list(twin.parameters), name
        assert [p.default for p in mine.parameters.values()] == [p.default for p in twin.parameters.values()], name
    head = list(inspect.signature(engine.SpfEngine.whatif_maint_lfa).parameters)[1:8]
    assert head == ["node_sets", "link_sets", "edge_sets", "metric_sets", "sources", "groups", "use_link_metric"]


def test_header_no_longer_lists_the_gap():
    text = re.sub(r"\s+", " ", open(HEADER).read())
    assert "a loop-free-alternate form of this sweep" not in text
    assert not re.search(r"Not covered:[^*]*loop-free[- ]alternate[^*]*maintenance", text)
    assert "openr_spf_whatif_maint_lfa below" in text
    src = re.sub(r"\s+", " ", open(os.path.join(CSRC, "spf_maint.hip")).read().replace("//", ""))
    assert not re.search(r"Not covered: loop-free alternates under a maintenance event", src)
    assert "openr_spf_whatif_maint_lfa" in src


def test_family_is_a_fourth_value_served_by_the_drain_instantiations():
    kernels_h = open(os.path.join(CSRC, "spf_kernels.h")).read()
    assert re.search(r"enum ElfaFamily : int \{[^}]*kElfaMaint = 3[^}]*\}", kernels_h)
    elfa = open(os.path.join(CSRC, "spf_elfa.hip")).read()
    # an explicit branch in both launchers, and no instantiation of its own
    assert len(re.findall(r"fam == kElfaDrain \|\| fam == kElfaMaint", elfa)) == 2
    assert len(re.findall(r"else if \(fam == kElfaRestore\)", elfa)) == 2
    assert not re.search(r"<\s*kElfaMaint", elfa)
    capi = open(os.path.join(CSRC, "spf_capi.hip")).read()
    assert len(re.findall(r"\bkElfaMaint\b", capi)) >= 2
