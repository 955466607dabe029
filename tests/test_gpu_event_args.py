"""Return codes of the event what-if entry points for malformed and degenerate calls.

Four event families (drain, metric, restore, maintenance) times six call forms (host, _device,
_routes, _routes_device, _lfa, _lfa_device) are 24 C entry points; openr_spf_whatif_routes_device
(family "sets" below) shares the route-level device form. Every case takes a well-formed call on
topology.grid(4) (V = 16, L = 24, E = 48, every metric 10), two sources, two events and one
group per node, changes the arguments it names and pins what the call returns: the code, and
what it left in out_total / out_solved (U: not written). The zero-size and hop-count cases pin
the words of ptr and changed as well (X: not written).

The tables are literals. They were recorded from the library before its entry layer was folded
and are the reference for that layer: a reordering of two checks that return different codes
shows up in the "exact" cases, which are invalid twice over.
"""
import ctypes
import dataclasses

import numpy as np
import pytest

from openr_amd import topology as T
from openr_amd import engine as E
from openr_amd.engine import E2BIG, EINVAL, ENOTSUP, OK, USE_LINK_METRIC  # noqa: F401 (the tables name them)
from wide_cases import METRIC_MAX, scaled

pytestmark = pytest.mark.gpu

U = 77  # out_total / out_solved before every call
X = -3  # every word of ptr and changed before every call (as a signed integer)
CAP = 256  # entries: 4 units of at most 16 nodes or groups fit several times over
SOURCES = [0, 15]
DOWN_LINK = 3  # out of service in the "down" graph, with 2^31 on one of its edges
WIDE_EDGE = 7  # carries 2^31 in the "exact" graph

FAMILIES = ("drain", "metric", "restore", "maint", "sets")
FORMS = ("host", "device", "routes", "routes_device", "lfa", "lfa_device")
SUFFIX = {"host": "", "device": "_device", "routes": "_routes", "routes_device": "_routes_device", "lfa": "_lfa",
          "lfa_device": "_lfa_device"}
ALL7 = ("node_ptr", "nodes", "link_ptr", "links", "edge_ptr", "edges", "metrics")
# the event arrays of a family, in the order of its events struct and of its device arguments
FIELDS = {"drain": ALL7[:4], "metric": ALL7[4:], "restore": ALL7, "maint": ALL7, "sets": ("set_ptr", "set_links")}
COUNTS = {"drain": ("n_events", "n_nodes", "n_links"), "metric": ("n_events", "n_edges"),
          "restore": ("n_events", "n_nodes", "n_links", "n_edges"), "maint": ("n_events", "n_nodes", "n_links", "n_edges"),
          "sets": ("n_events", "n_set_links")}
COUNT_OF = {"n_nodes": "nodes", "n_links": "links", "n_edges": "edges", "n_set_links": "set_links"}
STRUCTS = {"drain": E.DrainEvents, "metric": E.MetricEvents, "restore": E.RestoreEvents, "maint": E.MaintEvents}
GROUP_ARGS = ("d_group_ptr", "d_group_nodes", "n_groups", "n_group_nodes")
TAIL = {
    "host": ("sources", "n_sources", "flags", "changed", "delta", "out_solved"),
    "routes": ("sources", "n_sources", "flags", "groups", "changed", "delta", "out_solved"),
    "lfa": ("sources", "n_sources", "flags", "groups", "changed", "unprotected", "lost_backup", "delta", "out_solved"),
    "device": ("d_sources", "n_sources", "flags", "d_changed", "d_ptr", "d_node", "d_dist", "d_nh", "cap", "nh_bytes",
               "stream", "out_total", "out_solved"),
    "routes_device": ("d_sources", "n_sources", "flags") + GROUP_ARGS + (
        "d_changed", "d_ptr", "d_group", "d_metric", "d_nh", "d_n_best", "cap", "nh_bytes", "stream", "out_total",
        "out_solved"),
    "lfa_device": ("d_sources", "n_sources", "flags") + GROUP_ARGS + (
        "d_changed", "d_unprotected", "d_lost_backup", "d_ptr", "d_group", "d_metric", "d_nh", "d_alt", "cap",
        "nh_bytes", "stream", "out_total", "out_solved"),
}
# the caller's entry arrays behind `delta` (host forms) and their element types
DELTA = {"host": (E.WhatifDelta, (("node", np.uint32), ("dist", np.uint64), ("nh", np.uint8))),
         "routes": (E.WhatifRoutes, (("group", np.uint32), ("metric", np.uint64), ("nh", np.uint8),
                                     ("n_best", np.uint32))),
         "lfa": (E.WhatifLfa, (("group", np.uint32), ("metric", np.uint64), ("nh", np.uint8), ("alt", np.uint8)))}


def applies(fam, form):
    return form == "routes_device" if fam == "sets" else True


def event_lists(fam):
    """Two well-formed events of a family on the grid with every metric 10."""
    lists = {"node_ptr": [0, 1, 2], "nodes": [5, 10], "link_ptr": [0, 1, 1], "links": [DOWN_LINK],
             "edge_ptr": [0, 2, 3], "edges": [4, 9, 20], "metrics": [5, 7, 3] if fam == "restore" else [15, 17, 13],
             "set_ptr": [0, 1, 2], "set_links": [DOWN_LINK, 8]}
    return {k: lists[k] for k in FIELDS[fam]}


# --- graphs and engines ------------------------------------------------------------------------
def make_graphs():
    base = scaled(T.grid(4), 10)
    assert (base.num_nodes, base.num_links, base.num_dir_edges) == (16, 24, 48) and base.edge_up.all()
    m = base.metric.copy()
    m[WIDE_EDGE] = METRIC_MAX + 1  # a usable metric past 2^31 - 1: the base plan is the exact-order kernel
    exact = dataclasses.replace(base, metric=m)
    es = np.nonzero(base.link_id == DOWN_LINK)[0]
    assert len(es) == 2
    up, m = base.edge_up.copy(), base.metric.copy()
    up[es] = 0
    m[es[0]] = METRIC_MAX + 1  # not usable while the link is down: the plans stay fast
    return {"base": base, "exact": exact, "down": dataclasses.replace(base, metric=m, edge_up=up)}


@pytest.fixture(scope="module")
def engines():
    out = {}
    for name, g in make_graphs().items():
        out[name] = E.SpfEngine([0])  # one device: device_index 1 is the device count
        out[name].set_graph(g)
    assert all(e.nh_bytes == 1 for e in out.values())
    yield out
    for e in out.values():
        e.close()


# --- a well-formed call as a flat name -> value table -------------------------------------------
def host_array(values, dtype=np.uint32):
    return np.ascontiguousarray(values, dtype=dtype)


def device_array(values, dtype=np.int32):
    import torch

    return torch.from_numpy(np.ascontiguousarray(np.asarray(values, dtype=np.int64).astype(dtype))).to("cuda:0")


def filled(n, dtype, device):
    """n words of X (bytes: 0xEE), in host or device memory."""
    if not device:
        if dtype == np.uint8:
            return np.full(n, 0xEE, dtype=np.uint8)
        return np.full(n, X, dtype=np.dtype(dtype).str.replace("u", "i")).view(dtype)
    import torch

    tt = {np.uint32: torch.int32, np.uint64: torch.int64, np.uint8: torch.uint8}[dtype]
    return torch.full((n,), 0xEE if dtype == np.uint8 else X, dtype=tt, device="cuda:0")


def good_call(fam, form, nhb):
    """name -> value of a well-formed call: lists are the caller's input arrays, arrays and
    tensors its output buffers, integers go as they are."""
    dev = form.endswith("device")
    ev = event_lists(fam)
    a = {("d_" if dev else "ev.") + k: v for k, v in ev.items()}
    a["n_events" if dev else "ev.n_events"] = 2
    if dev:
        a.update({c: len(ev[COUNT_OF[c]]) for c in COUNTS[fam][1:]})
    units = 2 * len(SOURCES)
    a.update({"n_sources": len(SOURCES), "flags": USE_LINK_METRIC, "cap": CAP, "nh_bytes": nhb, "stream": None,
              "out_total": U, "out_solved": U})
    a["d_sources" if dev else "sources"] = list(SOURCES)
    a["d_changed" if dev else "changed"] = filled(units, np.uint32, dev)
    a["d_ptr" if dev else "delta.ptr"] = filled(units + 1, np.uint64, dev)
    if dev:
        a.update({"d_group_ptr": list(range(17)), "d_group_nodes": list(range(16)), "n_groups": 16,
                  "n_group_nodes": 16})
        for name, dtype in (("d_node", np.uint32), ("d_dist", np.uint64), ("d_group", np.uint32),
                            ("d_metric", np.uint64), ("d_nh", np.uint8), ("d_alt", np.uint8), ("d_n_best", np.uint32),
                            ("d_unprotected", np.uint32), ("d_lost_backup", np.uint32)):
            a[name] = filled(units if name in ("d_unprotected", "d_lost_backup") else CAP * nhb, dtype, True)
    else:
        a.update({"groups": True, "groups.n_groups": 16, "groups.group_ptr": list(range(17)),
                  "groups.group_nodes": list(range(16)), "delta": True, "unprotected": filled(units, np.uint32, False),
                  "lost_backup": filled(units, np.uint32, False)})
        for name, dtype in DELTA[form][1]:
            a["delta." + name] = filled(CAP * nhb, dtype, False)
    return a


def good_call_names(fam, form):
    dev = form.endswith("device")
    names = {("d_" if dev else "ev.") + k for k in FIELDS[fam]} | set(TAIL[form]) | {"device_index"}
    names |= set(COUNTS[fam]) if dev else {"ev.n_events", "delta.ptr", "cap", "nh_bytes"}
    if not dev:
        names |= {"delta." + k for k, _ in DELTA[form][1]}
        names.discard("device_index")
    return names


def run(eng, fam, form, changes, want_bufs=False):
    """The call with `changes` applied: (code, out_total, out_solved) of a device form, (code,
    out_solved) of a host form; with want_bufs also the words of ptr and of changed."""
    import torch

    dev = form.endswith("device")
    if not set(changes) <= good_call_names(fam, form):
        return None  # the case names an argument this entry point does not take
    a = good_call(fam, form, eng.nh_bytes)
    a.update(changes)
    keep = []

    def ptr(v):
        if v is None:
            return None
        if isinstance(v, (list, tuple)):
            v = device_array(v) if dev else host_array(v)
        keep.append(v)
        return ctypes.c_void_p(v.data_ptr() if dev else v.ctypes.data)

    total, solved = ctypes.c_uint64(a["out_total"]), ctypes.c_uint64(a["out_solved"])
    name = "openr_spf_whatif_routes_device" if fam == "sets" else f"openr_spf_whatif_{fam}{SUFFIX[form]}"
    fn = getattr(eng._lib, name)
    if dev:
        args = [a.get("device_index", 0)]
        args += [ptr(a["d_" + k]) for k in FIELDS[fam]] + [a[c] for c in COUNTS[fam]]
        for k in TAIL[form]:
            if k in ("out_total", "out_solved"):
                args.append(ctypes.byref(total if k == "out_total" else solved))
            else:
                args.append(a[k] if isinstance(a[k], int) else ptr(a[k]))
    else:
        evs = STRUCTS[fam](a["ev.n_events"], *(ptr(a["ev." + k]) for k in FIELDS[fam]))
        groups = E.SpfGroups(a["groups.n_groups"], ptr(a["groups.group_ptr"]), ptr(a["groups.group_nodes"]))
        cls, entries = DELTA[form]
        delta = cls(ptr(a["delta.ptr"]), *(ptr(a["delta." + k]) for k, _ in entries), a["cap"], a["nh_bytes"])
        args = [ctypes.byref(evs)]
        for k in TAIL[form]:
            if k == "out_solved":
                args.append(ctypes.byref(solved))
            elif k in ("groups", "delta"):
                args.append(ctypes.byref(groups if k == "groups" else delta) if a[k] else None)
            else:
                args.append(a[k] if isinstance(a[k], int) else ptr(a[k]))
    torch.cuda.synchronize()
    code = fn(eng._ctx, *args)
    torch.cuda.synchronize()
    cell = (code, int(total.value), int(solved.value)) if dev else (code, int(solved.value))
    if not want_bufs:
        return cell

    def words(v):
        if v is None:
            return None
        v = v.cpu().numpy() if dev else v
        return tuple(int(x) for x in v.view(np.dtype(v.dtype).str.replace("u", "i")))

    return cell + (words(a["d_ptr" if dev else "delta.ptr"]), words(a["d_changed" if dev else "changed"]))


# --- the cases -----------------------------------------------------------------------------------
@dataclasses.dataclass(frozen=True)
class Case:
    id: str
    host: dict = None  # the changes to a host form's call (None: the case has no host form)
    device: dict = None  # the changes to a device form's call
    graph: str = "base"
    fams: tuple = FAMILIES
    bufs: bool = False  # pin ptr and changed as well


def null_cases():
    out = []
    for k in ALL7:
        out.append(Case("null_" + k, host={"ev." + k: None}, device={"d_" + k: None}))
    # openr_spf_whatif_routes_device does not look at d_set_links: only its d_set_ptr is a case
    out.append(Case("null_set_ptr", device={"d_set_ptr": None}))
    out.append(Case("null_sources", host={"sources": None}, device={"d_sources": None}))
    out.append(Case("null_changed", host={"changed": None}, device={"d_changed": None}))
    out.append(Case("null_ptr", host={"delta.ptr": None}, device={"d_ptr": None}))
    for k in ("node", "dist", "group", "metric", "nh", "alt"):
        out.append(Case("null_entry_" + k, host={"delta." + k: None}, device={"d_" + k: None}))
    return out


CASES = [Case("well_formed", host={}, device={}, bufs=True),
         Case("counts_only", host={"delta": False})] + null_cases() + [
    Case("device_index_minus_1", device={"device_index": -1}),
    Case("device_index_count", device={"device_index": 1}),
    Case("no_events", host={"ev.n_events": 0}, device={"n_events": 0}, bufs=True),
    Case("no_sources", host={"n_sources": 0}, device={"n_sources": 0}, bufs=True),
    Case("hop_count", host={"flags": 0}, device={"flags": 0}, fams=("metric",), bufs=True),
    Case("hop_count_counts_only", host={"flags": 0, "delta": False}, fams=("metric",), bufs=True),
    Case("hop_count_device_index_count", device={"flags": 0, "device_index": 1}, fams=("metric",)),
    Case("hop_count_null_ptr", host={"flags": 0, "delta.ptr": None}, device={"flags": 0, "d_ptr": None},
         fams=("metric",)),
    Case("hop_count_null_sources", host={"flags": 0, "sources": None}, device={"flags": 0, "d_sources": None},
         fams=("metric",)),
    # the value checks of the host forms
    Case("node_out_of_range", host={"ev.nodes": [5, 16]}),
    Case("link_out_of_range", host={"ev.links": [24]}),
    Case("edge_out_of_range", host={"ev.edges": [4, 9, 48]}),
    Case("node_ptr_descends", host={"ev.node_ptr": [0, 2, 1]}),
    Case("link_ptr_descends", host={"ev.link_ptr": [0, 1, 0]}),
    Case("edge_ptr_descends", host={"ev.edge_ptr": [0, 3, 2]}),
    Case("edges_not_ascending", host={"ev.edges": [9, 4, 20]}),
    Case("edges_repeated", host={"ev.edges": [4, 4, 20]}),
    Case("lower", host={"ev.metrics": [15, 9, 13]}, fams=("metric", "maint")),
    Case("raise", host={"ev.metrics": [5, 11, 3]}, fams=("restore",)),
    Case("metric_zero", host={"ev.metrics": [5, 0, 3]}, fams=("restore",)),
    Case("metric_past_2_31", host={"ev.metrics": [15, METRIC_MAX + 1, 13]}, fams=("metric", "maint")),
    # the link comes up with 2^31 on an edge (the well-formed event's own entry would lower it into range)
    Case("restored_link_leaves_the_fast_plans", host={"ev.edge_ptr": None}, graph="down", fams=("restore",)),
    Case("restored_link_lowered_into_range", host={}, graph="down", fams=("restore",)),
    # invalid twice over, on the graph whose base plan is the exact-order kernel
    Case("exact", host={}, device={}, graph="exact"),
    Case("exact_hop_count", host={"flags": 0}, device={"flags": 0}, graph="exact", fams=("metric",)),
    Case("exact_device_index_minus_1", device={"device_index": -1}, graph="exact"),
    Case("exact_device_index_count", device={"device_index": 1}, graph="exact"),
    Case("exact_source_out_of_range", host={"sources": [0, 16]}, graph="exact"),
    Case("exact_null_sources", host={"sources": None}, device={"d_sources": None}, graph="exact"),
]
BY_ID = {c.id: c for c in CASES}
assert len(BY_ID) == len(CASES)


def run_case(engines, case, form):
    """family -> what the call gave, for the families the case and the form apply to."""
    changes = case.device if form.endswith("device") else case.host
    out = {}
    if changes is None:
        return out
    for fam in case.fams:
        if not applies(fam, form):
            continue
        got = run(engines[case.graph], fam, form, changes, case.bufs)
        if got is not None:
            out[fam] = got
    return out


# --- the recorded answers --------------------------------------------------------------------------
# EXPECT[case id][form][family]: (code, out_total, out_solved) of a device form, (code, out_solved)
# of a host form; then, in the cases that pin them, the words of ptr and of changed. One tuple
# in place of the families: every family the case and the form apply to gave it.
EXPECT = {
    "well_formed": {
        "host": {
            "drain": (OK, 6, (0, 5, 5, 5, 9), (5, 0, 0, 4)),
            "metric": (OK, 4, (0, 3, 3, 3, 3), (3, 0, 0, 0)),
            "restore": (OK, 4, (0, 9, 9, 13, 13), (9, 0, 4, 0)),
            "maint": (OK, 6, (0, 5, 5, 5, 9), (5, 0, 0, 4)),
        },
        "device": {
            "drain": (OK, 9, 6, (0, 5, 5, 5, 9), (5, 0, 0, 4)),
            "metric": (OK, 3, 4, (0, 3, 3, 3, 3), (3, 0, 0, 0)),
            "restore": (OK, 13, 4, (0, 9, 9, 13, 13), (9, 0, 4, 0)),
            "maint": (OK, 9, 6, (0, 5, 5, 5, 9), (5, 0, 0, 4)),
        },
        "routes": {
            "drain": (OK, 6, (0, 5, 5, 5, 9), (5, 0, 0, 4)),
            "metric": (OK, 4, (0, 3, 3, 3, 3), (3, 0, 0, 0)),
            "restore": (OK, 4, (0, 9, 9, 13, 13), (9, 0, 4, 0)),
            "maint": (OK, 6, (0, 5, 5, 5, 9), (5, 0, 0, 4)),
        },
        "routes_device": {
            "drain": (OK, 9, 6, (0, 5, 5, 5, 9), (5, 0, 0, 4)),
            "metric": (OK, 3, 4, (0, 3, 3, 3, 3), (3, 0, 0, 0)),
            "restore": (OK, 13, 4, (0, 9, 9, 13, 13), (9, 0, 4, 0)),
            "maint": (OK, 9, 6, (0, 5, 5, 5, 9), (5, 0, 0, 4)),
            "sets": (OK, 5, 6, (0, 3, 3, 5, 5), (3, 0, 2, 0)),
        },
        "lfa": {
            "drain": (OK, 18, (0, 5, 5, 5, 9), (5, 0, 0, 4)),
            "metric": (OK, 11, (0, 3, 3, 3, 3), (3, 0, 0, 0)),
            "restore": (OK, 11, (0, 12, 12, 16, 16), (12, 0, 4, 0)),
            "maint": (OK, 18, (0, 5, 5, 5, 9), (5, 0, 0, 4)),
        },
        "lfa_device": {
            "drain": (OK, 9, 18, (0, 5, 5, 5, 9), (5, 0, 0, 4)),
            "metric": (OK, 3, 11, (0, 3, 3, 3, 3), (3, 0, 0, 0)),
            "restore": (OK, 16, 11, (0, 12, 12, 16, 16), (12, 0, 4, 0)),
            "maint": (OK, 9, 18, (0, 5, 5, 5, 9), (5, 0, 0, 4)),
        },
    },
    "counts_only": {
        "host": {"drain": (OK, 6), "metric": (OK, 4), "restore": (OK, 4), "maint": (OK, 6)},
        "routes": {"drain": (OK, 6), "metric": (OK, 4), "restore": (OK, 4), "maint": (OK, 6)},
        "lfa": {"drain": (OK, 18), "metric": (OK, 11), "restore": (OK, 11), "maint": (OK, 18)},
    },
    "null_node_ptr": {
        "host": (EINVAL, U),
        "device": (EINVAL, U, U),
        "routes": (EINVAL, U),
        "routes_device": (EINVAL, U, U),
        "lfa": (EINVAL, 0),
        "lfa_device": (EINVAL, 0, 0),
    },
    "null_nodes": {
        "host": (EINVAL, U),
        "device": (EINVAL, U, U),
        "routes": (EINVAL, U),
        "routes_device": (EINVAL, U, U),
        "lfa": (EINVAL, 0),
        "lfa_device": (EINVAL, 0, 0),
    },
    "null_link_ptr": {
        "host": {"drain": (OK, 6), "restore": (OK, 4), "maint": (OK, 6)},
        "device": {"drain": (OK, 8, 6), "restore": (OK, 13, 4), "maint": (OK, 9, 6)},
        "routes": {"drain": (OK, 6), "restore": (OK, 4), "maint": (OK, 6)},
        "routes_device": {"drain": (OK, 8, 6), "restore": (OK, 13, 4), "maint": (OK, 9, 6)},
        "lfa": {"drain": (OK, 18), "restore": (OK, 11), "maint": (OK, 18)},
        "lfa_device": {"drain": (OK, 8, 18), "restore": (OK, 16, 11), "maint": (OK, 9, 18)},
    },
    "null_links": {
        "host": (EINVAL, U),
        "device": (EINVAL, U, U),
        "routes": (EINVAL, U),
        "routes_device": (EINVAL, U, U),
        "lfa": (EINVAL, 0),
        "lfa_device": (EINVAL, 0, 0),
    },
    "null_edge_ptr": {
        "host": {"metric": (EINVAL, U), "restore": (OK, 2), "maint": (OK, 6)},
        "device": {"metric": (EINVAL, U, U), "restore": (OK, 0, 2), "maint": (OK, 9, 6)},
        "routes": {"metric": (EINVAL, U), "restore": (OK, 2), "maint": (OK, 6)},
        "routes_device": {"metric": (EINVAL, U, U), "restore": (OK, 0, 2), "maint": (OK, 9, 6)},
        "lfa": {"metric": (EINVAL, 0), "restore": (OK, 6), "maint": (OK, 18)},
        "lfa_device": {"metric": (EINVAL, 0, 0), "restore": (OK, 0, 6), "maint": (OK, 9, 18)},
    },
    "null_edges": {
        "host": (EINVAL, U),
        "device": (EINVAL, U, U),
        "routes": (EINVAL, U),
        "routes_device": (EINVAL, U, U),
        "lfa": (EINVAL, 0),
        "lfa_device": (EINVAL, 0, 0),
    },
    "null_metrics": {
        "host": (EINVAL, U),
        "device": (EINVAL, U, U),
        "routes": (EINVAL, U),
        "routes_device": (EINVAL, U, U),
        "lfa": (EINVAL, 0),
        "lfa_device": (EINVAL, 0, 0),
    },
    "null_set_ptr": {
        "routes_device": (EINVAL, U, U),
    },
    "null_sources": {
        "host": (EINVAL, U),
        "device": (EINVAL, U, U),
        "routes": (EINVAL, U),
        "routes_device": (EINVAL, U, U),
        "lfa": (EINVAL, 0),
        "lfa_device": (EINVAL, 0, 0),
    },
    "null_changed": {
        "host": (EINVAL, U),
        "device": (EINVAL, U, U),
        "routes": (EINVAL, U),
        "routes_device": (EINVAL, U, U),
        "lfa": (EINVAL, 0),
        "lfa_device": (EINVAL, 0, 0),
    },
    "null_ptr": {
        "host": (EINVAL, U),
        "device": (EINVAL, U, U),
        "routes": (EINVAL, U),
        "routes_device": (EINVAL, U, U),
        "lfa": (EINVAL, 0),
        "lfa_device": (EINVAL, 0, 0),
    },
    "null_entry_node": {
        "host": (EINVAL, U),
        "device": (EINVAL, U, U),
    },
    "null_entry_dist": {
        "host": (EINVAL, U),
        "device": (EINVAL, U, U),
    },
    "null_entry_group": {
        "routes": (EINVAL, U),
        "routes_device": (EINVAL, U, U),
        "lfa": (EINVAL, 0),
        "lfa_device": (EINVAL, 0, 0),
    },
    "null_entry_metric": {
        "routes": (EINVAL, U),
        "routes_device": (EINVAL, U, U),
        "lfa": (EINVAL, 0),
        "lfa_device": (EINVAL, 0, 0),
    },
    "null_entry_nh": {
        "host": (EINVAL, U),
        "device": (EINVAL, U, U),
        "routes": (EINVAL, U),
        "routes_device": (EINVAL, U, U),
        "lfa": (EINVAL, 0),
        "lfa_device": (EINVAL, 0, 0),
    },
    "null_entry_alt": {
        "lfa": (EINVAL, 0),
        "lfa_device": (EINVAL, 0, 0),
    },
    "device_index_minus_1": {
        "device": (EINVAL, U, U),
        "routes_device": (EINVAL, U, U),
        "lfa_device": (EINVAL, 0, 0),
    },
    "device_index_count": {
        "device": (EINVAL, U, U),
        "routes_device": (EINVAL, U, U),
        "lfa_device": (EINVAL, 0, 0),
    },
    "no_events": {
        "host": (OK, 0, (0, X, X, X, X), (X, X, X, X)),
        "device": (OK, 0, 0, (0, X, X, X, X), (X, X, X, X)),
        "routes": (OK, 0, (0, X, X, X, X), (X, X, X, X)),
        "routes_device": (OK, 0, 0, (0, X, X, X, X), (X, X, X, X)),
        "lfa": (OK, 0, (0, X, X, X, X), (X, X, X, X)),
        "lfa_device": (OK, 0, 0, (0, X, X, X, X), (X, X, X, X)),
    },
    "no_sources": {
        "host": (OK, 0, (0, X, X, X, X), (X, X, X, X)),
        "device": (OK, 0, 0, (0, X, X, X, X), (X, X, X, X)),
        "routes": (OK, 0, (0, X, X, X, X), (X, X, X, X)),
        "routes_device": (OK, 0, 0, (0, X, X, X, X), (X, X, X, X)),
        "lfa": (OK, 0, (0, X, X, X, X), (X, X, X, X)),
        "lfa_device": (OK, 0, 0, (0, X, X, X, X), (X, X, X, X)),
    },
    "hop_count": {
        "host": (OK, 0, (0, 0, 0, 0, 0), (0, 0, 0, 0)),
        "device": (OK, 0, 0, (0, 0, 0, 0, 0), (0, 0, 0, 0)),
        "routes": (OK, 0, (0, 0, 0, 0, 0), (0, 0, 0, 0)),
        "routes_device": (OK, 0, 0, (0, 0, 0, 0, 0), (0, 0, 0, 0)),
        "lfa": (OK, 6, (0, 0, 0, 0, 0), (0, 0, 0, 0)),
        "lfa_device": (OK, 0, 6, (0, 0, 0, 0, 0), (0, 0, 0, 0)),
    },
    "hop_count_counts_only": {
        "host": (OK, 0, (X, X, X, X, X), (0, 0, 0, 0)),
        "routes": (OK, 0, (X, X, X, X, X), (0, 0, 0, 0)),
        "lfa": (OK, 6, (X, X, X, X, X), (0, 0, 0, 0)),
    },
    "hop_count_device_index_count": {
        "device": (EINVAL, U, U),
        "routes_device": (EINVAL, U, U),
        "lfa_device": (EINVAL, 0, 0),
    },
    "hop_count_null_ptr": {
        "host": (EINVAL, U),
        "device": (EINVAL, U, U),
        "routes": (EINVAL, U),
        "routes_device": (EINVAL, U, U),
        "lfa": (EINVAL, 0),
        "lfa_device": (EINVAL, 0, 0),
    },
    "hop_count_null_sources": {
        "host": (EINVAL, U),
        "device": (EINVAL, U, U),
        "routes": (EINVAL, U),
        "routes_device": (EINVAL, U, U),
        "lfa": (EINVAL, 0),
        "lfa_device": (EINVAL, 0, 0),
    },
    "node_out_of_range": {
        "host": (EINVAL, U),
        "routes": (EINVAL, U),
        "lfa": (EINVAL, 0),
    },
    "link_out_of_range": {
        "host": (EINVAL, U),
        "routes": (EINVAL, U),
        "lfa": (EINVAL, 0),
    },
    "edge_out_of_range": {
        "host": (EINVAL, U),
        "routes": (EINVAL, U),
        "lfa": (EINVAL, 0),
    },
    "node_ptr_descends": {
        "host": (EINVAL, U),
        "routes": (EINVAL, U),
        "lfa": (EINVAL, 0),
    },
    "link_ptr_descends": {
        "host": (EINVAL, U),
        "routes": (EINVAL, U),
        "lfa": (EINVAL, 0),
    },
    "edge_ptr_descends": {
        "host": (EINVAL, U),
        "routes": (EINVAL, U),
        "lfa": (EINVAL, 0),
    },
    "edges_not_ascending": {
        "host": (EINVAL, U),
        "routes": (EINVAL, U),
        "lfa": (EINVAL, 0),
    },
    "edges_repeated": {
        "host": (EINVAL, U),
        "routes": (EINVAL, U),
        "lfa": (EINVAL, 0),
    },
    "lower": {
        "host": (EINVAL, U),
        "routes": (EINVAL, U),
        "lfa": (EINVAL, 0),
    },
    "raise": {
        "host": (EINVAL, U),
        "routes": (EINVAL, U),
        "lfa": (EINVAL, 0),
    },
    "metric_zero": {
        "host": (EINVAL, U),
        "routes": (EINVAL, U),
        "lfa": (EINVAL, 0),
    },
    "metric_past_2_31": {
        "host": (EINVAL, U),
        "routes": (EINVAL, U),
        "lfa": (EINVAL, 0),
    },
    "restored_link_leaves_the_fast_plans": {
        "host": (ENOTSUP, U),
        "routes": (ENOTSUP, U),
        "lfa": (ENOTSUP, 0),
    },
    "restored_link_lowered_into_range": {
        "host": (OK, 5),
        "routes": (OK, 5),
        "lfa": (OK, 15),
    },
    "exact": {
        "host": (ENOTSUP, U),
        "device": (ENOTSUP, U, U),
        "routes": (ENOTSUP, U),
        "routes_device": (ENOTSUP, U, U),
        "lfa": (ENOTSUP, 0),
        "lfa_device": (ENOTSUP, 0, 0),
    },
    "exact_hop_count": {
        "host": (OK, 0),
        "device": (OK, 0, 0),
        "routes": (OK, 0),
        "routes_device": (OK, 0, 0),
        "lfa": (OK, 6),
        "lfa_device": (OK, 0, 6),
    },
    "exact_device_index_minus_1": {
        "device": (ENOTSUP, U, U),
        "routes_device": (EINVAL, U, U),
        "lfa_device": (ENOTSUP, 0, 0),
    },
    "exact_device_index_count": {
        "device": (ENOTSUP, U, U),
        "routes_device": (EINVAL, U, U),
        "lfa_device": (ENOTSUP, 0, 0),
    },
    "exact_source_out_of_range": {
        "host": (EINVAL, U),
        "routes": (EINVAL, U),
        "lfa": (EINVAL, 0),
    },
    "exact_null_sources": {
        "host": (EINVAL, U),
        "device": (ENOTSUP, U, U),
        "routes": (EINVAL, U),
        "routes_device": (EINVAL, U, U),
        "lfa": (EINVAL, 0),
        "lfa_device": (ENOTSUP, 0, 0),
    },
}


def pairs():
    return [(c.id, f) for c in CASES for f in FORMS if EXPECT.get(c.id, {}).get(f)]


@pytest.mark.parametrize("case_id,form", pairs())
def test_event_call(engines, case_id, form):
    got = run_case(engines, BY_ID[case_id], form)
    want = EXPECT[case_id][form]
    if isinstance(want, tuple):
        want = {fam: want for fam in got}
        assert want
    print(case_id, form, got)
    assert got == want


def test_table_is_complete(engines):
    """Every entry point is in the table, under every case that applies to it."""
    seen = set()
    for c in CASES:
        for f in FORMS:
            changes = c.device if f.endswith("device") else c.host
            if changes is None:
                continue
            fams = [m for m in c.fams if applies(m, f) and set(changes) <= set(good_call_names(m, f))]
            want = EXPECT.get(c.id, {}).get(f, {})
            assert isinstance(want, tuple) and fams or sorted(want) == sorted(fams), (c.id, f)
            seen.update((m, f) for m in fams)
    assert len(seen) == 25 and len({(m, f) for m, f in seen if m != "sets"}) == 24
