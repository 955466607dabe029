"""ctypes binding of the SPF engine's C-ABI (include/openr_spf.h).

``SpfEngine`` is a thin, typed wrapper: every call goes straight to
libopenr_spf.so and every failure raises ``SpfError`` with the library's
message. There is no Python or CPU implementation of the solve behind it.
"""
from __future__ import annotations

import ctypes
import os
from typing import Optional, Sequence, Tuple

import numpy as np

from .provenance import check_build_id

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "lib", "libopenr_spf.so")

USE_LINK_METRIC = 1
EMIT_TIGHT = 2
EMIT_ORDER = 4
EMIT_LEVELS8 = 8
EMIT_LEVELS16 = 16
STATUS_LEVEL_OVERFLOW = 1

OK, EIO, ENOMEM, ENODEV, EINVAL, E2BIG, ENOTSUP = 0, -5, -12, -19, -22, -7, -95

# Exported symbols of include/openr_spf.h (checked by tests/test_capi_symbols.py).
EXPORTS = (
    "openr_spf_abi_version",
    "openr_spf_build_id",
    "openr_spf_last_error",
    "openr_spf_last_kernels",
    "openr_spf_limits",
    "openr_spf_create",
    "openr_spf_destroy",
    "openr_spf_set_graph",
    "openr_spf_nh_bytes",
    "openr_spf_neighbor_map",
    "openr_spf_solve",
    "openr_spf_solve_order",
    "openr_spf_solve_ignore",
    "openr_spf_solve_device",
    "openr_spf_whatif",
    "openr_spf_whatif_device",
    "openr_spf_whatif_delta",
    "openr_spf_whatif_delta_device",
    "openr_spf_whatif_sets",
    "openr_spf_whatif_sets_device",
    "openr_spf_whatif_sets_delta",
    "openr_spf_whatif_sets_delta_device",
    "openr_spf_routes",
    "openr_spf_routes_device",
    "openr_spf_whatif_routes",
    "openr_spf_whatif_routes_device",
    "openr_spf_lfa_routes",
    "openr_spf_lfa_routes_device",
    "openr_spf_whatif_lfa",
    "openr_spf_whatif_lfa_device",
    "openr_spf_whatif_drain",
    "openr_spf_whatif_drain_device",
    "openr_spf_whatif_drain_routes",
    "openr_spf_whatif_drain_routes_device",
    "openr_spf_whatif_drain_lfa",
    "openr_spf_whatif_drain_lfa_device",
    "openr_spf_whatif_metric",
    "openr_spf_whatif_metric_device",
    "openr_spf_whatif_metric_routes",
    "openr_spf_whatif_metric_routes_device",
    "openr_spf_whatif_metric_lfa",
    "openr_spf_whatif_metric_lfa_device",
    "openr_spf_whatif_restore",
    "openr_spf_whatif_restore_device",
    "openr_spf_whatif_restore_routes",
    "openr_spf_whatif_restore_routes_device",
    "openr_spf_whatif_restore_lfa",
    "openr_spf_whatif_restore_lfa_device",
    "openr_spf_whatif_maint",
    "openr_spf_whatif_maint_device",
    "openr_spf_whatif_maint_routes",
    "openr_spf_whatif_maint_routes_device",
    "openr_spf_whatif_maint_lfa",
    "openr_spf_whatif_maint_lfa_device",
    "openr_spf_ksp2",
    "openr_spf_ksp2_device",
    "openr_spf_host_alloc",
    "openr_spf_host_free",
    "openr_spf_patch_graph",
    "openr_spf_refresh",
    "openr_spf_refresh_device",
    "openr_spf_get_stats",
    "openr_spf_take_status",
    "openr_spf_last_derived",
)


class SpfError(RuntimeError):
    def __init__(self, code: int, msg: str) -> None:
        super().__init__(f"openr_spf error {code}: {msg}")
        self.code = code


class SpfGraph(ctypes.Structure):
    _fields_ = [
        ("num_nodes", ctypes.c_uint32),
        ("num_dir_edges", ctypes.c_uint32),
        ("num_links", ctypes.c_uint32),
        ("row_ptr", ctypes.POINTER(ctypes.c_uint32)),
        ("col", ctypes.POINTER(ctypes.c_uint32)),
        ("metric", ctypes.POINTER(ctypes.c_uint64)),
        ("link_id", ctypes.POINTER(ctypes.c_uint32)),
        ("edge_up", ctypes.POINTER(ctypes.c_uint8)),
        ("node_overloaded", ctypes.POINTER(ctypes.c_uint8)),
        ("name_rank", ctypes.POINTER(ctypes.c_uint32)),
    ]


class SpfPatch(ctypes.Structure):
    _fields_ = [
        ("n_edges", ctypes.c_uint32),
        ("edge_ids", ctypes.c_void_p),
        ("metric", ctypes.c_void_p),
        ("n_links", ctypes.c_uint32),
        ("link_ids", ctypes.c_void_p),
        ("link_up", ctypes.c_void_p),
        ("n_nodes", ctypes.c_uint32),
        ("node_ids", ctypes.c_void_p),
        ("node_overloaded", ctypes.c_void_p),
    ]


class WhatifDelta(ctypes.Structure):  # openr_spf_whatif_delta_t
    _fields_ = [
        ("ptr", ctypes.c_void_p),
        ("node", ctypes.c_void_p),
        ("dist", ctypes.c_void_p),
        ("nh", ctypes.c_void_p),
        ("cap", ctypes.c_uint64),
        ("nh_bytes", ctypes.c_uint32),
    ]


class SpfGroups(ctypes.Structure):  # openr_spf_groups_t
    _fields_ = [
        ("n_groups", ctypes.c_uint32),
        ("group_ptr", ctypes.c_void_p),
        ("group_nodes", ctypes.c_void_p),
    ]


class WhatifRoutes(ctypes.Structure):  # openr_spf_whatif_routes_t
    _fields_ = [
        ("ptr", ctypes.c_void_p),
        ("group", ctypes.c_void_p),
        ("metric", ctypes.c_void_p),
        ("nh", ctypes.c_void_p),
        ("n_best", ctypes.c_void_p),
        ("cap", ctypes.c_uint64),
        ("nh_bytes", ctypes.c_uint32),
    ]


class LfaEntries(ctypes.Structure):  # openr_spf_lfa_entries_t
    _fields_ = [
        ("ptr", ctypes.c_void_p),
        ("nbr", ctypes.c_void_p),
        ("metric", ctypes.c_void_p),
        ("cap", ctypes.c_uint64),
    ]


class WhatifLfa(ctypes.Structure):  # openr_spf_whatif_lfa_t
    _fields_ = [
        ("ptr", ctypes.c_void_p),
        ("group", ctypes.c_void_p),
        ("metric", ctypes.c_void_p),
        ("nh", ctypes.c_void_p),
        ("alt", ctypes.c_void_p),
        ("cap", ctypes.c_uint64),
        ("nh_bytes", ctypes.c_uint32),
    ]


class DrainEvents(ctypes.Structure):  # openr_spf_drain_events_t
    _fields_ = [
        ("n_events", ctypes.c_uint32),
        ("node_ptr", ctypes.c_void_p),
        ("nodes", ctypes.c_void_p),
        ("link_ptr", ctypes.c_void_p),
        ("links", ctypes.c_void_p),
    ]


class MetricEvents(ctypes.Structure):  # openr_spf_metric_events_t
    _fields_ = [
        ("n_events", ctypes.c_uint32),
        ("edge_ptr", ctypes.c_void_p),
        ("edges", ctypes.c_void_p),
        ("metrics", ctypes.c_void_p),
    ]


class RestoreEvents(ctypes.Structure):  # openr_spf_restore_events_t
    _fields_ = [
        ("n_events", ctypes.c_uint32),
        ("node_ptr", ctypes.c_void_p),
        ("nodes", ctypes.c_void_p),
        ("link_ptr", ctypes.c_void_p),
        ("links", ctypes.c_void_p),
        ("edge_ptr", ctypes.c_void_p),
        ("edges", ctypes.c_void_p),
        ("metrics", ctypes.c_void_p),
    ]


class MaintEvents(ctypes.Structure):  # openr_spf_maint_events_t
    _fields_ = list(RestoreEvents._fields_)


class SpfLimits(ctypes.Structure):
    _fields_ = [("max_nodes", ctypes.c_uint32), ("max_nh_bits", ctypes.c_uint32)]


class SpfStats(ctypes.Structure):
    _fields_ = [
        ("spf_runs", ctypes.c_uint64),
        ("batches", ctypes.c_uint64),
        ("last_batch_ms", ctypes.c_double),
        ("last_kernel_ms", ctypes.c_double),
    ]


_lib = None


def load_library():
    """Load libopenr_spf.so; raises if it has not been built (no fallback)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise ImportError(
            f"{LIB_PATH} is missing: build the HIP engine first (python -c 'import __graft_entry__ as g; g.build()')"
        )
    l = ctypes.CDLL(LIB_PATH)
    vp, u32, P = ctypes.c_void_p, ctypes.c_uint32, ctypes.POINTER
    l.openr_spf_abi_version.restype = ctypes.c_int
    l.openr_spf_build_id.restype = ctypes.c_char_p
    check_build_id(l.openr_spf_build_id().decode(), LIB_PATH)
    l.openr_spf_last_error.restype = ctypes.c_char_p
    l.openr_spf_last_kernels.restype = ctypes.c_char_p
    l.openr_spf_limits.argtypes = [P(SpfLimits)]
    l.openr_spf_limits.restype = None
    l.openr_spf_create.argtypes = [vp, ctypes.c_int, P(vp)]
    l.openr_spf_destroy.argtypes = [vp]
    l.openr_spf_destroy.restype = None
    l.openr_spf_set_graph.argtypes = [vp, P(SpfGraph)]
    l.openr_spf_nh_bytes.argtypes = [vp, P(u32)]
    l.openr_spf_neighbor_map.argtypes = [vp, u32, vp, u32, P(u32)]
    l.openr_spf_solve.argtypes = [vp, vp, u32, u32, vp, vp, u32, vp]
    l.openr_spf_solve_order.argtypes = [vp, vp, u32, u32, vp, vp, vp, vp, u32, vp, vp]
    l.openr_spf_solve_ignore.argtypes = [vp, vp, u32, u32, vp, vp, vp, vp, u32, vp]
    l.openr_spf_solve_device.argtypes = [vp, ctypes.c_int, vp, u32, u32, vp, vp, vp, vp, u32, vp, vp]
    l.openr_spf_whatif.argtypes = [vp, vp, u32, vp, u32, u32, vp, P(ctypes.c_uint64)]
    l.openr_spf_whatif_device.argtypes = [vp, ctypes.c_int, vp, u32, vp, u32, u32, vp, vp, P(ctypes.c_uint64)]
    l.openr_spf_whatif_delta.argtypes = [vp, vp, u32, vp, u32, u32, vp, P(WhatifDelta), P(ctypes.c_uint64)]
    l.openr_spf_whatif_delta_device.argtypes = [vp, ctypes.c_int, vp, u32, vp, u32, u32, vp, vp, vp, vp, vp,
                                                ctypes.c_uint64, u32, vp, P(ctypes.c_uint64), P(ctypes.c_uint64)]
    l.openr_spf_whatif_sets.argtypes = [vp, vp, vp, u32, vp, u32, u32, vp, P(ctypes.c_uint64)]
    l.openr_spf_whatif_sets_device.argtypes = [vp, ctypes.c_int, vp, vp, u32, u32, vp, u32, u32, vp, vp,
                                               P(ctypes.c_uint64)]
    l.openr_spf_whatif_sets_delta.argtypes = [vp, vp, vp, u32, vp, u32, u32, vp, P(WhatifDelta), P(ctypes.c_uint64)]
    l.openr_spf_whatif_sets_delta_device.argtypes = [vp, ctypes.c_int, vp, vp, u32, u32, vp, u32, u32, vp, vp, vp, vp,
                                                     vp, ctypes.c_uint64, u32, vp, P(ctypes.c_uint64),
                                                     P(ctypes.c_uint64)]
    l.openr_spf_routes.argtypes = [vp, vp, u32, u32, P(SpfGroups), vp, vp, u32, vp]
    l.openr_spf_routes_device.argtypes = [vp, ctypes.c_int, vp, u32, u32, vp, vp, u32, u32, vp, vp, u32, vp, vp]
    l.openr_spf_whatif_routes.argtypes = [vp, vp, vp, u32, vp, u32, u32, P(SpfGroups), vp, P(WhatifRoutes),
                                          P(ctypes.c_uint64)]
    l.openr_spf_whatif_routes_device.argtypes = [vp, ctypes.c_int, vp, vp, u32, u32, vp, u32, u32, vp, vp, u32, u32,
                                                 vp, vp, vp, vp, vp, vp, ctypes.c_uint64, u32, vp,
                                                 P(ctypes.c_uint64), P(ctypes.c_uint64)]
    l.openr_spf_lfa_routes.argtypes = [vp, vp, u32, u32, P(SpfGroups), vp, vp, vp, u32, vp, P(LfaEntries),
                                       P(ctypes.c_uint64)]
    l.openr_spf_lfa_routes_device.argtypes = [vp, ctypes.c_int, vp, u32, u32, vp, vp, u32, u32, vp, vp, vp, u32, vp,
                                              vp, vp, vp, ctypes.c_uint64, vp, P(ctypes.c_uint64),
                                              P(ctypes.c_uint64)]
    l.openr_spf_whatif_lfa.argtypes = [vp, vp, vp, u32, vp, u32, u32, P(SpfGroups), vp, vp, vp, P(WhatifLfa),
                                       P(ctypes.c_uint64)]
    l.openr_spf_whatif_lfa_device.argtypes = [vp, ctypes.c_int, vp, vp, u32, u32, vp, u32, u32, vp, vp, u32, u32,
                                              vp, vp, vp, vp, vp, vp, vp, vp, ctypes.c_uint64, u32, vp,
                                              P(ctypes.c_uint64), P(ctypes.c_uint64)]
    l.openr_spf_whatif_drain.argtypes = [vp, P(DrainEvents), vp, u32, u32, vp, P(WhatifDelta), P(ctypes.c_uint64)]
    l.openr_spf_whatif_drain_device.argtypes = [vp, ctypes.c_int, vp, vp, vp, vp, u32, u32, u32, vp, u32, u32, vp, vp,
                                                vp, vp, vp, ctypes.c_uint64, u32, vp, P(ctypes.c_uint64),
                                                P(ctypes.c_uint64)]
    l.openr_spf_whatif_drain_routes.argtypes = [vp, P(DrainEvents), vp, u32, u32, P(SpfGroups), vp, P(WhatifRoutes),
                                                P(ctypes.c_uint64)]
    l.openr_spf_whatif_drain_routes_device.argtypes = [vp, ctypes.c_int, vp, vp, vp, vp, u32, u32, u32, vp, u32, u32,
                                                       vp, vp, u32, u32, vp, vp, vp, vp, vp, vp, ctypes.c_uint64,
                                                       u32, vp, P(ctypes.c_uint64), P(ctypes.c_uint64)]
    l.openr_spf_whatif_metric.argtypes = [vp, P(MetricEvents), vp, u32, u32, vp, P(WhatifDelta), P(ctypes.c_uint64)]
    l.openr_spf_whatif_metric_device.argtypes = [vp, ctypes.c_int, vp, vp, vp, u32, u32, vp, u32, u32, vp, vp, vp, vp,
                                                 vp, ctypes.c_uint64, u32, vp, P(ctypes.c_uint64),
                                                 P(ctypes.c_uint64)]
    l.openr_spf_whatif_metric_routes.argtypes = [vp, P(MetricEvents), vp, u32, u32, P(SpfGroups), vp, P(WhatifRoutes),
                                                 P(ctypes.c_uint64)]
    l.openr_spf_whatif_metric_routes_device.argtypes = [vp, ctypes.c_int, vp, vp, vp, u32, u32, vp, u32, u32, vp, vp,
                                                        u32, u32, vp, vp, vp, vp, vp, vp, ctypes.c_uint64, u32, vp,
                                                        P(ctypes.c_uint64), P(ctypes.c_uint64)]
    l.openr_spf_whatif_restore.argtypes = [vp, P(RestoreEvents), vp, u32, u32, vp, P(WhatifDelta), P(ctypes.c_uint64)]
    l.openr_spf_whatif_restore_device.argtypes = [vp, ctypes.c_int, vp, vp, vp, vp, vp, vp, vp, u32, u32, u32, u32, vp,
                                                  u32, u32, vp, vp, vp, vp, vp, ctypes.c_uint64, u32, vp,
                                                  P(ctypes.c_uint64), P(ctypes.c_uint64)]
    l.openr_spf_whatif_restore_routes.argtypes = [vp, P(RestoreEvents), vp, u32, u32, P(SpfGroups), vp,
                                                  P(WhatifRoutes), P(ctypes.c_uint64)]
    l.openr_spf_whatif_restore_routes_device.argtypes = [vp, ctypes.c_int, vp, vp, vp, vp, vp, vp, vp, u32, u32, u32,
                                                         u32, vp, u32, u32, vp, vp, u32, u32, vp, vp, vp, vp, vp, vp,
                                                         ctypes.c_uint64, u32, vp, P(ctypes.c_uint64),
                                                         P(ctypes.c_uint64)]
    l.openr_spf_whatif_maint.argtypes = [vp, P(MaintEvents)] + l.openr_spf_whatif_restore.argtypes[2:]
    l.openr_spf_whatif_maint_device.argtypes = l.openr_spf_whatif_restore_device.argtypes
    l.openr_spf_whatif_maint_routes.argtypes = [vp, P(MaintEvents)] + l.openr_spf_whatif_restore_routes.argtypes[2:]
    l.openr_spf_whatif_maint_routes_device.argtypes = l.openr_spf_whatif_restore_routes_device.argtypes
    # event arguments as the family's _routes[_device] call, then those of whatif_lfa[_device]
    lfa_host = [vp, u32, u32, P(SpfGroups), vp, vp, vp, P(WhatifLfa), P(ctypes.c_uint64)]
    lfa_dev = [vp, u32, u32, vp, vp, u32, u32, vp, vp, vp, vp, vp, vp, vp, vp, ctypes.c_uint64, u32, vp,
               P(ctypes.c_uint64), P(ctypes.c_uint64)]
    l.openr_spf_whatif_drain_lfa.argtypes = [vp, P(DrainEvents)] + lfa_host
    l.openr_spf_whatif_drain_lfa_device.argtypes = [vp, ctypes.c_int, vp, vp, vp, vp, u32, u32, u32] + lfa_dev
    l.openr_spf_whatif_metric_lfa.argtypes = [vp, P(MetricEvents)] + lfa_host
    l.openr_spf_whatif_metric_lfa_device.argtypes = [vp, ctypes.c_int, vp, vp, vp, u32, u32] + lfa_dev
    l.openr_spf_whatif_restore_lfa.argtypes = [vp, P(RestoreEvents)] + lfa_host
    l.openr_spf_whatif_restore_lfa_device.argtypes = [vp, ctypes.c_int, vp, vp, vp, vp, vp, vp, vp, u32, u32, u32,
                                                      u32] + lfa_dev
    l.openr_spf_whatif_maint_lfa.argtypes = [vp, P(MaintEvents)] + lfa_host
    l.openr_spf_whatif_maint_lfa_device.argtypes = l.openr_spf_whatif_restore_lfa_device.argtypes
    l.openr_spf_ksp2.argtypes = [vp, vp, vp, u32, u32, vp, vp]
    l.openr_spf_ksp2_device.argtypes = [vp, ctypes.c_int, vp, u32, vp, vp, u32, u32, vp, vp, vp]
    l.openr_spf_host_alloc.argtypes = [ctypes.c_size_t, P(vp)]
    l.openr_spf_host_free.argtypes = [vp]
    l.openr_spf_host_free.restype = None
    l.openr_spf_patch_graph.argtypes = [vp, P(SpfPatch)]
    l.openr_spf_refresh.argtypes = [vp, vp, u32, u32, vp, vp, u32, vp, P(u32)]
    l.openr_spf_refresh_device.argtypes = [vp, ctypes.c_int, vp, u32, u32, vp, vp, u32, vp, vp, P(u32)]
    l.openr_spf_get_stats.argtypes = [vp, P(SpfStats)]
    l.openr_spf_take_status.argtypes = [vp, ctypes.c_int, P(u32)]
    l.openr_spf_last_derived.argtypes = [vp, ctypes.c_int, P(u32)]
    for name in EXPORTS:
        if name not in ("openr_spf_last_error", "openr_spf_last_kernels", "openr_spf_limits", "openr_spf_destroy",
                        "openr_spf_build_id", "openr_spf_host_free"):
            getattr(l, name).restype = ctypes.c_int
    _lib = l
    return l


def _check(rc: int) -> None:
    if rc != OK:
        msg = _lib.openr_spf_last_error()
        raise SpfError(rc, msg.decode() if msg else "")


def _p(a: Optional[np.ndarray]):
    return None if a is None else ctypes.c_void_p(a.ctypes.data)


def _ignore_arrays(ignore: Sequence[Sequence[int]], n: int) -> Tuple[np.ndarray, np.ndarray]:
    """Per-solve ignore sets -> (ignore_ptr[n+1], ignore_links) CSR arrays."""
    ptr = np.zeros(n + 1, dtype=np.uint32)
    ptr[1:] = np.cumsum([len(x) for x in ignore])
    links = np.ascontiguousarray(np.concatenate([np.asarray(x, dtype=np.uint32) for x in ignore])
                                 if ptr[-1] else np.zeros(1, dtype=np.uint32), dtype=np.uint32)
    return ptr, links


class SpfEngine:
    """One engine context (= one LinkState's device-side SPF backend)."""

    def __init__(self, device_ids: Optional[Sequence[int]] = None) -> None:
        self._lib = load_library()
        self._ctx = ctypes.c_void_p()
        if device_ids:
            ids = (ctypes.c_int * len(device_ids))(*device_ids)
            rc = self._lib.openr_spf_create(ctypes.cast(ids, ctypes.c_void_p), len(device_ids), ctypes.byref(self._ctx))
        else:
            rc = self._lib.openr_spf_create(None, 0, ctypes.byref(self._ctx))
        _check(rc)
        self.g = None
        self._gs = None
        self.nh_bytes = 1

    def close(self) -> None:
        if self._ctx:
            self._lib.openr_spf_destroy(self._ctx)
            self._ctx = ctypes.c_void_p()

    def __del__(self) -> None:  # pragma: no cover - best effort
        try:
            self.close()
        except Exception:
            pass

    def set_graph(self, g) -> None:
        self._gs = g.ctypes_struct(SpfGraph)
        _check(self._lib.openr_spf_set_graph(self._ctx, ctypes.byref(self._gs)))
        self.g = g
        nb = ctypes.c_uint32()
        _check(self._lib.openr_spf_nh_bytes(self._ctx, ctypes.byref(nb)))
        self.nh_bytes = int(nb.value)

    def neighbor_map(self, src: int) -> np.ndarray:
        n = ctypes.c_uint32()
        _check(self._lib.openr_spf_neighbor_map(self._ctx, src, None, 0, ctypes.byref(n)))
        out = np.zeros(max(int(n.value), 1), dtype=np.uint32)
        _check(self._lib.openr_spf_neighbor_map(self._ctx, src, _p(out), out.shape[0], ctypes.byref(n)))
        return out[: int(n.value)]

    def solve(self, sources: Sequence[int], use_link_metric: bool = True, want_nh: bool = True,
              want_tight: bool = False, ignore: Optional[Sequence[Sequence[int]]] = None,
              nh_bytes: Optional[int] = None) -> Tuple[np.ndarray, Optional[np.ndarray], Optional[np.ndarray]]:
        """Batched SPF. Returns (dist[n,V] u64, nh[n,V,nh_bytes] u8 | None, tight[n,ceil(E/64)] u64 | None)."""
        g = self.g
        src = np.ascontiguousarray(sources, dtype=np.uint32)
        n, V = int(src.shape[0]), g.num_nodes
        nb = self.nh_bytes if nh_bytes is None else nh_bytes
        dist = np.empty((n, V), dtype=np.uint64)
        nh = np.empty((n, V, nb), dtype=np.uint8) if want_nh else None
        tw = (g.num_dir_edges + 63) // 64
        tight = np.empty((n, max(tw, 1)), dtype=np.uint64) if want_tight else None
        flags = (USE_LINK_METRIC if use_link_metric else 0) | (EMIT_TIGHT if want_tight else 0)
        if ignore is None:
            rc = self._lib.openr_spf_solve(self._ctx, _p(src), n, flags, _p(dist), _p(nh), nb, _p(tight))
        else:
            ptr, links = _ignore_arrays(ignore, n)
            rc = self._lib.openr_spf_solve_ignore(self._ctx, _p(src), n, flags, _p(ptr), _p(links), _p(dist),
                                                  _p(nh), nb, _p(tight))
        _check(rc)
        return dist, nh, tight

    def solve_order(self, sources: Sequence[int], use_link_metric: bool = True, want_tight: bool = True,
                    ignore: Optional[Sequence[Sequence[int]]] = None
                    ) -> Tuple[np.ndarray, np.ndarray, Optional[np.ndarray], np.ndarray]:
        """Exact-order solve: (dist, nh, tight | None, order[n,V] u32 pop index, UINT32_MAX unreached)."""
        g = self.g
        src = np.ascontiguousarray(sources, dtype=np.uint32)
        n, V = int(src.shape[0]), g.num_nodes
        dist = np.empty((n, V), dtype=np.uint64)
        nh = np.empty((n, V, self.nh_bytes), dtype=np.uint8)
        tw = (g.num_dir_edges + 63) // 64
        tight = np.empty((n, max(tw, 1)), dtype=np.uint64) if want_tight else None
        order = np.empty((n, V), dtype=np.uint32)
        flags = (USE_LINK_METRIC if use_link_metric else 0) | (EMIT_TIGHT if want_tight else 0)
        ptr, links = _ignore_arrays(ignore, n) if ignore is not None else (None, None)
        _check(self._lib.openr_spf_solve_order(self._ctx, _p(src), n, flags, _p(ptr), _p(links), _p(dist), _p(nh),
                                               self.nh_bytes, _p(tight), _p(order)))
        return dist, nh, tight, order

    def solve_device(self, d_sources: int, n: int, d_dist: int, d_nh: int = 0, nh_bytes: int = 0,
                     use_link_metric: bool = True, stream: int = 0, device_index: int = 0,
                     d_ignore_ptr: int = 0, d_ignore_links: int = 0, d_tight: int = 0, level_bytes: int = 0) -> None:
        """Device-pointer form (ints are raw device addresses, e.g. torch data_ptr()).
        level_bytes = 1 / 2: d_dist receives u8 / u16 level rows instead of u64 distances
        (OPENR_SPF_EMIT_LEVELS8 / 16: uniform-cost graphs on the level BFS family)."""
        flags = (USE_LINK_METRIC if use_link_metric else 0) | (EMIT_TIGHT if d_tight else 0)
        if level_bytes:
            flags |= {1: EMIT_LEVELS8, 2: EMIT_LEVELS16}[level_bytes]
        vp = ctypes.c_void_p
        _check(self._lib.openr_spf_solve_device(self._ctx, device_index, vp(d_sources), n, flags,
                                                vp(d_ignore_ptr or None), vp(d_ignore_links or None), vp(d_dist),
                                                vp(d_nh or None), nh_bytes or self.nh_bytes, vp(d_tight or None),
                                                vp(stream or None)))

    def take_status(self, device_index: int = 0) -> int:
        """OPENR_SPF_STATUS_* bits raised by device-form calls since the last take (waits
        for the device)."""
        st = ctypes.c_uint32()
        _check(self._lib.openr_spf_take_status(self._ctx, device_index, ctypes.byref(st)))
        return int(st.value)

    def last_derived(self, device_index: int = 0) -> int:
        """Rows of the device's last solve call that were derived from their neighbours'
        rows instead of solved (0: the batch was not split; waits for the device)."""
        n = ctypes.c_uint32()
        _check(self._lib.openr_spf_last_derived(self._ctx, device_index, ctypes.byref(n)))
        return int(n.value)

    def whatif(self, links: Sequence[int], sources: Sequence[int], use_link_metric: bool = True
               ) -> Tuple[np.ndarray, int]:
        """Per-link-failure sweep: (changed[n_links, n_sources] u32, SPFs run)."""
        lk = np.ascontiguousarray(links, dtype=np.uint32)
        src = np.ascontiguousarray(sources, dtype=np.uint32)
        changed = np.zeros((lk.shape[0], src.shape[0]), dtype=np.uint32)
        solved = ctypes.c_uint64()
        flags = USE_LINK_METRIC if use_link_metric else 0
        _check(self._lib.openr_spf_whatif(self._ctx, _p(lk), lk.shape[0], _p(src), src.shape[0], flags,
                                          _p(changed), ctypes.byref(solved)))
        return changed, int(solved.value)

    def whatif_device(self, d_links: int, n_links: int, d_sources: int, n_sources: int, d_changed: int,
                      use_link_metric: bool = True, stream: int = 0, device_index: int = 0) -> int:
        """Device-pointer form; returns the number of SPFs run."""
        vp = ctypes.c_void_p
        solved = ctypes.c_uint64()
        flags = USE_LINK_METRIC if use_link_metric else 0
        _check(self._lib.openr_spf_whatif_device(self._ctx, device_index, vp(d_links), n_links, vp(d_sources),
                                                 n_sources, flags, vp(d_changed), vp(stream or None),
                                                 ctypes.byref(solved)))
        return int(solved.value)

    def whatif_delta(self, links: Sequence[int], sources: Sequence[int], use_link_metric: bool = True,
                     cap: Optional[int] = None, nh_bytes: Optional[int] = None):
        """Per-link-failure sweep with each unit's delta (openr_spf_whatif_delta):
        (changed[n_links, n_sources] u32, ptr[n_units + 1] u64, node u32, dist u64,
        nh[entries, nh_bytes] u8, SPFs run). Unit u = i * n_sources + j owns entries
        [ptr[u], ptr[u + 1]), node ids ascending. cap None: sized from a count-only pass."""
        lk = np.ascontiguousarray(links, dtype=np.uint32)
        src = np.ascontiguousarray(sources, dtype=np.uint32)
        nb = nh_bytes if nh_bytes is not None else self.nh_bytes
        if cap is None:
            changed, _ = self.whatif(lk, src, use_link_metric)
            cap = int(changed.sum(dtype=np.uint64))
        changed = np.zeros((lk.shape[0], src.shape[0]), dtype=np.uint32)
        ptr = np.zeros(lk.shape[0] * src.shape[0] + 1, dtype=np.uint64)
        node = np.zeros(max(cap, 1), dtype=np.uint32)
        dist = np.zeros(max(cap, 1), dtype=np.uint64)
        nh = np.zeros((max(cap, 1), nb), dtype=np.uint8)
        d = WhatifDelta(_p(ptr), _p(node), _p(dist), _p(nh), cap, nb)
        solved = ctypes.c_uint64()
        flags = USE_LINK_METRIC if use_link_metric else 0
        _check(self._lib.openr_spf_whatif_delta(self._ctx, _p(lk), lk.shape[0], _p(src), src.shape[0], flags,
                                                _p(changed), ctypes.byref(d), ctypes.byref(solved)))
        n = int(ptr[-1])
        return changed, ptr, node[:n], dist[:n], nh[:n], int(solved.value)

    def whatif_delta_device(self, d_links: int, n_links: int, d_sources: int, n_sources: int, d_changed: int,
                            d_ptr: int, d_node: int, d_dist: int, d_nh: int, cap: int, nh_bytes: int,
                            use_link_metric: bool = True, stream: int = 0, device_index: int = 0,
                            allow_overflow: bool = False) -> Tuple[int, int]:
        """Device-pointer form: (total entries, SPFs run). d_ptr [n_units + 1] u64 CSR; unit
        u's entries are [ptr[u], ptr[u + 1]) in the repair's order."""
        vp = ctypes.c_void_p
        total = ctypes.c_uint64()
        solved = ctypes.c_uint64()
        flags = USE_LINK_METRIC if use_link_metric else 0
        rc = self._lib.openr_spf_whatif_delta_device(self._ctx, device_index, vp(d_links), n_links, vp(d_sources),
                                                     n_sources, flags, vp(d_changed), vp(d_ptr), vp(d_node or None),
                                                     vp(d_dist or None), vp(d_nh or None), cap, nh_bytes,
                                                     vp(stream or None), ctypes.byref(total), ctypes.byref(solved))
        if not (allow_overflow and rc == E2BIG):
            _check(rc)
        return int(total.value), int(solved.value)

    def whatif_sets(self, sets: Sequence[Sequence[int]], sources: Sequence[int], use_link_metric: bool = True
                    ) -> Tuple[np.ndarray, int]:
        """Link-set failure sweep (node failures, shared-risk groups; openr_spf_whatif_sets):
        (changed[n_sets, n_sources] u32, SPFs run). Unit (i, j) fails every link of sets[i]."""
        n = len(sets)
        sp, sl = _ignore_arrays(sets, n)
        src = np.ascontiguousarray(sources, dtype=np.uint32)
        changed = np.zeros((n, src.shape[0]), dtype=np.uint32)
        solved = ctypes.c_uint64()
        flags = USE_LINK_METRIC if use_link_metric else 0
        _check(self._lib.openr_spf_whatif_sets(self._ctx, _p(sp), _p(sl), n, _p(src), src.shape[0], flags,
                                               _p(changed), ctypes.byref(solved)))
        return changed, int(solved.value)

    def whatif_sets_device(self, d_set_ptr: int, d_set_links: int, n_sets: int, n_set_links: int, d_sources: int,
                           n_sources: int, d_changed: int, use_link_metric: bool = True, stream: int = 0,
                           device_index: int = 0) -> int:
        """Device-pointer form (d_set_ptr [n_sets + 1], d_set_links [n_set_links]); returns
        the number of SPFs run."""
        vp = ctypes.c_void_p
        solved = ctypes.c_uint64()
        flags = USE_LINK_METRIC if use_link_metric else 0
        _check(self._lib.openr_spf_whatif_sets_device(self._ctx, device_index, vp(d_set_ptr or None),
                                                      vp(d_set_links or None), n_sets, n_set_links, vp(d_sources),
                                                      n_sources, flags, vp(d_changed), vp(stream or None),
                                                      ctypes.byref(solved)))
        return int(solved.value)

    def whatif_sets_delta(self, sets: Sequence[Sequence[int]], sources: Sequence[int], use_link_metric: bool = True,
                          cap: Optional[int] = None, nh_bytes: Optional[int] = None):
        """Link-set failure sweep with each unit's delta (openr_spf_whatif_sets_delta): the
        return shape of whatif_delta, unit u = i * n_sources + j failing every link of sets[i].
        cap None: sized from a count-only pass."""
        n = len(sets)
        sp, sl = _ignore_arrays(sets, n)
        src = np.ascontiguousarray(sources, dtype=np.uint32)
        nb = nh_bytes if nh_bytes is not None else self.nh_bytes
        if cap is None:
            changed, _ = self.whatif_sets(sets, src, use_link_metric)
            cap = int(changed.sum(dtype=np.uint64))
        changed = np.zeros((n, src.shape[0]), dtype=np.uint32)
        ptr = np.zeros(n * src.shape[0] + 1, dtype=np.uint64)
        node = np.zeros(max(cap, 1), dtype=np.uint32)
        dist = np.zeros(max(cap, 1), dtype=np.uint64)
        nh = np.zeros((max(cap, 1), nb), dtype=np.uint8)
        d = WhatifDelta(_p(ptr), _p(node), _p(dist), _p(nh), cap, nb)
        solved = ctypes.c_uint64()
        flags = USE_LINK_METRIC if use_link_metric else 0
        _check(self._lib.openr_spf_whatif_sets_delta(self._ctx, _p(sp), _p(sl), n, _p(src), src.shape[0], flags,
                                                     _p(changed), ctypes.byref(d), ctypes.byref(solved)))
        k = int(ptr[-1])
        return changed, ptr, node[:k], dist[:k], nh[:k], int(solved.value)

    def whatif_sets_delta_device(self, d_set_ptr: int, d_set_links: int, n_sets: int, n_set_links: int,
                                 d_sources: int, n_sources: int, d_changed: int, d_ptr: int, d_node: int,
                                 d_dist: int, d_nh: int, cap: int, nh_bytes: int, use_link_metric: bool = True,
                                 stream: int = 0, device_index: int = 0,
                                 allow_overflow: bool = False) -> Tuple[int, int]:
        """Device-pointer form: (total entries, SPFs run). d_ptr [n_units + 1] u64 CSR; unit
        u's entries are [ptr[u], ptr[u + 1]) in the re-solve's order."""
        vp = ctypes.c_void_p
        total = ctypes.c_uint64()
        solved = ctypes.c_uint64()
        flags = USE_LINK_METRIC if use_link_metric else 0
        rc = self._lib.openr_spf_whatif_sets_delta_device(
            self._ctx, device_index, vp(d_set_ptr or None), vp(d_set_links or None), n_sets, n_set_links,
            vp(d_sources), n_sources, flags, vp(d_changed), vp(d_ptr), vp(d_node or None), vp(d_dist or None),
            vp(d_nh or None), cap, nh_bytes, vp(stream or None), ctypes.byref(total), ctypes.byref(solved))
        if not (allow_overflow and rc == E2BIG):
            _check(rc)
        return int(total.value), int(solved.value)

    def routes(self, sources: Sequence[int], groups: Sequence[Sequence[int]], use_link_metric: bool = True,
               want_nh: bool = True, want_n_best: bool = True, nh_bytes: Optional[int] = None):
        """Best-path selection over prefix groups (openr_spf_routes): (metric[n, G] u64,
        nh[n, G, nh_bytes] u8 | None, n_best[n, G] u32 | None). Group k's route at a source is
        the minimum distance over its members and the OR of their next-hop sets at that
        minimum. ``groups``: node-id lists, strictly ascending (topology.prefix_groups)."""
        gp, gn = _ignore_arrays(groups, len(groups))
        src = np.ascontiguousarray(sources, dtype=np.uint32)
        n, G = int(src.shape[0]), len(groups)
        nb = self.nh_bytes if nh_bytes is None else nh_bytes
        metric = np.zeros((n, G), dtype=np.uint64)
        nh = np.zeros((n, G, nb), dtype=np.uint8) if want_nh else None
        n_best = np.zeros((n, G), dtype=np.uint32) if want_n_best else None
        gs = SpfGroups(G, _p(gp), _p(gn))
        flags = USE_LINK_METRIC if use_link_metric else 0
        _check(self._lib.openr_spf_routes(self._ctx, _p(src), n, flags, ctypes.byref(gs), _p(metric), _p(nh), nb,
                                          _p(n_best)))
        return metric, nh, n_best

    def routes_device(self, d_sources: int, n: int, d_group_ptr: int, d_group_nodes: int, n_groups: int,
                      n_group_nodes: int, d_metric: int, d_nh: int = 0, nh_bytes: int = 0, d_n_best: int = 0,
                      use_link_metric: bool = True, stream: int = 0, device_index: int = 0) -> None:
        """Device-pointer form (openr_spf_routes_device): enqueues on ``stream``."""
        vp = ctypes.c_void_p
        flags = USE_LINK_METRIC if use_link_metric else 0
        _check(self._lib.openr_spf_routes_device(self._ctx, device_index, vp(d_sources), n, flags,
                                                 vp(d_group_ptr or None), vp(d_group_nodes or None), n_groups,
                                                 n_group_nodes, vp(d_metric), vp(d_nh or None),
                                                 nh_bytes or self.nh_bytes, vp(d_n_best or None), vp(stream or None)))

    def whatif_routes(self, sets: Sequence[Sequence[int]], sources: Sequence[int], groups: Sequence[Sequence[int]],
                      use_link_metric: bool = True, cap: Optional[int] = None, nh_bytes: Optional[int] = None):
        """Route-level link-set failure sweep (openr_spf_whatif_routes): (changed_routes[n_sets,
        n_sources] u32, ptr[n_units + 1] u64, group u32, metric u64, nh[entries, nh_bytes] u8,
        n_best u32, SPFs run). Unit u = i * n_sources + j owns entries [ptr[u], ptr[u + 1]):
        the groups whose route (metric or next hops) the failure of sets[i] changes at
        sources[j], group ids ascending, with the new route. cap None: sized from a
        count-only pass."""
        n = len(sets)
        sp, sl = _ignore_arrays(sets, n)
        gp, gn = _ignore_arrays(groups, len(groups))
        gs = SpfGroups(len(groups), _p(gp), _p(gn))
        src = np.ascontiguousarray(sources, dtype=np.uint32)
        nb = nh_bytes if nh_bytes is not None else self.nh_bytes
        flags = USE_LINK_METRIC if use_link_metric else 0
        changed = np.zeros((n, src.shape[0]), dtype=np.uint32)
        solved = ctypes.c_uint64()
        if cap is None:
            _check(self._lib.openr_spf_whatif_routes(self._ctx, _p(sp), _p(sl), n, _p(src), src.shape[0], flags,
                                                     ctypes.byref(gs), _p(changed), None, ctypes.byref(solved)))
            cap = int(changed.sum(dtype=np.uint64))
        ptr = np.zeros(n * src.shape[0] + 1, dtype=np.uint64)
        group = np.zeros(max(cap, 1), dtype=np.uint32)
        metric = np.zeros(max(cap, 1), dtype=np.uint64)
        nh = np.zeros((max(cap, 1), nb), dtype=np.uint8)
        n_best = np.zeros(max(cap, 1), dtype=np.uint32)
        d = WhatifRoutes(_p(ptr), _p(group), _p(metric), _p(nh), _p(n_best), cap, nb)
        _check(self._lib.openr_spf_whatif_routes(self._ctx, _p(sp), _p(sl), n, _p(src), src.shape[0], flags,
                                                 ctypes.byref(gs), _p(changed), ctypes.byref(d),
                                                 ctypes.byref(solved)))
        k = int(ptr[-1])
        return changed, ptr, group[:k], metric[:k], nh[:k], n_best[:k], int(solved.value)

    def whatif_routes_device(self, d_set_ptr: int, d_set_links: int, n_sets: int, n_set_links: int, d_sources: int,
                             n_sources: int, d_group_ptr: int, d_group_nodes: int, n_groups: int,
                             n_group_nodes: int, d_changed: int, d_ptr: int, d_group: int, d_metric: int, d_nh: int,
                             d_n_best: int, cap: int, nh_bytes: int, use_link_metric: bool = True, stream: int = 0,
                             device_index: int = 0, allow_overflow: bool = False) -> Tuple[int, int]:
        """Device-pointer form: (total entries, SPFs run). d_ptr [n_units + 1] u64 CSR; unit
        u's entries are [ptr[u], ptr[u + 1]) in the kernel's order."""
        vp = ctypes.c_void_p
        total = ctypes.c_uint64()
        solved = ctypes.c_uint64()
        flags = USE_LINK_METRIC if use_link_metric else 0
        rc = self._lib.openr_spf_whatif_routes_device(
            self._ctx, device_index, vp(d_set_ptr or None), vp(d_set_links or None), n_sets, n_set_links,
            vp(d_sources), n_sources, flags, vp(d_group_ptr or None), vp(d_group_nodes or None), n_groups,
            n_group_nodes, vp(d_changed), vp(d_ptr), vp(d_group or None), vp(d_metric or None), vp(d_nh or None),
            vp(d_n_best or None), cap, nh_bytes, vp(stream or None), ctypes.byref(total), ctypes.byref(solved))
        if not (allow_overflow and rc == E2BIG):
            _check(rc)
        return int(total.value), int(solved.value)

    def lfa_routes(self, sources: Sequence[int], groups: Sequence[Sequence[int]], use_link_metric: bool = True,
                   want_entries: bool = True, cap: Optional[int] = None, nh_bytes: Optional[int] = None):
        """Routes with their loop-free alternates (openr_spf_lfa_routes): (metric[n, G] u64,
        nh[n, G, nh_bytes] u8, alt[n, G, nh_bytes] u8, n_alt[n, G] u32, ptr[n * G + 1] u64 | None,
        nbr u32 | None, alt_metric u64 | None, rows solved). metric / nh are the routes of
        ``routes``; bit b of alt is set iff the source's b-th distinct neighbour (an up link to
        it) is a loop-free alternate for the group: some member d has dist_n(d) < metric +
        dist_n(source). Unit u = i * G + k owns entries [ptr[u], ptr[u + 1]): the set bits of alt
        ascending, each with the distance the reference keeps for that next hop. cap None:
        sized from a counts-only call."""
        gp, gn = _ignore_arrays(groups, len(groups))
        gs = SpfGroups(len(groups), _p(gp), _p(gn))
        src = np.ascontiguousarray(sources, dtype=np.uint32)
        n, G = int(src.shape[0]), len(groups)
        nb = self.nh_bytes if nh_bytes is None else nh_bytes
        flags = USE_LINK_METRIC if use_link_metric else 0
        metric = np.zeros((n, G), dtype=np.uint64)
        nh = np.zeros((n, G, nb), dtype=np.uint8)
        alt = np.zeros((n, G, nb), dtype=np.uint8)
        n_alt = np.zeros((n, G), dtype=np.uint32)
        solved = ctypes.c_uint64()

        def call(ent):
            return self._lib.openr_spf_lfa_routes(self._ctx, _p(src), n, flags, ctypes.byref(gs), _p(metric), _p(nh),
                                                  _p(alt), nb, _p(n_alt), ent, ctypes.byref(solved))

        if not want_entries:
            _check(call(None))
            return metric, nh, alt, n_alt, None, None, None, int(solved.value)
        if cap is None:
            _check(call(None))
            cap = int(n_alt.sum(dtype=np.uint64))
        ptr = np.zeros(n * G + 1, dtype=np.uint64)
        nbr = np.zeros(max(cap, 1), dtype=np.uint32)
        am = np.zeros(max(cap, 1), dtype=np.uint64)
        ent = LfaEntries(_p(ptr), _p(nbr), _p(am), cap)
        _check(call(ctypes.byref(ent)))
        k = int(ptr[-1])
        return metric, nh, alt, n_alt, ptr, nbr[:k], am[:k], int(solved.value)

    def lfa_routes_device(self, d_sources: int, n: int, d_group_ptr: int, d_group_nodes: int, n_groups: int,
                          n_group_nodes: int, d_metric: int, d_nh: int = 0, d_alt: int = 0, nh_bytes: int = 0,
                          d_n_alt: int = 0, d_ptr: int = 0, d_nbr: int = 0, d_alt_metric: int = 0, cap: int = 0,
                          use_link_metric: bool = True, stream: int = 0, device_index: int = 0,
                          allow_overflow: bool = False) -> Tuple[int, int]:
        """Device-pointer form (openr_spf_lfa_routes_device): (total entries, rows solved).
        d_ptr 0: no entry output. Synchronizes ``stream`` (see the header)."""
        vp = ctypes.c_void_p
        total = ctypes.c_uint64()
        solved = ctypes.c_uint64()
        flags = USE_LINK_METRIC if use_link_metric else 0
        rc = self._lib.openr_spf_lfa_routes_device(
            self._ctx, device_index, vp(d_sources), n, flags, vp(d_group_ptr or None), vp(d_group_nodes or None),
            n_groups, n_group_nodes, vp(d_metric), vp(d_nh or None), vp(d_alt or None), nh_bytes or self.nh_bytes,
            vp(d_n_alt or None), vp(d_ptr or None), vp(d_nbr or None), vp(d_alt_metric or None), cap,
            vp(stream or None), ctypes.byref(total), ctypes.byref(solved))
        if not (allow_overflow and rc == E2BIG):
            _check(rc)
        return int(total.value), int(solved.value)

    def whatif_lfa(self, sets: Sequence[Sequence[int]], sources: Sequence[int], groups: Sequence[Sequence[int]],
                   use_link_metric: bool = True, nh_bytes: Optional[int] = None, cap: Optional[int] = None,
                   want_counts: bool = True):
        """Post-failure loop-free alternates (openr_spf_whatif_lfa): (changed[n_sets, n_sources]
        u32, ptr[n_units + 1] u64, group u32, metric u64, nh[entries, nh_bytes] u8, alt[entries,
        nh_bytes] u8, unprotected[n_sets, n_sources] u32 | None, lost_backup[...] u32 | None, SPFs
        run). Unit u = i * n_sources + j owns entries [ptr[u], ptr[u + 1]): the groups whose LFA
        RIB entry (metric, nh or alt) the failure of sets[i] changes at sources[j], group ids
        ascending, with the new entry. unprotected counts the groups left live with a single next
        hop in nh | alt, lost_backup those that had two or more before (want_counts False: both
        None). cap None: sized from a counts-only call."""
        n = len(sets)
        sp, sl = _ignore_arrays(sets, n)
        gp, gn = _ignore_arrays(groups, len(groups))
        gs = SpfGroups(len(groups), _p(gp), _p(gn))
        src = np.ascontiguousarray(sources, dtype=np.uint32)
        nb = nh_bytes if nh_bytes is not None else self.nh_bytes
        flags = USE_LINK_METRIC if use_link_metric else 0
        changed = np.zeros((n, src.shape[0]), dtype=np.uint32)
        unprot = np.zeros((n, src.shape[0]), dtype=np.uint32) if want_counts else None
        lost = np.zeros((n, src.shape[0]), dtype=np.uint32) if want_counts else None
        solved = ctypes.c_uint64()

        def call(d):
            return self._lib.openr_spf_whatif_lfa(self._ctx, _p(sp), _p(sl), n, _p(src), src.shape[0], flags,
                                                  ctypes.byref(gs), _p(changed), _p(unprot), _p(lost), d,
                                                  ctypes.byref(solved))

        if cap is None:
            _check(call(None))
            cap = int(changed.sum(dtype=np.uint64))
        ptr = np.zeros(n * src.shape[0] + 1, dtype=np.uint64)
        group = np.zeros(max(cap, 1), dtype=np.uint32)
        metric = np.zeros(max(cap, 1), dtype=np.uint64)
        nh = np.zeros((max(cap, 1), max(nb, 1)), dtype=np.uint8)
        alt = np.zeros((max(cap, 1), max(nb, 1)), dtype=np.uint8)
        d = WhatifLfa(_p(ptr), _p(group), _p(metric), _p(nh), _p(alt), cap, nb)
        _check(call(ctypes.byref(d)))
        k = int(ptr[-1])
        return changed, ptr, group[:k], metric[:k], nh[:k], alt[:k], unprot, lost, int(solved.value)

    def whatif_lfa_device(self, d_set_ptr: int, d_set_links: int, n_sets: int, n_set_links: int, d_sources: int,
                          n_sources: int, d_group_ptr: int, d_group_nodes: int, n_groups: int, n_group_nodes: int,
                          d_changed: int, d_unprotected: int = 0, d_lost_backup: int = 0, d_ptr: int = 0,
                          d_group: int = 0, d_metric: int = 0, d_nh: int = 0, d_alt: int = 0, cap: int = 0,
                          nh_bytes: int = 0, use_link_metric: bool = True, stream: int = 0, device_index: int = 0,
                          allow_overflow: bool = False) -> Tuple[int, int]:
        """Device-pointer form (openr_spf_whatif_lfa_device): (total entries, SPFs run). d_ptr 0:
        counts only; else d_ptr [n_units + 1] u64 CSR, unit u's entries in the kernel's order.
        Synchronizes ``stream``."""
        vp = ctypes.c_void_p
        total = ctypes.c_uint64()
        solved = ctypes.c_uint64()
        flags = USE_LINK_METRIC if use_link_metric else 0
        rc = self._lib.openr_spf_whatif_lfa_device(
            self._ctx, device_index, vp(d_set_ptr or None), vp(d_set_links or None), n_sets, n_set_links,
            vp(d_sources or None), n_sources, flags, vp(d_group_ptr or None), vp(d_group_nodes or None), n_groups,
            n_group_nodes, vp(d_changed or None), vp(d_unprotected or None), vp(d_lost_backup or None),
            vp(d_ptr or None), vp(d_group or None), vp(d_metric or None), vp(d_nh or None), vp(d_alt or None), cap,
            nh_bytes or self.nh_bytes, vp(stream or None), ctypes.byref(total), ctypes.byref(solved))
        if not (allow_overflow and rc == E2BIG):
            _check(rc)
        return int(total.value), int(solved.value)

    # ---- the event sweeps: one body per call form; a family gives its C function and its events ----
    def _event_sweep(self, fn, ev, n: int, sources, use_link_metric, want_delta, cap, nh_bytes):
        """The host call ``fn`` over the events ``ev`` (n of them): the tuple whatif_sets_delta
        returns, or (changed, solved) with want_delta False. cap None: sized from a count-only pass."""
        src = np.ascontiguousarray(sources, dtype=np.uint32)
        flags = USE_LINK_METRIC if use_link_metric else 0
        changed = np.zeros((n, src.shape[0]), dtype=np.uint32)
        solved = ctypes.c_uint64()

        def call(d):
            return fn(self._ctx, ctypes.byref(ev), _p(src), src.shape[0], flags, _p(changed), d, ctypes.byref(solved))

        if not want_delta or cap is None:
            _check(call(None))
            if not want_delta:
                return changed, int(solved.value)
            cap = int(changed.sum(dtype=np.uint64))
        nb = nh_bytes if nh_bytes is not None else self.nh_bytes
        ptr = np.zeros(n * src.shape[0] + 1, dtype=np.uint64)
        node = np.zeros(max(cap, 1), dtype=np.uint32)
        dist = np.zeros(max(cap, 1), dtype=np.uint64)
        nh = np.zeros((max(cap, 1), nb), dtype=np.uint8)
        d = WhatifDelta(_p(ptr), _p(node), _p(dist), _p(nh), cap, nb)
        _check(call(ctypes.byref(d)))
        k = int(ptr[-1])
        return changed, ptr, node[:k], dist[:k], nh[:k], int(solved.value)

    def _event_routes(self, fn, ev, n: int, sources, groups, use_link_metric, cap, nh_bytes):
        """The host call ``fn`` over the events ``ev`` (n of them): the tuple whatif_routes returns."""
        gp, gn = _ignore_arrays(groups, len(groups))
        gs = SpfGroups(len(groups), _p(gp), _p(gn))
        src = np.ascontiguousarray(sources, dtype=np.uint32)
        nb = nh_bytes if nh_bytes is not None else self.nh_bytes
        flags = USE_LINK_METRIC if use_link_metric else 0
        changed = np.zeros((n, src.shape[0]), dtype=np.uint32)
        solved = ctypes.c_uint64()

        def call(d):
            return fn(self._ctx, ctypes.byref(ev), _p(src), src.shape[0], flags, ctypes.byref(gs), _p(changed), d,
                      ctypes.byref(solved))

        if cap is None:
            _check(call(None))
            cap = int(changed.sum(dtype=np.uint64))
        ptr = np.zeros(n * src.shape[0] + 1, dtype=np.uint64)
        group = np.zeros(max(cap, 1), dtype=np.uint32)
        metric = np.zeros(max(cap, 1), dtype=np.uint64)
        nh = np.zeros((max(cap, 1), nb), dtype=np.uint8)
        n_best = np.zeros(max(cap, 1), dtype=np.uint32)
        d = WhatifRoutes(_p(ptr), _p(group), _p(metric), _p(nh), _p(n_best), cap, nb)
        _check(call(ctypes.byref(d)))
        k = int(ptr[-1])
        return changed, ptr, group[:k], metric[:k], nh[:k], n_best[:k], int(solved.value)

    def _event_device(self, fn, event_args, d_sources, n_sources, d_changed, d_ptr, d_node, d_dist, d_nh, cap,
                      nh_bytes, use_link_metric, stream, device_index, allow_overflow) -> Tuple[int, int]:
        vp = ctypes.c_void_p
        total = ctypes.c_uint64()
        solved = ctypes.c_uint64()
        flags = USE_LINK_METRIC if use_link_metric else 0
        rc = fn(self._ctx, device_index, *event_args, vp(d_sources), n_sources, flags, vp(d_changed), vp(d_ptr),
                vp(d_node or None), vp(d_dist or None), vp(d_nh or None), cap, nh_bytes, vp(stream or None),
                ctypes.byref(total), ctypes.byref(solved))
        if not (allow_overflow and rc == E2BIG):
            _check(rc)
        return int(total.value), int(solved.value)

    def _event_routes_device(self, fn, event_args, d_sources, n_sources, d_group_ptr, d_group_nodes, n_groups,
                             n_group_nodes, d_changed, d_ptr, d_group, d_metric, d_nh, d_n_best, cap, nh_bytes,
                             use_link_metric, stream, device_index, allow_overflow) -> Tuple[int, int]:
        vp = ctypes.c_void_p
        total = ctypes.c_uint64()
        solved = ctypes.c_uint64()
        flags = USE_LINK_METRIC if use_link_metric else 0
        rc = fn(self._ctx, device_index, *event_args, vp(d_sources), n_sources, flags, vp(d_group_ptr or None),
                vp(d_group_nodes or None), n_groups, n_group_nodes, vp(d_changed), vp(d_ptr), vp(d_group or None),
                vp(d_metric or None), vp(d_nh or None), vp(d_n_best or None), cap, nh_bytes, vp(stream or None),
                ctypes.byref(total), ctypes.byref(solved))
        if not (allow_overflow and rc == E2BIG):
            _check(rc)
        return int(total.value), int(solved.value)

    @staticmethod
    def _device_events(addresses, *counts):
        """The leading event arguments of a device form: the CSR addresses (0: NULL), then the counts."""
        return tuple(ctypes.c_void_p(a or None) for a in addresses) + counts

    @staticmethod
    def _drain_events(node_sets: Sequence[Sequence[int]], link_sets: Optional[Sequence[Sequence[int]]]):
        """(DrainEvents, the arrays it points into) of per-event node and link lists."""
        n = len(node_sets)
        if link_sets is not None and len(link_sets) != n:
            raise ValueError("node_sets and link_sets differ in length")
        np_, nn = _ignore_arrays(node_sets, n)
        lp, ll = _ignore_arrays(link_sets, n) if link_sets is not None else (None, None)
        return DrainEvents(n, _p(np_), _p(nn), _p(lp), _p(ll)), (np_, nn, lp, ll)

    def whatif_drain(self, node_sets: Sequence[Sequence[int]], sources: Sequence[int],
                     link_sets: Optional[Sequence[Sequence[int]]] = None, use_link_metric: bool = True,
                     want_delta: bool = True, cap: Optional[int] = None, nh_bytes: Optional[int] = None):
        """Drain sweep (openr_spf_whatif_drain): event i overloads the nodes of node_sets[i] and
        takes the links of link_sets[i] out of service; unit u = i * n_sources + j. Returns the
        shape of whatif_sets_delta: (changed[n_events, n_sources] u32, ptr, node, dist, nh,
        solved), or (changed, solved) with want_delta=False. cap None: sized from a count-only
        pass."""
        ev, keep = self._drain_events(node_sets, link_sets)
        out = self._event_sweep(self._lib.openr_spf_whatif_drain, ev, len(node_sets), sources, use_link_metric,
                              want_delta, cap, nh_bytes)
        del keep
        return out

    def whatif_drain_device(self, d_node_ptr: int, d_nodes: int, d_link_ptr: int, d_links: int, n_events: int,
                            n_nodes: int, n_links: int, d_sources: int, n_sources: int, d_changed: int, d_ptr: int,
                            d_node: int, d_dist: int, d_nh: int, cap: int, nh_bytes: int,
                            use_link_metric: bool = True, stream: int = 0, device_index: int = 0,
                            allow_overflow: bool = False) -> Tuple[int, int]:
        """Device-pointer form: (total entries, solved). d_link_ptr 0: no links. d_ptr
        [n_units + 1] u64 CSR; unit u's entries are [ptr[u], ptr[u + 1]) in the kernel's order."""
        ev = self._device_events((d_node_ptr, d_nodes, d_link_ptr, d_links), n_events, n_nodes, n_links)
        return self._event_device(self._lib.openr_spf_whatif_drain_device, ev, d_sources, n_sources, d_changed, d_ptr,
                                  d_node, d_dist, d_nh, cap, nh_bytes, use_link_metric, stream, device_index,
                                  allow_overflow)

    def whatif_drain_routes(self, node_sets: Sequence[Sequence[int]], sources: Sequence[int],
                            groups: Sequence[Sequence[int]], link_sets: Optional[Sequence[Sequence[int]]] = None,
                            use_link_metric: bool = True, cap: Optional[int] = None,
                            nh_bytes: Optional[int] = None):
        """The drain sweep resolved to routes (openr_spf_whatif_drain_routes): the return shape
        of whatif_routes. cap None: sized from a count-only pass."""
        ev, keep = self._drain_events(node_sets, link_sets)
        out = self._event_routes(self._lib.openr_spf_whatif_drain_routes, ev, len(node_sets), sources, groups,
                               use_link_metric, cap, nh_bytes)
        del keep
        return out

    def whatif_drain_routes_device(self, d_node_ptr: int, d_nodes: int, d_link_ptr: int, d_links: int, n_events: int,
                                   n_nodes: int, n_links: int, d_sources: int, n_sources: int, d_group_ptr: int,
                                   d_group_nodes: int, n_groups: int, n_group_nodes: int, d_changed: int, d_ptr: int,
                                   d_group: int, d_metric: int, d_nh: int, d_n_best: int, cap: int, nh_bytes: int,
                                   use_link_metric: bool = True, stream: int = 0, device_index: int = 0,
                                   allow_overflow: bool = False) -> Tuple[int, int]:
        """Device-pointer form: (total entries, solved); outputs as whatif_routes_device."""
        ev = self._device_events((d_node_ptr, d_nodes, d_link_ptr, d_links), n_events, n_nodes, n_links)
        return self._event_routes_device(self._lib.openr_spf_whatif_drain_routes_device, ev, d_sources, n_sources,
                                         d_group_ptr, d_group_nodes, n_groups, n_group_nodes, d_changed, d_ptr,
                                         d_group, d_metric, d_nh, d_n_best, cap, nh_bytes, use_link_metric, stream,
                                         device_index, allow_overflow)

    @staticmethod
    def _metric_events(edge_sets: Sequence[Sequence[int]], metric_sets: Sequence[Sequence[int]]):
        """(MetricEvents, the arrays it points into) of per-event edge and new-metric lists (as
        given: topology.metric_events sorts and merges them)."""
        n = len(edge_sets)
        if len(metric_sets) != n or any(len(e) != len(m) for e, m in zip(edge_sets, metric_sets)):
            raise ValueError("edge_sets and metric_sets differ in length")
        ep, ee = _ignore_arrays(edge_sets, n)
        _, mm = _ignore_arrays(metric_sets, n)
        return MetricEvents(n, _p(ep), _p(ee), _p(mm)), (ep, ee, mm)

    def whatif_metric(self, edge_sets: Sequence[Sequence[int]], metric_sets: Sequence[Sequence[int]],
                      sources: Sequence[int], want_delta: bool = True, use_link_metric: bool = True,
                      cap: Optional[int] = None, nh_bytes: Optional[int] = None):
        """Metric sweep (openr_spf_whatif_metric): event i gives the directed edge edge_sets[i][k]
        the metric metric_sets[i][k] (raises only, edge ids strictly ascending: see
        topology.metric_events / soft_drain_events); unit u = i * n_sources + j. Returns the
        shape of whatif_drain: (changed[n_events, n_sources] u32, ptr, node, dist, nh, solved),
        or (changed, solved) with want_delta=False. cap None: sized from a count-only pass."""
        ev, keep = self._metric_events(edge_sets, metric_sets)
        out = self._event_sweep(self._lib.openr_spf_whatif_metric, ev, len(edge_sets), sources, use_link_metric,
                              want_delta, cap, nh_bytes)
        del keep
        return out

    def whatif_metric_device(self, d_edge_ptr: int, d_edges: int, d_metrics: int, n_events: int, n_edges: int,
                             d_sources: int, n_sources: int, d_changed: int, d_ptr: int, d_node: int, d_dist: int,
                             d_nh: int, cap: int, nh_bytes: int, use_link_metric: bool = True, stream: int = 0,
                             device_index: int = 0, allow_overflow: bool = False) -> Tuple[int, int]:
        """Device-pointer form: (total entries, solved). d_ptr [n_units + 1] u64 CSR; unit u's
        entries are [ptr[u], ptr[u + 1]) in the kernel's order."""
        ev = self._device_events((d_edge_ptr, d_edges, d_metrics), n_events, n_edges)
        return self._event_device(self._lib.openr_spf_whatif_metric_device, ev, d_sources, n_sources, d_changed,
                                  d_ptr, d_node, d_dist, d_nh, cap, nh_bytes, use_link_metric, stream, device_index,
                                  allow_overflow)

    def whatif_metric_routes(self, edge_sets: Sequence[Sequence[int]], metric_sets: Sequence[Sequence[int]],
                             sources: Sequence[int], groups: Sequence[Sequence[int]], use_link_metric: bool = True,
                             cap: Optional[int] = None, nh_bytes: Optional[int] = None):
        """The metric sweep resolved to routes (openr_spf_whatif_metric_routes): the return shape
        of whatif_routes. cap None: sized from a count-only pass."""
        ev, keep = self._metric_events(edge_sets, metric_sets)
        out = self._event_routes(self._lib.openr_spf_whatif_metric_routes, ev, len(edge_sets), sources, groups,
                               use_link_metric, cap, nh_bytes)
        del keep
        return out

    def whatif_metric_routes_device(self, d_edge_ptr: int, d_edges: int, d_metrics: int, n_events: int, n_edges: int,
                                    d_sources: int, n_sources: int, d_group_ptr: int, d_group_nodes: int,
                                    n_groups: int, n_group_nodes: int, d_changed: int, d_ptr: int, d_group: int,
                                    d_metric: int, d_nh: int, d_n_best: int, cap: int, nh_bytes: int,
                                    use_link_metric: bool = True, stream: int = 0, device_index: int = 0,
                                    allow_overflow: bool = False) -> Tuple[int, int]:
        """Device-pointer form: (total entries, solved); outputs as whatif_routes_device."""
        ev = self._device_events((d_edge_ptr, d_edges, d_metrics), n_events, n_edges)
        return self._event_routes_device(self._lib.openr_spf_whatif_metric_routes_device, ev, d_sources, n_sources,
                                         d_group_ptr, d_group_nodes, n_groups, n_group_nodes, d_changed, d_ptr,
                                         d_group, d_metric, d_nh, d_n_best, cap, nh_bytes, use_link_metric, stream,
                                         device_index, allow_overflow)

    @staticmethod
    def _restore_events(node_sets, link_sets, edge_sets, metric_sets, struct=RestoreEvents):
        """(RestoreEvents, the arrays it points into) of per-event node, link, edge and
        new-metric lists (as given: topology.restore_events sorts and merges them). None for
        a kind: no entry of it in any event. struct=MaintEvents: the same lists as a
        maintenance event (topology.maint_events)."""
        if (edge_sets is None) != (metric_sets is None):
            raise ValueError("edge_sets and metric_sets go together")
        counts = {len(x) for x in (node_sets, link_sets, edge_sets, metric_sets) if x is not None}
        if len(counts) > 1:
            raise ValueError("node_sets, link_sets, edge_sets and metric_sets differ in length")
        n = counts.pop() if counts else 0
        if edge_sets is not None and any(len(e) != len(m) for e, m in zip(edge_sets, metric_sets)):
            raise ValueError("edge_sets and metric_sets differ in length")
        np_, nn = _ignore_arrays(node_sets if node_sets is not None else [[]] * n, n)
        lp, ll = _ignore_arrays(link_sets, n) if link_sets is not None else (None, None)
        ep, ee = _ignore_arrays(edge_sets, n) if edge_sets is not None else (None, None)
        mm = _ignore_arrays(metric_sets, n)[1] if metric_sets is not None else None
        keep = (np_, nn, lp, ll, ep, ee, mm)
        return struct(n, *(_p(a) for a in keep)), keep, n

    def whatif_restore(self, node_sets: Optional[Sequence[Sequence[int]]], link_sets: Optional[Sequence[Sequence[int]]],
                       edge_sets: Optional[Sequence[Sequence[int]]], metric_sets: Optional[Sequence[Sequence[int]]],
                       sources: Sequence[int], use_link_metric: bool = True, want_delta: bool = True,
                       cap: Optional[int] = None, nh_bytes: Optional[int] = None):
        """Restore sweep (openr_spf_whatif_restore): event i clears the overload bit of the nodes
        of node_sets[i], puts the links of link_sets[i] back in service and gives the directed
        edge edge_sets[i][k] the lower metric metric_sets[i][k] (see topology.restore_events);
        None for a kind: none of it. Unit u = i * n_sources + j. Returns the shape of
        whatif_metric: (changed[n_events, n_sources] u32, ptr, node, dist, nh, solved), or
        (changed, solved) with want_delta=False. cap None: sized from a count-only pass."""
        ev, keep, n = self._restore_events(node_sets, link_sets, edge_sets, metric_sets)
        out = self._event_sweep(self._lib.openr_spf_whatif_restore, ev, n, sources, use_link_metric, want_delta, cap,
                              nh_bytes)
        del keep
        return out

    def whatif_restore_device(self, d_node_ptr: int, d_nodes: int, d_link_ptr: int, d_links: int, d_edge_ptr: int,
                              d_edges: int, d_metrics: int, n_events: int, n_nodes: int, n_links: int, n_edges: int,
                              d_sources: int, n_sources: int, d_changed: int, d_ptr: int, d_node: int, d_dist: int,
                              d_nh: int, cap: int, nh_bytes: int, use_link_metric: bool = True, stream: int = 0,
                              device_index: int = 0, allow_overflow: bool = False) -> Tuple[int, int]:
        """Device-pointer form: (total entries, solved). d_link_ptr / d_edge_ptr 0: no links /
        no metric entries. d_ptr [n_units + 1] u64 CSR; unit u's entries are [ptr[u],
        ptr[u + 1]) in the kernel's order."""
        ev = self._device_events((d_node_ptr, d_nodes, d_link_ptr, d_links, d_edge_ptr, d_edges, d_metrics), n_events,
                                 n_nodes, n_links, n_edges)
        return self._event_device(self._lib.openr_spf_whatif_restore_device, ev, d_sources, n_sources, d_changed,
                                  d_ptr, d_node, d_dist, d_nh, cap, nh_bytes, use_link_metric, stream, device_index,
                                  allow_overflow)

    def whatif_restore_routes(self, node_sets: Optional[Sequence[Sequence[int]]],
                              link_sets: Optional[Sequence[Sequence[int]]],
                              edge_sets: Optional[Sequence[Sequence[int]]],
                              metric_sets: Optional[Sequence[Sequence[int]]], sources: Sequence[int],
                              groups: Sequence[Sequence[int]], use_link_metric: bool = True,
                              cap: Optional[int] = None, nh_bytes: Optional[int] = None):
        """The restore sweep resolved to routes (openr_spf_whatif_restore_routes): the return
        shape of whatif_routes. cap None: sized from a count-only pass."""
        ev, keep, n = self._restore_events(node_sets, link_sets, edge_sets, metric_sets)
        out = self._event_routes(self._lib.openr_spf_whatif_restore_routes, ev, n, sources, groups, use_link_metric,
                               cap, nh_bytes)
        del keep
        return out

    def whatif_restore_routes_device(self, d_node_ptr: int, d_nodes: int, d_link_ptr: int, d_links: int,
                                     d_edge_ptr: int, d_edges: int, d_metrics: int, n_events: int, n_nodes: int,
                                     n_links: int, n_edges: int, d_sources: int, n_sources: int, d_group_ptr: int,
                                     d_group_nodes: int, n_groups: int, n_group_nodes: int, d_changed: int,
                                     d_ptr: int, d_group: int, d_metric: int, d_nh: int, d_n_best: int, cap: int,
                                     nh_bytes: int, use_link_metric: bool = True, stream: int = 0,
                                     device_index: int = 0, allow_overflow: bool = False) -> Tuple[int, int]:
        """Device-pointer form: (total entries, solved); outputs as whatif_routes_device."""
        ev = self._device_events((d_node_ptr, d_nodes, d_link_ptr, d_links, d_edge_ptr, d_edges, d_metrics), n_events,
                                 n_nodes, n_links, n_edges)
        return self._event_routes_device(self._lib.openr_spf_whatif_restore_routes_device, ev, d_sources, n_sources,
                                         d_group_ptr, d_group_nodes, n_groups, n_group_nodes, d_changed, d_ptr,
                                         d_group, d_metric, d_nh, d_n_best, cap, nh_bytes, use_link_metric, stream,
                                         device_index, allow_overflow)

    # ---- maintenance events: overloads, link-downs and metric raises together ---------------
    def whatif_maint(self, node_sets: Optional[Sequence[Sequence[int]]], link_sets: Optional[Sequence[Sequence[int]]],
                     edge_sets: Optional[Sequence[Sequence[int]]], metric_sets: Optional[Sequence[Sequence[int]]],
                     sources: Sequence[int], use_link_metric: bool = True, want_delta: bool = True,
                     cap: Optional[int] = None, nh_bytes: Optional[int] = None):
        """Maintenance sweep (openr_spf_whatif_maint): event i overloads the nodes of
        node_sets[i], takes the links of link_sets[i] out of service and gives the directed
        edge edge_sets[i][k] the higher metric metric_sets[i][k] (see topology.maint_events);
        None for a kind: none of it. Unit u = i * n_sources + j. Returns the shape of
        whatif_metric: (changed[n_events, n_sources] u32, ptr, node, dist, nh, solved), or
        (changed, solved) with want_delta=False. cap None: sized from a count-only pass."""
        ev, keep, n = self._restore_events(node_sets, link_sets, edge_sets, metric_sets, MaintEvents)
        out = self._event_sweep(self._lib.openr_spf_whatif_maint, ev, n, sources, use_link_metric, want_delta, cap,
                              nh_bytes)
        del keep
        return out

    def whatif_maint_device(self, d_node_ptr: int, d_nodes: int, d_link_ptr: int, d_links: int, d_edge_ptr: int,
                            d_edges: int, d_metrics: int, n_events: int, n_nodes: int, n_links: int, n_edges: int,
                            d_sources: int, n_sources: int, d_changed: int, d_ptr: int, d_node: int, d_dist: int,
                            d_nh: int, cap: int, nh_bytes: int, use_link_metric: bool = True, stream: int = 0,
                            device_index: int = 0, allow_overflow: bool = False) -> Tuple[int, int]:
        """Device-pointer form: (total entries, solved). d_link_ptr / d_edge_ptr 0: no links /
        no metric entries. d_ptr [n_units + 1] u64 CSR; unit u's entries are [ptr[u],
        ptr[u + 1]) in the kernel's order."""
        ev = self._device_events((d_node_ptr, d_nodes, d_link_ptr, d_links, d_edge_ptr, d_edges, d_metrics), n_events,
                                 n_nodes, n_links, n_edges)
        return self._event_device(self._lib.openr_spf_whatif_maint_device, ev, d_sources, n_sources, d_changed, d_ptr,
                                  d_node, d_dist, d_nh, cap, nh_bytes, use_link_metric, stream, device_index,
                                  allow_overflow)

    def whatif_maint_routes(self, node_sets: Optional[Sequence[Sequence[int]]],
                            link_sets: Optional[Sequence[Sequence[int]]],
                            edge_sets: Optional[Sequence[Sequence[int]]],
                            metric_sets: Optional[Sequence[Sequence[int]]], sources: Sequence[int],
                            groups: Sequence[Sequence[int]], use_link_metric: bool = True,
                            cap: Optional[int] = None, nh_bytes: Optional[int] = None):
        """The maintenance sweep resolved to routes (openr_spf_whatif_maint_routes): the return
        shape of whatif_routes. cap None: sized from a count-only pass."""
        ev, keep, n = self._restore_events(node_sets, link_sets, edge_sets, metric_sets, MaintEvents)
        out = self._event_routes(self._lib.openr_spf_whatif_maint_routes, ev, n, sources, groups, use_link_metric,
                               cap, nh_bytes)
        del keep
        return out

    def whatif_maint_routes_device(self, d_node_ptr: int, d_nodes: int, d_link_ptr: int, d_links: int,
                                   d_edge_ptr: int, d_edges: int, d_metrics: int, n_events: int, n_nodes: int,
                                   n_links: int, n_edges: int, d_sources: int, n_sources: int, d_group_ptr: int,
                                   d_group_nodes: int, n_groups: int, n_group_nodes: int, d_changed: int,
                                   d_ptr: int, d_group: int, d_metric: int, d_nh: int, d_n_best: int, cap: int,
                                   nh_bytes: int, use_link_metric: bool = True, stream: int = 0,
                                   device_index: int = 0, allow_overflow: bool = False) -> Tuple[int, int]:
        """Device-pointer form: (total entries, solved); outputs as whatif_routes_device."""
        ev = self._device_events((d_node_ptr, d_nodes, d_link_ptr, d_links, d_edge_ptr, d_edges, d_metrics), n_events,
                                 n_nodes, n_links, n_edges)
        return self._event_routes_device(self._lib.openr_spf_whatif_maint_routes_device, ev, d_sources, n_sources,
                                         d_group_ptr, d_group_nodes, n_groups, n_group_nodes, d_changed, d_ptr,
                                         d_group, d_metric, d_nh, d_n_best, cap, nh_bytes, use_link_metric, stream,
                                         device_index, allow_overflow)

    # ---- loop-free alternates under drain, metric, restore and maintenance events ------------
    def _event_lfa(self, fn, ev, n: int, sources, groups, use_link_metric, nh_bytes, cap, want_counts):
        """The host call ``fn`` over the events ``ev`` (n of them): the tuple whatif_lfa returns."""
        gp, gn = _ignore_arrays(groups, len(groups))
        gs = SpfGroups(len(groups), _p(gp), _p(gn))
        src = np.ascontiguousarray(sources, dtype=np.uint32)
        nb = nh_bytes if nh_bytes is not None else self.nh_bytes
        flags = USE_LINK_METRIC if use_link_metric else 0
        changed = np.zeros((n, src.shape[0]), dtype=np.uint32)
        unprot = np.zeros((n, src.shape[0]), dtype=np.uint32) if want_counts else None
        lost = np.zeros((n, src.shape[0]), dtype=np.uint32) if want_counts else None
        solved = ctypes.c_uint64()

        def call(d):
            return fn(self._ctx, ctypes.byref(ev), _p(src), src.shape[0], flags, ctypes.byref(gs), _p(changed),
                      _p(unprot), _p(lost), d, ctypes.byref(solved))

        if cap is None:
            _check(call(None))
            cap = int(changed.sum(dtype=np.uint64))
        ptr = np.zeros(n * src.shape[0] + 1, dtype=np.uint64)
        group = np.zeros(max(cap, 1), dtype=np.uint32)
        metric = np.zeros(max(cap, 1), dtype=np.uint64)
        nh = np.zeros((max(cap, 1), max(nb, 1)), dtype=np.uint8)
        alt = np.zeros((max(cap, 1), max(nb, 1)), dtype=np.uint8)
        d = WhatifLfa(_p(ptr), _p(group), _p(metric), _p(nh), _p(alt), cap, nb)
        _check(call(ctypes.byref(d)))
        k = int(ptr[-1])
        return changed, ptr, group[:k], metric[:k], nh[:k], alt[:k], unprot, lost, int(solved.value)

    def _event_lfa_device(self, fn, event_args, d_sources, n_sources, d_group_ptr, d_group_nodes, n_groups,
                          n_group_nodes, d_changed, d_unprotected, d_lost_backup, d_ptr, d_group, d_metric, d_nh,
                          d_alt, cap, nh_bytes, use_link_metric, stream, device_index,
                          allow_overflow) -> Tuple[int, int]:
        vp = ctypes.c_void_p
        total = ctypes.c_uint64()
        solved = ctypes.c_uint64()
        flags = USE_LINK_METRIC if use_link_metric else 0
        rc = fn(self._ctx, device_index, *event_args, vp(d_sources or None), n_sources, flags,
                vp(d_group_ptr or None), vp(d_group_nodes or None), n_groups, n_group_nodes, vp(d_changed or None),
                vp(d_unprotected or None), vp(d_lost_backup or None), vp(d_ptr or None), vp(d_group or None),
                vp(d_metric or None), vp(d_nh or None), vp(d_alt or None), cap, nh_bytes or self.nh_bytes,
                vp(stream or None), ctypes.byref(total), ctypes.byref(solved))
        if not (allow_overflow and rc == E2BIG):
            _check(rc)
        return int(total.value), int(solved.value)

    def whatif_drain_lfa(self, node_sets: Sequence[Sequence[int]], sources: Sequence[int],
                         groups: Sequence[Sequence[int]], link_sets: Optional[Sequence[Sequence[int]]] = None,
                         use_link_metric: bool = True, nh_bytes: Optional[int] = None, cap: Optional[int] = None,
                         want_counts: bool = True):
        """Loop-free alternates under drain events (openr_spf_whatif_drain_lfa): the events of
        whatif_drain, the return tuple of whatif_lfa (changed, ptr, group, metric, nh, alt,
        unprotected, lost_backup, solved) over units u = i * n_sources + j. cap None: sized from a
        counts-only call."""
        ev, keep = self._drain_events(node_sets, link_sets)
        out = self._event_lfa(self._lib.openr_spf_whatif_drain_lfa, ev, len(node_sets), sources, groups,
                              use_link_metric, nh_bytes, cap, want_counts)
        del keep
        return out

    def whatif_drain_lfa_device(self, d_node_ptr: int, d_nodes: int, d_link_ptr: int, d_links: int, n_events: int,
                                n_nodes: int, n_links: int, d_sources: int, n_sources: int, d_group_ptr: int,
                                d_group_nodes: int, n_groups: int, n_group_nodes: int, d_changed: int,
                                d_unprotected: int = 0, d_lost_backup: int = 0, d_ptr: int = 0, d_group: int = 0,
                                d_metric: int = 0, d_nh: int = 0, d_alt: int = 0, cap: int = 0, nh_bytes: int = 0,
                                use_link_metric: bool = True, stream: int = 0, device_index: int = 0,
                                allow_overflow: bool = False) -> Tuple[int, int]:
        """Device-pointer form (openr_spf_whatif_drain_lfa_device): (total entries, solved);
        events as whatif_drain_device, outputs as whatif_lfa_device."""
        ev = self._device_events((d_node_ptr, d_nodes, d_link_ptr, d_links), n_events, n_nodes, n_links)
        return self._event_lfa_device(self._lib.openr_spf_whatif_drain_lfa_device, ev, d_sources, n_sources,
                                      d_group_ptr, d_group_nodes, n_groups, n_group_nodes, d_changed, d_unprotected,
                                      d_lost_backup, d_ptr, d_group, d_metric, d_nh, d_alt, cap, nh_bytes,
                                      use_link_metric, stream, device_index, allow_overflow)

    def whatif_metric_lfa(self, edge_sets: Sequence[Sequence[int]], metric_sets: Sequence[Sequence[int]],
                          sources: Sequence[int], groups: Sequence[Sequence[int]], use_link_metric: bool = True,
                          nh_bytes: Optional[int] = None, cap: Optional[int] = None, want_counts: bool = True):
        """Loop-free alternates under metric events (openr_spf_whatif_metric_lfa): the events of
        whatif_metric, the return tuple of whatif_lfa. Under hop count nothing moves: changed is
        all zero and unprotected is each source's base count."""
        ev, keep = self._metric_events(edge_sets, metric_sets)
        out = self._event_lfa(self._lib.openr_spf_whatif_metric_lfa, ev, len(edge_sets), sources, groups,
                              use_link_metric, nh_bytes, cap, want_counts)
        del keep
        return out

    def whatif_metric_lfa_device(self, d_edge_ptr: int, d_edges: int, d_metrics: int, n_events: int, n_edges: int,
                                 d_sources: int, n_sources: int, d_group_ptr: int, d_group_nodes: int,
                                 n_groups: int, n_group_nodes: int, d_changed: int, d_unprotected: int = 0,
                                 d_lost_backup: int = 0, d_ptr: int = 0, d_group: int = 0, d_metric: int = 0,
                                 d_nh: int = 0, d_alt: int = 0, cap: int = 0, nh_bytes: int = 0,
                                 use_link_metric: bool = True, stream: int = 0, device_index: int = 0,
                                 allow_overflow: bool = False) -> Tuple[int, int]:
        """Device-pointer form (openr_spf_whatif_metric_lfa_device): (total entries, solved)."""
        ev = self._device_events((d_edge_ptr, d_edges, d_metrics), n_events, n_edges)
        return self._event_lfa_device(self._lib.openr_spf_whatif_metric_lfa_device, ev, d_sources, n_sources,
                                      d_group_ptr, d_group_nodes, n_groups, n_group_nodes, d_changed, d_unprotected,
                                      d_lost_backup, d_ptr, d_group, d_metric, d_nh, d_alt, cap, nh_bytes,
                                      use_link_metric, stream, device_index, allow_overflow)

    def whatif_restore_lfa(self, node_sets: Optional[Sequence[Sequence[int]]],
                           link_sets: Optional[Sequence[Sequence[int]]],
                           edge_sets: Optional[Sequence[Sequence[int]]],
                           metric_sets: Optional[Sequence[Sequence[int]]], sources: Sequence[int],
                           groups: Sequence[Sequence[int]], use_link_metric: bool = True,
                           nh_bytes: Optional[int] = None, cap: Optional[int] = None, want_counts: bool = True):
        """Loop-free alternates under restore events (openr_spf_whatif_restore_lfa): the events
        of whatif_restore, the return tuple of whatif_lfa. A link coming up can make a neighbour
        tested that was not."""
        ev, keep, n = self._restore_events(node_sets, link_sets, edge_sets, metric_sets)
        out = self._event_lfa(self._lib.openr_spf_whatif_restore_lfa, ev, n, sources, groups, use_link_metric,
                              nh_bytes, cap, want_counts)
        del keep
        return out

    def whatif_restore_lfa_device(self, d_node_ptr: int, d_nodes: int, d_link_ptr: int, d_links: int,
                                  d_edge_ptr: int, d_edges: int, d_metrics: int, n_events: int, n_nodes: int,
                                  n_links: int, n_edges: int, d_sources: int, n_sources: int, d_group_ptr: int,
                                  d_group_nodes: int, n_groups: int, n_group_nodes: int, d_changed: int,
                                  d_unprotected: int = 0, d_lost_backup: int = 0, d_ptr: int = 0, d_group: int = 0,
                                  d_metric: int = 0, d_nh: int = 0, d_alt: int = 0, cap: int = 0,
                                  nh_bytes: int = 0, use_link_metric: bool = True, stream: int = 0,
                                  device_index: int = 0, allow_overflow: bool = False) -> Tuple[int, int]:
        """Device-pointer form (openr_spf_whatif_restore_lfa_device): (total entries, solved)."""
        ev = self._device_events((d_node_ptr, d_nodes, d_link_ptr, d_links, d_edge_ptr, d_edges, d_metrics), n_events,
                                 n_nodes, n_links, n_edges)
        return self._event_lfa_device(self._lib.openr_spf_whatif_restore_lfa_device, ev, d_sources, n_sources,
                                      d_group_ptr, d_group_nodes, n_groups, n_group_nodes, d_changed, d_unprotected,
                                      d_lost_backup, d_ptr, d_group, d_metric, d_nh, d_alt, cap, nh_bytes,
                                      use_link_metric, stream, device_index, allow_overflow)

    def whatif_maint_lfa(self, node_sets: Optional[Sequence[Sequence[int]]],
                         link_sets: Optional[Sequence[Sequence[int]]],
                         edge_sets: Optional[Sequence[Sequence[int]]],
                         metric_sets: Optional[Sequence[Sequence[int]]], sources: Sequence[int],
                         groups: Sequence[Sequence[int]], use_link_metric: bool = True,
                         nh_bytes: Optional[int] = None, cap: Optional[int] = None, want_counts: bool = True):
        """Loop-free alternates under maintenance events (openr_spf_whatif_maint_lfa): the events
        of whatif_maint (overloads, link-downs and metric raises in one event), the return tuple
        of whatif_lfa. Under hop count the raises are ignored: the answer is whatif_drain_lfa's
        for the nodes and links."""
        ev, keep, n = self._restore_events(node_sets, link_sets, edge_sets, metric_sets, MaintEvents)
        out = self._event_lfa(self._lib.openr_spf_whatif_maint_lfa, ev, n, sources, groups, use_link_metric,
                              nh_bytes, cap, want_counts)
        del keep
        return out

    def whatif_maint_lfa_device(self, d_node_ptr: int, d_nodes: int, d_link_ptr: int, d_links: int,
                                d_edge_ptr: int, d_edges: int, d_metrics: int, n_events: int, n_nodes: int,
                                n_links: int, n_edges: int, d_sources: int, n_sources: int, d_group_ptr: int,
                                d_group_nodes: int, n_groups: int, n_group_nodes: int, d_changed: int,
                                d_unprotected: int = 0, d_lost_backup: int = 0, d_ptr: int = 0, d_group: int = 0,
                                d_metric: int = 0, d_nh: int = 0, d_alt: int = 0, cap: int = 0,
                                nh_bytes: int = 0, use_link_metric: bool = True, stream: int = 0,
                                device_index: int = 0, allow_overflow: bool = False) -> Tuple[int, int]:
        """Device-pointer form (openr_spf_whatif_maint_lfa_device): (total entries, solved);
        events as whatif_maint_device, outputs as whatif_lfa_device."""
        ev = self._device_events((d_node_ptr, d_nodes, d_link_ptr, d_links, d_edge_ptr, d_edges, d_metrics), n_events,
                                 n_nodes, n_links, n_edges)
        return self._event_lfa_device(self._lib.openr_spf_whatif_maint_lfa_device, ev, d_sources, n_sources,
                                      d_group_ptr, d_group_nodes, n_groups, n_group_nodes, d_changed, d_unprotected,
                                      d_lost_backup, d_ptr, d_group, d_metric, d_nh, d_alt, cap, nh_bytes,
                                      use_link_metric, stream, device_index, allow_overflow)

    def ksp2_tokens(self, src: Sequence[int], dst: Sequence[int], tok_cap: int = 256,
                    allow_overflow: bool = False) -> Tuple[np.ndarray, np.ndarray]:
        """getKthPaths(s, d, 1) and (.., 2) per pair as raw token rows [n, tok_cap] u32."""
        s_ = np.ascontiguousarray(src, dtype=np.uint32)
        d_ = np.ascontiguousarray(dst, dtype=np.uint32)
        n = int(s_.shape[0])
        t1 = np.zeros((n, tok_cap), dtype=np.uint32)
        t2 = np.zeros((n, tok_cap), dtype=np.uint32)
        rc = self._lib.openr_spf_ksp2(self._ctx, _p(s_), _p(d_), n, tok_cap, _p(t1), _p(t2))
        if not (allow_overflow and rc == E2BIG):
            _check(rc)
        return t1, t2

    def ksp2(self, src: Sequence[int], dst: Sequence[int], tok_cap: int = 256):
        """[(paths_k1, paths_k2)] per pair; a path = list of directed edge ids, src -> dest."""
        t1, t2 = self.ksp2_tokens(src, dst, tok_cap)
        return [(decode_paths(t1[i]), decode_paths(t2[i])) for i in range(t1.shape[0])]

    def ksp2_device(self, d_sources: int, n_sources: int, d_pair_row: int, d_pair_dst: int, n_pairs: int,
                    tok_cap: int, d_tok1: int, d_tok2: int, stream: int = 0, device_index: int = 0) -> None:
        vp = ctypes.c_void_p
        _check(self._lib.openr_spf_ksp2_device(self._ctx, device_index, vp(d_sources), n_sources, vp(d_pair_row),
                                               vp(d_pair_dst), n_pairs, tok_cap, vp(d_tok1), vp(d_tok2),
                                               vp(stream or None)))

    def patch(self, edges: Sequence[int] = (), metrics: Sequence[int] = (), links: Sequence[int] = (),
              link_up: Sequence[int] = (), nodes: Sequence[int] = (), node_overloaded: Sequence[int] = (),
              track: bool = True) -> None:
        """Attribute-only mirror update (openr_spf_patch_graph); with ``track`` also applies it
        to ``self.g`` (a patched copy of the host graph)."""
        e = np.ascontiguousarray(edges, dtype=np.uint32)
        m = np.ascontiguousarray(metrics, dtype=np.uint64)
        lk = np.ascontiguousarray(links, dtype=np.uint32)
        lu = np.ascontiguousarray(link_up, dtype=np.uint8)
        nd = np.ascontiguousarray(nodes, dtype=np.uint32)
        no = np.ascontiguousarray(node_overloaded, dtype=np.uint8)
        if e.shape != m.shape or lk.shape != lu.shape or nd.shape != no.shape:
            raise ValueError("patch id / value arrays differ in length")
        p = SpfPatch(int(e.shape[0]), _p(e), _p(m), int(lk.shape[0]), _p(lk), _p(lu), int(nd.shape[0]), _p(nd),
                     _p(no))
        _check(self._lib.openr_spf_patch_graph(self._ctx, ctypes.byref(p)))
        if track:
            self.g = self.g.patched(e, m, lk, lu, nd, no)

    def refresh(self, sources: Sequence[int], dist: np.ndarray, nh: Optional[np.ndarray] = None,
                tight: Optional[np.ndarray] = None, use_link_metric: bool = True) -> int:
        """Bring rows solved before the last patch up to date in place; returns rows re-solved."""
        src = np.ascontiguousarray(sources, dtype=np.uint32)
        for a in (dist, nh, tight):
            if a is not None and not a.flags.c_contiguous:
                raise ValueError("rows must be C-contiguous")
        nb = nh.shape[2] if nh is not None else self.nh_bytes
        flags = (USE_LINK_METRIC if use_link_metric else 0) | (EMIT_TIGHT if tight is not None else 0)
        out = ctypes.c_uint32()
        _check(self._lib.openr_spf_refresh(self._ctx, _p(src), int(src.shape[0]), flags, _p(dist), _p(nh), nb,
                                           _p(tight), ctypes.byref(out)))
        return int(out.value)

    def refresh_device(self, d_sources: int, n: int, d_dist: int, d_nh: int = 0, nh_bytes: int = 0,
                       use_link_metric: bool = True, stream: int = 0, device_index: int = 0,
                       d_tight: int = 0) -> int:
        vp = ctypes.c_void_p
        flags = (USE_LINK_METRIC if use_link_metric else 0) | (EMIT_TIGHT if d_tight else 0)
        out = ctypes.c_uint32()
        _check(self._lib.openr_spf_refresh_device(self._ctx, device_index, vp(d_sources), n, flags, vp(d_dist),
                                                  vp(d_nh or None), nh_bytes or self.nh_bytes, vp(d_tight or None),
                                                  vp(stream or None), ctypes.byref(out)))
        return int(out.value)

    def last_kernels(self) -> list:
        """Kernels this thread's last solve call enqueued (openr_spf_last_kernels)."""
        return [k for k in self._lib.openr_spf_last_kernels().decode().split(";") if k]

    def stats(self) -> SpfStats:
        s = SpfStats()
        _check(self._lib.openr_spf_get_stats(self._ctx, ctypes.byref(s)))
        return s


def decode_paths(tok: np.ndarray):
    """Token row [n_paths, len_0, e.., len_1, e.., ...] -> list of edge-id lists."""
    n = int(tok[0])
    if n == 0xFFFFFFFF:
        raise SpfError(E2BIG, "pair overflowed its token row")
    out, pos = [], 1
    for _ in range(n):
        ln = int(tok[pos])
        out.append(tok[pos + 1 : pos + 1 + ln].astype(np.int64).tolist())
        pos += 1 + ln
    return out


def limits() -> SpfLimits:
    l = load_library()
    s = SpfLimits()
    l.openr_spf_limits(ctypes.byref(s))
    return s
