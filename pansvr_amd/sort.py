"""Stable device order of 64-bit keys through the C ABI (psvr_sort_order_u64)."""
import ctypes as C

import numpy as np

from ._lib import check, lib


def sort_order(keys, device=0):
    """keys: 1-D array of uint64.  Returns the uint32 order of np.argsort(keys, kind="stable"), computed on HIP device `device`."""
    k = np.ascontiguousarray(keys, dtype=np.uint64)
    if k.ndim != 1:
        raise ValueError("sort_order wants a 1-D key array")
    out = np.empty(len(k), dtype=np.uint32)
    check(lib().psvr_sort_order_u64(C.c_int(device), C.c_int64(len(k)), k.ctypes.data_as(C.c_void_p), out.ctypes.data_as(C.c_void_p)))
    return out
