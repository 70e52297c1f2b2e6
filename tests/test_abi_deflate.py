"""psvr_bgzf_compress_members / psvr_bgzf_members_bound at the C boundary without launching anything: argument checks, the bound, and
the loud error where no device is visible."""
import ctypes as C

import numpy as np


def _call(L, device, buf, n, mb, out, cap, offs, off_cap, out_bytes=True):
    total, nm = C.c_int64(-7), C.c_int64(-7)
    rc = L.psvr_bgzf_compress_members(C.c_int(device), buf, C.c_int64(n), C.c_int32(mb), out, C.c_int64(cap), C.byref(total) if out_bytes else None,
                                      offs, C.c_int64(off_cap), C.byref(nm))
    return rc, total.value, nm.value


def test_bad_arguments_and_the_empty_input():
    from pansvr_amd import lib
    L = lib()
    data = np.arange(1000, dtype=np.uint8)
    out = np.zeros(2000, dtype=np.uint8)
    offs = np.zeros(8, dtype=np.int64)
    p, q, o = data.ctypes.data_as(C.c_void_p), out.ctypes.data_as(C.c_void_p), offs.ctypes.data_as(C.c_void_p)
    assert _call(L, 0, p, -1, 0, q, 2000, o, 7)[0] == 1
    assert _call(L, 0, None, 1000, 0, q, 2000, o, 7)[0] == 1
    assert _call(L, 0, p, 1000, 0, None, 2000, o, 7)[0] == 1
    assert _call(L, 0, p, 1000, 0, q, 2000, o, 7, out_bytes=False)[0] == 1
    assert _call(L, 0, p, 1000, 0, q, -1, o, 7)[0] == 1
    assert _call(L, 0, p, 1000, 0, q, 2000, o, -1)[0] == 1
    for mb in (1, 255, 0xff01, 65536, -5):
        assert _call(L, 0, p, 1000, mb, q, 2000, o, 7)[0] == 1, mb
    assert b"psvr_bgzf_compress_members" in L.psvr_last_error()
    offs[0] = 99
    assert _call(L, 0, p, 0, 0, q, 2000, o, 7) == (0, 0, 0) and offs[0] == 0      # no bytes: no members, and no device needed
    assert _call(L, 0, p, 1000, 256, q, 2000, o, 3)[0] == 6                      # four members, room for three offsets


def test_without_a_device_the_call_is_an_error():
    from pansvr_amd import lib
    L = lib()
    if L.psvr_device_count() > 0:
        return
    data = np.arange(1000, dtype=np.uint8)
    out = np.zeros(2000, dtype=np.uint8)
    offs = np.zeros(8, dtype=np.int64)
    rc, total, nm = _call(L, 0, data.ctypes.data_as(C.c_void_p), 1000, 0, out.ctypes.data_as(C.c_void_p), 2000, offs.ctypes.data_as(C.c_void_p), 7)
    assert rc == 3 and total == 0 and nm == 0
    assert b"no HIP device" in L.psvr_last_error()
    from pansvr_amd import EngineError
    from pansvr_amd.bgzf import bgzf_compress
    try:
        bgzf_compress(b"abc" * 100)
    except EngineError as ex:
        assert "no HIP device" in str(ex)
    else:
        raise AssertionError("compressed without a GPU: a CPU fallback must not exist")


def test_members_bound():
    from pansvr_amd import lib
    L = lib()
    L.psvr_bgzf_members_bound.restype = C.c_int64
    bound = lambda n, mb: L.psvr_bgzf_members_bound(C.c_int64(n), C.c_int32(mb))
    for mb in (0, 256, 4096, 0x4000, 0xff00):
        size = mb or 0xff00
        prev = 0
        ns = sorted(set(list(range(0, 3000, 7)) + [size - 1, size, size + 1, 5 * size, 5 * size + 1, 1 << 28, (1 << 28) + 1]))
        for n in ns:
            b = bound(n, mb)
            assert b >= n + 26 * ((n + size - 1) // size), (n, mb)
            assert b >= prev, (n, mb)
            prev = b
    assert bound(0, 0) == 0 and bound(1000, 0) == bound(1000, 0xff00)
