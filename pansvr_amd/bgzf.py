"""BGZF members inflated and compressed on the device through the C ABI (psvr_bgzf_decompress, psvr_bgzf_compress_members)."""
import ctypes as C

import numpy as np

from ._lib import EngineError, check, lib


class BgzfError(EngineError):
    """A member zlib would refuse; bad_member is its index, valid_bytes what the members in front of it inflate to."""

    def __init__(self, msg, bad_member, valid_bytes):
        EngineError.__init__(self, msg)
        self.bad_member, self.valid_bytes = bad_member, valid_bytes


def _call(device, buf, out, out_cap, offs, off_cap):
    used, total, nm, bad = C.c_int64(0), C.c_int64(0), C.c_int64(0), C.c_int64(-1)
    rc = lib().psvr_bgzf_decompress(C.c_int(device), buf.ctypes.data_as(C.c_void_p), C.c_int64(len(buf)), C.byref(used), out, C.c_int64(out_cap), C.byref(total),
                                    offs, C.c_int64(off_cap), C.byref(nm), C.byref(bad))
    return rc, used.value, total.value, nm.value, bad.value


def bgzf_sizes(data):
    """(bytes of the longest prefix of whole members, bytes they inflate to, their number); needs no device."""
    buf = np.frombuffer(bytes(data) or b"\0", dtype=np.uint8)[:len(data)]
    rc, used, total, nm, bad = _call(0, buf, None, 0, None, 0)
    if rc == 5:
        raise BgzfError(lib().psvr_last_error().decode(), bad, total)
    check(rc)
    return used, total, nm


def bgzf_decompress(data, device=0):
    """The whole members at the start of `data` inflated on HIP device `device`: (uint8 array, member offsets [n + 1], bytes of data used)."""
    buf = np.frombuffer(bytes(data) or b"\0", dtype=np.uint8)[:len(data)]
    rc, used, total, nm, bad = _call(device, buf, None, 0, None, 0)
    header_bad = rc == 5
    if not header_bad:
        check(rc)
    out = np.empty(max(total, 1), dtype=np.uint8)
    offs = np.zeros(nm + 1, dtype=np.int64)
    rc, used, total, nm, bad = _call(device, buf, out.ctypes.data_as(C.c_void_p), total, offs.ctypes.data_as(C.c_void_p), nm)
    if rc == 5:
        raise BgzfError(lib().psvr_last_error().decode(), bad, bytes(out[:offs[bad] if bad < nm else total]))
    check(rc)
    return out[:total], offs, used


def bgzf_compress(data, member_bytes=0xff00, device=0, effort=0):
    """`data` cut into members of member_bytes input bytes, each compressed by a wavefront of HIP device `device`:
    (uint8 array of the members side by side, member offsets [n + 1]).  effort 0..3: 0 is the greedy encoder with one hash-table candidate
    (psvr_bgzf_compress_members), 1 / 2 / 3 walk a hash chain of 4 / 8 / 16 candidates and match lazily (psvr_bgzf_compress_members_effort)."""
    buf = np.frombuffer(bytes(data) or b"\0", dtype=np.uint8)[:len(data)]
    L = lib()
    L.psvr_bgzf_members_bound.restype = C.c_int64
    cap = L.psvr_bgzf_members_bound(C.c_int64(len(buf)), C.c_int32(member_bytes))
    mb = member_bytes or 0xff00
    nm_cap = (len(buf) + mb - 1) // mb if mb > 0 else 0
    out = np.empty(max(cap, 1), dtype=np.uint8)
    offs = np.zeros(nm_cap + 1, dtype=np.int64)
    total, nm = C.c_int64(0), C.c_int64(0)
    args = (C.c_int(device), buf.ctypes.data_as(C.c_void_p), C.c_int64(len(buf)), C.c_int32(member_bytes), out.ctypes.data_as(C.c_void_p), C.c_int64(cap), C.byref(total),
            offs.ctypes.data_as(C.c_void_p), C.c_int64(nm_cap), C.byref(nm))
    check(L.psvr_bgzf_compress_members(*args) if effort == 0 else L.psvr_bgzf_compress_members_effort(*args, C.c_int32(effort)))
    return out[:total.value], offs[:nm.value + 1]


class BgzfStream:
    """One psvr_bgzf_stream_t: a BGZF byte stream in HBM, cut every member_bytes; the members of all takes, concatenated, are
    bgzf_compress's for everything appended at the same effort.  Single-owner."""

    def __init__(self, member_bytes=0xff00, device=0, effort=0):
        self.h = C.c_void_p()
        self.member_bytes = member_bytes or 0xff00
        L = lib()
        L.psvr_bgzf_stream_pending.restype = C.c_int64
        L.psvr_bgzf_members_bound.restype = C.c_int64
        L.psvr_bgzf_stream_destroy.restype = None
        check(L.psvr_bgzf_stream_create(C.c_int(device), C.c_int32(member_bytes), C.byref(self.h)))
        if effort:
            try:
                self.set_effort(effort)
            except EngineError:
                self.close()                                                   # (no stream is left behind by a constructor that raises)
                raise

    def set_effort(self, effort):
        """the encoder's effort (0..3, as bgzf_compress's) of every take from the next one on"""
        check(lib().psvr_bgzf_stream_set_effort(self.h, C.c_int32(effort)))

    def append(self, data):
        """bytes of the host behind what is pending"""
        buf = np.frombuffer(bytes(data) or b"\0", dtype=np.uint8)[:len(data)]
        check(lib().psvr_bgzf_stream_append(self.h, buf.ctypes.data_as(C.c_void_p), C.c_int64(len(buf))))

    def append_emit(self, emitter, first_pair, n_pairs):
        """the records of pairs [first_pair, first_pair + n_pairs) of a BamEmitter's last run, device to device; the emitter must not run
        again before a later take, pending or recover has returned"""
        check(lib().psvr_bgzf_stream_append_emit(self.h, emitter.h, C.c_int64(first_pair), C.c_int64(n_pairs)))

    @property
    def pending(self):
        n = lib().psvr_bgzf_stream_pending(self.h)
        if n < 0:
            check(int(-n))
        return n

    def take(self, finish=False, out_cap=None):
        """(uint8 array of the members made, member offsets [n + 1], stream bytes consumed); out_cap: the room offered, the bound by default"""
        L = lib()
        n = self.pending
        cap = L.psvr_bgzf_members_bound(C.c_int64(n), C.c_int32(self.member_bytes)) if out_cap is None else out_cap
        nm_cap = (n + self.member_bytes - 1) // self.member_bytes
        out = np.empty(max(cap, 1), dtype=np.uint8)
        offs = np.zeros(nm_cap + 1, dtype=np.int64)
        total, nm, used = C.c_int64(0), C.c_int64(0), C.c_int64(0)
        check(L.psvr_bgzf_stream_take(self.h, C.c_int(1 if finish else 0), out.ctypes.data_as(C.c_void_p), C.c_int64(cap), C.byref(total), offs.ctypes.data_as(C.c_void_p),
                                      C.c_int64(nm_cap), C.byref(nm), C.byref(used)))
        return out[:total.value], offs[:nm.value + 1], used.value

    def recover(self):
        """the pending bytes (uint8 array); the stream is empty afterwards"""
        n = self.pending
        out = np.empty(max(n, 1), dtype=np.uint8)
        got = C.c_int64(0)
        check(lib().psvr_bgzf_stream_recover(self.h, out.ctypes.data_as(C.c_void_p), C.c_int64(n), C.byref(got)))
        return out[:got.value]

    def close(self):
        if self.h:
            lib().psvr_bgzf_stream_destroy(self.h)
            self.h = None
