"""Stable device order of 64-bit keys (psvr_sort_order_u64) and the device-resident record store (psvr_bam_store_*) through the C ABI."""
import ctypes as C

import numpy as np

from ._lib import EngineError, check, lib  # noqa: F401


def sort_order(keys, device=0):
    """keys: 1-D array of uint64.  Returns the uint32 order of np.argsort(keys, kind="stable"), computed on HIP device `device`."""
    k = np.ascontiguousarray(keys, dtype=np.uint64)
    if k.ndim != 1:
        raise ValueError("sort_order wants a 1-D key array")
    out = np.empty(len(k), dtype=np.uint32)
    check(lib().psvr_sort_order_u64(C.c_int(device), C.c_int64(len(k)), k.ctypes.data_as(C.c_void_p), out.ctypes.data_as(C.c_void_p)))
    return out


def sort_order_names(names, tie=None, device=0):
    """names: a list of bytes (none holds a NUL); tie: None or one uint8 per name.  Returns the uint32 order of
    sorted(range(n), key=lambda i: (names[i], tie[i], i)), computed on HIP device `device` (psvr_sort_order_names)."""
    names = [bytes(x) for x in names]
    if any(b"\0" in x for x in names):
        raise ValueError("sort_order_names wants names without a NUL")
    n = len(names)
    blob = np.frombuffer(b"".join(x + b"\0" for x in names) or b"\0", dtype=np.uint8)
    off = np.zeros(max(n, 1), dtype=np.int64)
    if n > 1:
        off[1:n] = np.cumsum([len(x) + 1 for x in names[:-1]])
    t = None if tie is None else np.ascontiguousarray(tie, dtype=np.uint8)
    if t is not None and t.shape != (n,):
        raise ValueError("sort_order_names wants one tie key per name")
    out = np.empty(n, dtype=np.uint32)
    check(lib().psvr_sort_order_names(C.c_int(device), C.c_int64(n), blob.ctypes.data_as(C.c_void_p), C.c_int64(len(blob) if n else 0), off.ctypes.data_as(C.c_void_p),
                                      None if t is None or n == 0 else t.ctypes.data_as(C.c_void_p), out.ctypes.data_as(C.c_void_p)))
    return out


class StoreInfo(C.Structure):  # psvr_bam_store_info_t
    _fields_ = [("n_records", C.c_int64), ("n_bytes", C.c_int64), ("key_exact", C.c_int32), ("ordered", C.c_int32)]


class ChainInfo(C.Structure):  # psvr_bam_chain_info_t
    _fields_ = [("segments", C.c_int64), ("no_guess", C.c_int64), ("wrong_guess", C.c_int64), ("rewalked", C.c_int64), ("tail_bytes", C.c_int64)]


class RecMeta(C.Structure):  # psvr_bam_rec_meta_t
    _fields_ = [("end", C.c_int64), ("tid", C.c_int32), ("pos", C.c_int32), ("len", C.c_uint32), ("index", C.c_uint32), ("bin", C.c_uint16), ("flag", C.c_uint16),
                ("pad", C.c_uint32)]


META_DTYPE = np.dtype([("end", "<i8"), ("tid", "<i4"), ("pos", "<i4"), ("len", "<u4"), ("index", "<u4"), ("bin", "<u2"), ("flag", "<u2"), ("pad", "<u4")])


class BamStore:
    """One psvr_bam_store_t: BAM records kept in HBM, ordered there by samtools' coordinate key and handed to a BgzfStream in sorted order.
    Single-owner."""

    def __init__(self, device=0):
        self.h = C.c_void_p()
        lib().psvr_bam_store_destroy.restype = None
        check(lib().psvr_bam_store_create(C.c_int(device), C.byref(self.h)))

    def append(self, data):
        """BAM records back to back (block_size first) from the host"""
        buf = np.frombuffer(bytes(data) or b"\0", dtype=np.uint8)[:len(data)]
        check(lib().psvr_bam_store_append(self.h, buf.ctypes.data_as(C.c_void_p), C.c_int64(len(buf))))

    def append_emit(self, emitter, first_pair, n_pairs):
        """the records of pairs [first_pair, first_pair + n_pairs) of a BamEmitter's last run, device to device; the emitter must not run
        again before a later info, append, order or download has returned"""
        check(lib().psvr_bam_store_append_emit(self.h, emitter.h, C.c_int64(first_pair), C.c_int64(n_pairs)))

    def append_bgzf(self, data, skip=0, n_ref=-1):
        """whole BGZF members of a BAM file back to back, inflated and cut into records on the device; `skip` inflated bytes at the front are
        no records (the header's remainder), n_ref is the file's reference count (a hint).  Returns the bytes used (the whole members); a
        corrupt member raises EngineError (PSVR_ERR_IO) with the member's index as its `bad_member`"""
        buf = np.frombuffer(bytes(data) or b"\0", dtype=np.uint8)[:len(data)]
        used, bad = C.c_int64(0), C.c_int64(-1)
        try:
            check(lib().psvr_bam_store_append_bgzf(self.h, buf.ctypes.data_as(C.c_void_p), C.c_int64(len(buf)), C.c_int64(skip), C.c_int32(n_ref), C.byref(used), C.byref(bad)))
        except EngineError as e:
            e.bad_member = bad.value
            raise
        return used.value

    def chain_info(self):
        """ChainInfo (segments, no_guess, wrong_guess, rewalked summed over all append_bgzf calls, tail_bytes), after a wait"""
        i = ChainInfo()
        check(lib().psvr_bam_store_chain_info(self.h, C.byref(i)))
        return i

    def info(self):
        """StoreInfo (n_records, n_bytes, key_exact, ordered), after a wait for what is queued"""
        i = StoreInfo()
        check(lib().psvr_bam_store_info(self.h, C.byref(i)))
        return i

    def order(self):
        check(lib().psvr_bam_store_order(self.h))

    def order_names(self):
        """name order instead: the names with strcmp, flag & 0xc0, append order; info().ordered is 2 afterwards"""
        check(lib().psvr_bam_store_order_names(self.h))

    def meta(self, first_rank=0, n=None):
        """structured array (META_DTYPE) of sorted ranks [first_rank, first_rank + n); n = None: to the end"""
        if n is None:
            n = self.info().n_records - first_rank
        out = np.zeros(max(n, 1), dtype=META_DTYPE)
        check(lib().psvr_bam_store_meta(self.h, C.c_int64(first_rank), C.c_int64(n), out.ctypes.data_as(C.c_void_p)))
        return out[:n]

    def stream(self, bgzf_stream, first_rank, n):
        """the records of those sorted ranks behind the pending bytes of a BgzfStream, device to device"""
        check(lib().psvr_bam_store_stream(self.h, bgzf_stream.h, C.c_int64(first_rank), C.c_int64(n)))

    def download(self):
        """every record in append order, with the recomputed bin (uint8 array)"""
        n = self.info().n_bytes
        out = np.empty(max(n, 1), dtype=np.uint8)
        got = C.c_int64(0)
        check(lib().psvr_bam_store_download(self.h, out.ctypes.data_as(C.c_void_p), C.c_int64(n), C.byref(got)))
        return out[:got.value]

    def drop(self, n_front):
        """the first n_front records (append order) cease to exist; chunks that hold none of the rest are released (one is kept as a spare)"""
        check(lib().psvr_bam_store_drop(self.h, C.c_int64(n_front)))

    def footprint(self):
        """(chunks, bytes) the store holds in device memory for records: the live chunks and the spare one"""
        n, b = C.c_int64(0), C.c_int64(0)
        check(lib().psvr_bam_store_footprint(self.h, C.byref(n), C.byref(b)))
        return n.value, b.value

    def close(self):
        if self.h:
            lib().psvr_bam_store_destroy(self.h)
            self.h = None
