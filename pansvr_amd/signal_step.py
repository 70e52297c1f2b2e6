"""`panSVR signal -N` over a device-resident record store (psvr_signal_*, include/psvr_engine.h) through the C ABI: the pairs of a BamStore's
records judged and formatted as FASTQ text on the device."""
import ctypes as C

import numpy as np

from ._lib import EngineError, check, lib  # noqa: F401

MAX_ISIZE, MAX_LEN = 100000, 1000            # BamStat's two histograms


class SignalOpt(C.Structure):  # psvr_signal_opt_t
    _fields_ = [(n, C.c_int32) for n in ("gap_open", "gap_ex", "gap_open2", "gap_ex2", "match", "mismatch", "max_tid", "not_use_filter", "discard_full_match", "isize_min",
                                          "isize_max")] + [("stat", C.c_int32 * 4)]


class SignalInfo(C.Structure):  # psvr_signal_info_t
    _fields_ = [(n, C.c_int64) for n in ("pairs", "written", "declined", "first_error", "text_bytes", "consumed", "side_bytes")]


class SignalWindowInfo(C.Structure):  # psvr_signal_window_info_t
    _fields_ = [(n, C.c_int64) for n in ("n_bytes", "n_pairs", "n_host_pairs")]


class SignalPosOpt(C.Structure):  # psvr_signal_pos_opt_t (0: the default)
    _fields_ = [("block_records", C.c_int64), ("block_span", C.c_int64)]


class SignalPosInfo(C.Structure):  # psvr_signal_pos_info_t
    _fields_ = [(n, C.c_int64) for n in ("complete", "primaries", "consumed", "unmated", "left_bytes", "mate_failed", "notes", "replayed")]


class SignalLeftInfo(C.Structure):  # psvr_signal_left_info_t
    _fields_ = [(n, C.c_int64) for n in ("records", "pairs", "errors", "first_pair", "n_pairs", "more")]


NOTE_DTYPE = np.dtype([("number", "<i8"), ("index", "<i4"), ("block", "<i4"), ("tid", "<i4"), ("pos", "<i4"), ("name", "S256")])   # psvr_signal_mate_note_t
PAIR_DTYPE = np.dtype([("text_off", "<i8"), ("rec1", "<i8"), ("rec2", "<i8"), ("side_off", "<i8"), ("bytes", "<i4"), ("state", "u1"), ("note", "u1"), ("pad", "<u2")])   # psvr_signal_pair_t


def signal_opt(stat, isize_min, isize_max, not_use_filter=False, discard_full_match=False, max_tid=24, gap_open=16, gap_ex=1, gap_open2=32, gap_ex2=0, match=2, mismatch=12):
    """the step's options with the command's defaults; stat: the four numbers of STAT_ (read_len, min_i, mid_i, max_i)"""
    o = SignalOpt(gap_open, gap_ex, gap_open2, gap_ex2, match, mismatch, max_tid, int(not_use_filter), int(discard_full_match), isize_min, isize_max)
    for k in range(4):
        o.stat[k] = int(stat[k])
    return o


class Signal:
    """One psvr_signal_t.  Single-owner."""

    def __init__(self, opt, device=0):
        self.h = C.c_void_p()
        lib().psvr_signal_destroy.restype = None
        check(lib().psvr_signal_create(C.c_int(device), C.byref(opt), C.byref(self.h)))
        self.info = self.pos_info = None

    def run(self, store, first_record=0, finish=False):
        """the store's records [first_record, n_records) paired, judged and formatted; returns SignalInfo"""
        i = SignalInfo()
        check(lib().psvr_signal_run(self.h, store.h, C.c_int64(first_record), C.c_int32(int(finish)), C.byref(i)))
        self.info = i
        return i

    def run_pos(self, store, first_record=0, finish=False, block_records=0, block_span=0):
        """the block of the position-sorted mode at the store's front (psvr_signal_run_pos); returns (SignalInfo, SignalPosInfo); text(), pairs(),
        side() and stats() answer behind it as behind run(), when the block was complete"""
        i, pi, o = SignalInfo(), SignalPosInfo(), SignalPosOpt(block_records, block_span)
        check(lib().psvr_signal_run_pos(self.h, store.h, C.c_int64(first_record), C.c_int32(int(finish)), C.byref(o), C.byref(i), C.byref(pi)))
        self.info, self.pos_info = (i if pi.complete else None), pi
        return i, pi

    def mate_notes(self):
        """the last block's notes (NOTE_DTYPE): every 1000th "Mate failed" turn"""
        n = self.pos_info.notes if self.pos_info else 0
        out = np.zeros(max(n, 1), dtype=NOTE_DTYPE)
        check(lib().psvr_signal_mate_notes(self.h, out.ctypes.data_as(C.c_void_p), C.c_int64(n)))
        return out[:n]

    def left(self):
        """the last block's unmated records back to back (bytes), in block order"""
        n = self.pos_info.left_bytes if self.pos_info else 0
        out = np.empty(max(n, 1), dtype=np.uint8)
        check(lib().psvr_signal_left(self.h, out.ctypes.data_as(C.c_void_p), C.c_int64(n)))
        return out[:n].tobytes()

    def run_left(self, first_pair=0, max_pairs=1 << 20):
        """a slice of the by-name pass over the object's left store (psvr_signal_run_left; the first call orders the store); returns
        (SignalInfo, SignalLeftInfo); text(), pairs() (rec1 / rec2: indices into the left store), side() and stats() answer behind it"""
        i, li = SignalInfo(), SignalLeftInfo()
        check(lib().psvr_signal_run_left(self.h, C.c_int64(first_pair), C.c_int64(max_pairs), C.byref(i), C.byref(li)))
        self.info, self.pos_info, self.left_info = i, None, li
        return i, li

    def left_errors(self):
        """per pair of the last slice, the pairing-error steps of the whole pass in front of it (int64 array)"""
        n = self.left_info.n_pairs
        out = np.zeros(max(n, 1), dtype=np.int64)
        check(lib().psvr_signal_left_errors(self.h, out.ctypes.data_as(C.c_void_p), C.c_int64(n)))
        return out[:n]

    def text(self):
        """the last run's text (bytes): its state-1 pairs in front of the first error pair"""
        n = self.info.text_bytes if self.info else 0
        out = np.empty(max(n, 1), dtype=np.uint8)
        check(lib().psvr_signal_text(self.h, out.ctypes.data_as(C.c_void_p), C.c_int64(n)))
        return out[:n].tobytes()

    def pairs(self):
        """the last run's table (PAIR_DTYPE)"""
        n = self.info.pairs if self.info else 0
        out = np.zeros(max(n, 1), dtype=PAIR_DTYPE)
        check(lib().psvr_signal_pairs(self.h, out.ctypes.data_as(C.c_void_p), C.c_int64(n)))
        return out[:n]

    def side(self):
        """the last run's side records (bytes): at a pair's side_off the two records of a declined or noted pair, or of the error pair"""
        n = self.info.side_bytes if self.info else 0
        out = np.empty(max(n, 1), dtype=np.uint8)
        check(lib().psvr_signal_side(self.h, out.ctypes.data_as(C.c_void_p), C.c_int64(n)))
        return out[:n].tobytes()

    def pair_records(self, store, pair):
        """the two records of a pair of the last run, back to back (bytes)"""
        out = np.empty(1 << 16, dtype=np.uint8)
        got = C.c_int64(0)
        rc = lib().psvr_signal_pair_records(self.h, store.h, C.c_int64(pair), out.ctypes.data_as(C.c_void_p), C.c_int64(len(out)), C.byref(got))
        if rc == 6:                                                      # PSVR_ERR_OVERFLOW: the size came with the refusal
            out = np.empty(got.value, dtype=np.uint8)
            rc = lib().psvr_signal_pair_records(self.h, store.h, C.c_int64(pair), out.ctypes.data_as(C.c_void_p), C.c_int64(len(out)), C.byref(got))
        check(rc)
        return out[:got.value].tobytes()

    def stats(self):
        """(isize_n, len_n): BamStat::collect's histograms over every pair of all runs (uint64 arrays)"""
        a, b = np.zeros(MAX_ISIZE, dtype=np.uint64), np.zeros(MAX_LEN, dtype=np.uint64)
        check(lib().psvr_signal_stats(self.h, a.ctypes.data_as(C.c_void_p), b.ctypes.data_as(C.c_void_p)))
        return a, b

    def window(self, host_text=b"", host_off=(0,)):
        """psvr_signal_window: the last run's text and the host formatter's text of its state-2 pairs (host_text[host_off[i]:host_off[i + 1]]
        for the i-th of them in front of the first error pair) become one window in pair order on the device; returns SignalWindowInfo"""
        text = np.frombuffer(bytes(host_text) or b"\0", dtype=np.uint8)
        off = np.ascontiguousarray(host_off, dtype=np.int64)
        i = SignalWindowInfo()
        check(lib().psvr_signal_window(self.h, text.ctypes.data_as(C.c_void_p), C.c_int64(len(host_text)), off.ctypes.data_as(C.c_void_p), C.c_int64(len(off) - 1), C.byref(i)))
        self.window_info = i
        return i

    def window_add(self, host_text=b"", off=(0,), restart=False):
        """psvr_signal_window_add: the last run's window (as window() makes it) written behind what the object's kept window holds; restart
        empties the kept window first.  Returns SignalWindowInfo with the kept window's totals; window_text() reads it"""
        text = np.frombuffer(bytes(host_text) or b"\0", dtype=np.uint8)
        off = np.ascontiguousarray(off, dtype=np.int64)
        i = SignalWindowInfo()
        check(lib().psvr_signal_window_add(self.h, text.ctypes.data_as(C.c_void_p), C.c_int64(len(host_text)), off.ctypes.data_as(C.c_void_p), C.c_int64(len(off) - 1),
                                           C.c_int32(int(restart)), C.byref(i)))
        self.window_info = i
        return i

    def window_text(self, first=0, n=None):
        """bytes [first, first + n) of the window (to its end by default)"""
        if n is None:
            n = self.window_info.n_bytes - first
        out = np.empty(max(n, 1), dtype=np.uint8)
        check(lib().psvr_signal_window_text(self.h, out.ctypes.data_as(C.c_void_p), C.c_int64(first), C.c_int64(n)))
        return out[:n].tobytes()

    def close(self):
        if self.h:
            lib().psvr_signal_destroy(self.h)
            self.h = None
