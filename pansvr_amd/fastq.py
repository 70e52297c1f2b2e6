"""FASTQ text parsed on the device through the C ABI (psvr_fastq_*): the arrays psvr_engine_upload takes, made in HBM and handed to an
engine device to device (psvr_engine_upload_fastq)."""
import ctypes as C

import numpy as np

from ._lib import check, lib
from .aln import ORI_DTYPE


class FastqInfo(C.Structure):  # psvr_fastq_info_t
    _fields_ = [("n_pairs", C.c_int64), ("used_bytes", C.c_int64), ("total_bases", C.c_int64), ("n_lines", C.c_int64), ("stop", C.c_int32), ("reserved", C.c_int32)]


class FastqParser:
    """One psvr_fastq_t: device buffers of one parsed window, kept across calls while the next fits.  Single-owner."""

    def __init__(self, device=0):
        self.h = C.c_void_p()
        self.info = None
        check(lib().psvr_fastq_create(C.c_int(device), C.byref(self.h)))

    def parse(self, text, max_pairs, max_bases, at_end=True):
        """text: bytes-like (interleaved FASTQ, four lines per read).  Returns the FastqInfo of the window."""
        buf = np.frombuffer(bytes(text) or b"\0", dtype=np.uint8)[:len(text)]
        info = FastqInfo()
        check(lib().psvr_fastq_parse(self.h, buf.ctypes.data_as(C.c_char_p), C.c_int64(len(buf)), C.c_int(1 if at_end else 0), C.c_int64(max_pairs), C.c_int64(max_bases),
                                     C.byref(info)))
        self.info = info
        return info

    def parse_signal(self, signal, first_byte, max_pairs, max_bases):
        """psvr_fastq_parse_signal: the bytes from first_byte on of the window of a pansvr_amd.signal_step.Signal, parsed where they lie."""
        info = FastqInfo()
        check(lib().psvr_fastq_parse_signal(self.h, signal.h, C.c_int64(first_byte), C.c_int64(max_pairs), C.c_int64(max_bases), C.byref(info)))
        self.info = info
        return info

    def text(self, first, n):
        """psvr_fastq_text: bytes [first, first + n) of the text the last parse looked at"""
        out = np.empty(max(n, 1), dtype=np.uint8)
        check(lib().psvr_fastq_text(self.h, out.ctypes.data_as(C.c_void_p), C.c_int64(first), C.c_int64(n)))
        return out[:n].tobytes()

    def download(self, bases=True):
        """dict: line_start uint64[8P + 1], name_end uint16[2P], base_off int64[2P + 1], ori ORI_DTYPE[2P] and, on request, bases
        uint8[total_bases + 1] (the NUL included)."""
        P = self.info.n_pairs
        out = {"line_start": np.zeros(8 * P + 1, dtype=np.uint64), "name_end": np.zeros(2 * P, dtype=np.uint16), "base_off": np.zeros(2 * P + 1, dtype=np.int64),
               "ori": np.zeros(2 * P, dtype=ORI_DTYPE)}
        if bases:
            out["bases"] = np.full(self.info.total_bases + 1, 255, dtype=np.uint8)
        check(lib().psvr_fastq_download(self.h, out["line_start"].ctypes.data_as(C.c_void_p), out["name_end"].ctypes.data_as(C.c_void_p), out["base_off"].ctypes.data_as(C.c_void_p),
                                        out["ori"].ctypes.data_as(C.c_void_p), out["bases"].ctypes.data_as(C.c_void_p) if bases else None))
        return out

    def upload_to(self, engine, first_pair=0, n_pairs=None):
        """psvr_engine_upload_fastq: pairs [first_pair, first_pair + n_pairs) become the engine's batch, device to device."""
        if n_pairs is None:
            n_pairs = self.info.n_pairs - first_pair
        check(lib().psvr_engine_upload_fastq(engine.h, self.h, C.c_int64(first_pair), C.c_int64(n_pairs)))
        engine.n_pairs = n_pairs

    def close(self):
        if self.h:
            lib().psvr_fastq_destroy(self.h)
            self.h = None
