"""The main BAM file's records encoded on the device through the C ABI (psvr_bam_emit_*): from the window a FastqParser holds and a set of
results -- the caller's compact arrays (emit_results) or an engine's last run where it lies in HBM (emit_engine).  emit_ori_results /
emit_ori_engine do the same for the second (-p) file's records (psvr_bam_emit_ori_*); an emitter holds the records of its last run."""
import ctypes as C

import numpy as np

from ._lib import check, lib
from .aln import CAND_DTYPE, HDR_DTYPE, PAIR_DTYPE

NOT_ORI = 1  # PSVR_EMIT_NOT_ORI


class EmitInfo(C.Structure):  # psvr_bam_emit_info_t
    _fields_ = [("n_bytes", C.c_int64), ("n_records", C.c_int64), ("n_written_pairs", C.c_int64), ("n_declined_pairs", C.c_int64)]


class BamEmitter:
    """One psvr_bam_emit_t: device buffers of one emitted run of pairs.  Single-owner; `index` must outlive it."""

    def __init__(self, index):
        self.h = C.c_void_p()
        self.info = None
        self.n_pairs = 0
        check(lib().psvr_bam_emit_create(index.h, C.byref(self.h)))

    def emit_results(self, parser, hdr, pairs, cands, cigar, first_pair=0, flags=0):
        """hdr HDR_DTYPE[2P], pairs PAIR_DTYPE[P], cands CAND_DTYPE[], cigar uint32[] (the compact form of Engine.download_compact) for window
        pairs [first_pair, first_pair + P) of `parser`.  Returns the EmitInfo of the run."""
        hdr, pairs = np.ascontiguousarray(hdr, dtype=HDR_DTYPE), np.ascontiguousarray(pairs, dtype=PAIR_DTYPE)
        cands, cigar = np.ascontiguousarray(cands, dtype=CAND_DTYPE), np.ascontiguousarray(cigar, dtype=np.uint32)
        info = EmitInfo()
        check(lib().psvr_bam_emit_results(self.h, parser.h, C.c_int64(first_pair), C.c_int64(len(pairs)), hdr.ctypes.data_as(C.c_void_p), pairs.ctypes.data_as(C.c_void_p),
                                          cands.ctypes.data_as(C.c_void_p), C.c_int64(len(cands)), cigar.ctypes.data_as(C.c_void_p), C.c_int64(len(cigar)), C.c_int32(flags),
                                          C.byref(info)))
        self.info, self.n_pairs = info, len(pairs)
        return info

    def emit_engine(self, engine, parser, flags=0):
        """The results of engine's last run, device to device: its batch must have come from parser.upload_to(engine, ...)."""
        info = EmitInfo()
        check(lib().psvr_bam_emit_engine(self.h, engine.h, parser.h, C.c_int32(flags), C.byref(info)))
        self.info, self.n_pairs = info, engine.n_pairs
        return info

    def emit_ori_results(self, parser, hdr, pairs, cands, cigar, min_filter_score, first_pair=0):
        """The second file's records (psvr_bam_emit_ori_results) of the same arguments; min_filter_score is the gate of its pairs."""
        hdr, pairs = np.ascontiguousarray(hdr, dtype=HDR_DTYPE), np.ascontiguousarray(pairs, dtype=PAIR_DTYPE)
        cands, cigar = np.ascontiguousarray(cands, dtype=CAND_DTYPE), np.ascontiguousarray(cigar, dtype=np.uint32)
        info = EmitInfo()
        check(lib().psvr_bam_emit_ori_results(self.h, parser.h, C.c_int64(first_pair), C.c_int64(len(pairs)), hdr.ctypes.data_as(C.c_void_p), pairs.ctypes.data_as(C.c_void_p),
                                              cands.ctypes.data_as(C.c_void_p), C.c_int64(len(cands)), cigar.ctypes.data_as(C.c_void_p), C.c_int64(len(cigar)),
                                              C.c_int32(min_filter_score), C.byref(info)))
        self.info, self.n_pairs = info, len(pairs)
        return info

    def emit_ori_engine(self, engine, parser):
        """The second file's records of engine's last run, device to device; the gate is the engine's own min_filter_score."""
        info = EmitInfo()
        check(lib().psvr_bam_emit_ori_engine(self.h, engine.h, parser.h, C.byref(info)))
        self.info, self.n_pairs = info, engine.n_pairs
        return info

    def download(self):
        """(bytes uint8[n_bytes], pair_off int64[P + 1], pair_state uint8[P]) of the last run."""
        P = self.n_pairs
        data, off, state = np.full(self.info.n_bytes, 0xEE, dtype=np.uint8), np.zeros(P + 1, dtype=np.int64), np.full(P, 255, dtype=np.uint8)
        check(lib().psvr_bam_emit_download(self.h, data.ctypes.data_as(C.c_void_p), C.c_int64(len(data)), off.ctypes.data_as(C.c_void_p), state.ctypes.data_as(C.c_void_p)))
        return data, off, state

    def close(self):
        if self.h:
            lib().psvr_bam_emit_destroy.restype = None
            lib().psvr_bam_emit_destroy(self.h)
            self.h = None
