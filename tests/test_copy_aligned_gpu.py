"""-m gpu: the one destination-aligned copy (pansvr_amd/csrc/copy_aligned_device.h) through its two kernels, k_bs_append of the BGZF stream and
k_store_copy of the record store, at every residue of the destination modulo 16: records of an emitter's run appended device to device behind
0..15 host bytes, held to the emitter's own download."""
import tempfile

import numpy as np
import pytest

import bam_emit_cases as bc
import bam_stream
import fastq_cases as fc
from test_bam_emit_gpu import fx1  # noqa: F401  (fx1: index, parser and emitter of golden set fx1)
from test_bam_store_gpu import chunk_bytes, expectation, make_record

pytestmark = pytest.mark.gpu
MAGIC = b"BAM\1\0\0\0\0\0\0\0\0"


def test_the_shared_copy_at_every_destination_residue(fx1):
    from pansvr_amd.aln import CAND_DTYPE, HDR_DTYPE, PAIR_DTYPE
    from pansvr_amd.bgzf import BgzfStream
    from pansvr_amd.sort import BamStore
    index, n_header, anchors, parser, emitter = fx1
    c, = [c for c in bc.cases(golden=False) if c["name"] == "255 pairs"]
    s_, raw = bc.run_checker(bc.build_checker(tempfile.mkdtemp(prefix="psvr_cpy_"), False), c["text"], c["cls"], c["seed"], c["flags"], n_header=n_header, anchors=anchors)
    w = bc.split_out(raw)
    assert w["P"] == 255 and parser.parse(c["text"], fc.BIG_PAIRS, fc.BIG_BASES).n_pairs == 255
    arrays = [np.frombuffer(w[k], dtype=dt) for k, dt in (("hdr", HDR_DTYPE), ("pairs", PAIR_DTYPE), ("cands", CAND_DTYPE), ("cigar", np.uint32))]
    assert emitter.emit_results(parser, *arrays, flags=c["flags"]).n_bytes > 0
    data, off, state = emitter.download()
    rec = data.tobytes()
    # two short ranges, a long one, and two empty ones: behind (0, 1) and (1, 1) the destination has moved by a pair's bytes, so the ranges meet
    # other residues of source and destination than r alone.  A range shorter than its lead (under 16 bytes) does not exist: a record has at
    # least 36 bytes, so the empty form stands for it -- it leaves before the copy, with any lead
    ranges = ((0, 1), (1, 0), (1, 1), (2, 253), (255, 0))
    assert off[1] - off[0] > 36 and off[255] == len(rec)
    assert b"".join(rec[off[a]:off[a + n]] for a, n in ranges) == rec
    for r in range(16):
        s = BgzfStream()
        front = bytes(range(1, r + 1))
        s.append(front)
        for a, n in ranges:
            s.append_emit(emitter, a, n)
        got = s.recover().tobytes()
        assert got == front + rec, "stream, residue %d: %s" % (r, bam_stream.first_difference(MAGIC + got[r:], MAGIC + rec))
        s.close()
    records = bam_stream.split(MAGIC + rec)[1]
    for r in range(16):
        front = make_record(36 + r, 1, 1000 + r, 0, [(50, 0)], r)
        with chunk_bytes(4 * len(rec) + 4096):                                 # room for the host record and three ranges of at most the run's size: one chunk
            st = BamStore()
        st.append(front)                                                       # the chunk's fill has residue (36 + r) % 16
        for a, n in ranges:
            st.append_emit(emitter, a, n)
        want = b"".join(expectation([front] + records)[0])
        i = st.info()
        assert (i.n_records, i.n_bytes) == (1 + len(records), len(want)), r
        got = st.download().tobytes()
        assert got == want, "store, residue %d: %s" % ((36 + r) % 16, bam_stream.first_difference(MAGIC + got, MAGIC + want))
        st.close()
