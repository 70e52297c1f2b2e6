"""pansvr_amd/csrc/bam_record.h on its own, without a GPU: tests/tools/bam_record_check.cpp (plain and under AddressSanitizer + UBSan, a
stand-alone program both times) against a restatement of the record's rules written here: the validity layers, the CIGAR's reference span,
beg / end, the bin (tests/bam_reader.reg2bin), samtools' key and the range in which it is exact."""
import functools
import os
import random
import struct
import subprocess
import tempfile

import numpy as np
import pytest

import bam_reader
from test_bam_store_gpu import SPANS, make_record, make_records
from test_sort_device_gpu import _planted

HERE = os.path.dirname(os.path.abspath(__file__))
CHECK_SRC = os.path.join(HERE, "tools", "bam_record_check.cpp")
REF_OPS = (0, 2, 3, 7, 8)                                                      # M D N = X
POSITIONS = (-1, 0, 16383, 16384, (1 << 26) - 1, 1 << 29, (1 << 31) - 2, (1 << 31) - 1, -2)   # the last two: outside the key's exact range
KINDS = ("block_size 31", "negative l_seq", "name without NUL", "CIGAR leaves its record")
NOT_ASKED = " -1" * 10


@pytest.fixture(scope="module", params=[False, True], ids=["plain", "sanitized"])
def checker(request):
    tmp = tempfile.mkdtemp(prefix="psvr_rec_")
    exe = os.path.join(tmp, "bam_record_check_asan" if request.param else "bam_record_check")
    flags = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"] if request.param else ["-O2"]
    subprocess.check_call(["g++"] + flags + ["-std=c++17", "-Wall", "-o", exe, CHECK_SRC])
    return exe


def _run(exe, mode, data):
    tmp = tempfile.mkdtemp(prefix="psvr_rec_")
    with open(os.path.join(tmp, "in"), "wb") as f:
        f.write(data)
    r = subprocess.run([exe, mode, os.path.join(tmp, "in"), os.path.join(tmp, "out")], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600)
    assert r.returncode == 0 and not r.stderr, "bam_record_check: exit status %d\n%s" % (r.returncode, r.stderr.decode()[-4000:])
    return open(os.path.join(tmp, "out"), "rb").read()


# ---- the restatement ---------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def framed(rec):
    """the rest of the line of a record whose frame holds: rec = exactly its 4 + block_size bytes (nothing else of the buffer is the rules' business)"""
    bs, tid, pos, l_name = struct.unpack_from("<IiiB", rec, 0)
    n_cig, flag, l_seq = struct.unpack_from("<HHi", rec, 16)
    cigar = l_name + 4 * n_cig <= bs - 32                                      # the formatter's rule
    fields = l_seq >= 0 and l_name + 4 * n_cig + (l_seq + 1) // 2 + l_seq <= bs - 32
    reader = l_name >= 1 and fields                                            # the reader's rule
    nul = int(rec[36 + l_name - 1] == 0) if reader else -1
    out = " 1 %d %d %d %d" % (cigar, fields, reader, nul)
    if not cigar:
        return out + NOT_ASKED
    span = sum(w >> 4 for w in struct.unpack_from("<%dI" % n_cig, rec, 36 + l_name) if w & 15 in REF_OPS)
    beg = max(pos, 0)
    end = beg + (span or 1)
    key = ((tid & 0xffffffff) << 32) | ((((pos & 0xffffffff) + 1) << 1) & 0xffffffff) | ((flag >> 4) & 1)
    return out + " %d %d %d %d %d %d %d %d %d %d" % (span, beg, end, bam_reader.reg2bin(beg, end) & 0xffff, key, -1 <= pos <= (1 << 31) - 2, tid, pos, 4 + bs, flag)


def restate(c, buf):
    """the lines of case c: one record after the other while the frame holds (36 bytes, block_size >= 32, the record inside the buffer)"""
    at, n, lines = 0, len(buf), []
    while at < n:
        bs = struct.unpack_from("<I", buf, at)[0] if n - at >= 36 else 0
        if n - at < 36 or bs < 32 or bs > n - at - 4:
            lines.append("%d %d 0 -1 -1 -1 -1%s" % (c, at, NOT_ASKED))
            break
        lines.append("%d %d%s" % (c, at, framed(buf[at:at + 4 + bs])))
        at += 4 + bs
    lines.append("%d end %d" % (c, at))
    return lines


# ---- the inputs ---------------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def inputs():
    """(names, buffers, the lines the checker must print); made once for both builds"""
    cases = []
    recs = make_records(2048, 7)                                               # lengths 36..99 in turn, one of 70 000 bytes; unplaced records; every kind of CIGAR
    assert {len(r) for r in recs} == set(range(36, 100)) | {70000}
    assert any(struct.unpack_from("<ii", r, 4) == (-1, -1) for r in recs)
    cases.append(("generated", b"".join(recs)))
    for pos in POSITIONS:
        for k, cigar in enumerate(SPANS):
            cases.append(("pos %d cigar %d" % (pos, k), b"".join(make_record(99, tid, pos, flag, cigar, 31 * k + flag) for tid in (1, -1) for flag in (0, 16))))
    for op in range(9, 16):                                                    # nibbles that are no operator: no reference bases
        cases.append(("op %d" % op, make_record(80, 0, 1000, 0, [(50, op)], op) + make_record(80, 0, 1000, 0, [(10, 0), (50, op), (7, 2)], op)))
    for kind in KINDS:
        cases.append((kind, _planted(kind)))
    stream = b"".join(make_records(300, 9))
    whole = sum(map(len, make_records(300, 9)[:200]))
    for name, cut in (("cut inside a head", whole + 20), ("cut inside a body", whole + 36 + 9), ("cut inside a block_size", whole + 3), ("empty", 0)):
        cases.append((name, stream[:cut]))
    cases.append(("the stream that is mutated", stream))
    starts = [0]
    for r in make_records(300, 9):
        starts.append(starts[-1] + len(r))
    rng = random.Random(41)
    for i in range(2000):
        m = bytearray(stream)
        at = rng.randrange(len(m))
        m[at] ^= 1 << rng.randrange(8) if rng.random() < 0.5 else rng.randrange(1, 256)
        first = max(s for s in starts if s <= at)                              # (the records in front of the mutated one are the case above)
        cases.append(("mutation %d at byte %d" % (i, at), bytes(m[first:])))
    want = [l for c, (_, buf) in enumerate(cases) for l in restate(c, buf)]
    return [n for n, _ in cases], [b for _, b in cases], want


def test_every_layer_and_every_derived_field(checker):
    names, bufs, want = inputs()
    got = _run(checker, "records", struct.pack("<I", len(bufs)) + b"".join(struct.pack("<I", len(b)) + b for b in bufs)).decode().split("\n")
    assert got[-1] == "" and len(got) - 1 == len(want)
    if got[:-1] != want:
        k = next(i for i, (a, b) in enumerate(zip(got, want)) if a != b)
        raise AssertionError("case '%s': the checker prints\n%s\nthe restatement\n%s" % (names[int(want[k].split()[0])], got[k], want[k]))
    rows = [l.split() for l in want if l.split()[1] != "end"]
    # every layer has said yes and no, and the formatter's rule and the reader's are two rules: a 36-byte record has no name, which the formatter's takes
    for col in (2, 3, 4, 5, 6):
        assert {r[col] for r in rows} >= {"0", "1"}, col
    assert any(r[3] == "1" and r[5] == "0" for r in rows)
    by_case = {}
    for r in rows:
        by_case.setdefault(names[int(r[0])], []).append(r)
    for pos in POSITIONS:
        exact = {r[12] for k in range(len(SPANS)) for r in by_case["pos %d cigar %d" % (pos, k)]}
        assert exact == ({"0"} if pos in ((1 << 31) - 1, -2) else {"1"}), pos
    assert all(r[7] == "0" for r in by_case["op 9"][:1]) and [r[7] for r in by_case["op 15"]] == ["0", "17"]
    for kind, col in zip(KINDS, (2, 4, 6, 3)):                                 # the layer that refuses each planted record: frame, fields, the NUL, the CIGAR
        assert [r[col] for r in by_case[kind]].count("0") >= 1 and by_case[kind][1000][col] == "0", kind
    assert by_case["cut inside a head"][-1][2] == "0" and by_case["cut inside a body"][-1][2] == "0" and "empty" not in by_case


def test_cigar_ref_len_is_the_encoders_span_for_every_length_and_operator(checker):
    """bam_cigar_ref_len(be_cigar_word(len16, op)) against be_cigar_span(len16, op) as bam_emit_device.h had it before it called bam_record.h:
    int16(len16) & 0xfffffff for an operator that consumes reference, 0 otherwise; all 2^16 lengths, all 16 operators"""
    len16, op = np.meshgrid(np.arange(1 << 16, dtype=np.int64), np.arange(16, dtype=np.int64), indexing="ij")
    signed = len16.astype(np.uint16).astype(np.int16).astype(np.int64)         # the length after the round trip through "%d" of an int16
    word = (((signed & 0xffffffff) << 4) | op) & 0xffffffff                     # be_cigar_word
    want = np.where(np.isin(op, REF_OPS), signed & 0xfffffff, 0)
    got = np.frombuffer(_run(checker, "words", word.astype("<u4").tobytes()), dtype="<i8").reshape(word.shape)
    assert got.shape == want.shape and (got == want).all(), np.argwhere(got != want)[:4]
    assert int(want[0xffff, 0]) == 0xfffffff and int(want[1, 8]) == 1 and int(want[5, 1]) == 0
