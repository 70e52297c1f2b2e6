"""The record-chain finder of psvr_bam_store_append_bgzf without a GPU: the host build of pansvr_amd/csrc/bam_chain_device.h
(tests/tools/bam_chain_check.cpp, plain and under AddressSanitizer + UBSan as a stand-alone program) against a plain serial walk."""
import random
import tempfile

import pytest

import bam_chain_cases as cc

SEGS = (64, 256, 4096, 65536)


@pytest.fixture(scope="module", params=[False, True], ids=["plain", "sanitized"])
def checker(request):
    return cc.build_checker(tempfile.mkdtemp(prefix="psvr_chain_"), request.param)


@pytest.fixture(scope="module")
def stream():
    recs = cc.records(8200, 3, long_at=2733)
    assert {len(r) for r in recs} == set(range(37, 100)) | {70000}
    return recs, b"".join(recs)


def _hold(got, buf, start, seg, what):
    total, tail, bad, entries = cc.expected(buf, start, seg)
    assert (got["total"], got["tail"], got["first_malformed"]) == (total, tail, bad), (what, got["total"], got["tail"], got["first_malformed"], total, tail, bad)
    assert got["segments"] == (len(buf) + seg - 1) // seg and got["entries"] == entries, what
    assert got["entries"] == sorted(got["entries"]), what


def test_generated_records_every_segment_size(checker, stream):
    recs, buf = stream
    mid = sum(map(len, recs[:1234]))
    head_cut = buf[:sum(map(len, recs[:7000])) + 20]                         # ends inside a record's head
    body_cut = buf[:sum(map(len, recs[:7000])) + 36 + 9]                     # ... inside its body
    long_cut = buf[:sum(map(len, recs[:2733])) + 30000]                      # ... inside the long record, segments behind its start
    cases = [(b, start, cc.N_REF, seg) for seg in SEGS for b, start in ((buf, 0), (buf, mid), (head_cut, 0), (body_cut, mid), (long_cut, 0), (b"", 0), (buf[:40], 0))]
    got = cc.run_checker(checker, cases)
    for g, (b, start, _, seg) in zip(got, cases):
        _hold(g, b, start, seg, (len(b), start, seg))
    whole = [g for g, c in zip(got, cases) if c[0] is buf and c[1] == 0]
    assert [g["total"] for g in whole] == [8200] * 4 and [g["tail"] for g in whole] == [0] * 4
    for g, seg in zip(whole, SEGS):
        print("seg %d: segments %d, no guess %d, wrong %d, walked again %d" % (seg, g["segments"], g["no_guess"], g["wrong_guess"], g["rewalked"]))
    # without the hint of the reference count the result is the same
    free = cc.run_checker(checker, [(buf, 0, -1, seg) for seg in SEGS])
    for g, seg in zip(free, SEGS):
        _hold(g, buf, 0, seg, ("no n_ref", seg))


@pytest.mark.parametrize("tail", [5, 0])
def test_decoy_records_inside_a_long_record_are_repaired(checker, tail):
    buf = cc.decoy_stream(tail)
    g, = cc.run_checker(checker, [(buf, 0, cc.N_REF, 256)])
    _hold(g, buf, 0, 256, tail)
    assert g["total"] == 26 and g["tail"] == 0 and g["first_malformed"] == -1
    assert g["wrong_guess"] >= 1 and g["rewalked"] >= 1


def test_block_size_edges_at_segment_edges_whole_records_and_decoys(checker):
    buf, n = cc.edge_stream()
    assert n <= 200 and cc.walk(buf) == (cc.walk(buf)[0], len(buf), False) and len(cc.walk(buf)[0]) == n
    sizes = {len(buf[a:b]) for a, b in zip(cc.walk(buf)[0], cc.walk(buf)[0][1:] + [len(buf)])}
    assert sizes >= {37, 39, 40, 41}
    segs = (cc.EDGE_SEG, 256, 4096)
    got = cc.run_checker(checker, [(buf, 0, n_ref, seg) for seg in segs for n_ref in (cc.N_REF, -1)])
    for g, (seg, n_ref) in zip(got, [(seg, n_ref) for seg in segs for n_ref in (cc.N_REF, -1)]):
        _hold(g, buf, 0, seg, ("edges", seg, n_ref))
        assert (g["total"], g["tail"], g["first_malformed"]) == (n, 0, -1)
    # at the segment size the stream was made for, 7 long records cover 3 segments each: no record starts in those 21, so each has no guess or a
    # wrong one.  The decoys with block_size 33, 36, kBamRecStoreMaxBlock - 1 and kBamRecStoreMaxBlock are the lowest offset of their segment
    # that looks like a record (zeros lie in front of them): 12 wrong guesses at least.  (A decoy's other fields can read as a block_size too.)
    g = got[0]
    print("edge stream: %d records, %d segments, no guess %d, wrong %d, walked again %d" % (n, g["segments"], g["no_guess"], g["wrong_guess"], g["rewalked"]))
    assert g["wrong_guess"] >= 12 and g["no_guess"] + g["wrong_guess"] >= 21, (g["no_guess"], g["wrong_guess"])


def test_block_size_edges_where_the_stream_ends(checker):
    cases = cc.edge_ends()
    assert len(cases) == 42
    want = {"block_size 31": "bad", "block_size 32, 36 bytes": "bad", "block_size 32, 35 bytes": 35, "block_size 32, 4 bytes": 4, "block_size 33, 35 bytes": 35, "block_size 33, 36 bytes": 36, "block_size 33, whole": 0,
            "the last record ends the stream": 0, "the last record lacks a byte": 59, "a byte behind the last record": 1, "three bytes behind the last record": 3, "block_size kBamRecStoreMaxBlock - 1": 77,
            "block_size kBamRecStoreMaxBlock": 77, "block_size kBamRecStoreMaxBlock + 1": "bad"}
    got = cc.run_checker(checker, [(b, 0, cc.N_REF, seg) for _, b in cases for seg in (cc.EDGE_SEG, 64)])
    for k, (name, b) in enumerate(cases):
        w = want[max((p for p in want if name.startswith(p + " ")), key=len)]
        starts, last, bad = cc.walk(b)
        assert (bad, len(b) - last) == ((True, len(b) - last) if w == "bad" else (False, w)), name          # the walk says what the case is named for
        for g, seg in zip(got[2 * k:2 * k + 2], (cc.EDGE_SEG, 64)):
            _hold(g, b, 0, seg, (name, seg))
        if name == "block_size 33, 35 bytes at the segment's first byte":
            # chain_guess needs a record's 36 bytes to call it one the stream cut off: the second of the two segments holds nothing else and has no guess
            assert (got[2 * k]["segments"], got[2 * k]["no_guess"]) == (2, 1)


def test_a_record_the_hints_reject_is_still_a_record(checker):
    """reference ids beyond n_ref and positions below -1 make a record no candidate for a guess; on the chain it counts as any other (hints cost
    time, never a record): such records stand at the first byte of a segment, so the segment's guess is the record behind them"""
    seg = 4096
    parts, at = [], 0
    for k, (tid, pos) in enumerate(((7, 5), (0, -2), (cc.N_REF, 5), (-2, 5))):
        for r in cc.fill((k + 1) * seg - at, 3 + k, most=900):
            parts.append(r)
            at += len(r)
        parts.append(cc.record(60, 50 + k, tid=tid, pos=pos))
        at += 60
    parts += cc.fill(2000, 9)
    buf = b"".join(parts)
    assert cc.walk(buf) == (cc.walk(buf)[0], len(buf), False) and len(cc.walk(buf)[0]) == len(parts)
    got = cc.run_checker(checker, [(buf, 0, cc.N_REF, seg), (buf, 0, -1, seg)])
    for g in got:
        _hold(g, buf, 0, seg, "hints")
        assert g["total"] == len(parts) and g["tail"] == 0
    assert got[0]["wrong_guess"] == 4 and got[1]["wrong_guess"] == 2               # (without n_ref only the two negative fields are told)


def test_block_size_32_is_a_frame_and_no_record():
    """a block of the fixed part alone has no byte for the name's NUL: bam_record.h's frame holds and so does the formatter's rule (name + CIGAR
    inside), the reader's rule (a name of at least one byte) refuses it -- and the chain finder applies the reader's"""
    from test_bam_record import framed
    rec = cc.head(32, 0, b"")
    assert len(rec) == 36 and framed(rec).split()[:4] == ["1", "1", "1", "0"]      # frame, CIGAR inside, fields inside | the reader's rule
    assert cc.walk(rec + cc.record(50, 1)) == ([], 0, True)
    assert framed(cc.head(33)).split()[:5] == ["1", "1", "1", "1", "1"] and cc.walk(cc.head(33)) == ([0], 37, False)


def test_single_byte_mutations_name_the_same_first_malformed_record(checker):
    buf = b"".join(cc.records(300, 9))
    rng = random.Random(41)
    cases = []
    for _ in range(2000):
        m = bytearray(buf)
        at = rng.randrange(len(m))
        m[at] ^= 1 << rng.randrange(8) if rng.random() < 0.5 else rng.randrange(1, 256)
        cases.append((bytes(m), 0, cc.N_REF, rng.choice((64, 256, 4096))))
    got = cc.run_checker(checker, cases)
    seen = set()
    for g, (b, _, _, seg) in zip(got, cases):
        _hold(g, b, 0, seg, "mutation")
        seen.add("bad" if g["first_malformed"] >= 0 else "cut" if g["tail"] else "whole")
    assert seen == {"bad", "cut", "whole"}
