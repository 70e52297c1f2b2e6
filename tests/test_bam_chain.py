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
