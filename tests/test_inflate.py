"""The one-wavefront-per-member BGZF decoder behind psvr_bgzf_decompress (pansvr_amd/csrc/inflate_device.h), compiled for the host
(tests/tools/inflate_check.cpp) twice: -O2, and -O1 with AddressSanitizer + UBSan where every member and every output slice lives in a heap
block of exactly its size.  Valid members must give zlib's bytes; malformed ones zlib's verdict, without a report from the sanitizer; and a
member made by hand for one rule (inflate_cases.hand_bad, rule_edges) the status of that rule, not merely a refusal: most of them carry the
trailer of the data they were meant to hold, which would refuse them whatever the decoder did (tools/mutants.py keeps the evidence)."""
import os
import struct
import tempfile
import zlib

import pytest

import inflate_cases as ic


@pytest.fixture(scope="module")
def tmp():
    return tempfile.mkdtemp(prefix="psvr_inflate_")


@pytest.fixture(scope="module", params=["O2", "asan"])
def checker(request, tmp):
    return ic.build_checker(tmp, request.param == "asan")


@pytest.fixture(scope="module")
def asan_checker(tmp):
    return ic.build_checker(tmp, True)


def expect_bytes(checker, members, datas):
    got = ic.run_checker(checker, members)
    for k, ((status, out), want) in enumerate(zip(got, datas)):
        assert status == 0, "member %d: status %d" % (k, status)
        assert out == want, "member %d: bytes differ" % k


def test_golden_bam_members(checker):
    files = ic.golden_bams()
    assert len(files) == 36
    members = ic.golden_members()
    datas = [ic.oracle(m) for m in members]
    assert all(d is not None for d in datas)
    kinds = [(m[18] >> 1) & 3 for m in members]
    assert len(members) == 362 and kinds.count(2) == 326 and kinds.count(1) == 36
    assert sum(len(d) for d in datas) > 17 * 10 ** 6 and max(len(d) for d in datas) == 65269
    expect_bytes(checker, members, datas)


def test_zlib_levels_strategies_sizes_and_flushes(checker):
    cases = ic.zlib_members()
    names = [c[0] for c in cases]
    for must in ("bam-65536-l6", "equal-65280-l0", "equal-65536-l6", "equal-65536-rle", "random-65280-l0", "random-0-l0", "bam-1-fixed", "random-2-huffman", "bam-65280-l1", "bam-65280-l9",
                 "bam-65280-fixed", "bam-65280-huffman", "bam-65280-rle", "flush-sync-8", "flush-full-4", "mixed-l6"):
        assert must in names, must
    assert len(cases) >= 95
    for name, m, data in cases:
        assert ic.oracle(m) == data, name
    expect_bytes(checker, [c[1] for c in cases], [c[2] for c in cases])


def test_members_of_this_repositorys_encoder(checker, tmp):
    members, data = ic.own_encoder_members(tmp)
    datas = [data[i * 16384:(i + 1) * 16384] for i in range(len(members))]
    for m, d in zip(members, datas):
        assert ic.oracle(m) == d
    expect_bytes(checker, members, datas)


def test_streams_zlib_never_emits(checker):
    cases = ic.hand_valid()
    assert len(cases) >= 7
    for name, m, data in cases:
        assert ic.oracle(m) == data, name
    expect_bytes(checker, [c[1] for c in cases], [c[2] for c in cases])


def same_verdict(checker, bufs):
    got = ic.run_checker(checker, bufs)
    accepted = 0
    for k, (buf, (status, out)) in enumerate(zip(bufs, got)):
        want = ic.oracle(buf)
        assert (status == 0) == (want is not None), "case %d: status %d, zlib %s" % (k, status, "accepts" if want is not None else "refuses")
        if want is not None:
            assert out == want, "case %d: bytes differ" % k
            accepted += 1
    return accepted


STATUSES = ("kInfOk", "kInfHeader", "kInfBlockType", "kInfStored", "kInfTruncated", "kInfCounts", "kInfCodeLengths", "kInfNoEob", "kInfLitTable", "kInfDistTable", "kInfLitCode",
            "kInfDistCode", "kInfFarBack", "kInfTooLong", "kInfTooShort", "kInfCrc")


def test_constants_are_printed(checker, asan_checker):
    k = ic.constants(checker)
    assert k == ic.constants(asan_checker)
    assert set(k) == set(STATUSES) and k["kInfOk"] == 0 and len(set(k.values())) == len(STATUSES)


def named_status(checker, cases):
    """every member gets the status its case names -- not merely a refusal -- and an accepted one holds zlib's bytes"""
    k = ic.constants(checker)
    got = ic.run_checker(checker, [c[1] for c in cases])
    for (name, m, want), (status, out) in zip((c[:3] for c in cases), got):
        assert status == k[want], "%s: status %d, not %s = %d" % (name, status, want, k[want])
        if status == 0:
            assert out == ic.oracle(m), name


def test_each_failure_class_by_hand(checker):
    cases = ic.hand_bad()
    assert len(cases) >= 35
    for name, m, status in cases:
        assert (ic.oracle(m) is not None) == (status == "kInfOk"), name
    # every status but kInfHeader, which is not the decoder's to find (bgzf_member_header comes first: test_500_header_mutations)
    assert {c[2] for c in cases} == set(STATUSES) - {"kInfHeader"}
    named_status(checker, cases)


def test_each_rule_at_its_edge(checker):
    """zlib decides what is inside: an inside member is one zlib inflates to the bytes the case was built from"""
    cases = ic.rule_edges()
    assert len(cases) >= 100
    for name, m, status, data in cases:
        assert (status == "kInfOk") == (data is not None), name
        assert ic.oracle(m) == data, name                                       # (None: zlib refuses, or the trailer does not fit what zlib made)
        if data is None and not name.startswith("isize-"):                      # ... and for every rule but ISIZE it is zlib's inflate that refuses
            h = ic.header_rules(m)
            with pytest.raises(zlib.error):
                d = zlib.decompressobj(-15)
                d.decompress(m[12 + h[1]:h[0] - 8])
                if not d.eof:
                    raise zlib.error("the stream does not end")
    kinds = {n.rsplit("/", 1)[1] for n, _, s, _ in cases if s != "kInfOk"}
    assert kinds == {"trailer", "forged"}
    forged = [c for c in cases if c[0].endswith("/forged")]
    assert len(forged) >= 40 and all(struct.unpack("<I", c[1][-4:])[0] == ic.FORGED_ISIZE for c in forged)
    assert {c[2] for c in cases} >= set(STATUSES) - {"kInfHeader", "kInfTooShort"}
    named_status(checker, cases)


def test_inf_member_holds_its_caller_to_the_layout(checker):
    """inf_member as a caller with a layout of its own would call it (hdr, bsize and the slice's size are arguments): a member that has no room
    for its header and trailer is kInfHeader before a byte of it is read, and a slice of the right size under a trailer that names another is
    kInfTooShort"""
    k = ic.constants(checker)
    m = ic.wrap(ic.deflate(b"abc"), b"abc")
    empty = m[:18] + m[-8:]                                                    # header and trailer, nothing between
    lying = m[:-4] + struct.pack("<I", 4)
    cases = [(18, 3, m, "kInfOk"), (18, 0, empty, "kInfTruncated"), (18, 0, empty[:-1], "kInfHeader"), (18, 0, empty[:8], "kInfHeader"), (12, 3, m[:12] + m[18:], "kInfOk"),
             (11, 3, m[:11] + m[18:], "kInfHeader"), (0, 3, m[18:], "kInfHeader"), (18, 3, lying, "kInfTooShort"), (18, 4, lying, "kInfTooShort"), (18, 3, m[:-4] + struct.pack("<I", 2), "kInfTooShort"), (18, 2, m, "kInfTooLong")]
    got = ic.run_checker(checker, [struct.pack("<II", hdr, isize) + mem for hdr, isize, mem, _ in cases], direct=True)
    for (hdr, isize, mem, want), (status, out) in zip(cases, got):
        assert status == k[want], (hdr, isize, len(mem), status, want)
        assert out is None or out == b"abc"


def test_every_truncation_point(asan_checker):
    bufs = ic.truncations()
    assert len(bufs) > 600
    same_verdict(asan_checker, bufs)


def test_2000_payload_and_trailer_mutations(asan_checker):
    bufs = ic.payload_mutations(ic.golden_members())
    assert len(bufs) == 2000
    accepted = same_verdict(asan_checker, bufs)
    assert 0 < accepted < 2000          # both verdicts occur (slack bits behind the end-of-block code)


def test_500_header_mutations(asan_checker):
    bufs = ic.header_mutations(ic.golden_members())
    assert len(bufs) == 500
    accepted = same_verdict(asan_checker, bufs)
    assert 0 < accepted < 500


def test_entry_point_sizes_without_a_device():
    """out == NULL: the two sizes, no device needed (with an output buffer and no GPU: PSVR_ERR_DEVICE, the next test)."""
    from pansvr_amd import bgzf
    members = ic.golden_members()[:7]
    datas = [ic.oracle(m) for m in members]
    buf = b"".join(members)
    assert bgzf.bgzf_sizes(buf) == (len(buf), sum(len(d) for d in datas), 7)
    assert bgzf.bgzf_sizes(buf + members[0][:100]) == (len(buf), sum(len(d) for d in datas), 7)      # a cut-off member is the caller's to complete
    assert bgzf.bgzf_sizes(b"") == (0, 0, 0)
    with pytest.raises(bgzf.BgzfError) as e:
        bgzf.bgzf_sizes(buf + b"\x1f\x8b\x08\x00" + bytes(40))
    assert e.value.bad_member == 7 and "member 7 at byte %d" % len(buf) in str(e.value)


def test_entry_point_without_a_device_is_loud():
    from pansvr_amd import EngineError, bgzf, lib
    if lib().psvr_device_count() > 0:
        pytest.skip("a HIP device is visible: PSVR_ERR_DEVICE cannot be provoked here")
    with pytest.raises(EngineError) as e:
        bgzf.bgzf_decompress(b"".join(ic.golden_members()[:7]))
    assert "psvr error 3" in str(e.value) and "no HIP device" in str(e.value)
