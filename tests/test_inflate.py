"""The one-wavefront-per-member BGZF decoder behind psvr_bgzf_decompress (pansvr_amd/csrc/inflate_device.h), compiled for the host
(tests/tools/inflate_check.cpp) twice: -O2, and -O1 with AddressSanitizer + UBSan where every member and every output slice lives in a heap
block of exactly its size.  Valid members must give zlib's bytes; malformed ones zlib's verdict, without a report from the sanitizer."""
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


def test_each_failure_class_by_hand(asan_checker):
    cases = ic.hand_bad()
    assert len(cases) >= 35
    for name, m, accepted in cases:
        assert (ic.oracle(m) is not None) == accepted, name
    got = ic.run_checker(asan_checker, [c[1] for c in cases])
    for (name, m, accepted), (status, out) in zip(cases, got):
        assert (status == 0) == accepted, "%s: status %d" % (name, status)
        if accepted:
            assert out == ic.oracle(m), name


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
