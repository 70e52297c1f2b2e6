"""-m gpu: the wavefront BGZF encoder's efforts on the MI355X.  psvr_bgzf_compress_members_effort's bytes are the bytes of the encoder's host
build (tests/tools/deflate_effort_check.cpp) at every effort and member size, effort 0's are psvr_bgzf_compress_members'; a device stream
at an effort makes the one-call result however appends and takes fall, and a changed effort applies from the next take; the commands
with --deflate-effort 2 write the data of effort 0 in smaller, valid files."""
import ctypes as C
import gzip
import json
import os
import re
import tempfile

import numpy as np
import pytest

import aln_common as ac
import bam_reader
import deflate_effort_cases as de
import deflate_wave_cases as dc
import inflate_cases as ic
from test_deflate_wave_gpu import CLI, FALLBACK_LINE, _check_sorted_with_index, _members, _run

pytestmark = pytest.mark.gpu
PSVR_ERR_ARG = 1


@pytest.fixture(scope="module")
def checker():
    return de.build_checker(tempfile.mkdtemp(prefix="psvr_dfeg_"), False)


@pytest.fixture(scope="module")
def records():
    return dc.fx2_records()


@pytest.fixture(scope="module")
def crafted():
    return de.crafted()


def _effort_call(data, member_bytes, effort):
    """psvr_bgzf_compress_members_effort as it stands in the ABI: (status, the members' bytes)"""
    from pansvr_amd import lib
    L = lib()
    L.psvr_bgzf_members_bound.restype = C.c_int64
    buf = np.frombuffer(bytes(data), dtype=np.uint8)
    cap = L.psvr_bgzf_members_bound(C.c_int64(len(buf)), C.c_int32(member_bytes))
    out = np.empty(cap, dtype=np.uint8)
    total = C.c_int64(0)
    rc = L.psvr_bgzf_compress_members_effort(C.c_int(0), buf.ctypes.data_as(C.c_void_p), C.c_int64(len(buf)), C.c_int32(member_bytes), out.ctypes.data_as(C.c_void_p),
                                             C.c_int64(cap), C.byref(total), None, C.c_int64(0), None, C.c_int32(effort))
    return rc, out[:total.value].tobytes()


@pytest.mark.parametrize("member_bytes", dc.MEMBER_SIZES)
@pytest.mark.parametrize("effort", de.EFFORTS)
def test_device_bytes_equal_host_bytes(checker, records, crafted, effort, member_bytes):
    from pansvr_amd.bgzf import bgzf_compress
    for name, data in dc.cases(member_bytes, records) + crafted:
        out, offs = bgzf_compress(data, member_bytes, effort=effort)
        raw = out.tobytes()
        want = de.host_members(checker, data, member_bytes, effort)
        sizes = [len(m) for m in ic.split_members(want)] if want else []
        assert list(offs) == [sum(sizes[:i]) for i in range(len(sizes) + 1)], name
        assert raw == want, name
        dc.check_members(raw, data, member_bytes)                               # zlib inflates them
        if effort == 0 and data:                                               # the new entry point at effort 0 is the old one
            assert _effort_call(data, member_bytes, 0) == (0, raw), name


def test_an_effort_outside_0_to_3_is_an_argument_error():
    from pansvr_amd import lib
    from pansvr_amd._lib import EngineError
    from pansvr_amd.bgzf import BgzfStream, bgzf_compress
    data = ic.bam_like(5000, 2)
    for effort in (4, -1):
        assert _effort_call(data, 4096, effort) == (PSVR_ERR_ARG, b"")
        assert b"effort" in lib().psvr_last_error()
    with pytest.raises(EngineError, match="psvr error 1"):
        bgzf_compress(data, 4096, effort=4)
    s = BgzfStream(4096)
    with pytest.raises(EngineError, match="psvr error 1"):
        s.set_effort(4)
    s.append(data)                                                             # the stream is as it was: at effort 0
    out, offs, used = s.take(finish=True)
    assert out.tobytes() == bgzf_compress(data, 4096)[0].tobytes()
    s.close()


@pytest.mark.parametrize("member_bytes", [256, 4096, 0xff00])
def test_stream_at_effort_2_equals_the_one_call_result(checker, member_bytes):
    from pansvr_amd.bgzf import BgzfStream, bgzf_compress
    mb = member_bytes
    lengths = [0, 1, mb - 1, mb, mb + 1, 3 * mb + 1, 0, mb - 1]
    data = ic.bam_like(sum(lengths), 17)
    bufs, at = [], 0
    for n in lengths:
        bufs.append(data[at:at + n])
        at += n
    want = bgzf_compress(data, mb, effort=2)[0].tobytes()
    assert want == de.host_members(checker, data, mb, 2)
    for name, takes in (("after every append", set(range(len(bufs)))), ("only at the end", set()), ("at two places", {2, 5})):
        for at_create in (True, False):
            s = BgzfStream(mb, effort=2) if at_create else BgzfStream(mb)
            if not at_create:
                s.set_effort(2)
            got = b""
            for i, b in enumerate(bufs):
                s.append(b)
                if i in takes:
                    got += s.take()[0].tobytes()
            got += s.take(finish=True)[0].tobytes()
            assert s.pending == 0 and got == want, (name, at_create)
            s.close()


def test_a_changed_effort_applies_from_the_next_take(checker):
    from pansvr_amd.bgzf import BgzfStream
    mb = 4096
    data = ic.bam_like(5 * mb + 100, 23)
    host = {e: ic.split_members(de.host_members(checker, data, mb, e)) for e in (0, 2, 3)}
    assert host[0][:2] != host[2][:2] and host[2][2:4] != host[3][2:4] and host[3][4:] != host[0][4:]   # (the efforts differ on these bytes)
    s = BgzfStream(mb)
    s.append(data[:2 * mb + 50])
    a = s.take()[0].tobytes()                                                  # members 0, 1 at effort 0
    s.set_effort(2)                                                            # what is pending is compressed at the effort of its take, not of its append
    s.append(data[2 * mb + 50:4 * mb + 7])
    b = s.take()[0].tobytes()                                                  # members 2, 3 at effort 2
    s.append(data[4 * mb + 7:])
    s.set_effort(3)
    c = s.take(finish=True)[0].tobytes()                                       # members 4, 5 at effort 3
    s.close()
    assert a == b"".join(host[0][:2]) and b == b"".join(host[2][2:4]) and c == b"".join(host[3][4:])
    dc.check_members(a + b + c, data, mb)


# ---- the commands ------------------------------------------------------------------------------------------------------------------------------
def _e2e(err):
    return json.loads(re.search(r"e2e_json (\{.*\})", err).group(1))


def _smaller_and_the_same(lo, hi):
    """file `hi` (the higher effort) holds the payload of `lo` in valid members and fewer bytes"""
    assert b"".join(p for _, p in _members(hi)) == gzip.open(lo, "rb").read()
    assert bam_reader.check_bgzf(hi) >= 1
    assert os.path.getsize(hi) < os.path.getsize(lo), (os.path.getsize(hi), os.path.getsize(lo))


@pytest.mark.parametrize("route", ["--deflate-device", "--stream-device", "--sort-device"])
def test_aln_deflate_effort(route, tmp_path):
    w = ac.workdir("fx2")
    base = [ac.index_dir("fx2"), os.path.join(w, "reads150.fq"), os.path.join(w, "header.sam")]
    f = {k: str(tmp_path / (k + ".bam")) for k in ("o0", "p0", "o2", "p2")}
    err0 = _run([CLI, "aln", route, "-o", f["o0"], "-p", f["p0"]] + base, PSVR_BGZF_DEVICE_MIN_BLOCKS="1")
    err2 = _run([CLI, "aln", route, "--deflate-effort", "2", "-o", f["o2"], "-p", f["p2"]] + base, PSVR_BGZF_DEVICE_MIN_BLOCKS="1")
    for err in (err0, err2):
        assert FALLBACK_LINE not in err and " failed (" not in err, err[-2000:]                # (no route was left for the host)
    assert _e2e(err0)["deflate_effort"] == 0 and _e2e(err2)["deflate_effort"] == 2
    _smaller_and_the_same(f["o0"], f["o2"])
    assert gzip.open(f["p2"], "rb").read() == gzip.open(f["p0"], "rb").read()   # the ori file goes through the members call on every route
    assert bam_reader.check_bgzf(f["p2"]) >= 1 and os.path.getsize(f["p2"]) <= os.path.getsize(f["p0"])
    if route == "--sort-device":
        n, n_chunks, n_hits = _check_sorted_with_index(f["o2"], f["o0"])
        assert n > 100 and n_chunks > 0 and n_hits > 0


@pytest.mark.parametrize("route", ["--deflate-device", "--sort-device", "--nsort-device"])
def test_sort_deflate_effort(route, tmp_path):
    bam = os.path.join(ac.golden_dir("fx2"), "reads150.bam")
    s0, s2 = str(tmp_path / "s0.bam"), str(tmp_path / "s2.bam")
    err0 = _run([CLI, "sort", route, "-o", s0, bam])
    err2 = _run([CLI, "sort", route, "--deflate-effort", "2", "-o", s2, bam])
    for err in (err0, err2):
        assert FALLBACK_LINE not in err and " failed (" not in err, err[-2000:]                # (no route was left for the host)
    _smaller_and_the_same(s0, s2)
    if route == "--nsort-device":
        assert not os.path.exists(s2 + ".bai")
    else:
        n, n_chunks, n_hits = _check_sorted_with_index(s2, s0)
        assert n > 100 and n_chunks > 0 and n_hits > 0
