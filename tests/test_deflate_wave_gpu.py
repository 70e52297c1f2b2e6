"""psvr_bgzf_compress_members on the device: its bytes are the bytes of the encoder's host build (tests/tools/deflate_wave_check.cpp),
member for member; zlib and the device's own decoder give the input back; one large call; the commands with --deflate-device."""
import bisect
import glob
import gzip
import os
import struct
import subprocess
import tempfile
import zlib
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

import aln_common as ac
import bam_reader
import deflate_wave_cases as dc
import inflate_cases as ic
import test_bam_sort as tbs

pytestmark = pytest.mark.gpu
CLI = tbs.CLI
FALLBACK_LINE = "BGZF on the device failed"


@pytest.fixture(scope="module")
def checker():
    return dc.build_checker(tempfile.mkdtemp(prefix="psvr_dfw_"), False)


@pytest.fixture(scope="module")
def records():
    return dc.fx2_records()


@pytest.mark.parametrize("member_bytes", dc.MEMBER_SIZES)
def test_device_bytes_equal_host_bytes(checker, records, member_bytes):
    from pansvr_amd.bgzf import bgzf_compress, bgzf_decompress
    for name, data in dc.cases(member_bytes, records):
        out, offs = bgzf_compress(data, member_bytes)
        raw = out.tobytes()
        want = dc.host_members(checker, data, member_bytes)
        ms = dc.check_members(raw, data, member_bytes)                          # zlib inflates them
        sizes = [len(m) for m in ic.split_members(want)] if want else []
        assert list(offs) == [sum(sizes[:i]) for i in range(len(sizes) + 1)], name
        assert [len(m) for m in ms] == sizes, name
        assert raw == want, name
        if data:                                                               # and so does the device's decoder
            back, boffs, used = bgzf_decompress(raw)
            assert used == len(raw) and back.tobytes() == data, name
            assert list(boffs) == [min(i * member_bytes, len(data)) for i in range(len(ms) + 1)], name


def test_random_bytes_come_out_stored(records):
    from pansvr_amd.bgzf import bgzf_compress
    data = dict(dc.cases(0xff00, records))["random"]
    out, offs = bgzf_compress(data, 0xff00)
    ms = ic.split_members(out.tobytes())
    assert len(ms[0]) == 0xff00 + 31 and ms[0][18] == 1                         # BFINAL = 1, BTYPE = 00
    assert all(len(m) <= 65536 for m in ms)


def test_one_256_mb_call_then_a_small_one():
    from pansvr_amd.bgzf import bgzf_compress
    n = 256 << 20
    data = ic.bam_like_big(n, 31)
    out, offs = bgzf_compress(data)
    nm = (n + 0xff00 - 1) // 0xff00
    assert len(offs) == nm + 1 and offs[0] == 0 and offs[-1] == len(out)
    raw = out.tobytes()

    def inflate(i):
        m = raw[offs[i]:offs[i + 1]]
        assert len(m) <= 65536 and (m[16] | m[17] << 8) + 1 == len(m)
        return zlib.decompress(m, 31)
    with ThreadPoolExecutor(16) as ex:
        parts = list(ex.map(inflate, range(nm)))
    assert b"".join(parts) == data
    print("256 MB: %d members, %d bytes, ratio %.3f" % (nm, len(raw), n / len(raw)))
    small = ic.bam_like(5000, 2)
    out, offs = bgzf_compress(small, 4096)
    assert list(offs[:1]) == [0] and len(offs) == 3
    dc.check_members(out.tobytes(), small, 4096)


# ---- the commands ------------------------------------------------------------------------------------------------------------------------------


def _run(cmd, **env):
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=dict(os.environ, **env), timeout=900)
    assert r.returncode == 0, r.stderr.decode()[-2000:]
    return r.stderr.decode()


def test_aln_deflate_device_writes_the_default_routes_streams():
    w = ac.workdir("fx2")
    tmp = tempfile.mkdtemp(prefix="psvr_dfwc_")
    base = [ac.index_dir("fx2"), os.path.join(w, "reads150.fq"), os.path.join(w, "header.sam")]
    _run([CLI, "aln", "-o", os.path.join(tmp, "out.bam"), "-p", os.path.join(tmp, "ori.bam")] + base)
    err = _run([CLI, "aln", "--deflate-device", "-o", os.path.join(tmp, "outd.bam"), "-p", os.path.join(tmp, "orid.bam")] + base, PSVR_BGZF_DEVICE_MIN_BLOCKS="1")
    assert FALLBACK_LINE not in err
    for a, b in (("out", "outd"), ("ori", "orid")):
        fa, fb = os.path.join(tmp, a + ".bam"), os.path.join(tmp, b + ".bam")
        assert bam_reader.check_bgzf(fb) >= 1
        assert gzip.open(fb, "rb").read() == gzip.open(fa, "rb").read()
    assert open(os.path.join(tmp, "outd.bam"), "rb").read() != open(os.path.join(tmp, "out.bam"), "rb").read()   # (not zlib's members: the device made them)


def _members(path):
    """[(file offset, inflated bytes)] of every member but the EOF block, which must be there; every member within 64 KB"""
    data = open(path, "rb").read()
    assert data[-28:] == bytes([0x1f, 0x8b, 8, 4, 0, 0, 0, 0, 0, 0xff, 6, 0, 0x42, 0x43, 2, 0, 0x1b, 0, 3, 0, 0, 0, 0, 0, 0, 0, 0, 0])
    out, at = [], 0
    while at < len(data) - 28:
        m = data[at:at + struct.unpack_from("<H", data, at + 16)[0] + 1]
        assert len(m) <= 65536
        piece = ic.oracle(m)
        assert piece is not None and len(piece) <= 0xff00, at
        out.append((at, piece))
        at += len(m)
    assert at == len(data) - 28
    return out


def _check_sorted_with_index(path, default_path):
    """the inflated payload is the default route's; every chunk of the .bai starts and ends at a record boundary; region queries through the
    .bai find what a scan of the records finds"""
    mem = _members(path)
    stream = b"".join(p for _, p in mem)
    assert stream == gzip.open(default_path, "rb").read()
    # the records: (virtual offset of the start, tid, pos, end, name)
    l_text = struct.unpack_from("<i", stream, 4)[0]
    at = 8 + l_text
    n_ref = struct.unpack_from("<i", stream, at)[0]
    at += 4
    for _ in range(n_ref):
        at += 8 + struct.unpack_from("<i", stream, at)[0]
    starts, ustart = [], 0
    for c, p in mem:
        starts.append((ustart, c))
        ustart += len(p)

    def voff(u):
        i = bisect.bisect_right(starts, (u, 1 << 62)) - 1
        return starts[i][1] << 16 | (u - starts[i][0])
    recs, bound = [], {}
    while at < len(stream):
        bs = struct.unpack_from("<i", stream, at)[0]
        tid, pos, l_rn, _, _, n_cig, flag = struct.unpack_from("<iiBBHHH", stream, at + 4)
        cig = struct.unpack_from("<%dI" % n_cig, stream, at + 36 + l_rn)
        rlen = sum(c >> 4 for c in cig if (c & 15) in (0, 2, 3, 7, 8)) or 1
        bound[voff(at)] = len(recs)
        recs.append((tid, pos, pos + rlen, stream[at + 36:at + 36 + l_rn - 1], flag))
        at += 4 + bs
    assert at == len(stream)
    bound[voff(at)] = len(recs)
    if mem and at - starts[-1][0] == len(mem[-1][1]):                           # the end of the data may also be named as the end of the last member
        bound[starts[-1][1] << 16 | len(mem[-1][1])] = len(recs)
    bound[(os.path.getsize(path) - 28) << 16] = len(recs)                      # ... or as the EOF block
    bai = open(path + ".bai", "rb").read()
    assert bai[:4] == b"BAI\x01" and struct.unpack_from("<i", bai, 4)[0] == n_ref
    off, index, n_chunks = 8, [], 0
    for _ in range(n_ref):
        n_bin = struct.unpack_from("<i", bai, off)[0]
        off += 4
        bins = {}
        for _ in range(n_bin):
            b, n_chunk = struct.unpack_from("<Ii", bai, off)
            off += 8
            bins[b] = [struct.unpack_from("<QQ", bai, off + 16 * k) for k in range(n_chunk)]
            off += 16 * n_chunk
        n_intv = struct.unpack_from("<i", bai, off)[0]
        lin = list(struct.unpack_from("<%dQ" % n_intv, bai, off + 4))
        off += 4 + 8 * n_intv
        index.append((bins, lin))
        for b, chunks in bins.items():
            if b == 37450:
                continue
            for vb, ve in chunks:
                assert vb in bound and ve in bound and bound[vb] < bound[ve], (b, vb, ve)
                n_chunks += 1
        for v in lin:
            assert v == 0 or v in bound
    assert off + 8 == len(bai)
    rng = np.random.RandomState(9)
    placed = [r for r in recs if r[0] >= 0]
    n_hits = 0
    for q in range(40):
        tid, pos = placed[int(rng.randint(len(placed)))][:2] if placed else (0, 0)
        beg = max(0, pos - int(rng.choice([0, 50, 3000])))
        end = beg + int(rng.choice([1, 200, 5000, 1000000]))
        bins, lin = index[tid]
        want_bins = [0]
        for shift, base in ((26, 1), (23, 9), (20, 73), (17, 585), (14, 4681)):
            want_bins += list(range(base + (beg >> shift), base + ((end - 1) >> shift) + 1))
        lo = lin[beg >> 14] if (beg >> 14) < len(lin) else (lin[-1] if lin else 0)
        got = []
        for b in want_bins:
            for vb, ve in bins.get(b, []):
                if ve <= lo:
                    continue
                got += [r for r in recs[bound[vb]:bound[ve]] if r[0] == tid and r[1] < end and r[2] > beg]
        want = [r for r in recs if r[0] == tid and r[1] < end and r[2] > beg]
        assert sorted(got) == sorted(want), (tid, beg, end, len(got), len(want))
        n_hits += len(want)
    return len(recs), n_chunks, n_hits


@pytest.mark.parametrize("bam", sorted(glob.glob(os.path.join(ac.HERE, "golden", "fused", "*.bam"))), ids=os.path.basename)
def test_sort_deflate_device(bam, tmp_path):
    d, s = str(tmp_path / "default.bam"), str(tmp_path / "device.bam")
    _run([CLI, "sort", "-o", d, bam])
    err = _run([CLI, "sort", "--deflate-device", "-o", s, bam])
    assert FALLBACK_LINE not in err
    n, n_chunks, n_hits = _check_sorted_with_index(s, d)
    assert n > 0 and n_chunks > 0 and n_hits > 0
    assert open(s, "rb").read() != open(d, "rb").read()


def test_aln_sort_deflate_device(tmp_path):
    w = ac.workdir("fx2")
    base = [ac.index_dir("fx2"), os.path.join(w, "reads150.fq"), os.path.join(w, "header.sam")]
    d, s = str(tmp_path / "default.bam"), str(tmp_path / "device.bam")
    _run([CLI, "aln", "--sort", "-o", d, "-p", str(tmp_path / "p.bam")] + base)
    err = _run([CLI, "aln", "--sort", "--deflate-device", "-o", s, "-p", str(tmp_path / "pd.bam")] + base, PSVR_BGZF_DEVICE_MIN_BLOCKS="1")
    assert FALLBACK_LINE not in err
    n, n_chunks, n_hits = _check_sorted_with_index(s, d)
    assert n > 100 and n_chunks > 0 and n_hits > 0
    assert gzip.open(str(tmp_path / "pd.bam"), "rb").read() == gzip.open(str(tmp_path / "p.bam"), "rb").read()
    assert bam_reader.check_bgzf(str(tmp_path / "pd.bam")) >= 1
