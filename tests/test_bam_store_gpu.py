"""-m gpu: the device-resident record store (psvr_bam_store_*, pansvr_amd.sort.BamStore) and `panSVR aln --sort-device` on the MI355X.
The yardstick of the table is a plain Python restatement of samtools' key, the CIGAR's reference span and the bin, and a stable argsort; the
payload is also held to `panSVR sort` on a BAM of the same records; records appended from an emitter are held to the emitter's own download
put through the same restatement; the command is held to the three files of `aln --sort --deflate-device`, byte for byte."""
import contextlib
import gzip
import os
import random
import struct
import subprocess
import tempfile

import numpy as np
import pytest

import aln_common as ac
import bam_emit_cases as bc
import bam_stream
import fastq_cases as fc
import test_signal as ts
from test_bam_emit_gpu import _aln, _e2e, _with_tabs, fx1  # noqa: F401  (fx1: index, parser and emitter of golden set fx1)

pytestmark = pytest.mark.gpu
CLI = ts.CLI
REFS = [("chr1", 250000000), ("chr2", 250000000), ("chr3", 250000000)]


# ---- the restatement ---------------------------------------------------------------------------------------------------------------------------------
def reg2bin(beg, end):
    end -= 1
    for shift, first in ((14, 4681), (17, 585), (20, 73), (23, 9), (26, 1)):
        if beg >> shift == end >> shift:
            return first + (beg >> shift)
    return 0


def restate(rec):
    """(key, tid, pos, end, len, bin, flag) of one record (block_size first)"""
    bs, tid, pos, l_qname = struct.unpack_from("<IiiB", rec, 0)
    n_cig, flag = struct.unpack_from("<HH", rec, 16)
    span = 0
    for k in range(n_cig):
        c, = struct.unpack_from("<I", rec, 36 + l_qname + 4 * k)
        if c & 15 in (0, 2, 3, 7, 8):
            span += c >> 4
    span = span or 1
    beg = max(pos, 0)
    key = ((tid & 0xffffffff) << 32) | ((((pos & 0xffffffff) + 1) << 1) & 0xffffffff) | ((flag >> 4) & 1)
    return key, tid, pos, beg + span, 4 + bs, reg2bin(beg, beg + span) & 0xffff, flag       # (the record's bin field has 16 bits: a position beyond 2^29 keeps the low ones)


def with_bin(rec, b):
    return rec[:14] + struct.pack("<H", b) + rec[16:]


def make_record(length, tid, pos, flag, cigar, seed):
    """a record of exactly `length` bytes: a name (empty at 36 bytes), as much of `cigar` as fits, then bytes that are nobody's business"""
    room = length - 36
    n_cig = min(len(cigar), max(0, (room - 1) // 4))
    l_qname = 0 if room == 0 else min(room - 4 * n_cig, 1 + seed % 9)
    rng = random.Random(seed)
    name = bytes(rng.randrange(33, 127) for _ in range(max(l_qname - 1, 0))) + (b"\0" if l_qname else b"")
    cg = b"".join(struct.pack("<I", n << 4 | op) for n, op in cigar[:n_cig])
    rest = bytes(rng.randrange(256) for _ in range(min(room - l_qname - 4 * n_cig, 64)))
    rest += bytes(room - l_qname - 4 * n_cig - len(rest))
    body = struct.pack("<iiBBHHHiiii", tid, pos, l_qname, 60, 4680, n_cig, flag, 0, -1, -1, 0) + name + cg + rest
    assert len(body) + 4 == length
    return struct.pack("<I", len(body)) + body


SPANS = ([], [(1, 0)], [(100, 0)], [(20000, 0)], [(90, 0), (200000, 2)], [(10, 4), (2000000, 3), (5, 0)], [(100000000, 0)], [(7, 1), (9, 4)], [(30, 7), (40, 8)])


def make_records(n, seed, shortest=36):
    """n records of lengths shortest..99 in turn (every residue of a source and a destination address modulo 16, every head and tail), positions drawn
    from few values (ties, reverse-strand ties), unplaced records (tid -1 / pos -1: last), records without a CIGAR and CIGARs whose span
    moves the bin across the levels; from 2047 records on, one of 70 000 bytes (longer than a BGZF member)"""
    rng = random.Random(seed)
    recs = []
    for i in range(n):
        length = shortest + i % (100 - shortest)
        unplaced = rng.randrange(17) == 0
        tid, pos = (-1, -1) if unplaced else (rng.randrange(3), rng.choice((0, 16383, 16384, 131071, 1 << 20, (1 << 26) - 1, rng.randrange(300))))
        flag = (rng.randrange(2) << 4) | (4 if unplaced else 0) | (rng.randrange(2) << 6)
        if n >= 2047 and i == n // 3:
            length = 70000
        recs.append(make_record(length, tid, pos, flag, [] if unplaced else rng.choice(SPANS), seed * 100003 + i))
    return recs


def expectation(recs):
    """(records with the recomputed bin, the stable order, the meta rows in that order)"""
    info = [restate(r) for r in recs]
    fixed = [with_bin(r, f[5]) for r, f in zip(recs, info)]
    order = np.argsort(np.array([f[0] for f in info], dtype=np.uint64), kind="stable") if recs else np.zeros(0, dtype=np.int64)
    return fixed, order, info


def check_meta(meta, order, info):
    assert len(meta) == len(order)
    want = np.array([(info[i][3], info[i][1], info[i][2], info[i][4], i, info[i][5], info[i][6]) for i in order], dtype=np.int64).reshape(len(order), 7)
    got = np.stack([meta[k].astype(np.int64) for k in ("end", "tid", "pos", "len", "index", "bin", "flag")], axis=1) if len(order) else want
    bad = np.nonzero((got != want).any(axis=1))[0]
    assert len(bad) == 0, "rank %d: meta %s, the restatement %s" % (bad[0], got[bad[0]], want[bad[0]])
    assert not meta["pad"].any()


@contextlib.contextmanager
def chunk_bytes(n):
    """stores made inside fill chunks of n bytes (PSVR_BAM_STORE_CHUNK_BYTES), so that a few kilobytes of records lie in several"""
    old = os.environ.get("PSVR_BAM_STORE_CHUNK_BYTES")
    if n:
        os.environ["PSVR_BAM_STORE_CHUNK_BYTES"] = str(n)
    try:
        yield
    finally:
        os.environ.pop("PSVR_BAM_STORE_CHUNK_BYTES", None)
        if old is not None:
            os.environ["PSVR_BAM_STORE_CHUNK_BYTES"] = old


def streamed(store, n, window, take_every=0):
    """the inflated takes of the whole store streamed in windows of `window` ranks"""
    from pansvr_amd.bgzf import BgzfStream
    s = BgzfStream()
    out = b""
    for k, a in enumerate(range(0, n, window)):
        store.stream(s, a, min(window, n - a))
        if take_every and k % take_every == take_every - 1:
            out += s.take()[0].tobytes()
    out += s.take(finish=True)[0].tobytes()
    assert s.pending == 0
    s.close()
    return gzip.decompress(out) if out else b""


# ---- 1. appends from the host ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,chunk", [(0, 0), (1, 0), (2, 0), (3, 4096), (2047, 4096), (2048, 0), (2049, 65536), (4 * 2048 + 7, 4096), (4 * 2048 + 7, 0)])
def test_host_appends_meta_stream_and_download(n, chunk):
    from pansvr_amd.sort import BamStore
    recs = make_records(n, 7 + n)
    fixed, order, info = expectation(recs)
    if n > 100:
        assert {len(r) for r in recs} >= set(range(36, 100)) | {70000}
    with chunk_bytes(chunk):
        st = BamStore()
    st.append(b"".join(recs))
    i = st.info()
    assert (i.n_records, i.n_bytes, i.key_exact, i.ordered) == (n, sum(map(len, recs)), 1, 0)
    assert st.download().tobytes() == b"".join(fixed)
    st.order()
    assert st.info().ordered == 1
    check_meta(st.meta(), order, info)
    if n:
        check_meta(st.meta(n // 2, n - n // 2), order[n // 2:], info)
    want = b"".join(fixed[k] for k in order)
    for window, take_every in ((1, 0), (7, 5), (max(n, 1), 0)):
        if window == 1 and n > 2100:
            continue                                                           # (one rank per call is held on the smaller stores)
        got = streamed(st, n, window, take_every)
        assert got == want, "window %d: %s" % (window, bam_stream.first_difference(b"BAM\1\0\0\0\0\0\0\0\0" + got, b"BAM\1\0\0\0\0\0\0\0\0" + want))
    assert st.download().tobytes() == b"".join(fixed)                          # append order still, after the order
    st.close()


def test_split_appends_give_the_same_store():
    from pansvr_amd.sort import BamStore
    n = 2049
    recs = make_records(n, 11)
    fixed, order, info = expectation(recs)
    want = b"".join(fixed[k] for k in order)
    for cuts in ((1,), (64,), (1000, 1001), (n - 1,), (0, 700, 700, n)):
        with chunk_bytes(30000):
            st = BamStore()
        at = 0
        for c in cuts + (n,):
            st.append(b"".join(recs[at:c]))
            at = max(at, c)
        assert st.download().tobytes() == b"".join(fixed), cuts
        st.order()
        check_meta(st.meta(), order, info)
        assert streamed(st, n, 500) == want, cuts
        st.close()


def test_equal_keys_keep_append_order_and_panSVR_sort_agrees(tmp_path):
    """5 000 records sharing one key; then a set that `panSVR sort` can read (every record has a name): its sorted file's records are the stream's"""
    from pansvr_amd.sort import BamStore
    same = [make_record(40 + i % 50, 1, 12345, 16, [(50, 0)], 900000 + i) for i in range(5000)]
    st = BamStore()
    st.append(b"".join(same[:1234])), st.append(b"".join(same[1234:]))
    st.order()
    m = st.meta()
    assert (m["index"] == np.arange(5000)).all()
    fixed = expectation(same)[0]
    assert streamed(st, 5000, 5000) == b"".join(fixed)
    st.close()
    recs = make_records(4 * 2048 + 7, 23, shortest=37)
    fixed, order, info = expectation(recs)
    inp, out = str(tmp_path / "in.bam"), str(tmp_path / "sorted.bam")
    ts.write_bam(inp, recs, REFS)
    r = subprocess.run([CLI, "sort", "-t", "3", "-o", out, inp], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)
    assert r.returncode == 0, r.stderr.decode()
    sorted_recs = bam_stream.split(bam_stream.stream(out))[1]
    with chunk_bytes(1 << 20):
        st = BamStore()
    st.append(b"".join(recs))
    st.order()
    got = streamed(st, len(recs), 3000)
    assert got == b"".join(sorted_recs) == b"".join(fixed[k] for k in order)
    st.close()


# ---- 2. appends from an emitter ------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def emit_checker():
    return bc.build_checker(tempfile.mkdtemp(prefix="psvr_bsto_"), False)


def test_appends_from_the_emitter(emit_checker, fx1):
    from pansvr_amd.aln import CAND_DTYPE, HDR_DTYPE, PAIR_DTYPE
    from pansvr_amd._lib import EngineError
    from pansvr_amd.emit import BamEmitter
    from pansvr_amd.sort import BamStore
    index, n_header, anchors, parser, emitter = fx1
    picked = [c for c in bc.cases(golden=False) if c["name"] in ("1 pairs", "257 pairs", "4097 pairs", "a tab in the comment")]
    assert len(picked) == 4
    for c in picked:
        s_, raw = bc.run_checker(emit_checker, c["text"], c["cls"], c["seed"], c["flags"], n_header=n_header, anchors=anchors)
        w = bc.split_out(raw)
        P = w["P"]
        assert parser.parse(c["text"], fc.BIG_PAIRS, fc.BIG_BASES).n_pairs == P
        arrays = [np.frombuffer(w[k], dtype=dt) for k, dt in (("hdr", HDR_DTYPE), ("pairs", PAIR_DTYPE), ("cands", CAND_DTYPE), ("cigar", np.uint32))]
        emitter.emit_results(parser, *arrays, flags=c["flags"])
        data, off, state = emitter.download()
        rec = data.tobytes()
        between = make_records(40, P, shortest=37)
        rng = random.Random(P)
        a, b = sorted(rng.randrange(P + 1) for _ in range(2))
        # the whole run in three uneven ranges with host appends between them; empty ranges; a single pair; a range of pairs without bytes
        plan = [(0, 0), (0, a), b"".join(between[:13]), (a, b - a), (P, 0), b"".join(between[13:]), (b, P - b), (min(a, P - 1), 1)]
        quiet = next((p for p in range(P) if state[p] != 1), None)
        if quiet is not None:
            q1 = quiet
            while q1 < P and state[q1] != 1:
                q1 += 1
            plan.append((quiet, q1 - quiet))
        with chunk_bytes(max(len(rec), 4096)):                                 # (a run fills a chunk: the next range starts another)
            st = BamStore()
        want = []
        for step in plan:
            if isinstance(step, tuple):
                st.append_emit(emitter, step[0], step[1])
                want += bam_stream.split(b"BAM\1\0\0\0\0\0\0\0\0" + rec[off[step[0]]:off[step[0] + step[1]]])[1]
            else:
                st.append(step)
                want += bam_stream.split(b"BAM\1\0\0\0\0\0\0\0\0" + step)[1]
        fixed, order, info = expectation(want)
        i = st.info()
        assert (i.n_records, i.n_bytes, i.key_exact) == (len(want), sum(map(len, want)), 1), c["name"]
        assert st.download().tobytes() == b"".join(fixed), c["name"]
        st.order()
        check_meta(st.meta(), order, info)
        assert streamed(st, len(want), 100, 3) == b"".join(fixed[k] for k in order), c["name"]
        st.close()
        # ranges outside the run: ordinary refusals, the store as it was
        st = BamStore()
        for first, n in ((1, P), (P + 1, 0), (-1, 1)):
            with pytest.raises(EngineError, match="psvr error 1"):              # PSVR_ERR_ARG
                st.append_emit(emitter, first, n)
        assert st.info().n_records == 0
        st.close()
    fresh = BamEmitter(index)                                                  # an emitter without a run
    st = BamStore()
    with pytest.raises(EngineError, match="no emitted run"):
        st.append_emit(fresh, 0, 0)
    st.close(), fresh.close()


# ---- 3. refusals ----------------------------------------------------------------------------------------------------------------------------------------
def test_refusals_are_ordinary_error_returns():
    from pansvr_amd._lib import EngineError
    from pansvr_amd.bgzf import BgzfStream
    from pansvr_amd.sort import BamStore
    recs = make_records(300, 5)
    fixed = expectation(recs)[0]
    st = BamStore()
    st.append(b"".join(recs))
    good = b"".join(recs[:3])
    malformed = (good[:-1],                                                    # cut off by the end
                 good + struct.pack("<I", 31) + bytes(35),                      # a block_size below 32
                 good + struct.pack("<I", 1000) + bytes(40),                    # a block_size that leaves the stream
                 good + with_cigar_count(make_record(60, 0, 5, 0, [], 1), 100),  # a CIGAR that leaves its record
                 good + bytes(20))                                              # less than a fixed part
    for bad in malformed:
        with pytest.raises(EngineError, match="psvr error 1"):                  # PSVR_ERR_ARG
            st.append(bad)
        assert st.info().n_records == 300
    assert st.download().tobytes() == b"".join(fixed)                          # unchanged
    with pytest.raises(EngineError, match="psvr error 1"):
        st.meta(0, 1)                                                          # not ordered yet
    s = BgzfStream()
    with pytest.raises(EngineError, match="psvr error 1"):
        st.stream(s, 0, 1)
    st.order()
    with pytest.raises(EngineError, match="psvr error 1"):
        st.append(good)                                                        # appends after order
    for first, n in ((0, 301), (301, 0), (-1, 1)):
        with pytest.raises(EngineError, match="psvr error 1"):
            st.stream(s, first, n)
        with pytest.raises(EngineError, match="psvr error 1"):
            st.meta(first, n)
    assert s.pending == 0
    s.close(), st.close()
    # a position the key cannot hold
    st = BamStore()
    st.append(b"".join(recs[:10]) + make_record(50, 0, 0x7fffffff, 0, [], 3))
    assert st.info().key_exact == 0
    with pytest.raises(EngineError, match="psvr error 2"):                      # PSVR_ERR_UNSUPPORTED
        st.order()
    i = st.info()
    assert (i.n_records, i.ordered) == (11, 0)
    assert len(st.download()) == i.n_bytes                                     # and the records can still be had
    st.close()


def with_cigar_count(rec, n_cig):
    return rec[:16] + struct.pack("<H", n_cig) + rec[18:]


# ---- 4. the command --------------------------------------------------------------------------------------------------------------------------------------
def _three_files(o):
    return [open(o + ext, "rb").read() for ext in (".bam", ".bam.bai", ".ori.bam")]


def _no_failure(err):
    assert "failed" not in err, err[-2000:]


def _compare(tmp, tag, name, rname, extra, env=None, **kw):
    host, herr = _aln(tmp, tag + "_host", name, rname, ["--sort", "--deflate-device"] + extra, **kw)
    dev, derr = _aln(tmp, tag + "_dev", name, rname, ["--sort-device"] + extra, env=env, **kw)
    _no_failure(derr)
    j = _e2e(derr)
    assert j["sorter"] == "device" and _e2e(herr)["sorter"] == "host", (tag, j)
    want, got = _three_files(host), _three_files(dev)
    for ext, a, b in zip(("main", "bai", "ori"), got, want):
        assert a == b, "%s: the %s file differs (%d vs %d bytes)" % (tag, ext, len(a), len(b))
    payload = gzip.decompress(got[0])
    assert j["sort_device_bytes"] + j["sort_host_bytes"] == len(payload) and j["sort_records"] == len(bam_stream.split(payload)[1])
    assert j["sort_members"] == (len(payload) + 0xff00 - 1) // 0xff00
    print("%s: sort_device_bytes %d, sort_host_bytes %d, sort_records %d, sort_members %d, sort_s %.4f" % (tag, j["sort_device_bytes"], j["sort_host_bytes"], j["sort_records"],
                                                                                                         j["sort_members"], j["sort_s"]))
    return j, payload


@pytest.mark.parametrize("tag,name,rname,extra,env", [("fx1", "fx1", "reads150", [], None), ("fx2", "fx2", "reads250", [], None), ("fx3", "fx3", "ragged", [], None),
                                                      ("fx5", "fx5", "hicopy", [], None), ("fx1-batch", "fx1", "reads150", ["--batch", "97", "--sub-batch", "31"], None),
                                                      ("fx2-Q", "fx2", "reads150", ["-Q"], None), ("fx2-takes", "fx2", "reads150", [], {"PSVR_STREAM_TAKE_MEMBERS": "2"})])
def test_cli_sort_device_writes_the_files_of_sort_with_deflate_device(tag, name, rname, extra, env):
    j, payload = _compare(tempfile.mkdtemp(prefix="psvr_bsto_"), tag, name, rname, extra, env=env)
    assert j["sort_host_bytes"] == len(bam_stream.split(payload)[0])            # nothing but the header came from the host
    if env:
        assert j["sort_members"] > 4                                           # several windows of two members


def test_cli_sort_device_from_stdin():
    tmp = tempfile.mkdtemp(prefix="psvr_bsto_")
    fq = os.path.join(ac.workdir("fx3"), "ragged.fq")
    outs = []
    for flags in (["--sort", "--deflate-device"], ["--sort-device"]):
        rd, wr = os.pipe()                                 # a real pipe: the reader cannot map it or peek at it
        feeder = subprocess.Popen(["cat", fq], stdout=wr)
        os.close(wr)
        o, err = _aln(tmp, "stdin%d" % len(outs), "fx3", "ragged", flags, reads="-", stdin=rd)
        os.close(rd)
        assert feeder.wait() == 0
        outs.append((o, err))
    _no_failure(outs[1][1])
    assert _e2e(outs[1][1])["sorter"] == "device"
    assert _three_files(outs[1][0]) == _three_files(outs[0][0])


def test_cli_sort_device_declined_pairs_go_in_as_host_chunks():
    tmp = tempfile.mkdtemp(prefix="psvr_bsto_")
    text = open(os.path.join(ac.workdir("fx1"), "reads150.fq"), "rb").read() * 3
    fq = os.path.join(tmp, "tabs.fq")
    with open(fq, "wb") as f:
        f.write(_with_tabs(text, (3, 700, 1999)))
    j, payload = _compare(tmp, "tabs", "fx1", "reads150", ["--sub-batch", "1000"], reads=fq)
    assert j["emit_declined_pairs"] == 3
    assert j["sort_device_bytes"] > 0 and j["sort_host_bytes"] > len(bam_stream.split(payload)[0])   # both kinds of chunk occurred


def test_cli_sort_device_is_ignored_for_a_bam_read_file():
    """the run is that of --sort --deflate-device, with a note"""
    from test_fused_signal import GOLDEN, bam_of
    tmp = tempfile.mkdtemp(prefix="psvr_bsto_")
    name, rname, n_pairs, sig_flags = GOLDEN[0]
    inp = os.path.join(tmp, "in.bam")
    bam_of(name, rname, n_pairs, inp)
    outs = []
    for k, flags in enumerate((["--sort", "--deflate-device"], ["--sort-device"])):
        o = os.path.join(tmp, "o%d" % k)
        r = subprocess.run([CLI, "aln", "-N", "-t", "4", "-o", o + ".bam", "-p", o + ".ori.bam"] + sig_flags + flags + [ac.index_dir(name), inp, os.path.join(tmp, "h%d.sam" % k)],
                           stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)
        assert r.returncode == 0, r.stderr.decode()[-2000:]
        outs.append((o, r.stderr.decode()))
    assert "--sort-device applies to FASTQ text: ignored" in outs[1][1] and "--sort-device applies" not in outs[0][1]
    assert _e2e(outs[1][1])["sorter"] == "host"
    assert _three_files(outs[1][0]) == _three_files(outs[0][0])
