"""-m gpu: the device-resident BGZF stream (psvr_bgzf_stream_*, pansvr_amd.bgzf.BgzfStream) and `panSVR aln --stream-device` on the MI355X.
The yardstick of the members is the host build of the encoder (tests/tools/deflate_wave_check.cpp) on the concatenation of everything
appended, whatever the order of appends and takes; the records appended from an emitter are held to the emitter's own download; the command
is held to the host route's payloads and, member for member, to the host build's members of its own payload."""
import gzip
import os
import random
import subprocess
import tempfile

import numpy as np
import pytest

import aln_common as ac
import bam_emit_cases as bc
import bam_stream
import deflate_wave_cases as dc
import fastq_cases as fc
import inflate_cases as ic
from test_bam_emit_gpu import _aln, _check_same, _e2e, _payload, _with_tabs, fx1  # noqa: F401  (fx1: index, parser and emitter of golden set fx1)
from test_emu_aln import CASES

pytestmark = pytest.mark.gpu
EOF_BLOCK = bytes([0x1f, 0x8b, 8, 4, 0, 0, 0, 0, 0, 0xff, 6, 0, 0x42, 0x43, 2, 0, 0x1b, 0, 3, 0, 0, 0, 0, 0, 0, 0, 0, 0])
FAILED = ("on the device failed", "BGZF stream on the device failed")


@pytest.fixture(scope="module")
def checker():
    return dc.build_checker(tempfile.mkdtemp(prefix="psvr_bsg_"), False)


@pytest.fixture(scope="module")
def emit_checker():
    return bc.build_checker(tempfile.mkdtemp(prefix="psvr_bsg_"), False)


def _drain(s, finish, mb, log):
    """one take: the members, checked for what a take promises, appended to log = [members, bytes consumed]"""
    before = s.pending
    out, offs, used = s.take(finish=finish)
    want_used = before if finish else before // mb * mb
    assert used == want_used and s.pending == before - used
    assert len(offs) == (used + mb - 1) // mb + 1 and offs[0] == 0 and offs[-1] == len(out)
    assert all(0 < b - a <= 65536 for a, b in zip(offs[:-1], offs[1:]))
    log[0] += out.tobytes()
    log[1] += used


# ---- 1. members against the host build ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("member_bytes", [256, 4096, 0xff00])
def test_members_equal_the_host_builds_however_takes_fall(checker, member_bytes):
    from pansvr_amd.bgzf import BgzfStream
    mb = member_bytes
    lengths = [0, 1, mb - 1, mb, mb + 1, 3 * mb + 1, 0, mb - 1]
    data = ic.bam_like(sum(lengths), 17)
    bufs, at = [], 0
    for n in lengths:
        bufs.append(data[at:at + n])
        at += n
    want = dc.host_members(checker, data, mb)
    rng = random.Random(mb)
    schedules = {"after every append": set(range(len(bufs))), "only at the end": set(), "at two seeded places": set(rng.sample(range(len(bufs) - 1), 2))}
    for name, takes in schedules.items():
        s = BgzfStream(mb)
        log = [b"", 0]
        for i, b in enumerate(bufs):
            s.append(b)
            if i in takes:
                _drain(s, False, mb, log)
        assert s.pending == len(data) - log[1], name
        _drain(s, True, mb, log)
        assert log[1] == len(data) and s.pending == 0, name
        assert log[0] == want, name
        dc.check_members(log[0], data, mb)
        out, offs, used = s.take(finish=True)                                   # nothing is left: no member, not even an empty one
        assert len(out) == 0 and list(offs) == [0] and used == 0, name
        s.close()


def test_finish_on_an_empty_stream_and_on_a_member_boundary(checker):
    from pansvr_amd.bgzf import BgzfStream
    mb = 4096
    s = BgzfStream(mb)
    for finish in (False, True):
        out, offs, used = s.take(finish=finish)
        assert len(out) == 0 and list(offs) == [0] and used == 0
    data = ic.bam_like(2 * mb, 3)
    s.append(data)
    out, offs, used = s.take(finish=True)
    assert used == 2 * mb and len(offs) == 3 and out.tobytes() == dc.host_members(checker, data, mb)
    out, offs, used = s.take(finish=True)
    assert len(out) == 0 and used == 0
    # the same through a take without finish first: both members then, none at the end
    s.append(data)
    out, offs, used = s.take()
    assert used == 2 * mb and len(offs) == 3 and s.pending == 0
    out, offs, used = s.take(finish=True)
    assert len(out) == 0 and len(offs) == 1 and used == 0
    s.close()


def test_a_take_without_room_consumes_nothing(checker):
    from pansvr_amd import lib
    from pansvr_amd._lib import EngineError
    from pansvr_amd.bgzf import BgzfStream
    import ctypes as C
    mb = 4096
    data = ic.bam_like(2 * mb + 77, 5)
    s = BgzfStream(mb)
    s.append(data)
    bound = lib().psvr_bgzf_members_bound(C.c_int64(len(data)), C.c_int32(mb))
    assert bound == len(data) + 3 * 31
    for finish in (False, True):
        with pytest.raises(EngineError, match="psvr error 6"):                  # PSVR_ERR_OVERFLOW
            s.take(finish=finish, out_cap=bound - 1)
        assert s.pending == len(data)
    a, offs, used = s.take()
    assert used == 2 * mb
    b, offs, used = s.take(finish=True)
    assert used == 77 and a.tobytes() + b.tobytes() == dc.host_members(checker, data, mb)
    s.close()


# ---- 2. from the emitter ------------------------------------------------------------------------------------------------------------------------------
def _emitter_cases():
    picked = [c for c in bc.cases(golden=False) if c["name"] in ("1 pairs", "255 pairs", "256 pairs", "257 pairs", "4097 pairs", "a tab in the comment")]
    assert len(picked) == 6
    return picked


def test_appends_from_the_emitter(checker, emit_checker, fx1):
    from pansvr_amd.aln import CAND_DTYPE, HDR_DTYPE, PAIR_DTYPE
    from pansvr_amd._lib import EngineError
    from pansvr_amd.bgzf import BgzfStream
    from pansvr_amd.emit import BamEmitter
    index, n_header, anchors, parser, emitter = fx1
    mb = 4096                                                                  # (several members from a run of a few hundred pairs)
    counts = set()
    for c in _emitter_cases():
        s_, raw = bc.run_checker(emit_checker, c["text"], c["cls"], c["seed"], c["flags"], n_header=n_header, anchors=anchors)
        w = bc.split_out(raw)
        P = w["P"]
        assert parser.parse(c["text"], fc.BIG_PAIRS, fc.BIG_BASES).n_pairs == P
        arrays = [np.frombuffer(w[k], dtype=dt) for k, dt in (("hdr", HDR_DTYPE), ("pairs", PAIR_DTYPE), ("cands", CAND_DTYPE), ("cigar", np.uint32))]
        ei = emitter.emit_results(parser, *arrays, flags=c["flags"])
        data, off, state = emitter.download()
        rec = data.tobytes()
        if c["label"] == "declining":
            assert ei.n_bytes == 0 and ei.n_declined_pairs == P
        else:
            assert ei.n_bytes > 0
        counts.add(P)
        rng = random.Random(P)
        cuts = sorted(rng.randrange(P + 1) for _ in range(3))
        between = ic.bam_like(1000 + P % 17, P)
        s = BgzfStream(mb)
        # whole run; the run split at seeded pairs, with empty ranges and a host buffer between two ranges
        plan = [(0, P), (0, cuts[0]), (cuts[0], 0), between, (cuts[0], cuts[1] - cuts[0]), (P, 0), (cuts[1], cuts[2] - cuts[1]), (cuts[2], P - cuts[2]), (0, 0)]
        want, log = b"", [b"", 0]
        for k, step in enumerate(plan):
            if isinstance(step, tuple):
                s.append_emit(emitter, step[0], step[1])
                want += rec[off[step[0]]:off[step[0] + step[1]]]
            else:
                s.append(step)
                want += step
            if k == 4:                                                         # a take in the middle, right behind a queued append
                _drain(s, False, mb, log)
        assert s.pending == len(want) - log[1], c["name"]
        _drain(s, True, mb, log)
        assert len(want) == 2 * len(rec) + len(between)
        assert b"".join(ic.oracle(m) for m in ic.split_members(log[0])) == want, c["name"]
        assert log[0] == dc.host_members(checker, want, mb), c["name"]
        with pytest.raises(EngineError, match="psvr error 1"):                  # PSVR_ERR_ARG
            s.append_emit(emitter, 1, P)
        with pytest.raises(EngineError, match="psvr error 1"):
            s.append_emit(emitter, P + 1, 0)
        with pytest.raises(EngineError, match="psvr error 1"):
            s.append_emit(emitter, -1, 1)
        assert s.pending == 0
        s.close()
    assert {1, 255, 256, 257, 4097} <= counts
    fresh = BamEmitter(index)                                                  # an emitter without a run
    s = BgzfStream(mb)
    with pytest.raises(EngineError, match="no emitted run"):
        s.append_emit(fresh, 0, 0)
    s.close(), fresh.close()


# ---- 3. recover -------------------------------------------------------------------------------------------------------------------------------------
def test_recover_returns_the_untaken_bytes():
    from pansvr_amd.bgzf import BgzfStream
    mb = 256
    s = BgzfStream(mb)
    assert len(s.recover()) == 0 and s.pending == 0
    data = ic.bam_like(5 * mb + 100, 9)
    s.append(data[:700]), s.append(data[700:])
    out, offs, used = s.take()
    assert used == 5 * mb
    more = ic.bam_like(33, 4)
    s.append(more)
    assert s.pending == 133
    assert s.recover().tobytes() == data[5 * mb:] + more
    assert s.pending == 0
    out, offs, used = s.take(finish=True)
    assert len(out) == 0 and used == 0
    s.append(b"abc")                                                           # and it goes on from empty
    assert s.recover().tobytes() == b"abc"
    s.close()


# ---- 4.-7. the command ----------------------------------------------------------------------------------------------------------------------------
def _no_failure(err):
    assert not any(f in err for f in FAILED), err[-2000:]


def _main_is_the_host_builds(checker, o, payload):
    """the main file, byte for byte: the host build's members of its own payload at 0xff00, then the EOF block"""
    raw = open(o + ".bam", "rb").read()
    assert raw == dc.host_members(checker, payload, 0xff00) + EOF_BLOCK
    return raw


@pytest.mark.parametrize("name,rname", CASES)
def test_cli_stream_device_writes_the_host_routes_files(checker, name, rname):
    """with and without -Q: both payloads are the host route's; the stream's byte counts add up to the main payload (the BAM header is its first
    host append); declined pairs stay under 1 % of the pairs that reach the encoder; the main file is the host build's members of its payload;
    and on fx2 it is the file of --emit-device --deflate-device, whose every flush goes to the device"""
    tmp = tempfile.mkdtemp(prefix="psvr_bsg_")
    for q in ([], ["-Q"]):
        tag = "q" if q else "p"
        host, herr = _aln(tmp, "host_" + tag, name, rname, q)
        dev, derr = _aln(tmp, "dev_" + tag, name, rname, q + ["--stream-device"])
        _no_failure(derr)
        assert '"streamer":"device"' in derr and '"emitter":"device"' in derr and '"parser":"device"' in derr
        assert '"streamer":"host"' in herr
        want = _payload(host)
        _check_same(dev, want, "%s/%s %s" % (name, rname, tag))
        j, jh = _e2e(derr), _e2e(herr)
        assert jh["stream_device_bytes"] == jh["stream_host_bytes"] == jh["stream_members"] == 0
        print("%s/%s %s: stream_device_bytes %d, stream_host_bytes %d, stream_members %d, emit_declined_pairs %d" % (name, rname, tag, j["stream_device_bytes"], j["stream_host_bytes"],
                                                                                                                   j["stream_members"], j["emit_declined_pairs"]))
        assert j["stream_device_bytes"] + j["stream_host_bytes"] == len(want[0])
        assert j["stream_host_bytes"] == len(bam_stream.split(want[0])[0])      # nothing but the header came from the host
        assert j["stream_members"] == (len(want[0]) + 0xff00 - 1) // 0xff00
        assert j["emit_device_pairs"] + j["emit_declined_pairs"] == j["pairs"]
        assert j["emit_declined_pairs"] * 100 <= j["emit_device_pairs"] + j["emit_declined_pairs"]
        assert j["dropped"] == jh["dropped"]
        raw = _main_is_the_host_builds(checker, dev, want[0])
        if name == "fx2":
            both, berr = _aln(tmp, "both_" + tag, name, rname, q + ["--emit-device", "--deflate-device"], env={"PSVR_BGZF_DEVICE_MIN_BLOCKS": "1"})
            assert "on the device failed" not in berr
            assert open(both + ".bam", "rb").read() == raw


@pytest.fixture(scope="module")
def fx2_host():
    tmp = tempfile.mkdtemp(prefix="psvr_bsg_")
    o, err = _aln(tmp, "host", "fx2", "reads150", [])
    return tmp, _payload(o)


@pytest.mark.parametrize("route", ["batch", "batch-bases", "sub-batch", "stdin", "gz", "takes"])
def test_cli_stream_device_over_batch_limits_and_input_routes(checker, fx2_host, route):
    """'takes': a take after every piece that leaves a member pending (the product takes at 1024), so that members are made in the middle"""
    tmp, want = fx2_host
    fq = os.path.join(ac.workdir("fx2"), "reads150.fq")
    kw = {}
    extra = {"batch": ["--batch", "97"], "batch-bases": ["--batch-bases", "60000"], "sub-batch": ["--sub-batch", "31"], "takes": ["--sub-batch", "300"]}.get(route, [])
    if route == "takes":
        kw = dict(env={"PSVR_STREAM_TAKE_MEMBERS": "1"})
    if route == "stdin":
        rd, wr = os.pipe()                                 # a real pipe: the reader cannot map it or peek at it
        feeder = subprocess.Popen(["cat", fq], stdout=wr)
        os.close(wr)
        kw = dict(reads="-", stdin=rd)
    elif route == "gz":
        gz = os.path.join(tmp, "reads150.fq.gz")
        with gzip.open(gz, "wb") as f:
            f.write(open(fq, "rb").read())
        kw = dict(reads=gz)
    o, err = _aln(tmp, route, "fx2", "reads150", ["--stream-device"] + extra, **kw)
    if route == "stdin":
        os.close(rd)
        assert feeder.wait() == 0
    _no_failure(err)
    assert '"streamer":"device"' in err
    _check_same(o, want, route)
    _main_is_the_host_builds(checker, o, want[0])


def _bytes_of_pairs(payload, names, n_pairs):
    """bytes of the records of the first n_pairs pairs: the records follow the input's order, a pair's records carry its name"""
    head, recs = bam_stream.split(payload)
    p, total = 0, 0
    for r in recs:
        q = r[36:36 + r[12] - 1]
        while names[p] != q:
            p += 1
        if p < n_pairs:
            total += len(r)
    return len(head), total


def test_cli_stream_device_declined_pairs_go_in_as_host_chunks(checker):
    """6000 pairs, a tab in a comment of pairs 3, 700 and 1999: the chunks that hold them are formatted on the host whole and uploaded into the
    stream (one chunk of 4096 pairs of the one piece, or the first two pieces of --sub-batch 1000), the others never leave HBM"""
    tmp = tempfile.mkdtemp(prefix="psvr_bsg_")
    text = open(os.path.join(ac.workdir("fx1"), "reads150.fq"), "rb").read() * 3
    fq = os.path.join(tmp, "tabs.fq")
    with open(fq, "wb") as f:
        f.write(_with_tabs(text, (3, 700, 1999)))
    names = [l.split()[0][1:] for l in text.split(b"\n")[0::8] if l]
    assert len(names) == 6000
    host, herr = _aln(tmp, "host", "fx1", "reads150", [], reads=fq)
    want = _payload(host)
    for extra, host_pairs in ((["--sub-batch", "1000"], 2000), ([], 4096)):
        dev, derr = _aln(tmp, "dev%d" % len(extra), "fx1", "reads150", ["--stream-device"] + extra, reads=fq)
        _no_failure(derr)
        _check_same(dev, want, "tabs " + " ".join(extra))
        j = _e2e(derr)
        assert j["emit_declined_pairs"] == 3 and j["emit_device_pairs"] == 5997 and j["emit_spliced_pairs"] == 6000 - host_pairs, j
        assert j["streamer"] == "device+host"
        n_head, n_chunks = _bytes_of_pairs(want[0], names, host_pairs)
        assert j["stream_host_bytes"] == n_head + n_chunks, (j, n_head, n_chunks)   # the header and exactly the chunks that held a declined pair
        assert j["stream_device_bytes"] == len(want[0]) - n_head - n_chunks
        assert j["dropped"] == _e2e(herr)["dropped"]
        assert [l for l in derr.split("\n") if "ERROR" in l] == [l for l in herr.split("\n") if "ERROR" in l]
        _main_is_the_host_builds(checker, dev, want[0])


def test_cli_stream_device_takes_host_pieces_as_host_chunks(checker, fx2_host):
    tmp, want = fx2_host
    o, err = _aln(tmp, "fallback", "fx2", "reads150", ["--stream-device", "--sub-batch", "500"], env={"PSVR_PARSE_DEVICE_MAX_BYTES": "1000"})
    assert '"streamer":"host"' in err and '"emitter":"host"' in err and '"parser":"host"' in err
    j = _e2e(err)
    assert j["stream_device_bytes"] == 0 and j["stream_host_bytes"] == len(want[0])
    _check_same(o, want, "fallback")
    _main_is_the_host_builds(checker, o, want[0])
