"""-m gpu: psvr_bam_store_append_bgzf (pansvr_amd.sort.BamStore.append_bgzf: a BAM file's members inflated into the device-resident record store,
the records found there by the chain finder of bam_chain_device.h) and `panSVR sort --sort-device` on the MI355X.  The yardstick of the store is
tests/test_bam_store_gpu.py's restatement; the chain's counters are held to the host build of the same header (tests/tools/bam_chain_check.cpp);
the command is held to the files of `panSVR sort --deflate-device`, byte for byte."""
import contextlib
import gzip
import os
import struct
import subprocess
import tempfile

import pytest

import bam_chain_cases as cc
import bam_stream
import inflate_cases as ic
import test_signal as ts
from test_bam_store_gpu import REFS, check_meta, chunk_bytes, expectation, make_record, make_records, restate, streamed, with_cigar_count  # noqa: F401

pytestmark = pytest.mark.gpu
CLI = ts.CLI
EOF_BLOCK = ic.wrap(ic.deflate(b""), b"")
SKIP = 57


@contextlib.contextmanager
def seg_bytes(n):
    """stores made inside cut their streams into segments of n bytes (PSVR_BAM_STORE_SEG_BYTES); 0: the default"""
    old = os.environ.pop("PSVR_BAM_STORE_SEG_BYTES", None)
    if n:
        os.environ["PSVR_BAM_STORE_SEG_BYTES"] = str(n)
    try:
        yield
    finally:
        os.environ.pop("PSVR_BAM_STORE_SEG_BYTES", None)
        if old is not None:
            os.environ["PSVR_BAM_STORE_SEG_BYTES"] = old


def make_store(seg=0, chunk=0):
    from pansvr_amd.sort import BamStore
    with seg_bytes(seg), chunk_bytes(chunk):
        return BamStore()


_SETS = {}


def record_set(n):
    """(records, their stream behind SKIP bytes that are no records, the expectation) -- made once, shared, never changed"""
    if n not in _SETS:
        if n == "edges":                                                       # block_size at chain_record's edges, at the edges of 16 KiB segments
            buf, count = cc.edge_stream()
            recs = bam_stream.split(b"BAM\1\0\0\0\0\0\0\0\0" + buf)[1]
            assert len(recs) == count <= 200 and cc.EDGE_SEG == 16384
        else:
            recs = make_records(n, 7 + n, shortest=37)
        skip = SKIP if n else 0
        _SETS[n] = (recs, bytes(range(1, skip + 1)) + b"".join(recs), skip, expectation(recs))
    return _SETS[n]


_MEMBERS = {}


def members(n, block):
    if (n, block) not in _MEMBERS:
        _MEMBERS[(n, block)] = ic.members_of(record_set(n)[1], level=1, block=block) + [EOF_BLOCK]
    return _MEMBERS[(n, block)]


def hold_store(st, recs, exp):
    fixed, order, info = exp
    n = len(recs)
    i = st.info()
    assert (i.n_records, i.n_bytes, i.key_exact, i.ordered) == (n, sum(map(len, recs)), 1, 0)
    assert st.chain_info().tail_bytes == 0
    assert st.download().tobytes() == b"".join(fixed)
    st.order()
    check_meta(st.meta(), order, info)
    want = b"".join(fixed[k] for k in order)
    got = streamed(st, n, 3000, 2)
    assert got == want, bam_stream.first_difference(b"BAM\1\0\0\0\0\0\0\0\0" + got, b"BAM\1\0\0\0\0\0\0\0\0" + want)


# ---- 1. the ABI against the restatement ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,block,seg,chunk,every", [
    (0, 0xff00, 0, 0, 0), (1, 0xff00, 64, 0, 1), (1, 100, 0, 4096, 0), (2, 100, 64, 4096, 1), (2, 333, 256, 0, 7),
    (2047, 0xff00, 0, 0, 0), (2047, 0xff00, 256, 4096, 1), (2047, 100, 64, 4096, 7), (2047, 333, 256, 0, 1), (2047, 333, 0, 4096, 0),
    (4 * 2048 + 7, 0xff00, 0, 0, 0), (4 * 2048 + 7, 0xff00, 64, 4096, 7), (4 * 2048 + 7, 100, 256, 0, 7), (4 * 2048 + 7, 333, 0, 4096, 7), (4 * 2048 + 7, 333, 64, 0, 0),
    (4 * 2048 + 7, 0xff00, 256, 0, 1), ("edges", 0xff00, 16384, 0, 3)])
def test_members_in_records_out(n, block, seg, chunk, every):
    recs, stream, skip, exp = record_set(n)
    ms = members(n, block)
    n = len(recs)
    st = make_store(seg, chunk)
    every = every or len(ms)
    inflated, tails, last, count = bytearray(), set(), skip, 0
    assert st.append_bgzf(ms[0][:17], skip=skip, n_ref=len(REFS)) == 0           # no whole member yet: nothing happens, the skip is still due
    for a in range(0, len(ms), every):
        call = ms[a:a + every]
        data = b"".join(call)
        assert st.append_bgzf(data + data[:11], skip=skip if a == 0 else 0, n_ref=len(REFS)) == len(data)    # (a member that is cut off is left to the caller)
        inflated += b"".join(ic.oracle(m) for m in call)
        starts, last, bad = cc.walk(inflated, last)
        count += len(starts)
        ci = st.chain_info()
        assert not bad and ci.tail_bytes == len(inflated) - last, (a, ci.tail_bytes, len(inflated) - last)
        assert st.info().n_records == count
        tails.add(ci.tail_bytes != 0)
    assert bytes(inflated) == stream and count == n
    if n >= 100 and every < len(ms):
        assert True in tails                                                   # calls ended inside records
    ci = st.chain_info()
    assert ci.segments >= (len(stream) - skip + (seg or 16384) - 1) // (seg or 16384) and ci.rewalked <= ci.segments
    print("n %d block %d seg %d: segments %d, no guess %d, wrong %d, walked again %d" % (n, block, seg, ci.segments, ci.no_guess, ci.wrong_guess, ci.rewalked))
    hold_store(st, recs, exp)
    st.close()


@pytest.mark.parametrize("tail", [5, 0, "edges"])
def test_decoy_streams_are_repaired_as_on_the_host(tail):
    """the two decoy streams of tests/test_bam_chain.py and its stream of block_size edges (decoys with block_size 31 .. 36 and around
    kBamRecStoreMaxBlock at the edges of 16 KiB segments): the device's counters are those of the host build of the same header (the ABI does not hand
    the entries out: the records, and with them every entry that starts one, are compared instead)"""
    buf, seg, n = (cc.edge_stream()[0], cc.EDGE_SEG, cc.edge_stream()[1]) if tail == "edges" else (cc.decoy_stream(tail), 256, 26)
    host, = cc.run_checker(cc.build_checker(tempfile.mkdtemp(prefix="psvr_sdev_"), False), [(buf, 0, cc.N_REF, seg)])
    st = make_store(seg)
    data = b"".join(ic.members_of(buf, level=1, block=0xff00))
    assert st.append_bgzf(data, n_ref=cc.N_REF) == len(data)
    ci = st.chain_info()
    assert (ci.segments, ci.no_guess, ci.wrong_guess, ci.rewalked, ci.tail_bytes) == (host["segments"], host["no_guess"], host["wrong_guess"], host["rewalked"], 0)
    assert ci.wrong_guess >= 1 and st.info().n_records == host["total"] == n
    recs = bam_stream.split(b"BAM\1\0\0\0\0\0\0\0\0" + buf)[1]
    assert len(recs) == n and st.download().tobytes() == b"".join(expectation(recs)[0])
    st.close()


# ---- 2. refusals: ordinary checks, ordinary error returns ---------------------------------------------------------------------------------------------------
def _planted(kind):
    recs = record_set(2047)[0]
    good = make_record(60, 0, 5, 0, [], 1)
    bad = {"block_size 31": struct.pack("<I", 31) + good[4:35],
           "negative l_seq": good[:20] + struct.pack("<i", -1) + good[24:],
           "name without NUL": good[:36 + good[12] - 1] + b"x" + good[36 + good[12]:],
           "CIGAR leaves its record": with_cigar_count(good, 100)}[kind]
    return b"".join(recs[:1000]) + bad + b"".join(recs[1000:1200])


@pytest.mark.parametrize("kind", ["block_size 31", "negative l_seq", "name without NUL", "CIGAR leaves its record"])
def test_a_malformed_record_on_the_chain_makes_the_store_unusable(kind):
    from pansvr_amd._lib import EngineError
    buf = _planted(kind)
    assert cc.walk(buf)[2] and len(cc.walk(buf)[0]) == 1000
    st = make_store(256)
    with pytest.raises(EngineError, match="psvr error 3"):                      # PSVR_ERR_DEVICE, at the next call that waits
        st.append_bgzf(b"".join(ic.members_of(buf, level=1, block=333)), n_ref=len(REFS))
        st.info()
    for call in (st.info, st.chain_info, st.order, st.download):
        with pytest.raises(EngineError, match="psvr error 3"):
            call()
    st.close()


def test_a_truncated_tail_is_refused_by_order():
    from pansvr_amd._lib import EngineError
    recs, exp = record_set(2047)[0], record_set(2047)[3]
    buf = b"".join(recs[:500])
    st = make_store(64)
    st.append_bgzf(b"".join(ic.members_of(buf[:-9], level=1, block=333)), n_ref=len(REFS))
    assert st.chain_info().tail_bytes == len(recs[499]) - 9
    with pytest.raises(EngineError, match="truncated BAM stream"):
        st.order()
    with pytest.raises(EngineError, match="psvr error 1"):                      # PSVR_ERR_ARG
        st.order()
    for other in (lambda: st.append(recs[0]), ):
        with pytest.raises(EngineError, match="psvr error 1"):                  # only append_bgzf can complete the record
            other()
    i = st.info()
    assert (i.n_records, i.n_bytes, i.ordered) == (499, sum(map(len, recs[:499])), 0)
    assert st.download().tobytes() == b"".join(exp[0][:499])                    # whole records only
    st.append_bgzf(ic.wrap(ic.deflate(buf[-9:]), buf[-9:]))                     # ... and the next call completes it
    assert st.chain_info().tail_bytes == 0 and st.info().n_records == 500
    st.order()
    st.close()


def test_a_corrupt_member_refuses_its_call_only():
    from pansvr_amd._lib import EngineError
    recs, stream, skip, exp = record_set(2047)
    small = ic.members_of(stream, level=1, block=7001)                           # the same stream in members of 7001 bytes
    st = make_store(256)
    st.append_bgzf(b"".join(small[:3]), skip=skip, n_ref=len(REFS))
    before = (st.info().n_records, st.chain_info().tail_bytes)
    broken = bytearray(small[5])
    broken[-6] ^= 0x10                                                          # a CRC32 byte
    with pytest.raises(EngineError, match="psvr error 5") as e:                 # PSVR_ERR_IO
        st.append_bgzf(b"".join(small[3:5]) + bytes(broken) + b"".join(small[6:9]), n_ref=len(REFS))
    assert e.value.bad_member == 2
    assert (st.info().n_records, st.chain_info().tail_bytes) == before
    not_bgzf = b"".join(small[3:5]) + b"\x1f\x8b\x08\x00" + bytes(30)
    with pytest.raises(EngineError, match="psvr error 5") as e:
        st.append_bgzf(not_bgzf, n_ref=len(REFS))
    assert e.value.bad_member == 2 and (st.info().n_records, st.chain_info().tail_bytes) == before
    st.append_bgzf(b"".join(small[3:]), n_ref=len(REFS))                         # the good call still works
    hold_store(st, recs, exp)
    st.close()


def test_every_refused_rule_edge_member_refuses_its_call_and_names_its_status():
    """k_store_inflate is the decoder's second instantiation (it writes into a chunk): every refused member of inflate_cases.rule_edges(), between
    good members of a BAM stream, refuses its call with the member's index and the status of the rule it breaks -- the host build's, which is run
    first under the sanitizers on the identical bytes -- and the store goes on as if the call had not been made"""
    from pansvr_amd._lib import EngineError
    recs, stream, skip, exp = record_set(2047)
    small = ic.members_of(stream, level=1, block=7001)
    cases = [c for c in ic.rule_edges() if c[2] != "kInfOk"]
    assert len(cases) >= 80
    checker = ic.build_checker(tempfile.mkdtemp(prefix="psvr_sdev_"), True)
    K = ic.constants(checker)
    assert [s for s, _ in ic.run_checker(checker, [c[1] for c in cases])] == [K[c[2]] for c in cases]
    st = make_store(256)
    st.append_bgzf(b"".join(small[:3]), skip=skip, n_ref=len(REFS))
    before = (st.info().n_records, st.chain_info().tail_bytes)
    front = b"".join(small[3:5])
    seen = set()
    for name, m, status, _ in cases:
        with pytest.raises(EngineError, match="psvr error 5") as e:             # PSVR_ERR_IO
            st.append_bgzf(front + m + small[5], n_ref=len(REFS))
        assert e.value.bad_member == 2 and "member 2 at byte %d" % len(front) in str(e.value), name + ": " + str(e.value)
        assert "(status %d;" % K[status] in str(e.value), "%s: %s, not %s = %d" % (name, e.value, status, K[status])
        seen.add(status)
    assert (st.info().n_records, st.chain_info().tail_bytes) == before
    print("k_store_inflate returned", " ".join(sorted(seen)))
    st.append_bgzf(b"".join(small[3:]), n_ref=len(REFS))                         # the good call still works
    hold_store(st, recs, exp)
    st.close()


# ---- 3. the command ----------------------------------------------------------------------------------------------------------------------------------------
VARIANTS = {"default": {}, "batch-1000": {"PSVR_INFLATE_BATCH": "1000"}, "batch-70000": {"PSVR_INFLATE_BATCH": "70000"},
            "small-chunks": {"PSVR_INFLATE_BATCH": "70000", "PSVR_BAM_STORE_CHUNK_BYTES": "300000"}}
GOLDEN = {os.path.relpath(fn, os.path.join(ic.HERE, "golden")): fn for fn in ic.golden_bams()}
_TMP = tempfile.mkdtemp(prefix="psvr_sdev_")
_INPUT, _HOST = {}, {}


def _sort(flags, inp, out, env=None):
    r = subprocess.run([CLI, "sort", "-t", "4"] + flags + ["-o", out, inp], stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=dict(os.environ, **(env or {})), timeout=300)
    files = tuple(open(out + ext, "rb").read() if os.path.exists(out + ext) else None for ext in ("", ".bai"))
    return r.returncode, r.stderr.decode(), files


def _input(name):
    """the input file of that name, made once"""
    if name in _INPUT:
        return _INPUT[name]
    fn = GOLDEN.get(name) or os.path.join(_TMP, name.replace("/", "_") + ".in.bam")
    if name in ("aln-zlib", "aln-own"):
        from test_bam_emit_gpu import _aln
        fn = _aln(_TMP, name, "fx1", "reads150", [] if name == "aln-zlib" else ["--deflate-device"])[0] + ".bam"
        if name == "aln-own":
            assert all(len(ic.oracle(m)) == 0xff00 for m in ic.split_members(open(fn, "rb").read())[:-2])
    elif name == "header-only":
        ts.write_bam(fn, [], REFS)
    elif name == "position-2^31-1":
        recs = make_records(300, 5, shortest=37)
        ts.write_bam(fn, recs[:100] + [make_record(50, 0, 0x7fffffff, 0, [], 3)] + recs[100:], REFS)
    elif name == "malformed":
        ts.write_bam(fn, [_planted("negative l_seq")], REFS)
    elif name == "truncated":
        ts.write_bam(fn, make_records(2047, 5, shortest=37), REFS)
        raw = open(fn, "rb").read()
        open(fn, "wb").write(b"".join(ic.split_members(raw)[:-3]) + EOF_BLOCK)     # the stream ends inside a record
    _INPUT[name] = fn
    return fn


def _host(name):
    if name not in _HOST:
        _HOST[name] = _sort(["--deflate-device"], _input(name), os.path.join(_TMP, name.replace("/", "_") + ".host.bam"))
    return _HOST[name]


@pytest.mark.parametrize("variant", sorted(VARIANTS))
@pytest.mark.parametrize("name", sorted(GOLDEN) + ["aln-zlib", "aln-own", "header-only"])
def test_cli_writes_the_files_of_deflate_device(name, variant):
    rc, herr, want = _host(name)
    assert rc == 0, herr
    rc, err, got = _sort(["--sort-device"], _input(name), os.path.join(_TMP, "%s.%s.bam" % (name.replace("/", "_"), variant)), VARIANTS[variant])
    assert rc == 0 and "failed" not in err and "records kept on the device" in err, err[-2000:]
    for ext, a, b in zip(("bam", "bai"), got, want):
        assert a is not None and a == b, "%s %s: the %s file differs" % (name, variant, ext)
    if variant == "default":
        print(name, err.strip().split("\n")[-1])


@pytest.mark.parametrize("variant", sorted(VARIANTS))
def test_cli_leaves_the_route_for_a_position_the_key_cannot_hold(variant):
    rc, herr, want = _host("position-2^31-1")
    rcd, err, got = _sort(["--sort-device"], _input("position-2^31-1"), os.path.join(_TMP, "pos.%s.bam" % variant), VARIANTS[variant])
    assert (rcd, got) == (rc, want) and rc == 0, err[-2000:]
    assert "record store on the device failed (order:" in err and "records kept on the device" not in err, err


@pytest.mark.parametrize("variant", sorted(VARIANTS))
@pytest.mark.parametrize("name", ["malformed", "truncated"])
def test_cli_ends_as_the_deflate_device_route_on_a_bad_file(name, variant):
    rc, herr, want = _host(name)
    assert rc == 2 and want[1] is None
    rcd, err, got = _sort(["--sort-device"], _input(name), os.path.join(_TMP, "%s.%s.bam" % (name, variant)), VARIANTS[variant])
    assert rcd == rc and err.strip().split("\n")[-1] == herr.strip().split("\n")[-1], err
    assert "sort --sort-device:" in err and "sorted by the --deflate-device route" in err, err
    assert got[1] is None                                                      # no .bai
