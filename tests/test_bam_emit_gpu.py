"""-m gpu: the BAM record encoder's device route on the MI355X.  psvr_bam_emit_results (pansvr_amd.emit.BamEmitter) against the files that
tests/tools/bam_emit_device_check.cpp writes after holding the same rules to SamEmitter::main_pair, byte for byte; psvr_bam_emit_engine
against psvr_bam_emit_results on the same engine's compact download; and `panSVR aln --emit-device` against the host route's files, over
the batch limits, the input routes, --sort and --deflate-device, through declined pairs and through its fallback to the host formatter."""
import ctypes as C
import gzip
import json
import os
import subprocess
import tempfile

import numpy as np
import pytest

import aln_common as ac
import bam_emit_cases as bc
import bam_stream
import fastq_cases as fc
from test_emu_aln import CASES

pytestmark = pytest.mark.gpu
CLI = bc.CLI


@pytest.fixture(scope="module")
def checker():
    return bc.build_checker(tempfile.mkdtemp(prefix="psvr_beg_"), False)


@pytest.fixture(scope="module")
def fx1():
    """(index, its header's size, its anchors' strings, a parser, an emitter)"""
    import synth
    import test_abi_gpu as tag
    from pansvr_amd import lib
    from pansvr_amd.emit import BamEmitter
    from pansvr_amd.fastq import FastqParser
    index = tag._index("fx1")
    n_header = sum(1 for l in synth.header_text().split("\n") if l.startswith("@SQ"))
    L = lib()
    L.psvr_index_sv_print_string.restype = L.psvr_index_sv_vcf_id.restype = C.c_char_p
    anchors = [(L.psvr_index_sv_print_string(index.h, C.c_int32(i)), L.psvr_index_sv_vcf_id(index.h, C.c_int32(i))) for i in range(L.psvr_index_n_anchor(index.h))]
    assert len(anchors) == 20 and all(a is not None and b is not None for a, b in anchors)
    parser, emitter = FastqParser(), BamEmitter(index)
    yield index, n_header, anchors, parser, emitter
    emitter.close(), parser.close(), index.close()


def _same(got, want, name):
    data, off, state = got
    for key, a in (("state", state.tobytes()), ("pair_off", off.tobytes()), ("bytes", data.tobytes())):
        b = want[key]
        if a != b:
            first = next((i for i, (x, y) in enumerate(zip(a, b)) if x != y), min(len(a), len(b)))
            raise AssertionError("%s: %s differs from the checker's (%d vs %d bytes, first at byte %d)" % (name, key, len(a), len(b), first))


def test_emit_results_equal_the_checkers_files_on_every_case(checker, fx1):
    from pansvr_amd.aln import CAND_DTYPE, HDR_DTYPE, PAIR_DTYPE
    index, n_header, anchors, parser, emitter = fx1
    counts = set()
    for c in bc.cases():
        s, raw = bc.run_checker(checker, c["text"], c["cls"], c["seed"], c["flags"], n_header=n_header, anchors=anchors)
        want = bc.split_out(raw)
        info = parser.parse(c["text"], fc.BIG_PAIRS, fc.BIG_BASES)
        assert info.n_pairs == want["P"], c["name"]
        arrays = [np.frombuffer(want[k], dtype=dt) for k, dt in (("hdr", HDR_DTYPE), ("pairs", PAIR_DTYPE), ("cands", CAND_DTYPE), ("cigar", np.uint32))]
        ei = emitter.emit_results(parser, *arrays, flags=c["flags"])
        assert (ei.n_bytes, ei.n_records, ei.n_written_pairs, ei.n_declined_pairs) == (want["n_bytes"], want["n_records"], want["n_written"], want["n_declined"]), c["name"]
        _same(emitter.download(), want, c["name"])
        if c["label"] == "declining":
            assert ei.n_declined_pairs == want["P"] and ei.n_bytes == 0, c["name"]
        counts.add(want["P"])
    assert {1, 255, 256, 257, 4097} <= counts
    # a buffer that is too small, and a range that leaves the window
    from pansvr_amd import lib
    from pansvr_amd._lib import EngineError
    assert emitter.info.n_bytes > 8
    small = np.zeros(8, dtype=np.uint8)
    assert lib().psvr_bam_emit_download(emitter.h, small.ctypes.data_as(C.c_void_p), C.c_int64(8), None, None) == 6          # PSVR_ERR_OVERFLOW
    with pytest.raises(EngineError):
        emitter.emit_results(parser, *arrays, first_pair=1)


def test_emit_engine_equals_emit_results_on_the_compact_download(fx1):
    """parse -> upload_fastq -> run -> emit == emit_results on the same engine's download_compact; then the second half of the window alone;
    a re-parsed window and an engine fed by psvr_engine_upload are refused"""
    from pansvr_amd import aln
    index, n_header, anchors, parser, emitter = fx1
    text = open(os.path.join(ac.workdir("fx1"), "reads150.fq"), "rb").read()
    P = parser.parse(text, fc.BIG_PAIRS, fc.BIG_BASES).n_pairs
    assert P == 2000
    whole = None
    for first, n in ((0, P), (P // 2 + 1, P - P // 2 - 1)):
        e = aln.Engine(index)
        if first:                                                 # the pairs in front first: the half then starts in the draw streams where it did in the whole
            parser.upload_to(e, first_pair=0, n_pairs=first)
            e.run()
        parser.upload_to(e, first_pair=first, n_pairs=n)
        e.run()
        for flags in (0, 1):
            ei = emitter.emit_engine(e, parser, flags=flags)
            got = emitter.download()
            hdr, pairs, cands, cig = e.download_compact()
            ri = emitter.emit_results(parser, hdr, pairs, cands, cig, first_pair=first, flags=flags)
            want = emitter.download()
            assert (ei.n_bytes, ei.n_records, ei.n_written_pairs, ei.n_declined_pairs) == (ri.n_bytes, ri.n_records, ri.n_written_pairs, ri.n_declined_pairs)
            for a, b in zip(got, want):
                assert a.tobytes() == b.tobytes(), (first, flags)
            assert ei.n_written_pairs > n // 2 and ei.n_declined_pairs == 0 and len(got[0]) == ei.n_bytes > 100 * n
            if flags == 0 and first == 0:
                whole = got
            elif flags == 0:                                      # the second half alone: the corresponding slice of the whole
                data, off, state = whole
                assert state[first:].tobytes() == got[2].tobytes()
                assert (off[first:] - off[first]).tobytes() == got[1].tobytes()
                assert data[off[first]:].tobytes() == got[0].tobytes()
        if first == 0:
            e.close()
    # (e still holds the second half) a window parsed into again is gone
    parser.parse(text, fc.BIG_PAIRS, fc.BIG_BASES)
    with pytest.raises(aln.EngineError, match="parsed into since"):
        emitter.emit_engine(e, parser)
    # an engine whose batch came from host arrays has no text on the device
    d = parser.download()
    e.upload(d["bases"][:-1], d["base_off"][:201], d["ori"][:200])
    e.run()
    with pytest.raises(aln.EngineError, match="did not come from a psvr_fastq_t"):
        emitter.emit_engine(e, parser)
    # a batch that was not run
    parser.upload_to(e, first_pair=0, n_pairs=100)
    with pytest.raises(aln.EngineError, match="has not run"):
        emitter.emit_engine(e, parser)
    e.close()


# ---- the command ------------------------------------------------------------------------------------------------------------------------------
def _aln(tmp, tag, name, rname, extra, reads=None, stdin=None, env=None):
    w = ac.workdir(name)
    o = os.path.join(tmp, tag)
    cmd = [CLI, "aln", "-t", "4", "-o", o + ".bam", "-p", o + ".ori.bam"] + extra + [ac.index_dir(name), reads or os.path.join(w, rname + ".fq"), os.path.join(w, "header.sam")]
    r = subprocess.run(cmd, stdin=stdin, stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=dict(os.environ, **(env or {})), timeout=300)   # (a golden set takes seconds)
    assert r.returncode == 0, r.stderr.decode()[-2000:]
    return o, r.stderr.decode()


def _e2e(err):
    return json.loads([l for l in err.split("\n") if "e2e_json" in l][-1].split("e2e_json", 1)[1])


def _payload(o):
    return bam_stream.stream(o + ".bam"), bam_stream.stream(o + ".ori.bam")


def _check_same(o, want, what):
    got = _payload(o)
    assert got[0] == want[0], "%s: main file: %s" % (what, bam_stream.first_difference(got[0], want[0]))
    assert got[1] == want[1], "%s: ori file: %s" % (what, bam_stream.first_difference(got[1], want[1]))


@pytest.mark.parametrize("name,rname", CASES)
def test_cli_emit_device_writes_the_host_routes_files(name, rname):
    """with and without -Q; the declined pairs stay under 1 % of the pairs that reach the encoder, and the host formatter refuses nothing"""
    tmp = tempfile.mkdtemp(prefix="psvr_beg_")
    for q in ([], ["-Q"]):
        tag = "q" if q else "p"
        host, herr = _aln(tmp, "host_" + tag, name, rname, q)
        dev, derr = _aln(tmp, "dev_" + tag, name, rname, q + ["--emit-device"])
        assert "records on the device failed" not in derr and "parse on the device failed" not in derr
        assert '"emitter":"device"' in derr and '"parser":"device"' in derr and '"emitter":"host"' in herr
        _check_same(dev, _payload(host), "%s/%s %s" % (name, rname, tag))
        j, jh = _e2e(derr), _e2e(herr)
        assert j["emit_device_pairs"] + j["emit_declined_pairs"] == j["pairs"] and jh["emit_device_pairs"] == jh["emit_declined_pairs"] == jh["emit_spliced_pairs"] == 0
        assert j["emit_spliced_pairs"] == j["pairs"] or j["emit_declined_pairs"] > 0
        print("%s/%s %s: emit_device_pairs %d, emit_declined_pairs %d" % (name, rname, tag, j["emit_device_pairs"], j["emit_declined_pairs"]))
        assert j["emit_declined_pairs"] * 100 <= j["emit_device_pairs"] + j["emit_declined_pairs"]
        assert "@sam_parse1 ERROR" not in herr and "@sam_parse1 ERROR" not in derr
        assert j["dropped"] == jh["dropped"]


@pytest.fixture(scope="module")
def fx2_host():
    tmp = tempfile.mkdtemp(prefix="psvr_beg_")
    o, err = _aln(tmp, "host", "fx2", "reads150", [])
    return tmp, _payload(o)


@pytest.mark.parametrize("route", ["batch", "batch-bases", "sub-batch", "stdin", "gz", "deflate-device", "bgzf-fast", "compress-level"])
def test_cli_emit_device_over_batch_limits_input_routes_and_compressors(fx2_host, route):
    tmp, want = fx2_host
    fq = os.path.join(ac.workdir("fx2"), "reads150.fq")
    kw = {}
    extra = {"batch": ["--batch", "97"], "batch-bases": ["--batch-bases", "60000"], "sub-batch": ["--sub-batch", "31"], "deflate-device": ["--deflate-device"],
             "bgzf-fast": ["--bgzf-fast"], "compress-level": ["--compress-level", "1"]}.get(route, [])
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
    o, err = _aln(tmp, route, "fx2", "reads150", ["--emit-device"] + extra, **kw)
    if route == "stdin":
        os.close(rd)
        assert feeder.wait() == 0
    assert "on the device failed" not in err and '"emitter":"device"' in err
    _check_same(o, want, route)


def test_cli_emit_device_with_sort_writes_the_host_routes_sorted_file_and_index():
    tmp = tempfile.mkdtemp(prefix="psvr_beg_")
    host, _ = _aln(tmp, "host", "fx2", "reads150", ["--sort"])
    dev, err = _aln(tmp, "dev", "fx2", "reads150", ["--sort", "--emit-device"])
    assert "on the device failed" not in err and '"emitter":"device"' in err
    for ext in (".bam", ".bam.bai", ".ori.bam"):
        assert open(dev + ext, "rb").read() == open(host + ext, "rb").read(), ext


def _with_tabs(text, pairs):
    """the FASTQ text with a tab put into the comment of the first read of each listed pair"""
    lines = text.split(b"\n")
    for p in pairs:
        h = lines[8 * p]
        at = h.index(b" ") + 3
        lines[8 * p] = h[:at] + b"\t" + h[at:]
    return b"\n".join(lines)


def test_cli_declined_pairs_go_through_the_host_formatter():
    """three pairs with a tab in a comment, in two chunks of pairs (two pieces of --sub-batch, or one chunk of 4096 of a piece); the chunks behind
    them hold none and are spliced in from the device: the host route's files, three declined"""
    tmp = tempfile.mkdtemp(prefix="psvr_beg_")
    text = open(os.path.join(ac.workdir("fx1"), "reads150.fq"), "rb").read() * 3           # 6000 pairs: a piece of more than one chunk
    fq = os.path.join(tmp, "tabs.fq")
    with open(fq, "wb") as f:
        f.write(_with_tabs(text, (3, 700, 1999)))
    host, herr = _aln(tmp, "host", "fx1", "reads150", [], reads=fq)
    for extra, spliced in ((["--sub-batch", "1000"], 4000), ([], 6000 - 4096)):
        dev, derr = _aln(tmp, "dev%d" % len(extra), "fx1", "reads150", ["--emit-device"] + extra, reads=fq)
        _check_same(dev, _payload(host), "tabs " + " ".join(extra))
        j = _e2e(derr)
        assert j["emit_declined_pairs"] == 3 and j["emit_device_pairs"] == 5997 and j["emit_spliced_pairs"] == spliced, j
        assert j["dropped"] == _e2e(herr)["dropped"]
        assert [l for l in derr.split("\n") if "ERROR" in l] == [l for l in herr.split("\n") if "ERROR" in l]


def test_cli_emit_device_falls_back_to_the_host_formatter(fx2_host):
    tmp, want = fx2_host
    o, err = _aln(tmp, "fallback", "fx2", "reads150", ["--emit-device", "--sub-batch", "500"], env={"PSVR_PARSE_DEVICE_MAX_BYTES": "1000"})
    assert '"emitter":"host"' in err and '"parser":"host"' in err and '"emit_device_pairs":0' in err
    _check_same(o, want, "fallback")
