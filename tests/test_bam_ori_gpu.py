"""-m gpu: the second BAM file's device encoder on the MI355X.  psvr_bam_emit_ori_results (pansvr_amd.emit.BamEmitter.emit_ori_results)
against the files that tests/tools/bam_ori_device_check.cpp writes after holding the same rules to SamEmitter::ori_pair, byte for byte; and
psvr_bam_emit_ori_engine against psvr_bam_emit_ori_results on the same engine's compact download, with the engine form's refusals; and `panSVR aln --ori-device`
against the host route's files over the golden sets, the batch limits, the input routes, the compressors and the other device routes,
through declined pairs, resident pieces and its fallback to the host formatter."""
import gzip
import os
import subprocess
import tempfile

import numpy as np
import pytest

import aln_common as ac
import bam_ori_cases as oc
import fastq_cases as fc

pytestmark = pytest.mark.gpu
ENGINE_MFS = 520                                              # psvr_aln_params_default's min_filter_score: what aln.Engine(index) runs with


@pytest.fixture(scope="module")
def checker():
    return oc.build_checker(tempfile.mkdtemp(prefix="psvr_bog_"), False)


@pytest.fixture(scope="module")
def fx1():
    """(index, its header's size, a parser, an emitter)"""
    import synth
    import test_abi_gpu as tag
    from pansvr_amd.emit import BamEmitter
    from pansvr_amd.fastq import FastqParser
    index = tag._index("fx1")
    n_header = sum(1 for l in synth.header_text().split("\n") if l.startswith("@SQ"))
    parser, emitter = FastqParser(), BamEmitter(index)
    yield index, n_header, parser, emitter
    emitter.close(), parser.close(), index.close()


def _same(got, want, name):
    data, off, state = got
    for key, a in (("state", state.tobytes()), ("pair_off", off.tobytes()), ("bytes", data.tobytes())):
        b = want[key]
        if a != b:
            first = next((i for i, (x, y) in enumerate(zip(a, b)) if x != y), min(len(a), len(b)))
            raise AssertionError("%s: %s differs from the checker's (%d vs %d bytes, first at byte %d)" % (name, key, len(a), len(b), first))


def test_emit_ori_results_equal_the_checkers_files_on_every_case(checker, fx1):
    from pansvr_amd.aln import CAND_DTYPE, HDR_DTYPE, PAIR_DTYPE
    index, n_header, parser, emitter = fx1
    counts, states = set(), [0, 0, 0]
    for c in oc.cases():
        s, raw = oc.run_checker(checker, c["text"], c["cls"], c["seed"], c["mfs"], n_header=n_header)
        want = oc.split_out(raw)
        info = parser.parse(c["text"], fc.BIG_PAIRS, fc.BIG_BASES)
        assert info.n_pairs == want["P"], c["name"]
        arrays = [np.frombuffer(want[k], dtype=dt) for k, dt in (("hdr", HDR_DTYPE), ("pairs", PAIR_DTYPE), ("cands", CAND_DTYPE), ("cigar", np.uint32))]
        ei = emitter.emit_ori_results(parser, *arrays, min_filter_score=c["mfs"])
        assert (ei.n_bytes, ei.n_records, ei.n_written_pairs, ei.n_declined_pairs) == (want["n_bytes"], want["n_records"], want["n_written"], want["n_declined"]), c["name"]
        _same(emitter.download(), want, c["name"])
        if c["label"] == "declining":
            assert ei.n_declined_pairs == want["P"] and ei.n_bytes == 0, c["name"]
        else:
            assert ei.n_declined_pairs == 0, c["name"]
        counts.add(want["P"])
        for k in range(3):
            states[k] += s["state%d" % k]
    assert {1, 255, 256, 257, 4097} <= counts and all(n > 100 for n in states)
    # the emitter holds the records of its last run, whichever file they are for: a main-file run replaces them, a range that leaves the window is refused
    from pansvr_amd._lib import EngineError
    ori = emitter.download()[0].tobytes()
    emitter.emit_results(parser, *arrays)
    assert emitter.download()[0].tobytes() != ori
    with pytest.raises(EngineError, match="psvr_bam_emit_ori_results"):
        emitter.emit_ori_results(parser, *arrays, min_filter_score=oc.MFS, first_pair=1)


def test_emit_ori_engine_equals_emit_ori_results_on_the_compact_download(fx1):
    """parse -> upload_fastq -> run -> emit_ori_engine == emit_ori_results on the same engine's download_compact with the engine's own
    min_filter_score; then the second half of the window alone; a re-parsed window, an engine fed by psvr_engine_upload and a batch that was
    not run are refused"""
    from pansvr_amd import aln
    index, n_header, parser, emitter = fx1
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
        ei = emitter.emit_ori_engine(e, parser)
        got = emitter.download()
        hdr, pairs, cands, cig = e.download_compact()
        ri = emitter.emit_ori_results(parser, hdr, pairs, cands, cig, min_filter_score=ENGINE_MFS, first_pair=first)
        want = emitter.download()
        assert (ei.n_bytes, ei.n_records, ei.n_written_pairs, ei.n_declined_pairs) == (ri.n_bytes, ri.n_records, ri.n_written_pairs, ri.n_declined_pairs)
        for a, b in zip(got, want):
            assert a.tobytes() == b.tobytes(), first
        # (a quarter of fx1/reads150's records go to the second file)
        assert ei.n_written_pairs > n // 10 and ei.n_records == 2 * ei.n_written_pairs and ei.n_declined_pairs == 0 and len(got[0]) == ei.n_bytes > 300 * ei.n_written_pairs
        if first == 0:
            whole = got
            e.close()
        else:                                                     # the second half alone: the corresponding slice of the whole
            data, off, state = whole
            assert state[first:].tobytes() == got[2].tobytes()
            assert (off[first:] - off[first]).tobytes() == got[1].tobytes()
            assert data[off[first]:].tobytes() == got[0].tobytes()
    # (e still holds the second half) a window parsed into again is gone
    parser.parse(text, fc.BIG_PAIRS, fc.BIG_BASES)
    with pytest.raises(aln.EngineError, match="parsed into since"):
        emitter.emit_ori_engine(e, parser)
    # an engine whose batch came from host arrays has no text on the device
    d = parser.download()
    e.upload(d["bases"][:-1], d["base_off"][:201], d["ori"][:200])
    e.run()
    with pytest.raises(aln.EngineError, match="did not come from a psvr_fastq_t"):
        emitter.emit_ori_engine(e, parser)
    # a batch that was not run
    parser.upload_to(e, first_pair=0, n_pairs=100)
    with pytest.raises(aln.EngineError, match="has not run"):
        emitter.emit_ori_engine(e, parser)
    e.close()


# ---- the command ------------------------------------------------------------------------------------------------------------------------------
import bam_stream                                             # noqa: E402
import test_bam_emit_gpu as teg                               # noqa: E402  (its command helpers: _aln, _e2e, _payload, _check_same, _with_tabs)
from test_emu_aln import CASES                                # noqa: E402

ORI_FIELDS = ("ori_emitter", "ori_device_pairs", "ori_declined_pairs", "ori_spliced_pairs", "resident_pieces", "text_d2h_bytes")


@pytest.mark.parametrize("name,rname", CASES)
def test_cli_ori_device_writes_the_host_routes_files(name, rname):
    """with and without -Q: both files' inflated payload is the host route's, the ori payload the golden file's; no pair of a golden set is
    declined by the ori encoder; a line without the option ends as it did"""
    tmp = tempfile.mkdtemp(prefix="psvr_bog_")
    for q in ([], ["-Q"]):
        tag = "q" if q else "p"
        host, herr = teg._aln(tmp, "host_" + tag, name, rname, q)
        dev, derr = teg._aln(tmp, "dev_" + tag, name, rname, q + ["--ori-device"])
        assert "on the device failed" not in derr
        teg._check_same(dev, teg._payload(host), "%s/%s %s" % (name, rname, tag))
        golden = os.path.join(ac.HERE, "golden", name, rname + (".notori" if q else "") + ".ori.bam")
        if os.path.exists(golden):
            assert bam_stream.first_difference(bam_stream.stream(dev + ".ori.bam"), bam_stream.stream(golden)) is None
        j, jh = teg._e2e(derr), teg._e2e(herr)
        assert not any(k in jh for k in ORI_FIELDS) and list(j)[-6:] == list(ORI_FIELDS)
        assert j["ori_emitter"] == "device" and j["emitter"] == "device" and j["ori_declined_pairs"] == 0
        assert j["ori_device_pairs"] == j["ori_spliced_pairs"] == j["pairs"]
        assert j["text_d2h_bytes"] == 0                       # (a FASTQ file's text is the host's own)
        if j["emit_declined_pairs"] == 0:
            assert j["resident_pieces"] == j["pieces"]
        if j["resident_pieces"] == j["pieces"]:
            assert j["d2h_bytes"] == 0 < jh["d2h_bytes"]
        assert "ERROR" not in derr and j["dropped"] == jh["dropped"]


@pytest.mark.parametrize("route", ["batch", "batch-bases", "sub-batch", "stdin", "gz", "deflate-device", "stream-device"])
def test_cli_ori_device_over_batch_limits_input_routes_and_compressors(route):
    tmp, want = _fx2_host()
    fq = os.path.join(ac.workdir("fx2"), "reads150.fq")
    kw = {}
    extra = {"batch": ["--batch", "97"], "batch-bases": ["--batch-bases", "60000"], "sub-batch": ["--sub-batch", "31"], "deflate-device": ["--deflate-device"], "stream-device": ["--stream-device"]}.get(route, [])
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
    o, err = teg._aln(tmp, "ori_" + route, "fx2", "reads150", ["--ori-device"] + extra, **kw)
    if route == "stdin":
        os.close(rd)
        assert feeder.wait() == 0
    assert "on the device failed" not in err and '"ori_emitter":"device"' in err and '"ori_declined_pairs":0' in err
    teg._check_same(o, want, route)


_FX2 = []


def _fx2_host():
    if not _FX2:
        tmp = tempfile.mkdtemp(prefix="psvr_bog_")
        o, _ = teg._aln(tmp, "host", "fx2", "reads150", [])
        _FX2.append((tmp, teg._payload(o)))
    return _FX2[0]


def test_cli_ori_device_with_sort_device_writes_the_three_files_of_the_host_sort():
    tmp = tempfile.mkdtemp(prefix="psvr_bog_")
    host, _ = teg._aln(tmp, "host", "fx2", "reads150", ["--sort", "--deflate-device"])
    dev, err = teg._aln(tmp, "dev", "fx2", "reads150", ["--sort-device", "--ori-device"])
    assert "on the device failed" not in err and '"ori_emitter":"device"' in err and '"sorter":"device"' in err
    for ext in (".bam", ".bam.bai", ".ori.bam"):
        assert open(dev + ext, "rb").read() == open(host + ext, "rb").read(), ext


def test_cli_ori_device_behind_bam_device_keeps_resident_pieces_text_on_the_device():
    """-N --bam-device: four pieces, none with a declined pair: no results come to the host, and only the first piece's text"""
    import test_bam_device_gpu as tbd
    from test_fused_signal import GOLDEN, bam_of
    name, rname, n_pairs, flags = GOLDEN[0]
    tmp = tempfile.mkdtemp(prefix="psvr_bog_")
    bam = os.path.join(tmp, "in.bam")
    bam_of(name, rname, n_pairs, bam)
    opts = flags + ["--bam-device", "--stream-device", "--sub-batch", str(n_pairs // 4)]
    herr, want = tbd.aln(tmp, "plain", name, bam, opts, 70000)
    err, files = tbd.aln(tmp, "ori", name, bam, opts + ["--ori-device"], 70000)
    tbd.on_the_device(err, n_pairs)
    for f in ("o.bam", "p.bam"):
        assert bam_stream.first_difference(bam_stream.stream(os.path.join(tmp, "ori", f)), bam_stream.stream(os.path.join(tmp, "plain", f))) is None, f
    j, jh = teg._e2e(err.decode()), teg._e2e(herr.decode())
    window_bytes = int(tbd.STAT_LINE.search(err).group(5))
    assert j["pieces"] == jh["pieces"] >= 4 and j["resident_pieces"] == j["pieces"] and j["ori_declined_pairs"] == 0, j
    assert j["d2h_bytes"] == 0 < jh["d2h_bytes"] and 0 < j["text_d2h_bytes"] <= window_bytes // 3, (j, window_bytes)


def test_cli_ori_device_behind_mate_device():
    import test_aln_mate_device_gpu as tmd
    from test_fused_signal import GOLDEN, bam_of
    import signal_mate_cases as mc
    import test_signal as ts
    name, rname, n_pairs, _ = GOLDEN[0]
    tmp = tempfile.mkdtemp(prefix="psvr_bog_")
    bam_of(name, rname, n_pairs, os.path.join(tmp, "by_name.bam"))
    head, recs = tmd.records_of(os.path.join(tmp, "by_name.bam"))
    open(os.path.join(tmp, "in.bam"), "wb").write(ts.bgzf(head + b"".join(mc.by_position(recs))))
    inp = (tmp, os.path.join(tmp, "in.bam"), n_pairs, 0, ac.index_dir(name))
    opts = ["-D", "--mate-device", "--stream-device", "--sub-batch", str(n_pairs // 4)]
    herr, want = tmd.aln(inp, "plain", opts)
    err, files = tmd.aln(inp, "ori", opts + ["--ori-device"])
    assert b"failed" not in err
    for f in files:
        if f.endswith(".bam"):
            assert bam_stream.first_difference(bam_stream.stream(os.path.join(tmp, "ori", f)), bam_stream.stream(os.path.join(tmp, "plain", f))) is None, f
    j, jh = teg._e2e(err.decode()), teg._e2e(herr.decode())
    assert j["resident_pieces"] > 0 and j["ori_declined_pairs"] == 0 and j["ori_emitter"] == "device", j
    assert j["d2h_bytes"] < jh["d2h_bytes"] and j["text_d2h_bytes"] > 0
    if j["resident_pieces"] == j["pieces"]:
        assert j["d2h_bytes"] == 0


def test_cli_ori_device_declined_pairs_go_through_the_host_formatter():
    """the tab-comment input of the main encoder's test: the three pairs are declined by both encoders (their chunks are formatted on the host
    whole, the pieces that hold them are not resident), the files and the ERROR lines are the host route's"""
    tmp = tempfile.mkdtemp(prefix="psvr_bog_")
    text = open(os.path.join(ac.workdir("fx1"), "reads150.fq"), "rb").read() * 3           # 6000 pairs: a piece of more than one chunk
    fq = os.path.join(tmp, "tabs.fq")
    with open(fq, "wb") as f:
        f.write(teg._with_tabs(text, (3, 700, 1999)))
    host, herr = teg._aln(tmp, "host", "fx1", "reads150", [], reads=fq)
    jh = teg._e2e(herr)
    for extra, spliced, resident in ((["--sub-batch", "1000"], 4000, 4), ([], 6000 - 4096, 0)):
        dev, derr = teg._aln(tmp, "dev%d" % len(extra), "fx1", "reads150", ["--ori-device"] + extra, reads=fq)
        teg._check_same(dev, teg._payload(host), "tabs " + " ".join(extra))
        j = teg._e2e(derr)
        assert j["emit_declined_pairs"] == 3 and j["emit_spliced_pairs"] == spliced, j
        # (a pair with a tab whose score is over the gate is in state 0 for the second file: at most three are declined there)
        assert j["ori_declined_pairs"] <= 3 and j["ori_device_pairs"] + j["ori_declined_pairs"] == 6000 and j["ori_spliced_pairs"] >= spliced, j
        assert j["resident_pieces"] == resident and j["pieces"] == (6 if extra else 1), j
        assert 0 < j["d2h_bytes"] < jh["d2h_bytes"] or not resident
        assert j["dropped"] == jh["dropped"]
        assert sorted(l for l in derr.split("\n") if "ERROR" in l) == sorted(l for l in herr.split("\n") if "ERROR" in l)


def test_cli_ori_device_falls_back_to_the_host_formatter():
    tmp, want = _fx2_host()
    o, err = teg._aln(tmp, "fallback", "fx2", "reads150", ["--ori-device", "--sub-batch", "500"], env={"PSVR_PARSE_DEVICE_MAX_BYTES": "1000"})
    j = teg._e2e(err)
    assert j["ori_emitter"] == "host" and j["emitter"] == "host" and j["parser"] == "host" and j["ori_device_pairs"] == 0 and j["resident_pieces"] == 0
    teg._check_same(o, want, "fallback")
