"""-m gpu: the FASTQ parser's device route on the MI355X.  psvr_fastq_parse (pansvr_amd.fastq.FastqParser) against the files that
tests/fastq_check.cpp writes after holding the same rules to fastq_batch.h, byte for byte; the hand-over to an engine; and
`panSVR aln --parse-device` against the reference's records and SAM files, over the batch limits and input routes, and through its
fallback to the host parser."""
import gzip
import os
import subprocess
import tempfile

import numpy as np
import pytest

import aln_common as ac
import fastq_cases as fc
from test_emu_aln import CASES, normalise

pytestmark = pytest.mark.gpu
CLI = fc.CLI
KEYS = ("line_start", "name_end", "base_off", "ori", "bases")


@pytest.fixture(scope="module")
def checker():
    return fc.build_checker(tempfile.mkdtemp(prefix="psvr_fqg_"), False)


@pytest.fixture(scope="module")
def parser():
    from pansvr_amd.fastq import FastqParser
    p = FastqParser()
    yield p
    p.close()


def _got(parser, text, at_end, max_pairs, max_bases):
    i = parser.parse(text, max_pairs, max_bases, at_end=bool(at_end))
    assert i.reserved == 0
    d = parser.download()
    d["info"] = [i.n_pairs, i.used_bytes, i.total_bases, i.n_lines, i.stop]
    return d


def _same(got, want, name):
    assert got["info"] == want["info"], "%s: info %s, the host parser's %s" % (name, got["info"], want["info"])
    for k in KEYS:
        a, b = got[k].tobytes(), want[k].tobytes()
        if a != b:
            first = next(i for i, (x, y) in enumerate(zip(a, b)) if x != y) if len(a) == len(b) else -1
            raise AssertionError("%s: %s differs (%d vs %d bytes, first at byte %d)" % (name, k, len(a), len(b), first))


def test_parser_bytes_equal_the_host_parsers_on_every_case(checker, parser):
    T = fc.constants(checker)["tile_bytes"]
    n_fx2 = 0
    for name, text, at_end, max_pairs, max_bases in fc.cases(T):
        want = fc.split_out(fc.run_checker(checker, text, at_end, max_pairs, max_bases))
        _same(_got(parser, text, at_end, max_pairs, max_bases), want, name)
        if name == "fx2/reads150":
            n_fx2 = len(text)
    assert n_fx2 > 100 * T                                  # every scan of that case spans many workgroups


def test_a_text_cut_on_both_sides_of_a_tile_boundary_gives_the_whole(checker, parser):
    T = fc.constants(checker)["tile_bytes"]
    text = fc.sixteen_pairs()
    n = len(text)
    assert n > T + 64
    whole = fc.split_out(fc.run_checker(checker, text, 1, fc.BIG_PAIRS, fc.BIG_BASES))
    assert whole["info"][0] == 16
    cuts = [0, 1, 15, 16, T - 17, T - 16, T - 1, T, T + 1, T + 15, T + 16, T + 17, n // 2, n - 2, n - 1, n]
    assert len(cuts) == 16 and any(c < T for c in cuts) and any(c > T for c in cuts)
    for c in cuts:
        a = _got(parser, text[:c], 0, fc.BIG_PAIRS, fc.BIG_BASES)
        u = a["info"][1]
        b = _got(parser, text[u:], 1, fc.BIG_PAIRS, fc.BIG_BASES)
        joined = {"info": [a["info"][0] + b["info"][0], u + b["info"][1], a["info"][2] + b["info"][2], whole["info"][3], whole["info"][4]],
                  "line_start": np.concatenate([a["line_start"], b["line_start"][1:] + np.uint64(u)]),
                  "name_end": np.concatenate([a["name_end"], b["name_end"]]),
                  "base_off": np.concatenate([a["base_off"], b["base_off"][1:] + a["info"][2]]),
                  "ori": np.concatenate([a["ori"], b["ori"]]),
                  "bases": np.concatenate([a["bases"][:-1], b["bases"]])}
        _same(joined, whole, "cut at %d" % c)


def test_engine_takes_the_parsed_batch_device_to_device(parser):
    """parse -> upload_to(engine) -> run -> download == Engine.upload of the downloaded arrays -> run -> download; then the second half alone"""
    from pansvr_amd import aln
    import test_abi_gpu as tag
    text = open(os.path.join(ac.workdir("fx1"), "reads150.fq"), "rb").read()
    info = parser.parse(text, fc.BIG_PAIRS, fc.BIG_BASES)
    P = info.n_pairs
    assert P == 2000 and info.stop == 2
    d = parser.download()
    bases, base_off, ori = d["bases"][:-1], d["base_off"], d["ori"]
    lens = np.diff(base_off)
    index = tag._index("fx1")
    for first, n in ((0, P), (P // 2 + 1, P - P // 2 - 1)):
        e1, e2 = aln.Engine(index), aln.Engine(index)
        parser.upload_to(e1, first_pair=first, n_pairs=n)
        e2.upload(bases, base_off[2 * first:2 * (first + n) + 1], ori[2 * first:2 * (first + n)])
        outs = []
        for e in (e1, e2):
            e.run()
            r, p, c = e.download()
            outs.append((p.tobytes(), ac.engine_records(r, p, c, ori[2 * first:], lens[2 * first:], 0, n)))
            e.close()
        assert outs[0] == outs[1], "pairs [%d, %d)" % (first, first + n)
        assert len(outs[0][1]) == n
    # a range that leaves the parsed window is refused
    e = aln.Engine(index)
    with pytest.raises(aln.EngineError):
        parser.upload_to(e, first_pair=P - 1, n_pairs=2)
    e.close(), index.close()


def _run(tmp, tag, name, rname, extra, reads=None, stdin=None, env=None):
    w = ac.workdir(name)
    o = os.path.join(tmp, tag)
    cmd = [CLI, "aln", "-S", "-t", "4", "-o", o + ".sam", "-p", o + ".ori.sam", "--records", o + ".jsonl", "--trace"] + extra + \
          [ac.index_dir(name), reads or os.path.join(w, rname + ".fq"), os.path.join(w, "header.sam")]
    r = subprocess.run(cmd, stdin=stdin, stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=dict(os.environ, **(env or {})))
    assert r.returncode == 0, r.stderr.decode()[-2000:]
    return o, r.stderr.decode()


@pytest.mark.parametrize("name,rname", CASES)
def test_cli_parse_device_matches_reference_records_and_sam_files(name, rname):
    tmp = tempfile.mkdtemp(prefix="psvr_fqg_")
    o, err = _run(tmp, "dev", name, rname, ["--parse-device"])
    assert "parse on the device failed" not in err
    assert '"parser":"device"' in err
    got = [l for l in open(o + ".jsonl").read().split("\n") if l.strip()]
    want = ac.golden_lines(name, rname)
    assert len(got) == len(want)
    bad = [i for i, (a, b) in enumerate(zip(want, got)) if normalise(a) != normalise(b)]
    assert not bad, "%d/%d pairs differ; first %d:\nref: %s\ngpu: %s" % (len(bad), len(want), bad[0], want[bad[0]], got[bad[0]])
    for ext, gext in ((".sam", ".sam.gz"), (".ori.sam", ".ori.sam.gz")):
        with gzip.open(os.path.join(ac.golden_dir(name), rname + gext), "rb") as f:
            assert open(o + ext, "rb").read() == f.read(), "%s differs from the reference's file" % ext


@pytest.fixture(scope="module")
def fx2_single():
    tmp = tempfile.mkdtemp(prefix="psvr_fqg_")
    o, err = _run(tmp, "one", "fx2", "reads150", ["--parse-device"])
    assert "parse on the device failed" not in err
    return tmp, {ext: open(o + ext, "rb").read() for ext in (".sam", ".ori.sam", ".jsonl")}


@pytest.mark.parametrize("route", ["batch", "batch-bases", "sub-batch", "stdin", "gz"])
def test_cli_parse_device_over_batch_limits_and_input_routes(fx2_single, route):
    tmp, one = fx2_single
    fq = os.path.join(ac.workdir("fx2"), "reads150.fq")
    kw = {}
    extra = {"batch": ["--batch", "97"], "batch-bases": ["--batch-bases", "60000"], "sub-batch": ["--sub-batch", "31"]}.get(route, [])
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
    o, err = _run(tmp, route, "fx2", "reads150", ["--parse-device"] + extra, **kw)
    if route == "stdin":
        os.close(rd)
        assert feeder.wait() == 0
    assert "parse on the device failed" not in err and '"parser":"device"' in err
    if route in ("batch", "batch-bases", "sub-batch"):
        assert err.count("Processing ") >= 5 or route == "sub-batch"
    for ext, want in one.items():
        assert open(o + ext, "rb").read() == want, (route, ext)


def test_cli_parse_device_falls_back_to_the_host_parser(fx2_single):
    tmp, one = fx2_single
    o, err = _run(tmp, "fallback", "fx2", "reads150", ["--parse-device", "--sub-batch", "500"], env={"PSVR_PARSE_DEVICE_MAX_BYTES": "1000"})
    assert err.count("FASTQ parse on the device failed (") == 1 and "parsing on the host threads from here on" in err
    assert '"parser":"host"' in err
    for ext, want in one.items():
        assert open(o + ext, "rb").read() == want, ext
