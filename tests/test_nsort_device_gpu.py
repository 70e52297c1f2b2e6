"""-m gpu: `panSVR sort --nsort-device` and the device order of plain `panSVR sort -n` on the MI355X.  The yardstick is the file of
`panSVR sort -n --deflate-device`, whose own order (psvr_sort_order_names) is held to the restatement, Python's sorted() on (name, flag & 0xc0, index):
the golden BAMs tests/test_sort_device_gpu.py uses, a header-only file, the names of tests/name_cases.py, pieces of 1 000 and 70 000
compressed bytes; the output is the -N input of `panSVR signal`."""
import gzip
import os
import subprocess
import tempfile

import numpy as np
import pytest

import bam_stream
import inflate_cases as ic
import name_cases as nc
import test_signal as ts
from test_bam_store_gpu import REFS

pytestmark = pytest.mark.gpu
CLI = ts.CLI
VARIANTS = {"default": {}, "batch-1000": {"PSVR_INFLATE_BATCH": "1000"}, "batch-70000": {"PSVR_INFLATE_BATCH": "70000"}}
GOLDEN = {os.path.relpath(fn, os.path.join(ic.HERE, "golden")): fn for fn in ic.golden_bams()}
_TMP = tempfile.mkdtemp(prefix="psvr_nsdev_")
_INPUT, _HOST = {}, {}


def _sort(flags, inp, out, env=None):
    r = subprocess.run([CLI, "sort", "-t", "4"] + flags + ["-o", out, inp], stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=dict(os.environ, **(env or {})), timeout=300)
    return r.returncode, r.stderr.decode(), open(out, "rb").read() if os.path.exists(out) else None, os.path.exists(out + ".bai")


def _input(name):
    if name not in _INPUT:
        fn = GOLDEN.get(name) or os.path.join(_TMP, name.replace("/", "_") + ".in.bam")
        if name == "header-only":
            ts.write_bam(fn, [], REFS)
        elif name == "name-cases":
            ts.write_bam(fn, nc.records(nc.groups()["everything"], seed=6) + nc.bulk(5000, 31), REFS)
        elif name == "pairs":
            recs, refs = ts.make_pairs(23, 1200)
            ts.write_bam(fn, [recs[i] for i in np.random.RandomState(4).permutation(len(recs))], refs)
        _INPUT[name] = fn
    return _INPUT[name]


def _host(name):
    """(stderr, the file) of `sort -n --deflate-device` on that input, made once: the yardstick of the device route, itself held to the restatement below"""
    if name not in _HOST:
        rc, err, data, bai = _sort(["-n", "--deflate-device"], _input(name), os.path.join(_TMP, name.replace("/", "_") + ".host.bam"))
        assert rc == 0 and not bai, err
        _HOST[name] = (err, data)
    return _HOST[name]


def _records(bam_bytes):
    return bam_stream.split(gzip.decompress(bam_bytes))[1]


@pytest.mark.parametrize("name", sorted(GOLDEN) + ["header-only", "name-cases", "pairs"])
def test_plain_name_order_is_computed_on_the_device(name):
    err, data = _host(name)
    recs_in, got = _records(open(_input(name), "rb").read()), _records(data)
    if recs_in:
        assert "name order, ordered on the device" in err and "failed" not in err, err
    # the file holds the input's records (the bin is recomputed: bytes 14-15 are left out) in the restated order
    strip = lambda r: r[:14] + r[16:]
    assert [strip(r) for r in got] == [strip(recs_in[i]) for i in nc.restated_order(recs_in)]
    assert b"SO:queryname" in gzip.decompress(data)[:200]


@pytest.mark.parametrize("variant", sorted(VARIANTS))
@pytest.mark.parametrize("name", sorted(GOLDEN) + ["header-only", "name-cases", "pairs"])
def test_cli_writes_the_file_of_name_order_with_deflate_device(name, variant):
    herr, want = _host(name)
    rc, err, got, bai = _sort(["--nsort-device"], _input(name), os.path.join(_TMP, "%s.%s.bam" % (name.replace("/", "_"), variant)), VARIANTS[variant])
    assert rc == 0 and "failed" not in err and "records kept on the device" in err and "name order" in err, err[-2000:]
    assert got is not None and got == want and not bai, "%s %s: the file differs" % (name, variant)
    if variant == "default":
        print(name, err.strip().split("\n")[-1])


def test_the_output_is_the_name_sorted_input_of_signal():
    herr, want = _host("pairs")
    dev = os.path.join(_TMP, "pairs.signal.bam")
    rc, err, got, bai = _sort(["--nsort-device"], _input("pairs"), dev)
    assert rc == 0 and got == want, err
    out = []
    for fn, tag in ((dev, "dev"), (os.path.join(_TMP, "pairs.host.bam"), "host")):
        r = subprocess.run([CLI, "signal", "-N", "-D", "-H", os.path.join(_TMP, tag + ".h.sam"), "-S", os.path.join(_TMP, tag + ".s.txt"), fn], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)
        assert r.returncode == 0, r.stderr.decode()
        out.append(r.stdout)
    assert out[0] == out[1] and out[0].count(b"\n") >= 8 * 900
