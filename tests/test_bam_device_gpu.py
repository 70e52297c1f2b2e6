"""-m gpu: `panSVR aln -N --bam-device` on the MI355X: a name-sorted BAM goes in, its pairs are formatted as FASTQ text and parsed in GPU memory,
and the files are those of the routes they replace -- the reference's two steps' SAM files (tests/golden/fused), the reference's BAM
streams with --stream-device, the three files of `aln -N -D --sort --deflate-device` with --sort-device -- whatever the pieces of the input
(PSVR_INFLATE_BATCH: several windows) and of the batches (--sub-batch: pieces cut inside a window) are."""
import os
import re
import subprocess
import tempfile

import pytest

import aln_common as ac
import signal_device_cases as sc
from test_fused_signal import CLI, GOLDEN, _golden, bam_of

pytestmark = pytest.mark.gpu

STAT_LINE = re.compile(rb"aln --bam-device: (\d+) pairs, (\d+) formatted on the device, (\d+) formatted by the host, (\d+) runs, (\d+) window bytes, peak footprint (\d+) chunks \((\d+) bytes\)")


@pytest.fixture(scope="module")
def inputs():
    """name: (directory, in.bam)"""
    out = {}
    for name, rname, n_pairs, _ in GOLDEN:
        tmp = tempfile.mkdtemp(prefix="psvr_bamdev_")
        bam_of(name, rname, n_pairs, os.path.join(tmp, "in.bam"))
        out[name] = (tmp, os.path.join(tmp, "in.bam"))
    return out


def aln(tmp, tag, name, bam, options, piece=None, index=None):
    """runs the command under its own time limit; (stderr, {file name behind the tag: bytes})"""
    d = os.path.join(tmp, tag)
    os.makedirs(d, exist_ok=True)
    for f in os.listdir(d):
        os.remove(os.path.join(d, f))
    env = dict(os.environ)
    env.pop("PSVR_INFLATE_BATCH", None)
    if piece:
        env["PSVR_INFLATE_BATCH"] = str(piece)
    sam = "-S" in options
    r = subprocess.run([CLI, "aln", "-N"] + options + ["-o", os.path.join(d, "o.sam" if sam else "o.bam"), "-p", os.path.join(d, "p.sam" if sam else "p.bam"), index or ac.index_dir(name), bam,
                        os.path.join(d, "h.sam")], stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=env, timeout=120)
    assert r.returncode == 0, r.stderr.decode()[-2500:]
    return r.stderr, {f: open(os.path.join(d, f), "rb").read() for f in sorted(os.listdir(d))}


def on_the_device(err, n_pairs, runs_at_least=1):
    """the route ran to its end: its statistics line, the parser of every piece, no line of a stage that gave up"""
    m = STAT_LINE.search(err)
    assert m, err.decode()[-2500:]
    pairs, on_device, by_host, runs, window_bytes, _, _ = (int(x) for x in m.groups())
    assert pairs == n_pairs and on_device + by_host <= n_pairs and runs >= runs_at_least and window_bytes > 0
    assert b'"parser":"device"' in err and b"failed" not in err
    return on_device, by_host


@pytest.mark.parametrize("piece", [1000, 70000])
@pytest.mark.parametrize("sub", ["97", "65536"])
@pytest.mark.parametrize("name,rname,n_pairs,flags", GOLDEN)
def test_sam_files_are_the_references_two_steps(inputs, name, rname, n_pairs, flags, sub, piece):
    tmp, bam = inputs[name]
    err, files = aln(tmp, "sam", name, bam, flags + ["-S", "--bam-device", "--sub-batch", sub], piece)
    want = _golden(name, rname)
    assert files["o.sam"] == want[0] and files["p.sam"] == want[1]
    on_device, by_host = on_the_device(err, n_pairs, 2)
    assert on_device == n_pairs and by_host == 0                          # (-D: every pair is written, none of these reads has an odd base code)
    host, _ = aln(tmp, "sam_host", name, bam, flags + ["-S", "--sub-batch", sub])
    assert files["h.sam"] == open(os.path.join(tmp, "sam_host", "h.sam"), "rb").read() and files["h.sam.status"] == open(os.path.join(tmp, "sam_host", "h.sam.status"), "rb").read()
    assert [l for l in err.split(b"\n") if l.startswith(b"BAM/CRAM status")] == [l for l in host.split(b"\n") if l.startswith(b"BAM/CRAM status")]


@pytest.mark.parametrize("name,rname,n_pairs,flags", GOLDEN)
def test_stream_device_writes_the_references_bam_streams(inputs, name, rname, n_pairs, flags):
    import bam_reader
    import bam_stream
    tmp, bam = inputs[name]
    err, files = aln(tmp, "stream", name, bam, flags + ["--bam-device", "--stream-device"], 70000)
    on_the_device(err, n_pairs)
    assert b'"emitter":"device"' in err and b"ignored" not in err
    for f, ext in (("o.bam", ".bam"), ("p.bam", ".ori.bam")):
        got = os.path.join(tmp, "stream", f)
        bam_reader.check_bgzf(got)
        diff = bam_stream.first_difference(bam_stream.stream(got), bam_stream.stream(os.path.join(ac.HERE, "golden", "fused", "%s_%s%s" % (name, rname, ext))))
        assert diff is None, "%s: %s" % (ext, diff)


@pytest.mark.parametrize("name,rname,n_pairs,flags", GOLDEN)
def test_sort_device_writes_the_three_files_of_the_host_fused_sort(inputs, name, rname, n_pairs, flags):
    tmp, bam = inputs[name]
    _, want = aln(tmp, "sort_host", name, bam, flags + ["--sort", "--deflate-device"])
    err, files = aln(tmp, "sort", name, bam, flags + ["--bam-device", "--sort-device"], 70000)
    on_the_device(err, n_pairs)
    assert b"ignored" not in err
    names = [f for f in want if f.endswith((".bam", ".bai"))]
    assert len(names) == 3 and all(files[f] == want[f] for f in names), [f for f in names if files.get(f) != want[f]]


def test_state_2_pairs_take_their_place(inputs):
    """the crafted pairs of every rule edge (one of them with a base code that has no letter: the host formats it, the window holds it at its
    place) through the fx1 index: both files are those of the host fused route.  The two pairs with a read of 2047 / 2048 bases stay out: the
    engine takes reads of up to 1600 bases, and `aln` ends on a longer one on every route"""
    tmp = tempfile.mkdtemp(prefix="psvr_bamdev_")
    bam = os.path.join(tmp, "in.bam")
    cases = [c for c in sc.crafted() if not c[0].startswith("len2047")]
    assert len(cases) == len(sc.crafted()) - 2 and sum(c[2] == 2 for c in cases) == 1
    sc.write_bam(bam, [r for _, pair, _ in cases for r in pair])
    _, want = aln(tmp, "host", "fx1", bam, ["-D", "-S"])
    for piece in (None, 1000):
        err, files = aln(tmp, "dev", "fx1", bam, ["-D", "-S", "--bam-device", "--sub-batch", "7"], piece)
        on_device, by_host = on_the_device(err, len(cases))
        assert by_host == 1 and on_device == len(cases) - 1
        # (reads drawn at random find little in the index: what there is to write is in the ori file, names, comments and qualities from the window)
        assert files == want and len(files["p.sam"]) > len(files["h.sam"])
