"""-m gpu: `panSVR aln --mate-device` on the MI355X: a position-sorted BAM goes in, its blocks are mated, judged and formatted in GPU memory, the
windows of the runs are put together there and parsed where they lie, and the files are those of two routes this option does not touch:
the host fused route (`aln in.bam`) and the two steps (`signal in.bam > fq`, `aln fq`) -- whatever the pieces of the input
(PSVR_INFLATE_BATCH), of the blocks (--block-records) and of the batches (--sub-batch: the kept window's pair threshold) are; with
--stream-device the BAM streams, with --sort-device the three files of `aln --sort --deflate-device`.  Every command is a fresh child under
its own time limit."""
import gzip
import os
import re
import struct
import subprocess
import tempfile

import pytest

import aln_common as ac
import signal_device_cases as sc
import signal_mate_cases as mc
import test_signal as ts
from test_fused_signal import CLI, GOLDEN, bam_of
from test_mate_window_route import LEFT_LINE, STAT_LINE, sorted_crafted

pytestmark = pytest.mark.gpu

# what the route does with these files, checked without a GPU on the host-memory backend (tests/tools/mate_window_route_check.cpp): no call of
# it declines anything on them.  name: {--block-records: (blocks, pairs of the by-name pass)}
SHAPE = {"fx1": {None: (2, 76), 64: (64, 1646)}, "fx2": {None: (2, 51), 64: (48, 587)}}
PIECES = re.compile(rb'"pieces":(\d+)')


def records_of(path):
    """(the inflated header, [record]) of a BAM file"""
    d = gzip.decompress(open(path, "rb").read())
    at = 8 + struct.unpack_from("<i", d, 4)[0]
    n_ref = struct.unpack_from("<i", d, at)[0]
    at += 4
    for _ in range(n_ref):
        at += 8 + struct.unpack_from("<i", d, at)[0]
    head, recs = d[:at], []
    while at < len(d):
        n = 4 + struct.unpack_from("<i", d, at)[0]
        recs.append(d[at:at + n])
        at += n
    return head, recs


@pytest.fixture(scope="module")
def inputs():
    """name: (directory, in.bam, pairs, pairs the host formats, index): the golden reads in coordinate order, and the crafted rule pairs"""
    out = {}
    for name, rname, n_pairs, _ in GOLDEN:
        tmp = tempfile.mkdtemp(prefix="psvr_matedev_")
        bam_of(name, rname, n_pairs, os.path.join(tmp, "by_name.bam"))
        head, recs = records_of(os.path.join(tmp, "by_name.bam"))
        assert len(recs) == 2 * n_pairs
        open(os.path.join(tmp, "in.bam"), "wb").write(ts.bgzf(head + b"".join(mc.by_position(recs))))
        out[name] = (tmp, os.path.join(tmp, "in.bam"), n_pairs, 0, ac.index_dir(name))
    tmp = tempfile.mkdtemp(prefix="psvr_matedev_")
    sc.write_bam(os.path.join(tmp, "in.bam"), sorted_crafted())
    out["crafted"] = (tmp, os.path.join(tmp, "in.bam"), 50, 1, ac.index_dir("fx1"))
    return out


def run(tmp, tag, args, piece=None, stdout=None):
    env = dict(os.environ)
    env.pop("PSVR_INFLATE_BATCH", None)
    if piece:
        env["PSVR_INFLATE_BATCH"] = str(piece)
    r = subprocess.run([CLI] + args, stdout=stdout or subprocess.PIPE, stderr=subprocess.PIPE, env=env, timeout=120)
    assert r.returncode == 0, (tag, r.stderr.decode()[-2500:])
    return r.stderr


def aln(inp, tag, options, piece=None, reads=None, header=None):
    """runs the command under its own time limit; (stderr, {file name behind the tag: bytes}).  reads, header: FASTQ text and the header file it is
    read with (a BAM input writes its own)"""
    tmp, bam, _, _, index = inp
    d = os.path.join(tmp, tag)
    os.makedirs(d, exist_ok=True)
    for f in os.listdir(d):
        os.remove(os.path.join(d, f))
    sam = "-S" in options
    err = run(tmp, tag, ["aln"] + options + ["-o", os.path.join(d, "o.sam" if sam else "o.bam"), "-p", os.path.join(d, "p.sam" if sam else "p.bam"), index, reads or bam,
                         header or os.path.join(d, "h.sam")], piece)
    return err, {f: open(os.path.join(d, f), "rb").read() for f in sorted(os.listdir(d))}


def block_flags(block):
    return ["--block-records", str(block)] if block else []


def on_the_device(err, inp, sub=65536):
    """the route ran to its end: its summary line, the parser of every piece, no line of a side that gave up; the line's numbers"""
    m = STAT_LINE.search(err)
    assert m and not LEFT_LINE.search(err) and b" failed (" not in err, err.decode()[-2500:]
    pairs, on_device, by_host, by_name, blocks, windows, window_bytes = (int(x) for x in m.groups())
    assert pairs == inp[2] and by_host == inp[3] and on_device == pairs - by_host and window_bytes > 0     # (-D: every pair is written)
    assert windows <= (on_device + by_host) // sub + 1 and int(PIECES.search(err).group(1)) >= windows >= 1
    assert b'"parser":"device"' in err
    return by_name, blocks, windows


@pytest.fixture(scope="module")
def yardsticks(inputs):
    """(name, --block-records): the SAM files of the host fused route and of the two steps, the former's header and status file and status lines"""
    cache = {}

    def get(name, block):
        if (name, block) not in cache:
            inp = inputs[name]
            err, fused = aln(inp, "fused", ["-D", "-S"] + block_flags(block))
            fq = os.path.join(inp[0], "two_steps.fq")
            with open(fq, "wb") as f:
                run(inp[0], "signal", ["signal", "-D"] + block_flags(block) + ["-H", os.path.join(inp[0], "two.h.sam"), "-S", os.path.join(inp[0], "two.status"), inp[1]], stdout=f)
            _, two = aln(inp, "two", ["-S"], reads=fq, header=os.path.join(inp[0], "two.h.sam"))
            assert fused["o.sam"] == two["o.sam"] and fused["p.sam"] == two["p.sam"] and len(fused["p.sam"]) > len(fused["h.sam"])
            cache[(name, block)] = (fused, [l for l in err.split(b"\n") if l.startswith(b"BAM/CRAM status")])
        return cache[(name, block)]
    return get


@pytest.mark.parametrize("piece", [1000, 70000])
@pytest.mark.parametrize("block", [64, None])
@pytest.mark.parametrize("sub", [97, 65536])
@pytest.mark.parametrize("name", ["fx1", "fx2", "crafted"])
def test_sam_files_are_those_of_the_host_fused_route_and_of_the_two_steps(inputs, yardsticks, name, sub, block, piece):
    inp = inputs[name]
    want, status_lines = yardsticks(name, block)
    err, files = aln(inp, "sam", ["-D", "-S", "--mate-device", "--sub-batch", str(sub)] + block_flags(block), piece)
    assert files["o.sam"] == want["o.sam"] and files["p.sam"] == want["p.sam"]
    assert files["h.sam"] == want["h.sam"] and files["h.sam.status"] == want["h.sam.status"]
    assert [l for l in err.split(b"\n") if l.startswith(b"BAM/CRAM status")] == status_lines and len(status_lines) == 2
    by_name, blocks, _ = on_the_device(err, inp, sub)
    if name in SHAPE:
        assert (blocks, by_name) == SHAPE[name][block]
    assert b"ignored" not in err and b"refused" not in err


@pytest.mark.parametrize("name", ["fx1", "fx2"])
def test_stream_device_writes_the_host_fused_routes_bam_streams(inputs, name):
    import bam_reader
    import bam_stream
    inp = inputs[name]
    aln(inp, "bam_host", ["-D"])
    err, _ = aln(inp, "stream", ["-D", "--mate-device", "--stream-device"], 70000)
    on_the_device(err, inp)
    assert b'"emitter":"device"' in err and b"ignored" not in err
    for f in ("o.bam", "p.bam"):
        got = os.path.join(inp[0], "stream", f)
        bam_reader.check_bgzf(got)
        diff = bam_stream.first_difference(bam_stream.stream(got), bam_stream.stream(os.path.join(inp[0], "bam_host", f)))
        assert diff is None, "%s: %s" % (f, diff)


@pytest.mark.parametrize("name", ["fx1", "fx2"])
def test_sort_device_writes_the_three_files_of_the_host_fused_sort(inputs, name):
    inp = inputs[name]
    _, want = aln(inp, "sort_host", ["-D", "--sort", "--deflate-device"])
    err, files = aln(inp, "sort", ["-D", "--mate-device", "--sort-device"], 70000)
    on_the_device(err, inp)
    assert b"ignored" not in err
    names = [f for f in want if f.endswith((".bam", ".bai"))]
    assert len(names) == 3 and all(files[f] == want[f] for f in names), [f for f in names if files.get(f) != want[f]]


def test_decreasing_positions_leave_the_route_on_one_line(inputs):
    tmp = tempfile.mkdtemp(prefix="psvr_matedev_")
    inp = (tmp, mc.write(os.path.join(tmp, "in.bam"), mc.decreasing()), 0, 0, ac.index_dir("fx1"))
    _, want = aln(inp, "host", ["-D", "-S"])
    err, files = aln(inp, "dev", ["-D", "-S", "--mate-device"])
    own = mc.own_lines(err, b"[panSVR-amd] aln --mate-device")
    m = LEFT_LINE.search(err)
    assert len(own) == 1 and m and m.group(1) == b"signal run_pos" and int(m.group(3)) == 0, own
    assert files == want and files["h.sam"] and files["h.sam.status"]
