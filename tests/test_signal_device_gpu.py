"""-m gpu: `panSVR signal -N --signal-device` on the MI355X against `panSVR signal -N` of the same build: stdout byte for byte, the header file,
the status file and the final status line; the statistics line says that the device ran.  No input in an error state is run here (the host loop
aborts on those: tests/test_signal_device_route.py holds them on the CPU)."""
import os
import re
import subprocess

import pytest

import signal_device_cases as sc
import test_signal as ts

pytestmark = pytest.mark.gpu
STAT_LINE = re.compile(rb"signal --signal-device: (\d+) pairs, (\d+) written on the device, (\d+) declined to the host, (\d+) runs, (\d+) text bytes, peak footprint (\d+) chunks \((\d+) bytes\)")


def run(tmp, bam, flags, device, env=None):
    tag = "d" if device else "h"
    e = dict(os.environ)
    e.update(env or {})
    r = subprocess.run([sc.CLI, "signal", "-N"] + (["--signal-device"] if device else []) + flags + ["-H", os.path.join(tmp, tag + ".sam"), "-S", os.path.join(tmp, tag + ".txt"), bam],
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=e, timeout=120)
    return r, open(os.path.join(tmp, tag + ".sam"), "rb").read(), open(os.path.join(tmp, tag + ".txt"), "rb").read()


def last_status(err):
    at = err.rindex(b"BAM/CRAM status: ave_read_depth")                 # ("Wrong base!" comes without a newline: the line may begin with some)
    return err[at:err.index(b"\n", at)]


def both_routes(tmp, recs, flags, env=None):
    """the device route's statistics, after it has been held to the host route"""
    bam = os.path.join(tmp, "in.bam")
    sc.write_bam(bam, recs)
    h, h_sam, h_txt = run(tmp, bam, flags, False)
    d, d_sam, d_txt = run(tmp, bam, flags, True, env)
    assert h.returncode == 0 and d.returncode == 0, d.stderr.decode()[-2000:]
    assert b"failed" not in d.stderr and b"refused" not in d.stderr, d.stderr.decode()[-2000:]
    assert d.stdout == h.stdout and d_sam == h_sam and d_txt == h_txt
    assert last_status(d.stderr) == last_status(h.stderr)
    assert d.stderr.count(b"Wrong base!") == h.stderr.count(b"Wrong base!") and d.stderr.count(b" wrong ISIZE: ") == h.stderr.count(b" wrong ISIZE: ")
    m = STAT_LINE.search(d.stderr)
    assert m, d.stderr.decode()[-2000:]
    return [int(x) for x in m.groups()], d.stdout


@pytest.mark.parametrize("flags,seed", sc.FLAG_SETS)
def test_device_route_writes_the_host_routes_files(tmp_path, flags, seed):
    recs, _ = ts.make_pairs(seed, 600)
    (pairs, written, declined, runs, text_bytes, chunks, _), out = both_routes(str(tmp_path), recs, flags)
    assert pairs == 600 and runs == 1 and declined > 0 and written > 300 and chunks == 1
    assert 0 < text_bytes < len(out)                                    # (the declined pairs' text is the host's)
    # the wire format, as test_signal looks at it: `aln`'s comment parser reads tokens 0-8 and the two flag quartets
    names = out.split(b"\n")[0:-1:4]
    assert all(l.startswith(b"@pair") for l in names) and sum(b"_STAT_" in l for l in names) == 1 and b"_STAT_" in names[0]
    for l in names[:50]:
        tok = l.split(b" ", 1)[1].split(b"_")
        assert all(t.lstrip(b"-").isdigit() for t in tok[:9]) and len(tok[9]) == 4 and len(tok[10]) == 4


@pytest.mark.parametrize("piece", [1000, 70000])
def test_small_pieces(tmp_path, piece):
    recs, _ = ts.make_pairs(20241, 600)
    (pairs, _, declined, runs, _, _, _), _ = both_routes(str(tmp_path), recs, ["-D"], {"PSVR_INFLATE_BATCH": str(piece)})
    assert pairs == 600 and declined > 0 and runs >= 2


def test_small_chunks_are_filled_and_released_and_the_footprint_stays_bounded(tmp_path):
    recs, _ = ts.make_pairs(20244, 1200)
    chunk = 80000
    (pairs, _, _, runs, _, chunks, nbytes), _ = both_routes(str(tmp_path), recs, ["-D", "-U", "-I", "22"],
                                                           {"PSVR_INFLATE_BATCH": "20000", "PSVR_BAM_STORE_CHUNK_BYTES": str(chunk), "PSVR_BAM_STORE_SEG_BYTES": "4096"})
    # about 330 KB of records in pieces of one member: several chunks are filled, never more than the one being filled, the one with the
    # carried record and the spare are held
    assert pairs == 1200 and runs >= 5 and 2 <= chunks <= 3 and nbytes == chunks * chunk


def test_crafted_edges_and_a_header_only_file(tmp_path):
    recs = [r for _, pair, _ in sc.crafted() for r in pair]
    (pairs, written, declined, _, _, _, _), _ = both_routes(str(tmp_path), recs, [])
    assert pairs == len(sc.crafted()) and declined == 1 and written > 30
    (pairs, written, declined, runs, text_bytes, chunks, _), out = both_routes(str(tmp_path), [], ["-D"])
    assert (pairs, written, declined, text_bytes) == (0, 0, 0, 0) and out == b""
