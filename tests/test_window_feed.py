"""`panSVR aln -N --bam-device`'s blocking hand-over without a GPU (tests/tools/window_feed_check.cpp, built with AddressSanitizer + UBSan):
WindowFeed on two threads, and the signal step's thread, a route that offers windows and FastqReader::read_window put together as the
command puts them together.  Whatever ends or fails on either side, neither thread may wait for the other for good: every run has a time
limit, and running into it is the failure these tests are about.  Where pairs flow, the text the reader prints is `panSVR signal -N -D`'s."""
import os
import subprocess

import pytest

import signal_device_cases as sc
import test_signal as ts
from test_signal_device_route import run

LIMIT = 60                                                     # seconds; a run takes a fraction of one


@pytest.fixture(scope="module")
def check():
    return sc.build("window_feed_check", sc.tmpdir("wf"), True)


@pytest.fixture(scope="module")
def signal_text():
    """(directory, in.bam of 300 pairs, the file with `signal -N -D`'s stdout, that text, the host route's stderr)"""
    tmp = sc.tmpdir("wf")
    recs, _ = ts.make_pairs(20241, 300)
    bam, fq = os.path.join(tmp, "in.bam"), os.path.join(tmp, "signal.fq")
    sc.write_bam(bam, recs)
    h, _ = run(sc.CLI, tmp, bam, ["-D"], "h", device=False)
    assert h.returncode == 0 and h.stdout.count(b"\n") == 300 * 8
    open(fq, "wb").write(h.stdout)
    return tmp, bam, fq, h.stdout, h.stderr


FEED_CASES = {
    "producer_ends": "next -1\n",
    "consumer_fails_first": "offer 0 (no parser) next -1\n",
    "consumer_fails_mid": "next 1 at 0 left 10 same 1\nnext 1 at 100 left 6\noffer 4 (piece 2) next -1\n",
    "consumer_aborts": "next 1 offers 10 7 ()\n",
    "two_windows": "at 0 left 5\nat 11 left 3\nat 22 left 1\nat 0 left 3\nat 11 left 1\nnext 0 offers 5 0 3 ()\n",
    "closed_twice": "next 0\n",
}


@pytest.mark.parametrize("case", sorted(FEED_CASES))
def test_neither_side_of_the_feed_waits_for_one_that_is_gone(check, case):
    r = subprocess.run([check, "feed", case], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=LIMIT)
    assert r.returncode == 0 and r.stdout.decode() == FEED_CASES[case], (r.stdout, r.stderr.decode()[-2000:])


def step(check, bam, fq, window, piece, fail=None):
    return subprocess.run([check, "step", bam, fq, str(window), str(piece)] + ([fail] if fail else []), stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=LIMIT)


@pytest.mark.parametrize("window,piece", [(300, 1 << 20), (100, 37), (7, 37)])
def test_the_reader_takes_every_window_in_pieces(check, signal_text, window, piece):
    tmp, bam, fq, text, _ = signal_text
    r = step(check, bam, fq, window, piece)
    assert r.returncode == 0 and r.stdout == text, r.stderr.decode()[-2000:]
    pieces = sum(-(-min(window, 300 - p) // piece) for p in range(0, 300, window))     # (a piece never spans two windows)
    assert b"pieces: %d from windows, 0 from the feed\n" % pieces in r.stderr


@pytest.mark.parametrize("fail,handed,pieces", [("create", 0, 0), ("parse_signal:1", 0, 0), ("parse_signal:4", 100, 3), ("download:2", 37, 1), ("text:3", 74, 2)])
def test_a_failing_call_of_the_readers_side_reaches_the_producer(check, signal_text, fail, handed, pieces):
    """windows of 100 pairs, pieces of 37 (so 37, 37 and 26 pairs a window): the producer hears of the failure (it is waiting in offer(), or offers
    next), says how many pairs were taken, and the host route hands the rest over through the PairFeed, silent for those: the text is whole"""
    tmp, bam, fq, text, _ = signal_text
    r = step(check, bam, fq, 100, 37, fail)
    assert r.returncode == 0 and r.stdout == text, r.stderr.decode()[-2000:]
    call = fail.split(":")[0]
    assert b"step rc 0, %d pairs handed over before the route was left: fastq %s: injected failure of %s\n" % (handed, call.encode(), call.encode()) in r.stderr
    assert b"pieces: %d from windows, %d from the feed\n" % (pieces, -(-(300 - handed) // 37)) in r.stderr


def test_a_signal_step_that_ends_in_front_of_the_route_ends_the_reader(check, signal_text):
    """a truncated file and one with a corrupt member: the statistics pass refuses them, the step's thread ends with status 1 before the route
    has started -- as on the host fused route, with its message -- and the reader, waiting for the first window, is told"""
    tmp, bam, fq, _, _ = signal_text
    data = open(bam, "rb").read()
    second = int.from_bytes(data[16:18], "little") + 1
    broken = bytearray(data)
    broken[second + 200] ^= 0x55
    for name, blob in (("corrupt", bytes(broken)), ("cut", data[:second + 5000])):
        other = os.path.join(tmp, name + ".bam")
        open(other, "wb").write(blob)
        h, _ = run(sc.CLI, tmp, other, ["-D"], "hb", device=False)
        r = step(check, other, fq, 100, 37)
        assert h.returncode == 1 and r.returncode == 11 and r.stdout == b"", (name, r.stderr.decode()[-2000:])
        said = [l for l in h.stderr.split(b"\n") if l.startswith(b"[panSVR-amd] signal: ")]
        assert len(said) == 1 and said[0] + b"\n" in r.stderr, name
        assert b"step rc 1, -1 pairs handed over" in r.stderr and b"pieces: 0 from windows, 0 from the feed\n" in r.stderr, name
