"""`panSVR aln -N --bam-device`'s route without a GPU: pansvr_amd/csrc/signal_device_route.h in window mode over the host-memory backend, the window
built by the host build of signal_window_device.h, with a reader that takes every window in pieces and prints what it took
(tests/tools/bam_device_route_check.cpp, built with AddressSanitizer + UBSan).  The printed text must be `panSVR signal -N`'s stdout: whole
when the route runs to its end, and also when any call on either side fails at its first or at a later occurrence and the host route takes
over, silent for the pairs that were handed over."""
import os
import re

import pytest

import signal_device_cases as sc
import test_signal as ts
from test_signal_device_route import last_status, run

CALLS = ("store_create", "store_append_bgzf", "store_footprint", "store_drop", "store_chain_info", "signal_create", "signal_run", "signal_pairs", "signal_side", "signal_stats",
         "host_alloc", "signal_window", "window_parse")
STAT_LINE = re.compile(rb"aln --bam-device: (\d+) pairs, (\d+) formatted on the device, (\d+) formatted by the host, (\d+) runs, (\d+) window bytes, peak footprint (\d+) chunks \((\d+) bytes\)")
LEFT_LINE = re.compile(rb"aln --bam-device: (.*) failed \((.*)\): (\d+) pairs are handed over, the host fused route reads the file from its beginning, silent up to there\n")


@pytest.fixture(scope="module")
def route():
    return sc.build("bam_device_route_check", sc.tmpdir("bdr"), True)


def held_to_host(route, tmp, bam, flags, env):
    h, hf = run(sc.CLI, tmp, bam, flags, "h", device=False)
    e = {k: v for k, v in env.items() if v is not None}
    d, df = run(route, tmp, bam, flags, "d", e)
    assert h.returncode == 0 and d.returncode == 0, d.stderr.decode()[-3000:]
    assert d.stdout == h.stdout and df == hf
    assert last_status(d.stderr) == last_status(h.stderr)
    assert d.stdout.count(b"STAT_") == (1 if d.stdout else 0)
    assert b"signal --signal-device" not in d.stderr
    return d


@pytest.fixture(scope="module")
def files():
    out = {}
    tmp = sc.tmpdir("bdr")
    for flags, seed in sc.FLAG_SETS:
        recs, _ = ts.make_pairs(seed, 600)
        out[seed] = os.path.join(tmp, "in%d.bam" % seed)
        sc.write_bam(out[seed], recs)
    recs, _ = ts.make_pairs(20241, 1200)
    out["long"] = os.path.join(tmp, "long.bam")
    sc.write_bam(out["long"], recs)
    return tmp, out


@pytest.mark.parametrize("limit", [37, 1 << 20])
@pytest.mark.parametrize("piece", [1000, 70000])
@pytest.mark.parametrize("flags,seed", sc.FLAG_SETS)
def test_the_pieces_the_reader_takes_are_the_host_routes_text(route, files, flags, seed, piece, limit):
    tmp, bams = files
    d = held_to_host(route, tmp, bams[seed], flags, {"PSVR_INFLATE_BATCH": str(piece), "PSVR_CHECK_PIECE_PAIRS": str(limit)})
    m = STAT_LINE.search(d.stderr)
    assert m and not LEFT_LINE.search(d.stderr), d.stderr.decode()[-2000:]
    pairs, on_device, by_host, runs, window_bytes, chunks, _ = (int(x) for x in m.groups())
    assert pairs == 600 and by_host > 0 and on_device > 300 and window_bytes == len(d.stdout) and chunks == 1 and runs >= 2
    assert d.stderr.count(b"Wrong base!") >= by_host


@pytest.mark.parametrize("call", CALLS)
def test_every_call_failing_on_either_side_leaves_the_host_routes_text(route, files, call):
    """on the first piece and on a later one (pieces of 70 000 bytes: at least one whole member each; the reader takes 37 pairs a piece)"""
    tmp, bams = files
    once = call in ("store_create", "signal_create", "store_chain_info", "signal_stats")
    for nth in (1,) if once else (1, 3):
        d = held_to_host(route, tmp, bams["long"], ["-D"], {"PSVR_INFLATE_BATCH": "70000", "PSVR_CHECK_PIECE_PAIRS": "37", "PSVR_CHECK_FAIL": "%s:%d" % (call, nth)})
        m = LEFT_LINE.findall(d.stderr)
        assert len(m) == 1, (call, nth, d.stderr.decode()[-2000:])
        said, why, done = m[0][0].decode(), m[0][1], int(m[0][2])
        assert b"injected failure of " + call.encode() in why and not STAT_LINE.search(d.stderr)
        if call == "window_parse":
            # -D: every pair is written, so the pairs handed over are exactly the pieces the reader printed before its nth one failed
            assert said == "taking a window" and done == 37 * (nth - 1)
        elif call in ("store_chain_info", "signal_stats"):
            assert done == 1200
        elif call == "host_alloc":
            assert done == 0
        else:
            assert call.replace("store_", "").replace("signal_", "").replace("_", " ") in said.replace("_", " "), said
            assert (done > 0) == (nth > 1 or call == "store_drop"), (call, nth, done)
        assert done <= 1200


def test_damage_in_mid_file_is_named_and_the_host_route_takes_over(route, files):
    tmp, bams = files
    data = open(bams["long"], "rb").read()
    members, at = [], 0
    while at < len(data):
        members.append(at)
        at += int.from_bytes(data[at + 16:at + 18], "little") + 1
    assert len(members) >= 6
    broken = bytearray(data)
    broken[members[3] + 200] ^= 0x55
    for name, blob, why in (("corrupt", bytes(broken), b"corrupt BGZF block"), ("cut_member", data[:members[4] - 100], b"truncated BGZF block"),
                            ("cut_record", data[:members[4]], b"truncated BAM stream")):
        other = os.path.join(tmp, name + ".bam")
        open(other, "wb").write(blob)
        d = held_to_host(route, tmp, bams["long"], ["-D"], {"PSVR_INFLATE_BATCH": "70000", "PSVR_CHECK_PIECE_PAIRS": "37", "PSVR_CHECK_ROUTE_INPUT": other})
        m = LEFT_LINE.search(d.stderr)
        assert m and why in m.group(2), (name, d.stderr.decode()[-2000:])
        assert 0 < int(m.group(3)) < 1200, name


def test_a_damaged_input_ends_as_the_host_route_ends(route, tmp_path):
    recs, _ = ts.make_pairs(20241, 300)
    tmp = str(tmp_path)
    data, _ = sc.bam_file(recs)
    second = int.from_bytes(data[16:18], "little") + 1
    broken = bytearray(data)
    broken[second + 200] ^= 0x55
    for name, blob in (("corrupt", bytes(broken)), ("cut", data[:second + 5000])):
        bam = os.path.join(tmp, name + ".bam")
        open(bam, "wb").write(blob)
        h, hf = run(sc.CLI, tmp, bam, ["-D"], "h", device=False)
        d, df = run(route, tmp, bam, ["-D"], "d", {"PSVR_CHECK_PIECE_PAIRS": "37"})
        assert h.returncode == d.returncode == 1 and d.stdout == h.stdout and df == hf, name
        assert d.stderr == h.stderr and b"[panSVR-amd] signal: " in h.stderr, name


@pytest.mark.parametrize("state", [3, 4, 5])
def test_an_error_pair_hands_the_front_over_and_returns_its_state(route, tmp_path, state):
    front = [r for _, pair, _ in sc.crafted()[:6] for r in pair]
    tmp = str(tmp_path)
    bam, short = os.path.join(tmp, "in.bam"), os.path.join(tmp, "front.bam")
    sc.write_bam(bam, front + sc.error_pairs()[state] + front)
    sc.write_bam(short, front)
    flags = ["-D", "--isize", "100,300,500"]
    want, _ = run(sc.CLI, tmp, short, flags, "w", device=False)
    h, _ = run(sc.CLI, tmp, bam, flags, "h", device=False)
    d, _ = run(route, tmp, bam, flags, "d", {"PSVR_CHECK_PIECE_PAIRS": "4"})
    assert want.returncode == 0 and h.returncode == -6 and d.returncode == 30 + state
    assert d.stdout == want.stdout and d.stdout.count(b"\n") == 6 * 8
    assert b"route returned state %d behind 6 pairs\n" % state in d.stderr
    msg = [l for l in h.stderr.split(b"\n") if l.startswith(b"[panSVR-amd] signal: ")]
    assert len(msg) == 1 and msg[0] + b"\n" in d.stderr
