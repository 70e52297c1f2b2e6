"""The window of a signal run without a GPU: the one-lane host build of pansvr_amd/csrc/signal_window_device.h (what psvr_signal_window's kernels
run: segment table by a scan, output tiles that find and copy their segments) as a program of its own, plain and under AddressSanitizer +
UBSan (tests/tools/signal_window_check.cpp), against plain concatenation: the text `panSVR signal -N` writes for the same pairs."""
import os
import subprocess

import pytest

import signal_device_cases as sc
import signal_window_cases as wc


@pytest.fixture(scope="module")
def tools():
    tmp = sc.tmpdir("swr")
    return {"rules": sc.build("signal_device_check", tmp, False), "plain": sc.build("signal_window_check", tmp, False), "asan": sc.build("signal_window_check", tmp, True)}


def write_case(tmp, pairs, n_host=None, host_off=None, host_bytes=None):
    """the checker's three input files for [(state, text)]; the keyword arguments replace what follows from the pairs"""
    toff, at, off = [], 0, [0]
    for st, t in pairs:
        toff.append(at)
        if st == 1:
            at += len(t)
        elif st == 2:
            off.append(off[-1] + len(t))
    text, host = b"".join(t for st, t in pairs if st == 1), b"".join(t for st, t in pairs if st == 2)
    n_host = len(off) - 1 if n_host is None else n_host
    host_off = off if host_off is None else host_off
    lines = ["%d %d %d %d" % (len(pairs), len(text), len(host) if host_bytes is None else host_bytes, n_host)] + ["%d %d" % (st, o) for (st, _), o in zip(pairs, toff)]
    if n_host > 0:
        lines.append(" ".join(str(x) for x in host_off))
    names = [os.path.join(tmp, n) for n in ("case.txt", "text.bin", "host.bin", "out.bin")]
    open(names[0], "w").write("\n".join(lines) + "\n")
    open(names[1], "wb").write(text)
    open(names[2], "wb").write(host)
    return names


def window(tools, tmp, pairs, **kw):
    """(exit status, stdout, window) on which the two builds agree"""
    names = write_case(tmp, pairs, **kw)
    got = []
    for build in ("plain", "asan"):
        if os.path.exists(names[3]):
            os.remove(names[3])
        r = subprocess.run([tools[build]] + names, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120)
        assert r.returncode in (0, 3), (build, r.stderr.decode()[-3000:])
        got.append((r.returncode, r.stdout, open(names[3], "rb").read() if r.returncode == 0 else None))
    assert got[0] == got[1]
    return got[0]


def segments(stdout):
    return [tuple(int(x) for x in l.split()) for l in stdout.decode().splitlines()]


@pytest.fixture(scope="module")
def runs(tools):
    """name: (pairs, text, segments, window) of every pattern"""
    out = {}
    for name, (states, error) in wc.PATTERNS.items():
        tmp = sc.tmpdir("swr")
        recs, front = wc.records(states, error=error)
        s, tab, text = wc.expected(recs, front, tmp, tools["rules"])
        assert s["first_error"] == (-1 if error is None else len(states)) and [t[0] for t in tab[:len(states)]] == states, name
        pairs = wc.cut_by_table(text, tab)
        assert b"".join(t for st, t in pairs if st == 1) == open(os.path.join(tmp, "dump.fq"), "rb").read(), name
        rc, stdout, win = window(tools, tmp, pairs)
        assert rc == 0, name
        out[name] = (pairs, text, segments(stdout), win)
    return out


@pytest.mark.parametrize("name", sorted(wc.PATTERNS))
def test_window_equals_plain_concatenation(runs, name):
    pairs, text, segs, win = runs[name]
    assert win == text == b"".join(t for _, t in pairs)
    H = sum(st == 2 for st, _ in pairs)
    assert len(segs) == 2 * H + 1 and [s[0] for s in segs] == [k & 1 for k in range(2 * H + 1)]
    # the table tiles the window without a gap, and each source is walked front to back without a gap
    at, src_at = 0, [0, 0]
    for src, off, n, out in segs:
        assert out == at and off == src_at[src] and n >= 0
        at, src_at[src] = at + n, src_at[src] + n
    assert at == len(text)


def test_patterns_are_what_they_are_called(runs):
    assert all(s[0] == 0 for s in runs["no_host_pair"][2]) and len(runs["no_host_pair"][2]) == 1 and 0 < len(runs["no_host_pair"][1]) < wc.TILE
    assert all(st == 2 for st, _ in runs["every_pair_host"][0]) and all(n == 0 for src, _, n, _ in runs["every_pair_host"][2] if src == 0)
    assert len(runs["every_pair_host"][1]) > wc.TILE                     # (more than one tile, every tile with many segments)
    segs = runs["host_first_last_adjacent"][2]
    assert segs[0][2] == 0 and segs[-1][2] == 0 and sum(1 for s in segs[2:-1:2] if s[2] == 0) >= 8      # host pairs first, last, and side by side
    assert runs["error_pair"][1] and len(runs["error_pair"][0]) == 18 and b"@behind" not in runs["error_pair"][1]
    for name in ("error_pair_first", "empty_run", "only_zeros"):
        assert runs[name][1] == b"" and runs[name][3] == b"" and len(runs[name][2]) == 1


def test_segments_start_on_every_residue_of_source_and_destination(runs):
    seen = {0: set(), 1: set(), "out": set()}
    for _, _, segs, _ in runs.values():
        for src, off, n, out in segs:
            if n:
                seen[src].add(off % 16), seen["out"].add(out % 16)
                seen[(src, "both")] = seen.get((src, "both"), set()) | {(off % 16, out % 16)}
    assert seen[0] == seen[1] == seen["out"] == set(range(16))
    assert len(seen[(0, "both")]) > 40 and len(seen[(1, "both")]) > 40   # (source and destination differ modulo 16 in many ways)


def test_window_lengths_around_a_tile(tools):
    """a whole number of tiles, and one byte more (test_patterns_are_what_they_are_called has one below a tile)"""
    tmp = sc.tmpdir("swr")
    have = len(wc.host_route(wc.sized_records(0), tmp, wc.ISIZE)[0])
    whole = (have // wc.TILE + 1) * wc.TILE
    assert whole == 2 * wc.TILE
    for target in (whole, whole + 1):
        recs = wc.sized_records(target - have)
        _, tab, text = wc.expected(recs, recs, tmp, tools["rules"])
        assert len(text) == target
        rc, _, win = window(tools, tmp, wc.cut_by_table(text, tab))
        assert rc == 0 and win == text


def test_bad_arguments_are_refused(tools, runs):
    pairs = runs["zeros_in_between"][0]
    sizes = [len(t) for st, t in pairs if st == 2]
    H, off = len(sizes), [0]
    for n in sizes:
        off.append(off[-1] + n)
    tmp = sc.tmpdir("swr")
    assert window(tools, tmp, pairs)[0] == 0
    swapped = off[:3] + [off[2] - 1] + off[4:]
    for why, kw in ((b"not the number", dict(n_host=H - 1, host_off=off[:-1], host_bytes=off[-2])), (b"not the number", dict(n_host=H + 1, host_off=off + [off[-1]])),
                    (b"not monotone", dict(host_off=swapped)), (b"last offset", dict(host_bytes=off[-1] + 1)), (b"last offset", dict(host_off=off[:-1] + [off[-1] - 1])),
                    (b"first offset", dict(host_off=[1] + off[1:]))):
        rc, stdout, _ = window(tools, tmp, pairs, **kw)
        assert rc == 3 and stdout.startswith(b"refused: ") and why in stdout, (kw, stdout)
    rc, stdout, _ = window(tools, tmp, runs["no_host_pair"][0], host_bytes=5)
    assert rc == 3 and b"without a host pair" in stdout
