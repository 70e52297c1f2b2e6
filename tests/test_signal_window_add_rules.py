"""The kept window of psvr_signal_window_add without a GPU: the one-lane host build of the add rule of pansvr_amd/csrc/signal_window_device.h
(a run's window written behind the bytes the kept window holds; tiles of the whole window, an add's first tile off a 16-byte boundary, two
adds inside one tile) as a program of its own, plain and under AddressSanitizer + UBSan (tests/tools/signal_window_add_check.cpp), against
plain concatenation of the runs' windows.  The program itself checks that an add changes no byte but its own."""
import os
import subprocess

import numpy as np
import pytest

import signal_device_cases as sc
import test_signal_window_rules as wr
from signal_window_cases import TILE


@pytest.fixture(scope="module")
def tools():
    tmp = sc.tmpdir("swa")
    return {"plain": sc.build("signal_window_add_check", tmp, False), "asan": sc.build("signal_window_add_check", tmp, True), "window": sc.build("signal_window_check", tmp, False)}


def run_of(rng, n_bytes, states=(1, 2, 0, 1, 1, 2, 2, 0)):
    """[(state, text)] of a run whose window has n_bytes bytes: pairs in these states (again and again), texts of 1 to 200 bytes until n_bytes
    are reached; a state-0 pair has none.  n_bytes == 0: no pair at all"""
    pairs, left, k = [], n_bytes, 0
    while left > 0:
        st = states[k % len(states)]
        n = 0 if st == 0 else min(left, int(rng.randint(1, 201)))
        pairs.append((st, rng.randint(0, 256, n, dtype=np.uint8).tobytes()))
        left, k = left - n, k + 1
    return pairs


def window_of(pairs):
    return b"".join(t for _, t in pairs)


def adds(tools, runs, **bad):
    """runs: [(restart, pairs)] or [(restart, pairs, keyword arguments of write_case)].  (the lines of stdout, the kept window) on which the two
    builds agree"""
    tmp = sc.tmpdir("swa")
    args = []
    for k, run in enumerate(runs):
        d = os.path.join(tmp, str(k))
        os.mkdir(d)
        args += [str(int(run[0]))] + wr.write_case(d, run[1], **(run[2] if len(run) > 2 else {}))[:3]
    got = []
    for build in ("plain", "asan"):
        out = os.path.join(tmp, "out.bin")
        r = subprocess.run([tools[build], out] + args, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120)
        assert r.returncode == 0, (build, r.returncode, r.stderr.decode()[-3000:])
        got.append((r.stdout.decode().splitlines(), open(out, "rb").read()))
    assert got[0] == got[1]
    return got[0]


def added(line):
    w = line.split()
    assert w[0] == "added", line
    return tuple(int(x) for x in w[1:])


def test_a_first_add_is_the_window_of_the_run(tools):
    """with and without restart: what sw_window_host makes of the same run (tests/tools/signal_window_check.cpp)"""
    rng = np.random.RandomState(1)
    pairs = run_of(rng, 2 * TILE + 777)
    tmp = sc.tmpdir("swa")
    rc, _, want = wr.window({"plain": tools["window"], "asan": tools["window"]}, tmp, pairs)
    assert rc == 0 and want == window_of(pairs)
    for restart in (0, 1):
        lines, win = adds(tools, [(restart, pairs)])
        assert win == want and added(lines[0]) == (0, len(want), len(want), sum(st != 0 for st, _ in pairs), sum(st == 2 for st, _ in pairs))


@pytest.mark.parametrize("residue", range(16))
def test_a_second_add_begins_at_every_residue(tools, residue):
    rng = np.random.RandomState(100 + residue)
    first, second = run_of(rng, 3 * 16 + residue), run_of(rng, TILE + 1234)
    lines, win = adds(tools, [(1, first), (0, second)])
    assert added(lines[1])[:2] == (48 + residue, TILE + 1234) and win == window_of(first) + window_of(second)


def test_empty_and_tiny_adds(tools):
    """0 bytes with 0 pairs; pairs in state 0 only; 0 device bytes with host pairs only; 1 byte from either source"""
    rng = np.random.RandomState(2)
    a = run_of(rng, 1000)
    host_only = run_of(rng, 300, states=(2, 0, 2))
    one_dev, one_host = [(1, b"x")], [(0, b""), (2, b"y")]
    runs = [(1, a), (0, []), (0, [(0, b"")] * 5), (0, host_only), (0, one_dev), (0, one_host), (0, run_of(rng, 50))]
    lines, win = adds(tools, runs)
    assert win == b"".join(window_of(p) for _, p in runs)
    assert [added(l)[1] for l in lines] == [1000, 0, 0, 300, 1, 1, 50]
    assert added(lines[3])[4] - added(lines[2])[4] == sum(st == 2 for st, _ in host_only) and added(lines[-1])[3] == sum(st != 0 for _, p in runs for st, _ in p)
    # the same, beginning with nothing
    lines, win = adds(tools, [(1, []), (0, one_host), (0, one_dev)])
    assert win == b"yx" and [added(l)[:2] for l in lines] == [(0, 0), (0, 1), (1, 1)]


@pytest.mark.parametrize("n", [2, 3])
def test_adds_inside_one_tile(tools, n):
    rng = np.random.RandomState(3 + n)
    runs = [(int(k == 0), run_of(rng, 501 + 333 * k)) for k in range(n)]
    lines, win = adds(tools, runs)
    assert added(lines[-1])[2] < TILE and win == b"".join(window_of(p) for _, p in runs)


@pytest.mark.parametrize("end", [TILE - 1, TILE, TILE + 1])
def test_an_add_ends_around_a_tile(tools, end):
    """from base 0 and from an unaligned base; the next add begins where it ended"""
    rng = np.random.RandomState(end)
    for base in (0, 1003):
        runs = [(1, run_of(rng, base)), (0, run_of(rng, end - base)), (0, run_of(rng, 700))]
        lines, win = adds(tools, runs)
        assert added(lines[1])[:3] == (base, end - base, end) and added(lines[2])[0] == end
        assert win == b"".join(window_of(p) for _, p in runs)


def test_an_add_spans_three_tiles_from_an_unaligned_base(tools):
    rng = np.random.RandomState(9)
    base = TILE - 4093                                                   # (an odd residue: 3 modulo 16)
    runs = [(1, run_of(rng, base)), (0, run_of(rng, 4093 + TILE + 5)), (0, run_of(rng, 3 * TILE))]
    lines, win = adds(tools, runs)
    assert base % 16 == 3 and added(lines[1])[0] // TILE == 0 and (added(lines[1])[2] - 1) // TILE == 2
    assert win == b"".join(window_of(p) for _, p in runs)
    # every pair from the host: every tile finds many segments, the first one of the add among them
    runs = [(1, run_of(rng, base)), (0, run_of(rng, 4093 + TILE + 5, states=(2,)))]
    _, win = adds(tools, runs)
    assert win == b"".join(window_of(p) for _, p in runs)


def test_restart_empties_the_window(tools):
    rng = np.random.RandomState(10)
    a, b, c = run_of(rng, TILE + 99), run_of(rng, 77), run_of(rng, 3000)
    lines, win = adds(tools, [(1, a), (0, b), (1, c), (0, b)])
    assert win == window_of(c) + window_of(b) and added(lines[2])[:3] == (0, 3000, 3000) and added(lines[3])[0] == 3000


def test_a_refused_add_leaves_the_window_untouched(tools):
    """every reason of sw_args_bad, between two adds: the window is the concatenation of the accepted ones"""
    rng = np.random.RandomState(11)
    a, c = run_of(rng, 1500), run_of(rng, 900)
    b = run_of(rng, 2000, states=(0, 1, 2, 2, 1, 2))
    sizes = [len(t) for st, t in b if st == 2]
    H, off = len(sizes), [0]
    for n in sizes:
        off.append(off[-1] + n)
    swapped = off[:3] + [off[2] - 1] + off[4:]
    none = run_of(rng, 400, states=(1, 0))
    for why, pairs, kw in (("a negative count", b, dict(n_host=-1)), ("a negative count", b, dict(host_bytes=-1)), ("not the number", b, dict(n_host=H - 1, host_off=off[:-1], host_bytes=off[-2])),
                           ("not the number", b, dict(n_host=H + 1, host_off=off + [off[-1]])), ("without a host pair", none, dict(host_bytes=5)), ("no offsets", b, dict(host_off=[])), ("first offset", b, dict(host_off=[1] + off[1:])),
                           ("not monotone", b, dict(host_off=swapped)), ("last offset", b, dict(host_bytes=off[-1] + 1)), ("last offset", b, dict(host_off=off[:-1] + [off[-1] - 1]))):
        lines, win = adds(tools, [(1, a), (0, pairs, kw), (0, c)])
        assert lines[1].startswith("refused: ") and why in lines[1], (why, lines)
        assert win == window_of(a) + window_of(c) and added(lines[2])[0] == 1500
    lines, win = adds(tools, [(1, a), (0, b), (0, c)])
    assert win == window_of(a) + window_of(b) + window_of(c)
