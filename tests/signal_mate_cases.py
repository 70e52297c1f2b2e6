"""What the tests of `panSVR signal --mate-device` share: position-sorted inputs (test_signal's make_pairs in coordinate order, and a crafted
file with the smallest shapes at which the mate rules can go wrong), the two stand-alone checkers' builds, and the command's runner."""
import os
import struct
import subprocess

import numpy as np

import signal_device_cases as sc
import test_signal as ts

CLI = sc.CLI
REFS = [("chr%d" % (i + 1), 200000000) for i in range(8)]
FLAG_SETS = [[], ["-D"], ["-U"], ["-D", "-U"]]


def by_position(recs):
    """the records in coordinate order, unmapped chromosome last (as tests/test_signal_device_cmd.py sorts them)"""
    def key(i):
        tid, pos = struct.unpack_from("<ii", recs[i], 4)
        return (tid if tid >= 0 else 1 << 31, pos, i)
    return [recs[i] for i in sorted(range(len(recs)), key=key)]


def rec(name, flag, tid, pos, mtid, mpos, rng, L=30, isize=0):
    cigar = [] if flag & 4 else [(L, "M")]
    return ts.record(name, flag, tid, pos, 0 if flag & 4 else 30, cigar, mtid, mpos, isize, sc.seq(L, rng), sc.q(L), [] if flag & 4 else [("NM", "C", 1)])


def crafted():
    """the records of the crafted file in file order: no shape in it makes the host loop abort, and the left-overs are even in number"""
    rng = np.random.RandomState(4242)
    out = []

    def pair(name, tid, p1, p2, f1=0x61, f2=0x91):
        return rec(name, f1, tid, p1, tid, p2, rng, isize=p2 - p1 + 30), rec(name, f2, tid, p2, tid, p1, rng, isize=-(p2 - p1 + 30))

    # ---- chromosome 1.  A mate exactly at pos[0]: e0/1 begins the block and finds e0/2, e0/2's own mate position is not above pos[0]
    e1, e2 = pair("e0", 0, 100, 500)
    out.append(e1)
    out.append(rec("sec", 0x181, 0, 200, 0, 200, rng))                  # secondary and supplementary records in between
    out.append(rec("sup", 0x841, 0, 210, 0, 210, rng))
    out.append(rec("w", 0x41, 0, 300, 5, 77, rng))                      # its mate lies on another chromosome and is not in the file
    out.append(e2)
    # 70 primaries at one position, the mates 35 apart; s10/2 carries a wrong mate position
    for k in range(35):
        out.append(rec("s%02d" % k, 0x61, 0, 1000, 0, 1000, rng, isize=30))
    for k in range(35):
        out.append(rec("s%02d" % k, 0x91, 0, 1000, 0, 999 if k == 10 else 1000, rng, isize=-30))
    # three primaries of one name at matching positions, in both orders
    out += [rec("tri", 0x61, 0, 2000, 0, 2100, rng), rec("tri", 0x91, 0, 2100, 0, 2000, rng), rec("tri", 0x91, 0, 2100, 0, 2000, rng)]
    # (two second reads in front of the first read: whatever the blocks, the by-name pass finds first / second in template)
    out += [rec("trj", 0x91, 0, 2200, 0, 2300, rng), rec("trj", 0x91, 0, 2200, 0, 2300, rng), rec("trj", 0x61, 0, 2300, 0, 2200, rng)]
    # a mapped record and its unmapped mate, placed at the same position
    out += [rec("um", 0x49, 0, 3000, 0, 3000, rng), rec("um", 0x85, 0, 3000, 0, 3000, rng)]
    # pairs across chromosomes, for the by-name pass: names of 7, 8, 9, 17 and 40 bytes, two that differ only behind byte 8
    cross = ["abcdefg", "abcdefgh", "abcdefghi", "abcdefghX", "abcdefgh" + "k" * 9, "n" * 40]
    for k, n in enumerate(cross):
        out.append(rec(n, 0x41, 0, 4000 + k, 2, 700 - k, rng))
    out.append(rec("between", 0x901, 0, 5000, 0, 5000, rng))
    # a mate at pos[n - 2]: f/1 does not look (its mate position is not below pos[n - 2]), f/2 does
    f1, f2 = pair("f", 0, 8000, 9000)
    out += [f1, f2]
    # ---- chromosome 2.  g/1 ends the block above as its last record; its mate lies in the next block
    g1, g2 = pair("g", 1, 50, 300)
    p1a, p1b = pair("p1", 1, 100, 250)
    out += [g1, p1a, p1b, g2]
    out += list(pair("p2", 1, 400, 420))
    # a block ended by a span of 60 000 001: h/1 is its last record, h/2 begins the next
    far = 100 + 60000001
    h1, h2 = pair("h", 1, far, far + 100)
    out += [h1, h2]
    out += list(pair("p3", 1, far + 200, far + 300))
    for k, n in enumerate(reversed(cross)):
        out.append(rec(n, 0x81, 2, 700 - len(cross) + 1 + k, 0, 4000 + len(cross) - 1 - k, rng))
    # ---- unmapped: zz/1 ends the block above; then A A B B T T T C with C = zz/2
    def un(name, first):
        return rec(name, 0x4d if first else 0x8d, -1, -1, -1, -1, rng)
    out += [un("zz", True), un("A", True), un("A", False), un("B", True), un("B", False), un("T", True), un("T", False), un("T", False), un("zz", False)]
    return out


def many_failures(n_pairs=1300):
    """2 n_pairs records on one chromosome whose mate positions point at nothing: nearly every turn is a "Mate failed" """
    rng = np.random.RandomState(77)
    out = []
    for k in range(n_pairs):
        out.append(rec("m%05d" % k, 0x61, 0, 1000 + 10 * k, 0, 1003 + 10 * ((k * 7) % n_pairs), rng, L=20))
        out.append(rec("m%05d" % k, 0x91, 0, 1005 + 10 * k, 0, 1003 + 10 * ((k * 11) % n_pairs), rng, L=20))
    return out


def decreasing():
    rng = np.random.RandomState(5)
    out = []
    for k in range(40):
        a, b = rec("d%02d" % k, 0x61, 0, 100 + 50 * k, 0, 120 + 50 * k, rng), rec("d%02d" % k, 0x91, 0, 120 + 50 * k, 0, 100 + 50 * k, rng)
        out += [a, b]
    out[10], out[30] = out[30], out[10]
    return out


def write(path, recs):
    ts.write_bam(path, recs, REFS)
    return path


def make_pairs_sorted(seed, n):
    recs, refs = ts.make_pairs(seed, n)
    return by_position(recs), refs


def build(src, tmp, sanitize=False):
    return sc.build(src, tmp, sanitize)


def run_cmd(exe, tmp, bam, flags, tag, env=None, sub="signal"):
    """(CompletedProcess, header file, status file) of `exe signal flags bam`"""
    e = dict(os.environ)
    e.update(env or {})
    hf, sf = os.path.join(tmp, tag + ".sam"), os.path.join(tmp, tag + ".txt")
    for f in (hf, sf):
        if os.path.exists(f):
            os.remove(f)
    r = subprocess.run([exe, sub] + flags + ["-H", hf, "-S", sf, bam], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120, env=e)
    rd = lambda f: open(f, "rb").read() if os.path.exists(f) else None
    return r, rd(hf), rd(sf)


def own_lines(stderr, word=b"[panSVR-amd] signal --mate-device"):
    """the route's own lines (each from its tag on: "Wrong base!" is printed without a line end in front of whatever follows)"""
    return [l[l.index(word):] for l in stderr.split(b"\n") if word in l]


def without(stderr, lines):
    for l in lines:
        stderr = stderr.replace(l + b"\n", b"", 1)
    return stderr
