"""Inputs and helpers for the tests of the wavefront BGZF encoder's efforts 0..3 (hash chains and lazy matching: dfw_member_effort of
pansvr_amd/csrc/deflate_wave_device.h): tests/test_deflate_effort.py on the host build (tests/tools/deflate_effort_check.cpp),
tests/test_deflate_effort_gpu.py through psvr_bgzf_compress_members_effort.  The crafted inputs are the smallest at which the rule can go
wrong; each says, as a predicate over the host build's tokens, what the rule must have done with it."""
import gzip
import os
import random
import struct
import subprocess
import tempfile
import zlib

import aln_common as ac

HERE = os.path.dirname(os.path.abspath(__file__))
CHECK_SRC = os.path.join(HERE, "tools", "deflate_effort_check.cpp")
EFFORTS = (0, 1, 2, 3)
DEPTH = {0: 1, 1: 4, 2: 8, 3: 16}


def build_checker(tmp, sanitize):
    exe = os.path.join(tmp, "deflate_effort_check_asan" if sanitize else "deflate_effort_check")
    flags = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"] if sanitize else ["-O2"]
    subprocess.check_call(["g++"] + flags + ["-std=c++17", "-Wall", "-o", exe, CHECK_SRC])
    return exe


def host_members(exe, data, member_bytes, effort, dirty=False, tokens=False, timeout=900):
    """The bytes the encoder's host build writes for `data` at `effort` (with tokens=True: and every member's tokens as a list of words);
    the sanitizer's report, if any, fails the call."""
    tmp = tempfile.mkdtemp(prefix="psvr_dfe_")
    with open(os.path.join(tmp, "in"), "wb") as f:
        f.write(data)
    cmd = [exe] + (["--dirty"] if dirty else []) + (["--tokens", os.path.join(tmp, "tok")] if tokens else [])
    r = subprocess.run(cmd + [str(effort), str(member_bytes), os.path.join(tmp, "in"), os.path.join(tmp, "out")], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=timeout)
    assert r.returncode == 0 and not r.stderr, "deflate_effort_check: exit status %d\n%s" % (r.returncode, r.stderr.decode()[-4000:])
    raw = open(os.path.join(tmp, "out"), "rb").read()
    if not tokens:
        return raw
    t = open(os.path.join(tmp, "tok"), "rb").read()
    return raw, list(struct.unpack("<%dI" % (len(t) // 4), t))


def token_map(toks):
    """{position: byte, or (length, distance)} of one member's tokens"""
    out, pos = {}, 0
    for x in toks:
        if x == 0x40000100:
            break
        if x & 0x80000000:
            out[pos] = (((x >> 16) & 0xff) + 3, (x & 0xffff) + 1)
            pos += out[pos][0]
        else:
            out[pos] = x
            pos += 1
    return out


def h3(a, b, c):
    """the encoder's hash of three bytes"""
    return (((a | b << 8 | c << 16) * 0x9E3779B1) & 0xffffffff) >> 20


def bucket(data, h):
    """the positions of data that enter the table under hash h"""
    return [p for p in range(len(data) - 3) if h3(data[p], data[p + 1], data[p + 2]) == h]


class Filler:
    """Bytes 0..63 (six bits each, so a member of them comes out Huffman-coded, not stored) in which no three bytes occur twice and none hash
    into `avoid`: nothing in them matches, and they visit none of the buckets a case counts visits of.  Forced bytes are the case's own."""

    def __init__(self, seed, avoid=()):
        self.r, self.seen, self.avoid, self.out = random.Random(seed), set(), set(avoid), bytearray()

    def push(self, b):
        if len(self.out) >= 2:
            self.seen.add((self.out[-2], self.out[-1], b))
        self.out.append(b)

    def fill(self, n):
        for _ in range(n):
            while True:
                b = self.r.randrange(64)
                t = (self.out[-2], self.out[-1], b) if len(self.out) >= 2 else None
                if t is None or (t not in self.seen and h3(*t) not in self.avoid):
                    break
            self.push(b)
        return bytes(self.out[-n:]) if n else b""

    def fill_to(self, pos):
        assert pos >= len(self.out)
        self.fill(pos - len(self.out))

    def force(self, bs):
        for b in bs:
            self.push(b)


def key(r):
    """the three bytes whose bucket repetition r of a case visits: outside the filler's alphabet"""
    return (200 + 3 * r, 201 + 3 * r, 202 + 3 * r)


def chain_visits(visits, spacing, tail_len, reps, seed):
    """`reps` times, each with bytes of its own: one hash bucket visited `visits` times, `spacing` bytes apart, the first visit followed by
    `tail_len` bytes T, the others by a byte of their own; then the three bytes and T once more (the probe).  The longest match of the probe
    is at the OLDEST visit, `visits` links down the chain.  Returns (data, [(probe position, first visit's position)])."""
    f = Filler(seed, [h3(*key(r)) for r in range(reps)])
    f.fill(128 - 1)
    probes = []
    for r in range(reps):
        first, T = None, None
        for i in range(visits + 1):
            f.force([64 + i])                                  # (in front of every visit a byte of its own: nothing longer than the case means)
            at = len(f.out)
            f.force(key(r))
            if i == 0:
                first, T = at, f.fill(tail_len)
            elif i < visits:
                f.force([96 + i])
            else:
                f.force(T)
                probes.append((at, first))
            f.fill_to(at - 1 + spacing)
        f.fill_to((len(f.out) + 63) // 64 * 64 + 64 - 1)       # (the next repetition starts a group later, at 64 m + 63 again)
    f.fill(40)
    data = bytes(f.out)
    for r in range(reps):
        assert len(bucket(data, h3(*key(r)))) == visits + 1, "the case's bucket has visitors of its own"
    return data, probes


def chain_far(dist, seed=23):
    """the three bytes and 200 bytes T, the three bytes again 300 bytes on (so that the table's entry is this one and T's lies a link behind
    it), and the probe `dist` bytes behind the first: (data, probe position)"""
    f = Filler(seed, [h3(*key(0))])
    f.fill(9)
    f.force([64])
    a = len(f.out)
    f.force(key(0))
    T = f.fill(200)
    f.fill_to(a + 300 - 1)
    f.force([65])
    f.force(key(0) + (97,))
    f.fill_to(a + dist - 1)
    f.force([66])
    assert len(f.out) == a + dist
    f.force(key(0))
    f.force(T)
    f.fill(50)
    data = bytes(f.out)
    assert bucket(data, h3(*key(0))) == [a, a + 300, a + dist]
    return data, a + dist


K4 = (210, 211, 212, 213)


def lazy_pair(f, at, lead=()):
    """at `at`: four bytes that match four bytes earlier, and from at + 1 on three of them and twelve more that match fifteen: the longer match
    starts one position behind the shorter.  The two earlier places are put down first, at the filler's current end; `lead` goes right in
    front of `at`."""
    f.fill(8)
    f.force(K4 + (120,))
    f.fill(20)
    f.force((121,) + K4[1:])
    L = f.fill(12)
    f.fill_to(at - len(lead))
    f.force(lead)
    f.force(K4)
    f.force(L)
    f.fill(30)
    data = bytes(f.out)
    assert len(bucket(data, h3(*K4[:3]))) == 2 and len(bucket(data, h3(*K4[1:]))) == 3
    return data


def lazy_at(pos, seed=29):
    """lazy_pair at `pos`: (data, pos)"""
    return lazy_pair(Filler(seed, [h3(*K4[:3]), h3(*K4[1:])]), pos), pos


def carried_then_lazy(q, seed=31):
    """ten bytes at q (64 m + 60) that match ten bytes earlier and so cover the first six positions of the next group, and lazy_pair right
    behind them, at q + 10: (data, q)"""
    f = Filler(seed, [h3(*K4[:3]), h3(*K4[1:])])
    M = tuple(range(220, 230))
    f.fill(5)
    f.force(M)
    return lazy_pair(f, q + 10, M), q


def crafted():
    """[(name, data)]: the inputs of the rule's edges, for members of 0xff00 bytes (test_deflate_effort.py says what each must give)"""
    out = []
    for v in (3, 6, 10, 20):
        out.append(("bucket visited %d times, 70 apart" % v, chain_visits(v, 70, 40, 6, 100 + v)[0]))
    for v in (6, 7):                                           # (7: the most that fits a group at this spacing)
        out.append(("bucket visited %d times inside one group" % v, chain_visits(v, 8, 4, 1, 17)[0]))
    out.append(("chain candidate at distance 32768", chain_far(32768)[0]))
    out.append(("chain candidate at distance 32769", chain_far(32769)[0]))
    out.append(("longer match behind a group's last position", lazy_at(64 * 3 + 63)[0]))
    out.append(("longer match behind a group's last but one position", lazy_at(64 * 3 + 62)[0]))
    out.append(("carried match, then a lazy pair", carried_then_lazy(64 * 3 + 60)[0]))
    for n, d in ((1, b"q"), (3, b"aaa"), (4, b"aaaa"), (5, b"aaaaa"), (5, b"abcab")):
        out.append(("%d bytes %r" % (n, d), d))
    return out


def golden_records(path):
    """the BAM records of a golden file as they lie, each with its block_size"""
    s = gzip.open(path, "rb").read()
    at = 8 + struct.unpack_from("<i", s, 4)[0]
    n_ref = struct.unpack_from("<i", s, at)[0]
    at += 4
    for _ in range(n_ref):
        at += 8 + struct.unpack_from("<i", s, at)[0]
    recs = []
    while at < len(s):
        bs = struct.unpack_from("<i", s, at)[0]
        recs.append(s[at:at + 4 + bs])
        at += 4 + bs
    assert at == len(s)
    return recs


def size_inputs():
    """[(name, bytes)]: the records of two golden BAMs as they lie and reordered by (tid, pos), unplaced last"""
    out = []
    for name, fn in (("fx1 reads150", os.path.join(ac.golden_dir("fx1"), "reads150.bam")), ("fx2 reads250", os.path.join(ac.golden_dir("fx2"), "reads250.bam"))):
        recs = golden_records(fn)
        out.append((name + " unsorted", b"".join(recs)))
        out.append((name + " sorted", b"".join(sorted(recs, key=lambda r: struct.unpack_from("<II", r, 4)))))
    return out


def zlib_total(data, level, member_bytes=0xff00):
    """what zlib at `level` makes of data cut into members, 26 wrapper bytes each"""
    total = 0
    for i in range(0, len(data), member_bytes):
        c = zlib.compressobj(level, zlib.DEFLATED, -15, 8)
        total += len(c.compress(data[i:i + member_bytes]) + c.flush()) + 26
    return total
