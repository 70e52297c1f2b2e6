"""BGZF members for the inflate tests (tests/test_inflate.py on the host build of pansvr_amd/csrc/inflate_device.h, tests/test_inflate_gpu.py
through psvr_bgzf_decompress): members made by zlib, by this repository's encoder and by hand, members broken on purpose, and the oracle
that judges them -- zlib: a member is accepted exactly when its header passes the rules of bam_reader.h's next_block(), raw inflate of its
payload reaches the end of the stream having produced ISIZE bytes, and their CRC32 is the trailer's."""
import glob
import os
import random
import struct
import subprocess
import tempfile
import zlib

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CHECK_SRC = os.path.join(HERE, "tools", "inflate_check.cpp")


# ---- the oracle ------------------------------------------------------------------------------------------------------------------------
def header_rules(buf):
    """(bsize, xlen) of the member buf starts with, or None: magic, CM, FEXTRA, a BC subfield of length 2 anywhere in the extra field
    (the last one counts), BSIZE large enough for header and trailer and not beyond the buffer."""
    if len(buf) < 18 or buf[0] != 0x1f or buf[1] != 0x8b or buf[2] != 8 or not buf[3] & 4:
        return None
    xlen = buf[10] | buf[11] << 8
    if len(buf) < 12 + xlen:
        return None
    bsize, o = 0, 0
    while o + 4 <= xlen:
        slen = buf[12 + o + 2] | buf[12 + o + 3] << 8
        if buf[12 + o] == 0x42 and buf[12 + o + 1] == 0x43 and slen == 2 and o + 6 <= xlen:
            bsize = (buf[12 + o + 4] | buf[12 + o + 5] << 8) + 1
        o += 4 + slen
    if bsize < 12 + xlen + 8 or bsize > len(buf):
        return None
    return bsize, xlen


def oracle(buf):
    """The inflated bytes of the member at the start of buf, or None when it must be refused."""
    h = header_rules(buf)
    if h is None:
        return None
    bsize, xlen = h
    crc, isize = struct.unpack("<II", buf[bsize - 8:bsize])
    d = zlib.decompressobj(-15)
    try:
        out = d.decompress(bytes(buf[12 + xlen:bsize - 8]))
    except zlib.error:
        return None
    if not d.eof or len(out) != isize or zlib.crc32(out) != crc:
        return None
    return out


# ---- making members ------------------------------------------------------------------------------------------------------------------------
def wrap(payload, data=None, crc=None, isize=None, extra=None):
    """A BGZF member around a raw DEFLATE payload (CRC32 / ISIZE of `data` unless given)."""
    if crc is None:
        crc = zlib.crc32(data)
    if isize is None:
        isize = len(data)
    xf = extra if extra is not None else b"BC\x02\x00\x00\x00"
    total = 12 + len(xf) + len(payload) + 8
    assert total <= 65536, total
    m = bytearray(b"\x1f\x8b\x08\x04\x00\x00\x00\x00\x00\xff" + struct.pack("<H", len(xf)) + xf + payload + struct.pack("<II", crc & 0xffffffff, isize & 0xffffffff))
    at = m.index(b"BC\x02\x00", 12) + 4
    m[at:at + 2] = struct.pack("<H", total - 1)
    return bytes(m)


def deflate(data, level=6, strategy=zlib.Z_DEFAULT_STRATEGY, flushes=()):
    """Raw DEFLATE of data; flushes = ((offset, mode), ...) cuts the stream there with a flush of that mode."""
    c = zlib.compressobj(level, zlib.DEFLATED, -15, 8, strategy)
    out, at = [], 0
    for off, mode in flushes:
        out.append(c.compress(data[at:off]))
        out.append(c.flush(mode))
        at = off
    out.append(c.compress(data[at:]))
    out.append(c.flush())
    return b"".join(out)


def bam_like(n, seed):
    """n bytes that look like BAM records: binary core fields, names that count up, 4-bit bases, qualities in runs, text tags."""
    rng = random.Random(seed)
    out = bytearray()
    i = 0
    while len(out) < n:
        l_seq = 150
        name = b"read%07d\0" % (seed * 1000 + i)
        seq = bytes(rng.choice(b"\x11\x12\x14\x18\x21\x22\x24\x28\x41\x42\x44\x48\x81\x82\x84\x88") for _ in range(l_seq // 2))
        q, qual = 30, bytearray()
        while len(qual) < l_seq:
            q = max(2, min(40, q + rng.choice((-3, 0, 0, 0, 2))))
            qual += bytes([q]) * rng.randint(1, 9)
        tags = b"ASi" + struct.pack("<i", rng.randint(0, 300)) + b"OAZ%d,%d,%d,M;\0" % (rng.randint(0, 23), rng.randint(1, 10 ** 8), rng.randint(0, 60))
        body = struct.pack("<iiBBHHHiiii", rng.randint(0, 23), 10000 + 37 * i, len(name), rng.randint(0, 60), 4681, 1, 0x63, l_seq, 0, 10300 + 37 * i, 450) \
            + name + struct.pack("<I", l_seq << 4) + seq + bytes(qual[:l_seq]) + tags
        out += struct.pack("<i", len(body)) + body
        i += 1
    return bytes(out[:n])


def data_sets():
    r = random.Random(11)
    return (("bam", lambda n: bam_like(n, 3)), ("random", lambda n: bytes(r.getrandbits(8) for _ in range(n))), ("equal", lambda n: b"\x07" * n))


def zlib_members():
    """[(name, member, data)]: zlib at levels 0 / 1 / 6 / 9 and the strategies Z_FIXED, Z_HUFFMAN_ONLY, Z_RLE over BAM-like records, random
    bytes and all-equal bytes of 0, 1, 2, 65 280 and 65 536 bytes, and members of several blocks.  A combination whose member would exceed
    the 65 536 bytes that BSIZE can express (incompressible bytes at the two large sizes) does not exist as a BGZF member and is left out;
    which ones were made is checked by the tests."""
    out = []
    modes = [("l0", 0, zlib.Z_DEFAULT_STRATEGY), ("l1", 1, zlib.Z_DEFAULT_STRATEGY), ("l6", 6, zlib.Z_DEFAULT_STRATEGY), ("l9", 9, zlib.Z_DEFAULT_STRATEGY),
             ("fixed", 6, zlib.Z_FIXED), ("huffman", 6, zlib.Z_HUFFMAN_ONLY), ("rle", 6, zlib.Z_RLE)]
    for dname, gen in data_sets():
        for n in (0, 1, 2, 65280, 65536):
            data = gen(n)
            for mname, level, strat in modes:
                p = deflate(data, level, strat)
                if 18 + len(p) + 8 <= 65536:
                    out.append(("%s-%d-%s" % (dname, n, mname), wrap(p, data), data))
    data = bam_like(40000, 5)
    for mode, mn in ((zlib.Z_SYNC_FLUSH, "sync"), (zlib.Z_FULL_FLUSH, "full")):
        # a flush ends the block and appends an empty stored block at whatever bit position the block ended; the next block has a new type
        for cuts in ((1,), (7, 8, 9, 10, 11, 12, 13, 14), (100, 20000, 20001, 39999)):
            p = deflate(data, 6, zlib.Z_DEFAULT_STRATEGY, tuple((c, mode) for c in cuts))
            out.append(("flush-%s-%d" % (mn, len(cuts)), wrap(p, data), data))
    mixed = bytes(random.Random(2).getrandbits(8) for _ in range(3000)) + b"A" * 5000 + bam_like(9000, 9)
    for level, strat, mn in ((6, zlib.Z_DEFAULT_STRATEGY, "l6"), (6, zlib.Z_FIXED, "fixed"), (0, zlib.Z_DEFAULT_STRATEGY, "l0")):
        p = deflate(mixed, level, strat, ((3000, zlib.Z_FULL_FLUSH), (8000, zlib.Z_SYNC_FLUSH)))
        out.append(("mixed-%s" % mn, wrap(p, mixed), mixed))
    return out


def split_members(raw):
    """The members of a BGZF file's bytes."""
    out, at = [], 0
    while at < len(raw):
        h = header_rules(raw[at:])
        assert h is not None, at
        out.append(raw[at:at + h[0]])
        at += h[0]
    return out


def golden_bams():
    return sorted(glob.glob(os.path.join(HERE, "golden", "*", "*.bam")))


def golden_members():
    out = []
    for fn in golden_bams():
        out += split_members(open(fn, "rb").read())
    return out


def own_encoder_members(tmp):
    """Members of this repository's encoder (deflate_check --members: 16 KB members, the 4-bit fixed code-length alphabet)."""
    exe = os.path.join(tmp, "deflate_check")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-o", exe, os.path.join(HERE, "tools", "deflate_check.cpp"), "-lz"])
    data = bam_like(300000, 21) + bytes(random.Random(4).getrandbits(8) for _ in range(20000)) + b"\0" * 40000
    open(os.path.join(tmp, "own.in"), "wb").write(data)
    subprocess.check_call([exe, "--members", "16384", os.path.join(tmp, "own.in"), os.path.join(tmp, "own.out")])
    ms = split_members(open(os.path.join(tmp, "own.out"), "rb").read())
    assert len(ms) == (len(data) + 16383) // 16384
    return ms, data


# ---- streams by hand ---------------------------------------------------------------------------------------------------------------------
class Bits:
    """LSB-first bit writer; Huffman codes go in most significant bit first (RFC 1951 3.1.1)."""

    def __init__(self):
        self.acc, self.n, self.out = 0, 0, bytearray()

    def put(self, v, k):
        self.acc |= (v & ((1 << k) - 1)) << self.n
        self.n += k
        while self.n >= 8:
            self.out.append(self.acc & 255)
            self.acc >>= 8
            self.n -= 8

    def code(self, c):
        v, k = c
        for i in range(k - 1, -1, -1):
            self.put(v >> i & 1, 1)

    def align(self):
        if self.n:
            self.put(0, 8 - self.n)

    def bytes(self):
        self.align()
        return bytes(self.out)


def canon(lengths):
    """{symbol: (code, length)} of the canonical code with these lengths (RFC 1951 3.2.2)."""
    count = [0] * 16
    for l in lengths:
        count[l] += 1
    count[0] = 0
    nxt, c = [0] * 16, 0
    for b in range(1, 16):
        c = (c + count[b - 1]) << 1
        nxt[b] = c
    out = {}
    for s, l in enumerate(lengths):
        if l:
            out[s] = (nxt[l], l)
            nxt[l] += 1
    return out


LBASE = [3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258]
LEXT = [0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0]
DBASE = [1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097, 6145, 8193, 12289, 16385, 24577]
DEXT = [0, 0, 0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 7, 7, 8, 8, 9, 9, 10, 10, 11, 11, 12, 12, 13, 13]
FIXED_LIT = [8] * 144 + [9] * 112 + [7] * 24 + [8] * 8
FIXED_DIST = [5] * 32
CL_ORDER = [16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15]
CL_PLAIN = [4] * 16 + [0, 0, 0]                       # the lengths 0..15 in four bits each, no run symbols
CL_RUNS = [4] * 14 + [5, 5, 5, 5, 0]                  # with 16 and 17


def tokens(b, toks, lit, dist, top_285=True):
    """literal bytes, (length, distance) matches, ("lit", symbol) / ("dist", length, symbol, extra) raw symbols; then the end of block"""
    for t in toks:
        if isinstance(t, int):
            b.code(lit[t])
        elif t[0] == "lit":
            b.code(lit[t[1]])
        elif t[0] == "dist":
            i = max(k for k in range(29) if LBASE[k] <= t[1])
            b.code(lit[257 + i]), b.put(t[1] - LBASE[i], LEXT[i])
            b.code(dist[t[2]]), b.put(t[3], 13)
        else:
            ln, d = t
            i = 28 if ln == 258 and top_285 else max(k for k in range(28) if LBASE[k] <= ln)
            b.code(lit[257 + i]), b.put(ln - LBASE[i], LEXT[i])
            j = max(k for k in range(30) if DBASE[k] <= d)
            b.code(dist[j]), b.put(d - DBASE[j], DEXT[j])


def fixed_block(b, toks, final=True, eob=True):
    b.put(1 if final else 0, 1), b.put(1, 2)
    tokens(b, toks, canon(FIXED_LIT), canon(FIXED_DIST))
    if eob:
        b.code(canon(FIXED_LIT)[256])


def dynamic_header(b, litlens, distlens, cl=CL_PLAIN, clsyms=None, final=True, hlit=None, hdist=None, ncl=19):
    """clsyms: the code-length symbols to send, as symbols 0..15 or (16 | 17 | 18, extra); default one symbol per length"""
    b.put(1 if final else 0, 1), b.put(2, 2)
    b.put(len(litlens) - 257 if hlit is None else hlit, 5), b.put(len(distlens) - 1 if hdist is None else hdist, 5), b.put(ncl - 4, 4)
    for s in CL_ORDER[:ncl]:
        b.put(cl[s], 3)
    cc = canon(cl)
    for s in (clsyms if clsyms is not None else list(litlens) + list(distlens)):
        if isinstance(s, int):
            b.code(cc[s])
        else:
            b.code(cc[s[0]]), b.put(s[1], {16: 2, 17: 3, 18: 7}[s[0]])


def dynamic_block(b, toks, litlens, distlens, eob=True, **kw):
    dynamic_header(b, litlens, distlens, **kw)
    tokens(b, toks, canon(litlens), canon(distlens))
    if eob:
        b.code(canon(litlens)[256])


def expand(toks):
    out = bytearray()
    for t in toks:
        if isinstance(t, int):
            out.append(t)
        else:
            for _ in range(t[0]):
                out.append(out[-t[1]])
    return bytes(out)


def lens(n, d):
    v = [0] * n
    for k, l in d.items():
        v[k] = l
    return v


def hand_valid():
    """[(name, member, data)] for what zlib never emits."""
    out = []
    r = random.Random(8)

    def add(name, b, data):
        out.append((name, wrap(b.bytes(), data), data))
    # a match at distance 32 768 (zlib stops at 32 506) -- stored bytes first, so that the member fits; and length code 285
    head = bytes(r.getrandbits(8) for _ in range(32768))
    b = Bits()
    b.put(0, 1), b.put(0, 2), b.align(), b.put(32768, 16), b.put(32768 ^ 0xffff, 16)
    b.out += head
    toks = [(200, 32768), 65, (258, 1), (258, 32768), (3, 32768)]
    fixed_block(b, toks)
    full = bytearray(head)
    for t in toks:
        if isinstance(t, int):
            full.append(t)
        else:
            for _ in range(t[0]):
                full.append(full[-t[1]])
    add("distance-32768-length-285", b, bytes(full))
    # length 258 sent as code 284 + 31 extra: zlib accepts it
    b = Bits()
    b.put(1, 1), b.put(1, 2)
    tokens(b, [66, (258, 1)], canon(FIXED_LIT), canon(FIXED_DIST), top_285=False)
    b.code(canon(FIXED_LIT)[256])
    add("length-258-by-code-284", b, expand([66, (258, 1)]))
    # a dynamic block with a single distance code (an incomplete code zlib lets pass)
    b = Bits()
    toks = [97, (10, 1), 98, (4, 1)]
    dynamic_block(b, toks, lens(265, {97: 2, 98: 2, 256: 2, 257 + 1: 3, 257 + 7: 3}), [1])
    add("single-distance-code", b, expand(toks))
    # ... with the lone code on distance symbol 3, and a single literal/length code (an empty block) in front
    b = Bits()
    dynamic_block(b, [], lens(257, {256: 1}), [0], final=False)
    toks = [1, 2, 3, 4, (4, 4), (5, 4)]
    dynamic_block(b, toks, lens(260, {1: 3, 2: 3, 3: 3, 4: 3, 256: 3, 258: 3, 259: 2}), [0, 0, 0, 1])
    add("single-codes", b, expand(toks))
    # no distance code at all: literals only
    b = Bits()
    toks = [104, 105, 104, 104]
    dynamic_block(b, toks, lens(257, {104: 1, 105: 2, 256: 2}), [0])
    add("no-distance-code", b, expand(toks))
    # 15-bit codes in both alphabets
    ll = lens(286, dict([(97 + i, i + 2) for i in range(13)] + [(200, 15), (256, 15), (257, 1)]))
    dl = [i + 1 for i in range(14)] + [15, 15]
    toks = [97, 98, 109, 200, (3, 1), (3, 2), 108, (3, 5)] + [97] * 75 + [200] * 110 + [(3, 129), (3, 193)]
    b = Bits()
    dynamic_block(b, toks, ll, dl)
    add("15-bit-codes", b, expand(toks))
    # a code-length run that crosses from the literal/length lengths into the distance lengths, sent with the run symbols
    ll = lens(260, {97: 1, 256: 3, 257: 3, 258: 3, 259: 3})
    dl = [3] * 8
    syms = [(18, 97 - 11), 1, (18, 138 - 11), (18, 20 - 11), 3, (16, 6 - 3), (16, 5 - 3)]   # 97 x 0, 1, 158 x 0, 3, 6 x 3 across the border, 5 x 3
    toks = [97, 97, 97, (3, 1), (4, 2), (5, 6), (5, 8), 97]
    b = Bits()
    dynamic_block(b, toks, ll, dl, cl=[2, 3, 0, 3] + [0] * 12 + [2, 3, 3], clsyms=syms)
    add("run-across-the-border", b, expand(toks))
    return out


def hand_bad():
    """[(name, member, accepted)]: one member for every way of refusing, built by hand; and a few odd ones that must pass."""
    out = []
    ok_lit = lens(258, {97: 1, 256: 2, 257: 2})

    def add(name, b, data=b"", accepted=False, **kw):
        payload = b.bytes() if isinstance(b, Bits) else b
        out.append((name, wrap(payload, data, **kw), accepted))
    b = Bits()
    b.put(1, 1), b.put(3, 2), b.put(0, 13)
    add("block-type-3", b)
    b = Bits()
    b.put(1, 1), b.put(0, 2), b.align(), b.put(3, 16), b.put(3 ^ 0xfffe, 16)
    b.out += b"abc"
    add("stored-len-nlen", b, b"abc")
    b = Bits()
    b.put(1, 1), b.put(0, 2), b.align(), b.put(30, 16), b.put(30 ^ 0xffff, 16)
    b.out += b"abc"
    add("stored-longer-than-the-input", b, b"abc")
    b = Bits()
    b.put(1, 1), b.put(0, 2), b.align(), b.put(3, 16)
    add("stored-header-cut", b, b"")
    b = Bits()
    dynamic_block(b, [97], lens(286, {97: 1, 256: 2, 257: 2}), [1], hlit=30)
    add("hlit-287", b, b"a")
    b = Bits()
    dynamic_block(b, [97], ok_lit, [1] + [0] * 29, hdist=30)
    add("hdist-31", b, b"a")
    b = Bits()
    dynamic_block(b, [97], lens(258, {97: 1, 98: 1, 256: 2, 257: 2}), [1])
    add("literal-code-over-subscribed", b, b"a")
    b = Bits()
    dynamic_block(b, [97], lens(258, {97: 2, 256: 2, 257: 2}), [1])
    add("literal-code-incomplete", b, b"a")
    b = Bits()
    dynamic_block(b, [97], ok_lit, [1, 1, 1])
    add("distance-code-over-subscribed", b, b"a")
    b = Bits()
    dynamic_block(b, [97], ok_lit, [2, 2])
    add("distance-code-incomplete", b, b"a")
    b = Bits()
    dynamic_block(b, [97], ok_lit, [1], cl=[4] * 15 + [0, 0, 0, 0])
    add("code-length-code-incomplete", b, b"a")
    b = Bits()
    dynamic_block(b, [97], ok_lit, [1], cl=[3] * 9 + [0] * 10, clsyms=[0] * 259)
    add("code-length-code-over-subscribed", b, b"a")
    b = Bits()
    dynamic_header(b, ok_lit, [1], cl=CL_RUNS, clsyms=[(16, 0)] + [0] * 256)
    add("repeat-without-a-previous-length", b)
    b = Bits()
    dynamic_header(b, ok_lit, [1], cl=CL_RUNS, clsyms=[0] * 97 + [1] + [0] * 158 + [2, 2, 1, (16, 0)])
    add("repeat-past-the-end", b)
    b = Bits()
    dynamic_header(b, ok_lit, [1], cl=CL_RUNS, clsyms=[0] * 97 + [1] + [0] * 158 + [2, 2, (17, 0)])
    add("zero-run-past-the-end", b)
    b = Bits()
    dynamic_header(b, lens(258, {97: 1, 257: 1}), [1])
    b.put(0, 16)
    add("no-end-of-block-code", b, b"a")
    for s in (286, 287):
        b = Bits()
        fixed_block(b, [97, ("lit", s)])
        add("fixed-symbol-%d" % s, b, b"a")
    for s in (30, 31):
        b = Bits()
        fixed_block(b, [97, 97, 97, ("dist", 3, s, 0)])
        add("fixed-distance-symbol-%d" % s, b, b"aaa")
    b = Bits()
    fixed_block(b, [97, 98, (3, 3)])
    add("distance-in-front-of-the-member", b, b"ab")
    b = Bits()
    dynamic_header(b, lens(258, {97: 2, 256: 2, 257: 1}), [1])
    cl_ = canon(lens(258, {97: 2, 256: 2, 257: 1}))
    b.code(cl_[97]), b.code(cl_[257]), b.put(1, 1)                         # the lone distance code is "0"; "1" is unassigned
    b.put(0, 16)
    add("unassigned-distance-code", b, b"a")
    b = Bits()
    dynamic_header(b, lens(257, {97: 1, 256: 1}), [0])
    b.put(0, 1), b.put(1, 1)
    add("a-block-of-two-1-bit-codes", b, b"a", accepted=True)
    b = Bits()
    dynamic_header(b, lens(258, {97: 2, 256: 2, 257: 1}), [0])
    b.code(cl_[97]), b.code(cl_[257]), b.put(0, 16)
    add("match-without-a-distance-code", b, b"aaaa")
    b = Bits()
    fixed_block(b, [97, 98, 99])
    add("longer-than-isize", b, b"ab", crc=zlib.crc32(b"ab"))
    add("shorter-than-isize", b, b"abcd")
    b = Bits()
    fixed_block(b, [97, (258, 1), (258, 1)])
    add("a-match-longer-than-isize", b, b"a" * 300)
    add("crc", b, b"a" * 517, crc=zlib.crc32(b"a" * 517) ^ 0x100)
    add("isize-out-of-reach", b, b"", crc=0, isize=0xfff00000)
    b = Bits()
    fixed_block(b, [97, 98, 99], eob=False)
    add("no-end-of-block", b, b"abc")
    b = Bits()
    fixed_block(b, [97, 98, 99], final=False)
    add("no-final-block", b, b"abc")
    add("empty-payload", b"", b"")
    b = Bits()
    fixed_block(b, [97, 98, 99])
    add("bytes-behind-the-stream", b.bytes() + b"\xff\x00\x12garbage", b"abc", accepted=True)
    add("a-second-subfield", b.bytes(), b"abc", accepted=True, extra=b"XY\x03\x00abcBC\x02\x00\x00\x00ZZ\x00\x00")
    b = Bits()
    b.put(1, 1), b.put(0, 2), b.put(0, 5), b.put(0, 16), b.put(0xffff, 16)
    add("an-empty-stored-block", b, b"", accepted=True)
    return out


def truncations():
    """Three small members cut at every byte: as a buffer that ends early, and with the payload cut and the member wrapped again."""
    out = []
    data = bam_like(600, 1)
    b = Bits()
    fixed_block(b, list(b"hello hello ") + [(20, 6)])
    for payload, d in ((deflate(data, 6), data), (deflate(data[:80], 0), data[:80]), (b.bytes(), expand(list(b"hello hello ") + [(20, 6)]))):
        m = wrap(payload, d)
        assert oracle(m) == d
        for k in range(len(m)):
            out.append(m[:k])
        for k in range(len(payload)):
            out.append(wrap(payload[:k], d))
    return out


def payload_mutations(members, n=2000, seed=77):
    """n single-byte mutations of the payload and the trailer of golden members"""
    r = random.Random(seed)
    out = []
    for _ in range(n):
        m = bytearray(r.choice(members))
        at = r.randrange(18, len(m))
        m[at] ^= 1 << r.randrange(8) if r.random() < 0.5 else r.randrange(1, 256)
        out.append(bytes(m))
    return out


def header_mutations(members, n=500, seed=78):
    """n single-byte mutations of the 18 header bytes -- the extra field included -- of golden members and of a member with a longer one"""
    r = random.Random(seed)
    pool = list(members[:40]) + [wrap(deflate(b"abcabcabc"), b"abcabcabc", extra=b"XY\x03\x00abcBC\x02\x00\x00\x00ZZ\x00\x00")] * 10
    out = []
    for _ in range(n):
        m = bytearray(r.choice(pool))
        xlen = m[10] | m[11] << 8
        at = r.randrange(0, 12 + xlen)
        m[at] ^= 1 << r.randrange(8) if r.random() < 0.5 else r.randrange(1, 256)
        out.append(bytes(m))
    return out


# ---- the host build of the decoder ---------------------------------------------------------------------------------------------------------
def build_checker(tmp, sanitize):
    exe = os.path.join(tmp, "inflate_check_asan" if sanitize else "inflate_check")
    flags = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"] if sanitize else ["-O2"]
    subprocess.check_call(["g++"] + flags + ["-std=c++17", "-Wall", "-o", exe, CHECK_SRC])
    return exe


def run_checker(exe, bufs, timeout=600):
    """[(status, bytes or None)] of the decoder's host build for every buffer; the sanitizer's report, if any, fails the call."""
    tmp = tempfile.mkdtemp(prefix="psvr_infl_")
    with open(os.path.join(tmp, "cases"), "wb") as f:
        f.write(struct.pack("<I", len(bufs)))
        for b in bufs:
            f.write(struct.pack("<I", len(b)) + bytes(b))
    r = subprocess.run([exe, os.path.join(tmp, "cases"), os.path.join(tmp, "results")], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=timeout)
    assert r.returncode == 0 and not r.stderr, "inflate_check: exit status %d\n%s" % (r.returncode, r.stderr.decode()[-4000:])
    raw = open(os.path.join(tmp, "results"), "rb").read()
    out, at = [], 0
    for _ in bufs:
        status, n = struct.unpack_from("<II", raw, at)
        at += 8
        if status == 0:
            out.append((0, raw[at:at + n]))
            at += n
        else:
            out.append((status, None))
    assert at == len(raw)
    return out


def malformed_sets(members):
    """name -> buffers; every buffer is judged by oracle()"""
    return {"by hand": [m for _, m, _ in hand_bad()], "truncations": truncations(), "payload mutations": payload_mutations(members), "header mutations": header_mutations(members)}


def classify(buf):
    """'ok' / 'bad' by oracle(), or 'cut' when the buffer ends before the member does (the order of bgzf_member_header's checks)"""
    if len(buf) < 18:
        return "cut"
    if buf[0] != 0x1f or buf[1] != 0x8b or buf[2] != 8 or not buf[3] & 4:
        return "bad"
    xlen = buf[10] | buf[11] << 8
    if len(buf) < 12 + xlen:
        return "cut"
    if header_rules(buf) is None:
        h = header_rules(bytes(buf) + b"\0" * 65536)
        return "bad" if h is None else "cut"
    return "ok" if oracle(buf) is not None else "bad"


def bam_like_big(n, seed):
    """n bytes of BAM-like records made with numpy (fixed 256-byte records: core fields, a counting name, random 4-bit bases, qualities in runs)"""
    import numpy as np
    rng = np.random.RandomState(seed)
    nrec = (n + 255) // 256
    rec = np.zeros((nrec, 256), dtype=np.uint8)
    idx = np.arange(nrec, dtype=np.int64)
    rec[:, 0:4] = np.frombuffer(struct.pack("<i", 252), dtype=np.uint8)
    rec[:, 4] = rng.randint(0, 24, size=nrec)
    pos = (10000 + 37 * idx).astype("<i4").view(np.uint8).reshape(nrec, 4)
    rec[:, 8:12] = pos
    rec[:, 12] = 12
    rec[:, 13] = rng.randint(0, 61, size=nrec)
    rec[:, 18:20] = (0x63, 0)
    rec[:, 20] = 150
    rec[:, 28:32] = pos
    name = np.char.zfill(idx.astype("U11"), 11).astype("S11").view(np.uint8).reshape(nrec, 11)
    rec[:, 36:47] = name
    rec[:, 48:52] = np.frombuffer(struct.pack("<I", 150 << 4), dtype=np.uint8)
    nib = np.array([1, 2, 4, 8], dtype=np.uint8)
    rec[:, 52:127] = nib[rng.randint(0, 4, size=(nrec, 75))] << 4 | nib[rng.randint(0, 4, size=(nrec, 75))]
    k = nrec * 150 // 3 + 16
    q = np.repeat(rng.randint(2, 41, size=k).astype(np.uint8), rng.randint(1, 10, size=k))
    while len(q) < nrec * 125:
        q = np.concatenate([q, q])
    rec[:, 127:252] = q[:nrec * 125].reshape(nrec, 125)
    rec[:, 252:256] = rng.randint(48, 58, size=(nrec, 4))
    return rec.reshape(-1)[:n].tobytes()


def members_of(data, level=6, block=0xff00, threads=16):
    """data cut into members of `block` bytes, zlib at `level`, on a few threads"""
    from concurrent.futures import ThreadPoolExecutor
    chunks = [data[i:i + block] for i in range(0, len(data), block)]
    with ThreadPoolExecutor(threads) as ex:
        return list(ex.map(lambda c: wrap(deflate(c, level), c), chunks))
