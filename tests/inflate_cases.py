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


def inf_isize_possible(buf):
    """inflate_device.h's rule of that name for the member buf starts with (its header passes): a payload of n bytes holds 1032 n bytes at most;
    a member whose ISIZE is beyond that is refused where the batch is laid out, as a bad header is"""
    bsize, xlen = header_rules(buf)
    return struct.unpack_from("<I", buf, bsize - 4)[0] <= 1032 * (bsize - 12 - xlen - 8)


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
    """[(name, member, status)]: one member for every way of refusing, built by hand, with the name of the status inflate_device.h must
    give it (the first rule it breaks in stream order); and a few odd ones that must pass ("kInfOk").  Every refused member but "crc" and
    the ISIZE ones carries the CRC32 and ISIZE of the data it was meant to hold: a decoder that lacked the rule would be caught by the
    trailer all the same, which is why the status is asserted and not only the refusal.  Where a member breaks two rules:
      stored-longer-than-the-input   LEN is more than the payload has left and more than ISIZE: the input is looked at first, kInfTruncated
      no-end-of-block                the padding bits behind the last literal are the start of a code the payload's end cuts off: kInfTruncated
      isize-out-of-reach             refused where the batch is laid out (inf_isize_possible), before the decoder runs: the host checker
                                     calls that kInfTooShort, psvr_bgzf_decompress reports the member as a bad header (kInfHeader)"""
    out = []
    ok_lit = lens(258, {97: 1, 256: 2, 257: 2})

    def add(name, status, b, data=b"", **kw):
        payload = b.bytes() if isinstance(b, Bits) else b
        out.append((name, wrap(payload, data, **kw), status))
    b = Bits()
    b.put(1, 1), b.put(3, 2), b.put(0, 13)
    add("block-type-3", "kInfBlockType", b)
    b = Bits()
    b.put(1, 1), b.put(0, 2), b.align(), b.put(3, 16), b.put(3 ^ 0xfffe, 16)
    b.out += b"abc"
    add("stored-len-nlen", "kInfStored", b, b"abc")
    b = Bits()
    b.put(1, 1), b.put(0, 2), b.align(), b.put(30, 16), b.put(30 ^ 0xffff, 16)
    b.out += b"abc"
    add("stored-longer-than-the-input", "kInfTruncated", b, b"abc")
    b = Bits()
    b.put(1, 1), b.put(0, 2), b.align(), b.put(3, 16)
    add("stored-header-cut", "kInfTruncated", b, b"")
    b = Bits()
    dynamic_block(b, [97], lens(286, {97: 1, 256: 2, 257: 2}), [1], hlit=30)
    add("hlit-287", "kInfCounts", b, b"a")
    b = Bits()
    dynamic_block(b, [97], ok_lit, [1] + [0] * 29, hdist=30)
    add("hdist-31", "kInfCounts", b, b"a")
    b = Bits()
    dynamic_block(b, [97], lens(258, {97: 1, 98: 1, 256: 2, 257: 2}), [1])
    add("literal-code-over-subscribed", "kInfLitTable", b, b"a")
    b = Bits()
    dynamic_block(b, [97], lens(258, {97: 2, 256: 2, 257: 2}), [1])
    add("literal-code-incomplete", "kInfLitTable", b, b"a")
    b = Bits()
    dynamic_block(b, [97], ok_lit, [1, 1, 1])
    add("distance-code-over-subscribed", "kInfDistTable", b, b"a")
    b = Bits()
    dynamic_block(b, [97], ok_lit, [2, 2])
    add("distance-code-incomplete", "kInfDistTable", b, b"a")
    b = Bits()
    dynamic_block(b, [97], ok_lit, [1], cl=[4] * 15 + [0, 0, 0, 0])
    add("code-length-code-incomplete", "kInfCodeLengths", b, b"a")
    b = Bits()
    dynamic_block(b, [97], ok_lit, [1], cl=[3] * 9 + [0] * 10, clsyms=[0] * 259)
    add("code-length-code-over-subscribed", "kInfCodeLengths", b, b"a")
    b = Bits()
    dynamic_header(b, ok_lit, [1], cl=CL_RUNS, clsyms=[(16, 0)] + [0] * 256)
    add("repeat-without-a-previous-length", "kInfCodeLengths", b)
    b = Bits()
    dynamic_header(b, ok_lit, [1], cl=CL_RUNS, clsyms=[0] * 97 + [1] + [0] * 158 + [2, 2, (16, 0)])         # (258 lengths, then 3 more for the 1 that is left)
    add("repeat-past-the-end", "kInfCodeLengths", b)
    b = Bits()
    dynamic_header(b, ok_lit, [1], cl=CL_RUNS, clsyms=[0] * 97 + [1] + [0] * 158 + [2, 2, (17, 0)])
    add("zero-run-past-the-end", "kInfCodeLengths", b)
    b = Bits()
    dynamic_header(b, lens(258, {97: 1, 257: 1}), [1])
    b.put(0, 16)
    add("no-end-of-block-code", "kInfNoEob", b, b"a")
    for s in (286, 287):
        b = Bits()
        fixed_block(b, [97, ("lit", s)])
        add("fixed-symbol-%d" % s, "kInfLitCode", b, b"a")
    for s in (30, 31):
        b = Bits()
        fixed_block(b, [97, 97, 97, ("dist", 3, s, 0)])
        add("fixed-distance-symbol-%d" % s, "kInfDistCode", b, b"aaa")
    b = Bits()
    fixed_block(b, [97, 98, (3, 3)])
    add("distance-in-front-of-the-member", "kInfFarBack", b, b"ab")
    b = Bits()
    dynamic_header(b, lens(258, {97: 2, 256: 2, 257: 1}), [1])
    cl_ = canon(lens(258, {97: 2, 256: 2, 257: 1}))
    b.code(cl_[97]), b.code(cl_[257]), b.put(1, 1)                         # the lone distance code is "0"; "1" is unassigned
    b.put(0, 16)
    add("unassigned-distance-code", "kInfDistCode", b, b"a")
    b = Bits()
    dynamic_header(b, lens(257, {97: 1, 256: 1}), [0])
    b.put(0, 1), b.put(1, 1)
    add("a-block-of-two-1-bit-codes", "kInfOk", b, b"a")
    b = Bits()
    dynamic_header(b, lens(258, {97: 2, 256: 2, 257: 1}), [0])
    b.code(cl_[97]), b.code(cl_[257]), b.put(0, 16)
    add("match-without-a-distance-code", "kInfDistCode", b, b"aaaa")
    b = Bits()
    fixed_block(b, [97, 98, 99])
    add("longer-than-isize", "kInfTooLong", b, b"ab", crc=zlib.crc32(b"ab"))
    add("shorter-than-isize", "kInfTooShort", b, b"abcd")
    b = Bits()
    fixed_block(b, [97, (258, 1), (258, 1)])
    add("a-match-longer-than-isize", "kInfTooLong", b, b"a" * 300)
    add("crc", "kInfCrc", b, b"a" * 517, crc=zlib.crc32(b"a" * 517) ^ 0x100)
    add("isize-out-of-reach", "kInfTooShort", b, b"", crc=0, isize=0xfff00000)
    b = Bits()
    fixed_block(b, [97, 98, 99], eob=False)
    add("no-end-of-block", "kInfTruncated", b, b"abc")
    b = Bits()
    fixed_block(b, [97, 98, 99], final=False)
    add("no-final-block", "kInfTruncated", b, b"abc")
    add("empty-payload", "kInfTruncated", b"", b"")
    b = Bits()
    fixed_block(b, [97, 98, 99])
    add("bytes-behind-the-stream", "kInfOk", b.bytes() + b"\xff\x00\x12garbage", b"abc")
    add("a-second-subfield", "kInfOk", b.bytes(), b"abc", extra=b"XY\x03\x00abcBC\x02\x00\x00\x00ZZ\x00\x00")
    b = Bits()
    b.put(1, 1), b.put(0, 2), b.put(0, 5), b.put(0, 16), b.put(0xffff, 16)
    add("an-empty-stored-block", "kInfOk", b, b"")
    return out


PRE = bytes(range(32, 96))                            # what every member of rule_edges() holds in a stored block in front of the block in question
FORGED_ISIZE = 0xff00
# the code-length code of rule_edges(): 0 and 18 in two bits, the lengths 1..15 and 16 in five (complete; no 17)
CL_EDGE = [2] + [5] * 16 + [0, 2]


def zeros(n):
    """n zero lengths as code-length symbols: runs of 11..138 by symbol 18, the rest one by one"""
    out = []
    while n >= 11:
        k = min(n, 138)
        out.append((18, k - 11))
        n -= k
    return out + [0] * n


def run_lengths(lengths):
    """the code-length symbols for these lengths: the zero runs by zeros(), everything else as itself"""
    out, k = [], 0
    for l in list(lengths) + [None]:
        if l == 0:
            k += 1
            continue
        out += zeros(k)
        k = 0
        if l is not None:
            out.append(l)
    return out


def rule_edges():
    """[(name, member, status, data or None)]: for every rule of inflate_device.h a member just inside its edge (status "kInfOk", `data` the bytes
    it holds, which must be zlib's) and members just outside, each with the status of that very rule.  An outside member comes twice: as
    ".../trailer" with the CRC32 and ISIZE of the data it was meant to hold, and as ".../forged" with ISIZE = 0xff00 and another CRC32 -- a
    trailer that does not know the right answer, so that the refusal cannot be the trailer check's.  Every member starts with a stored block
    of 64 bytes (PRE), not the final one: an ISIZE of 0xff00 is out of reach of a payload of fewer than 64 bytes (inf_isize_possible), and
    such a member would be refused before the decoder ran.  The symbols no code may use (286, 287; 30, 31) stand first in their block, behind
    a few literals, and as the last code before the payload ends.
    Where a member breaks two rules (the order is the one of inflate_device.h's head comment):
      distance-and-room               a match that starts in front of the member and ends behind ISIZE: kInfFarBack
      unassigned-*-code-at-the-end    no code matches and the payload ends within 15 bits: kInfTruncated; with two more bytes of payload
                                      (".../padded") the same bits are kInfLitCode / kInfDistCode"""
    out = []
    FL, FD = canon(FIXED_LIT), canon(FIXED_DIST)
    ok_lit = lens(258, {97: 1, 256: 2, 257: 2})

    def start():
        b = Bits()
        b.put(0, 1), b.put(0, 2), b.align(), b.put(len(PRE), 16), b.put(len(PRE) ^ 0xffff, 16)
        b.out += PRE
        return b

    def inside(name, b, data):
        payload = b.bytes() if isinstance(b, Bits) else b
        out.append((name, wrap(payload, PRE + data), "kInfOk", PRE + data))

    def outside(name, status, b, data=b"", forged=True):
        payload = b.bytes() if isinstance(b, Bits) else b
        out.append((name + "/trailer", wrap(payload, PRE + data), status, None))
        if forged:
            assert len(payload) >= 64
            out.append((name + "/forged", wrap(payload, crc=zlib.crc32(PRE + data) ^ 0x5a5a5a5a, isize=FORGED_ISIZE), status, None))

    def fixed(b, items, eob=True):
        """a final fixed block of literals, ("L", symbol) and ("D", symbol) raw codes and ("X", value, bits) raw bits"""
        b.put(1, 1), b.put(1, 2)
        for it in items:
            if isinstance(it, int):
                b.code(FL[it])
            elif it[0] == "L":
                b.code(FL[it[1]])
            elif it[0] == "D":
                b.code(FD[it[1]])
            else:
                b.put(it[1], it[2])
        if eob:
            b.code(FL[256])
        return b

    def dyn(b, toks, litlens, distlens, cl=CL_EDGE, clsyms=None, eob=True, **kw):
        dynamic_header(b, litlens, distlens, cl=cl, clsyms=clsyms if clsyms is not None else run_lengths(list(litlens) + list(distlens)), **kw)
        if toks is not None:
            tokens(b, toks, canon(litlens), canon(distlens))
            if eob:
                b.code(canon(litlens)[256])
        return b

    def held(toks):
        return expand(list(PRE) + toks)[len(PRE):]

    # ---- HLIT and HDIST: 286 / 30 codes are the most; the members outside are whole and consistent for a decoder that counted further
    for nl in (286, 287, 288):
        b = dyn(start(), [97], lens(nl, {97: 1, 256: 2, 257: 2}), [1])
        inside("hlit-286", b, b"a") if nl == 286 else outside("hlit-%d" % nl, "kInfCounts", b, b"a")
    for nd in (30, 31, 32):
        b = dyn(start(), [97, (3, 1)], lens(259, {97: 1, 256: 2, 257: 3, 258: 3}), [1] + [0] * (nd - 1))
        inside("hdist-30", b, b"aaaa") if nd == 30 else outside("hdist-%d" % nd, "kInfCounts", b, b"aaaa")
    # ---- literal/length symbols 285 | 286, 287 and distance symbols 29 | 30, 31 of the fixed code, at three places
    far = [0] + [(258, 1)] * 96                                                # 24 833 bytes lie in front: distance symbol 29 starts at 24 577
    for place, front, back, eob in (("first", [], [97, 98], True), ("behind-literals", [97, 98, 99], [100], True), ("last", [97, 98, 99], [], False)):
        toks = front + [(258, 1)] + (back if eob else [])
        b = start()
        fixed_block(b, toks)
        inside("symbol-285-%s" % place, b, held(toks))
        toks = front + [(3, 24577)] + (back if eob else [])
        b = start()
        fixed_block(b, far, final=False)
        fixed_block(b, toks)
        inside("distance-symbol-29-%s" % place, b, held(far + toks))
        for s in (286, 287):
            # behind the symbol, where there is a behind: what a decoder that took it for a length would go on with (a distance code, literals)
            b = fixed(start(), front + [("L", s)] + ([("D", 0)] + back if eob else []), eob=eob)
            outside("symbol-%d-%s" % (s, place), "kInfLitCode", b, bytes(front))
        for s in (30, 31):
            b = fixed(start(), front + [("L", 257), ("D", s)] + ([("X", 0, 13)] + back if eob else []), eob=eob)
            outside("distance-symbol-%d-%s" % (s, place), "kInfDistCode", b, bytes(front))
    # ---- block types and the stored block's LEN / NLEN
    inside("btype-1", fixed(start(), [97]), b"a")
    inside("btype-2", dyn(start(), [97], ok_lit, [1]), b"a")
    b = start()
    b.put(1, 1), b.put(3, 2), b.put(0, 29)
    outside("btype-3", "kInfBlockType", b)
    for flip in (0, 1, 0x8000):
        b = start()
        b.put(1, 1), b.put(0, 2), b.align(), b.put(3, 16), b.put(3 ^ 0xffff ^ flip, 16)
        b.out += b"abc"
        inside("stored-len-nlen", b, b"abc") if not flip else outside("stored-len-nlen-bit-%x" % flip, "kInfStored", b, b"abc")
    b = start()                                                                  # (the member above: a stored block may reach the payload's last byte)
    b.put(1, 1), b.put(0, 2), b.align(), b.put(4, 16), b.put(4 ^ 0xffff, 16)
    b.out += b"abc"
    outside("stored-block-a-byte-longer-than-the-payload", "kInfTruncated", b, b"abc")
    # ---- the code lengths: a repeat needs a length in front of it, and no run may pass the last length
    inside("repeat-behind-a-length", dyn(start(), [0, 1, 2, 3], lens(257, {0: 3, 1: 3, 2: 3, 3: 3, 256: 1}), [0], clsyms=[3, (16, 0)] + zeros(252) + [1, 0]), bytes([0, 1, 2, 3]))
    outside("repeat-without-a-previous-length", "kInfCodeLengths",                # (a decoder that repeated "0": lengths for 3, 4, 5, 6)
            dyn(start(), [3, 4, 5, 6], lens(257, {3: 3, 4: 3, 5: 3, 6: 3, 256: 1}), [0], clsyms=[(16, 0), 3, (16, 0)] + zeros(249) + [1, 0]), bytes([3, 4, 5, 6]))
    front = zeros(97) + [1] + zeros(158) + [2, 2]                                 # ok_lit
    cl_runs = lens(19, {0: 2, 18: 2, 1: 3, 2: 3, 16: 3, 17: 3})
    for sym, tail, nd in ((16, [2, (16, 0)], 4), (17, [1, (17, 0)], 4), (18, [1, (18, 0)], 12)):
        dl = [2] * 4 if sym == 16 else [1] + [0] * (nd - 1)
        inside("run-%d-to-the-end" % sym, dyn(start(), [97], ok_lit, dl, cl=cl_runs, clsyms=front + tail), b"a")
        outside("run-%d-past-the-end" % sym, "kInfCodeLengths", dyn(start(), [97], ok_lit, dl[:nd - 1], cl=cl_runs, clsyms=front + tail), b"a")
    # ---- the end-of-block symbol needs a code
    b = dyn(start(), None, lens(258, {97: 1, 257: 1}), [1])
    b.put(0, 16)
    outside("no-end-of-block-code", "kInfNoEob", b, b"a")
    # ---- complete | over-subscribed, incomplete -- by one code of the longest length -- for each of the three codes
    full = dict([(97, 1), (256, 2), (257, 3)] + [(k, k + 4) for k in range(12)] + [(12, 15)])      # 1, 2, ..., 15, 15 bits
    inside("literal-code-complete", dyn(start(), [97, 0, 12], lens(258, full), [1]), bytes([97, 0, 12]))
    over, under = dict(full), dict(full)
    over[13] = 15
    del under[12]
    b = dyn(start(), None, lens(258, over), [1])
    b.put(0, 16)
    outside("literal-code-over-subscribed-by-one", "kInfLitTable", b, b"a")
    outside("literal-code-incomplete-by-one", "kInfLitTable", dyn(start(), [97, 0], lens(258, under), [1]), bytes([97, 0]))
    inside("literal-code-of-one-bit", dyn(start(), [], lens(257, {256: 1}), [0]), b"")
    outside("literal-code-of-two-bits", "kInfLitTable", dyn(start(), [], lens(257, {256: 2}), [0]))
    dfull = list(range(1, 16)) + [15]
    inside("distance-code-complete", dyn(start(), [97, (3, 1)], ok_lit, dfull), b"aaaa")
    b = dyn(start(), None, ok_lit, dfull + [15])
    b.put(0, 16)
    outside("distance-code-over-subscribed-by-one", "kInfDistTable", b, b"a")
    outside("distance-code-incomplete-by-one", "kInfDistTable", dyn(start(), [97, (3, 1)], ok_lit, dfull[:15]), b"aaaa")
    inside("distance-code-of-one-bit", dyn(start(), [97, (3, 1)], ok_lit, [1]), b"aaaa")
    outside("distance-code-of-two-bits", "kInfDistTable", dyn(start(), [97, (3, 1)], ok_lit, [2]), b"aaaa")
    cfull = lens(19, {18: 1, 0: 2, 1: 3, 2: 4, 3: 5, 4: 6, 5: 7, 6: 7})            # the code-length code has 7 bits at most
    inside("code-length-code-complete", dyn(start(), [97], ok_lit, [1], cl=cfull), b"a")
    cover, cunder = list(cfull), list(cfull)
    cover[7], cunder[6] = 7, 0
    b = start()
    dynamic_header(b, ok_lit, [1], cl=cover, clsyms=[])
    b.put(0, 32)
    outside("code-length-code-over-subscribed-by-one", "kInfCodeLengths", b, b"a")
    outside("code-length-code-incomplete-by-one", "kInfCodeLengths", dyn(start(), [97], ok_lit, [1], cl=cunder), b"a")
    # ---- a match may reach the member's first byte and no further
    for name, toks in (("first", []), ("behind-literals", [97, 98])):
        at = len(PRE) + len(toks)
        b = start()
        fixed_block(b, toks + [(3, at)])
        inside("distance-to-the-first-byte-%s" % name, b, held(toks + [(3, at)]))
        b = start()
        fixed_block(b, toks + [(3, at + 1)])
        outside("distance-in-front-of-the-member-%s" % name, "kInfFarBack", b, bytes(toks))
    b = start()
    fixed_block(b, [97, 98, (258, len(PRE) + 3)])
    out.append(("distance-and-room/trailer", wrap(b.bytes(), PRE + b"ab" + bytes(10)), "kInfFarBack", None))
    # ---- a code no symbol has, in front of more payload and at its end
    one, two = lens(257, {256: 1}), lens(258, {97: 2, 256: 2, 257: 1})
    for pad in (16, 0):
        b = dyn(start(), None, one, [0])
        b.put(1, 1), b.put(0, pad)                                               # "0" is the end of the block, "1" is nothing
        outside("unassigned-literal-code-" + ("padded" if pad else "at-the-end"), "kInfLitCode" if pad else "kInfTruncated", b)
        b = dyn(start(), None, two, [1])
        b.code(canon(two)[97]), b.code(canon(two)[257]), b.put(1, 1), b.put(0, pad)   # the lone distance code is "0"
        outside("unassigned-distance-code-" + ("padded" if pad else "at-the-end"), "kInfDistCode" if pad else "kInfTruncated", b, b"a")
    # ... and exactly at the rule's edge: with 14 bits left a code of 15 may have been cut off, with 15 left there is no such code
    cl_few = lens(19, {0: 2, 1: 3, 2: 3, 18: 1})

    def with_bits_left(make, left):
        for cl, ncl in ((CL_EDGE, 19), (cl_few, 19), (cl_few, 18)):               # (headers of odd and even lengths)
            for k in range(4):
                b = start()
                for _ in range(k):
                    fixed_block(b, [], final=False)                               # 10 bits
                make(b, cl, ncl)
                if (b.n + left) % 8 == 0:
                    b.put(1, 1), b.put(0, left - 1)
                    assert b.n == 0
                    return b
        raise AssertionError(left)

    def lit_at(b, cl, ncl):
        dyn(b, None, one, [0], cl=cl, ncl=ncl)

    def dist_at(b, cl, ncl):
        dyn(b, None, two, [1], cl=cl, ncl=ncl)
        b.code(canon(two)[97]), b.code(canon(two)[257])
    for left in (14, 15):
        outside("unassigned-literal-code-%d-bits-left" % left, "kInfLitCode" if left == 15 else "kInfTruncated", with_bits_left(lit_at, left))
        outside("unassigned-distance-code-%d-bits-left" % left, "kInfDistCode" if left == 15 else "kInfTruncated", with_bits_left(dist_at, left), b"a")
    # ---- the payload ends one bit short of what a field needs (a decoder that did not count would read the absent bit as 0 and go on)
    def cut(name, b, data=b""):
        assert b.n == 0, name                                                     # the missing bit would be the payload's next
        outside(name + "-cut-by-a-bit", "kInfTruncated", b, data)
    b = start()
    fixed_block(b, [200] * 4, final=False)                                        # 3 + 4 x 9 + 7 bits
    b.put(1, 2)
    cut("block-header", b, bytes([200] * 4))
    b = start()
    b.put(1, 1), b.put(2, 2), b.put(0, 13)
    cut("dynamic-header", b)
    b = start()
    b.put(1, 1), b.put(2, 2), b.put(0, 5), b.put(0, 5), b.put(15, 4)
    for _ in range(7):
        b.put(1, 3)
    b.put(1, 2)
    cut("code-length-code-length", b)
    b = start()
    dynamic_header(b, ok_lit, [1], cl=cfull, clsyms=[])
    v, k = canon(cfull)[5]
    assert k == 7
    for i in range(k - 1, 0, -1):
        b.put(v >> i & 1, 1)
    cut("code-length-code", b)
    b = start()
    dynamic_header(b, ok_lit, [1], cl=cfull, clsyms=[1, 0, 0])
    b.code(canon(cfull)[18]), b.put(0, 6)
    cut("zero-run-extra-bits", b)
    b = fixed(start(), [200, 200, 200, ("L", 277), ("X", 0, 3)], eob=False)         # symbol 277: 4 extra bits
    cut("length-extra-bits", b, bytes([200] * 3))
    b = fixed(start(), [("L", 257), ("D", 6), ("X", 0, 1)], eob=False)             # distance symbol 6: 2 extra bits
    cut("distance-extra-bits", b)
    # ---- ISIZE bytes and ISIZE + 1: by a literal, by a match, by a stored block; the trailer's ISIZE is the rule here, so these come once
    def isize_pair(name, b, data):
        inside("isize-reached-by-" + name, b, data)
        short = PRE + data[:-1]
        out.append(("isize-passed-by-%s/trailer" % name, wrap(b.bytes(), short), "kInfTooLong", None))
    b = start()
    fixed_block(b, [97, 98, 99])
    isize_pair("a-literal", b, b"abc")
    b = start()
    fixed_block(b, [97, (3, 1)])
    isize_pair("a-match", b, b"aaaa")
    b = start()
    b.put(1, 1), b.put(0, 2), b.align(), b.put(3, 16), b.put(3 ^ 0xffff, 16)
    b.out += b"abc"
    isize_pair("a-stored-block", b, b"abc")
    # ... and at ISIZE = 0xff00 with a CRC32 that is not the data's: 0xff01 bytes are refused for their number, 0xff00 for the CRC32
    for extra, status in ((0, "kInfCrc"), (1, "kInfTooLong")):
        toks = [97] + [(258, 1)] * 252 + [(199 + extra, 1)]
        assert len(PRE) + len(held(toks)) == FORGED_ISIZE + extra
        b = start()
        fixed_block(b, toks)
        out.append(("isize-0xff00-%s/forged" % ("passed" if extra else "reached"), wrap(b.bytes(), crc=zlib.crc32(PRE + held(toks)) ^ 0x5a5a5a5a, isize=FORGED_ISIZE), status, None))
        if not extra:
            inside("isize-0xff00-reached", b, held(toks))
    names = [c[0] for c in out]
    assert len(set(names)) == len(names)
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


def constants(exe):
    """{name: number} of inflate_device.h's statuses, as the checker prints them"""
    w = subprocess.run([exe, "constants"], stdout=subprocess.PIPE, check=True).stdout.split()
    return {w[i].decode(): int(w[i + 1]) for i in range(0, len(w), 2)}


def run_checker(exe, bufs, timeout=600, direct=False):
    """[(status, bytes or None)] of the decoder's host build for every buffer; the sanitizer's report, if any, fails the call.
    direct: every buffer is u32 hdr, u32 isize and a member, and inf_member is called with just that (no bgzf_member_header in front)"""
    tmp = tempfile.mkdtemp(prefix="psvr_infl_")
    with open(os.path.join(tmp, "cases"), "wb") as f:
        f.write(struct.pack("<I", len(bufs)))
        for b in bufs:
            f.write(struct.pack("<I", len(b)) + bytes(b))
    r = subprocess.run([exe] + (["direct"] if direct else []) + [os.path.join(tmp, "cases"), os.path.join(tmp, "results")], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=timeout)
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
    return {"by hand": [m for _, m, _ in hand_bad()], "rule edges": [c[1] for c in rule_edges()], "truncations": truncations(), "payload mutations": payload_mutations(members), "header mutations": header_mutations(members)}


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
