"""Inflated BAM streams for the record-chain finder (pansvr_amd/csrc/bam_chain_device.h): tests/test_bam_chain.py runs its host build,
tests/test_sort_device_gpu.py the device's through psvr_bam_store_append_bgzf.  The yardstick is walk(): one record after the other by the rules
of BamReader::next (bam_reader.h) and the store's bound on block_size, in the reader's order."""
import os
import random
import struct
import subprocess
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
CHECK_SRC = os.path.join(HERE, "tools", "bam_chain_check.cpp")
N_REF = 3


def walk(buf, start=0):
    """(starts of the whole records, where the chain ends, malformed): the chain ends at the first byte that is no whole good record's --
    the stream's end, a record the stream cuts off (its tail), or a malformed record (malformed = True)"""
    at, n, starts = start, len(buf), []
    while True:
        if n - at < 4:
            return starts, at, False
        bs, = struct.unpack_from("<I", buf, at)
        if bs < 32 or bs > 0x7ffffff0:
            return starts, at, True
        if n - at < 36 or at + 4 + bs > n:
            return starts, at, False
        l_name, = struct.unpack_from("<B", buf, at + 12)
        n_cig, = struct.unpack_from("<H", buf, at + 16)
        l_seq, = struct.unpack_from("<i", buf, at + 20)
        if l_seq < 0 or l_name + 4 * n_cig + (l_seq + 1) // 2 + l_seq > bs - 32:
            return starts, at, True
        if l_name == 0 or buf[at + 36 + l_name - 1] != 0:
            return starts, at, True
        starts.append(at)
        at += 4 + bs


def expected(buf, start, seg):
    """what the checker must print: (total, tail, first_malformed, entries)"""
    starts, last, bad = walk(buf, start)
    n_seg = (len(buf) + seg - 1) // seg
    chain = starts + [last]
    entries, k = [], 0
    for s in range(n_seg + 1):
        while k < len(chain) - 1 and chain[k] < s * seg:
            k += 1
        entries.append(chain[k])                               # (behind the chain's end no record starts: its end stands for all of them)
    return len(starts), len(buf) - last, len(starts) if bad else -1, entries


def record(length, seed, tid=None, pos=None, l_seq=None):
    """a valid record of exactly `length` bytes (>= 37): a name of at least its NUL, no CIGAR, a few bases, then random bytes"""
    rng = random.Random(seed)
    room = length - 36
    l_name = min(room, 1 + seed % 9)
    rest = room - l_name
    if l_seq is None:
        l_seq = min(rest * 2 // 3, seed % 5)
    assert (l_seq + 1) // 2 + l_seq <= rest
    name = bytes(rng.randrange(33, 127) for _ in range(l_name - 1)) + b"\0"
    tail = bytes(rng.randrange(256) for _ in range(rest)) if rest <= 200 else bytes(rest)
    body = struct.pack("<iiBBHHHiiii", rng.randrange(-1, N_REF) if tid is None else tid, rng.randrange(-1, 1 << 28) if pos is None else pos, l_name, 60, 4680, 0, rng.randrange(2) << 4,
                       l_seq, -1, -1, 0) + name + tail
    assert len(body) + 4 == length
    return struct.pack("<I", len(body)) + body


def records(n, seed, long_at=None):
    """n records of 37..99 bytes in turn with random tails; at index long_at one of 70 000 bytes (it covers whole segments)"""
    return [record(70000 if i == long_at else 37 + i % 63, seed * 100003 + i) for i in range(n)]


def decoy_stream(tail):
    """Segments of 256 bytes: five small records, then a long one whose body holds two complete small records 3 bytes behind a segment
    boundary and ends `tail` filler bytes behind them, inside that same segment; then twenty small records.  26 records."""
    small = [record(40, 5000 + i, tid=i % N_REF, pos=100 + i) for i in range(27)]
    head = b"".join(small[:5])
    assert len(head) == 200
    decoy = small[5] + small[6]
    long_len = 515 + len(decoy) + tail - len(head)            # the long record: [200, 595 + tail)
    name = b"long\0"
    body = struct.pack("<iiBBHHHiiii", 1, 77, len(name), 60, 4680, 0, 0, 0, -1, -1, 0) + name
    body += bytes(515 - len(head) - 4 - len(body)) + decoy + b"\xff" * tail
    long_rec = struct.pack("<I", len(body)) + body
    assert len(long_rec) == long_len and (len(head) + long_len) // 256 == 515 // 256
    out = head + long_rec + b"".join(small[7:27])
    assert out[515:515 + len(decoy)] == decoy
    return out


# ---- block_size at the edges of chain_record's rules, at the edges of a segment ----------------------------------------------------------------------
EDGE_SEG = 16384
MIN_BLOCK, HEAD, STORE_MAX_BLOCK = 32, 36, 0x7ffffff0                          # bam_record.h: kBamRecMinBlock, kBamRecHead, kBamRecStoreMaxBlock
PLACES = (("at the segment's first byte", 0), ("in its last four bytes", -4), ("across the edge", -2))


def fill(n, seed, most=99):
    """whole records of n bytes altogether (n = 0, or n >= 37), none longer than `most`"""
    out, k = [], 0
    assert n == 0 or n >= 37, n
    while n > most + 37:
        s = most - (seed + 7 * k) % 62
        out.append(record(s, seed * 1009 + k))
        n -= s
        k += 1
    if n > most:
        out.append(record(n - 50, seed * 1009 + k))
        n = 50
    if n:
        out.append(record(n, seed * 1009 + k + 1))
    return out


def head(block_size, l_name=1, name=b"\0"):
    """the first 36 bytes of a record that passes every hint, with this block_size, and its name"""
    return struct.pack("<IiiBBHHHiiii", block_size, 0, 5, l_name, 60, 4680, 0, 0, 0, -1, -1, 0) + name


def edge_stream(seg=EDGE_SEG):
    """One stream of whole records, its segments `seg` bytes: records with block_size 33 (the shortest the reader takes: a name of one NUL), 35, 36
    and 37 (around kBamRecHead), each once at every place of PLACES; then per decoy one long record that covers three segments whole and holds the
    decoy at every place of PLACES -- decoys: 36 bytes with block_size 31, 32 (no record), 33 and 36 with a small record behind them (guessed,
    wrongly), and a head with block_size kBamRecStoreMaxBlock - 1, kBamRecStoreMaxBlock (a record the stream cuts off: guessed, wrongly) and
    kBamRecStoreMaxBlock + 1 (no record).  Nothing of that length is ever allocated.  -> (stream, number of records)"""
    parts, at, k = [], 0, 1

    def upto(target, seed):
        nonlocal at
        for r in fill(target - at, seed, most=8000):
            parts.append(r)
            at += len(r)
    for length in (4 + MIN_BLOCK + 1, 4 + HEAD - 1, 4 + HEAD, 4 + HEAD + 1):
        for _, off in PLACES:
            upto(k * seg + off, 31 * k)
            parts.append(record(length, 77 * k + length))
            at += length
            k += 1
    small = record(40, 4242, tid=1, pos=9)
    for bs in (MIN_BLOCK - 1, MIN_BLOCK, MIN_BLOCK + 1, HEAD, STORE_MAX_BLOCK - 1, STORE_MAX_BLOCK, STORE_MAX_BLOCK + 1):
        decoy = head(bs, 0, b"") if bs <= MIN_BLOCK else head(bs) + bytes(bs - 33) + small if bs < 100 else head(bs)
        upto(k * seg - 300, 57 * k)
        body = bytearray(record(3 * seg + 600, 999 + bs % 1000))
        for j, (_, off) in enumerate(PLACES):
            o = 300 + (j + 1) * seg + off - (seg if off == 0 else 0)            # the decoy's block_size: at k*seg, (k+2)*seg - 4, (k+3)*seg - 2
            assert body[o:o + len(decoy)] == bytes(len(decoy))
            body[o:o + len(decoy)] = decoy
        parts.append(bytes(body))
        at += len(body)
        k += 4
    upto(at + 200, 5)
    return b"".join(parts), len(parts)


def edge_ends(seg=EDGE_SEG):
    """[(name, stream)]: whole records up to a place of PLACES in the second segment, and there the stream's last thing:
    block_size 31 (malformed) and 32 with its 36 bytes (malformed: no room for the name's NUL -- the reader's rule, not the frame's);
    block_size 32 with fewer than 36 bytes left (the head is cut off: a tail, whatever block_size says);
    a record of exactly the bytes that are left, one byte more than that (cut off: a tail), one byte less (a tail of one byte);
    a head with block_size kBamRecStoreMaxBlock - 1 and kBamRecStoreMaxBlock (cut off: a tail) and kBamRecStoreMaxBlock + 1 (malformed)"""
    out = []
    whole = record(60, 8)
    for place, off in PLACES:
        front = b"".join(fill(seg + off, 13, most=8000))
        for name, last in (("block_size 31", head(31, 0, b"")), ("block_size 32, 36 bytes", head(32, 0, b"")), ("block_size 32, 35 bytes", head(32, 0, b"")[:35]),
                           ("block_size 32, 4 bytes", head(32, 0, b"")[:4]), ("block_size 33, 35 bytes", head(33)[:35]), ("block_size 33, 36 bytes", head(33)[:36]), ("block_size 33, whole", head(33)),
                           ("the last record ends the stream", whole), ("the last record lacks a byte", whole[:-1]), ("a byte behind the last record", whole + b"\x25"), ("three bytes behind the last record", whole + b"\x25\0\0"),
                           ("block_size kBamRecStoreMaxBlock - 1", head(STORE_MAX_BLOCK - 1) + bytes(40)), ("block_size kBamRecStoreMaxBlock", head(STORE_MAX_BLOCK) + bytes(40)),
                           ("block_size kBamRecStoreMaxBlock + 1", head(STORE_MAX_BLOCK + 1) + bytes(40))):
            out.append(("%s %s" % (name, place), front + last))
    return out


def build_checker(tmp, sanitize):
    exe = os.path.join(tmp, "bam_chain_check_asan" if sanitize else "bam_chain_check")
    flags = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"] if sanitize else ["-O2"]
    subprocess.check_call(["g++"] + flags + ["-std=c++17", "-Wall", "-o", exe, CHECK_SRC])
    return exe


def run_checker(exe, cases, timeout=600):
    """cases: [(stream, start, n_ref, seg)] -> [dict(total, tail, segments, no_guess, wrong_guess, rewalked, first_malformed, entries)]"""
    tmp = tempfile.mkdtemp(prefix="psvr_chain_")
    with open(os.path.join(tmp, "cases"), "wb") as f:
        f.write(struct.pack("<I", len(cases)))
        for buf, start, n_ref, seg in cases:
            f.write(struct.pack("<qiqI", start, n_ref, seg, len(buf)) + bytes(buf))
    r = subprocess.run([exe, os.path.join(tmp, "cases"), os.path.join(tmp, "results")], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=timeout)
    assert r.returncode == 0 and not r.stderr, "bam_chain_check: exit status %d\n%s" % (r.returncode, r.stderr.decode()[-4000:])
    out = []
    for line in open(os.path.join(tmp, "results")):
        head, _, ent = line.partition("|")
        v = [int(x) for x in head.split()]
        out.append(dict(zip(("total", "tail", "segments", "no_guess", "wrong_guess", "rewalked", "first_malformed"), v), entries=[int(x) for x in ent.split()]))
    assert len(out) == len(cases)
    return out
