"""Names at which a name order cut into 8-byte chunks can go wrong, as BAM records, and the order restated: what the host check
(test_name_key.py), the sink's check (test_nsort_sink.py) and the GPU tests (test_sort_names_gpu.py, test_store_names_gpu.py) share.
A case is a list of (name field, flag): the field is what lies in the record's l_read_name bytes, its NUL included, so a field may hold an
early NUL with other bytes behind it.  The order is `panSVR sort -n`'s: the name up to its first NUL as unsigned bytes, flag & 0xc0, arrival."""
import itertools
import random
import struct

from test_bam_store_gpu import SPANS, make_record

LENGTHS = (1, 7, 8, 9, 15, 16, 17, 23, 24, 25, 254)
P16 = b"0123456789abcdef"
P24 = P16 + b"ghijklmn"


def _f(name):
    return name + b"\0"


def groups():
    """name -> [(field, flag)]"""
    rng = random.Random(5)
    g = {}
    # every length twice with different last bytes, and once more as a prefix of the others
    g["lengths"] = [(_f(bytes(rng.randrange(33, 127) for _ in range(n))), rng.choice((0x40, 0x80))) for n in LENGTHS for _ in range(2)]
    g["same letter, every length"] = [(_f(b"a" * n), 0x40) for n in reversed(LENGTHS)] + [(_f(b"a" * n), 0x80) for n in LENGTHS]
    g["prefixes"] = [(_f(b"read12"), 0x40), (_f(b"read1"), 0x80), (_f(b"read"), 0x40), (_f(b"read123456789"), 0x80), (_f(b"read1234"), 0x40), (_f(b"read12345"), 0x40), (_f(b"r"), 0x80)]
    g["chunk edges"] = [(_f(b"abcdefgY"), 0x40), (_f(b"abcdefgX"), 0x40), (_f(b"abcdefghY"), 0x80), (_f(b"abcdefghX"), 0x80), (_f(b"abcdefgh"), 0x40), (_f(b"abcdefg"), 0x40),
                        (_f(b"abcdefghijklmnoQ"), 0x40), (_f(b"abcdefghijklmnoP"), 0x80), (_f(b"abcdefghijklmnopB"), 0x40), (_f(b"abcdefghijklmnopA"), 0x80)]
    g["shared prefix of 16"] = [(_f(P16 + t), f) for t, f in ((b"zz", 0x40), (b"z", 0x80), (b"a", 0x40), (b"zz", 0x80), (b"b" * 9, 0x40), (b"b" * 8, 0x40), (b"a", 0x80))]
    g["shared prefix of 24"] = [(_f(P24 + t), f) for t, f in ((b"9", 0x40), (b"1", 0x80), (b"10", 0x40), (b"1", 0x40), (b"9" * 8, 0x80), (b"9" * 9, 0x80), (b"2", 0x40))]
    g["unsigned bytes"] = [(_f(b"a" + bytes([c])), 0x40) for c in (0xff, 0x7f, 0x80, 0x7e, 0x41, 0xfe, 0x01, 0x81)] + [(_f(bytes([0x80]) * 9), 0x40), (_f(b"z" * 9), 0x40),
                                                                                                                        (_f(b"z" * 8 + bytes([0x80])), 0x80), (_f(b"z" * 8 + b"~"), 0x80)]
    g["early NUL"] = [(b"ab\0ZZ\0", 0x80), (b"ab\0AA\0", 0x40), (_f(b"ab"), 0x80), (b"ab\0\xff\xff\xff\xff\xff\xff\xff\0", 0x40), (_f(b"abc"), 0x40), (b"a\0c\0", 0x40), (b"\0bc\0", 0x80), (_f(b""), 0x40),
                      (b"abcdefgh\0XYZ\0", 0x40), (_f(b"abcdefgh"), 0x40), (b"abcdefg\0hij\0", 0x80)]
    g["flags in every arrival order"] = [(_f(b"pair%02d" % k), f | extra) for k, p in enumerate(itertools.permutations((0x40, 0x80, 0, 0xc0)))
                                         for f, extra in zip(p, (0x1, 0x10, 0x23, 0x400))]
    g["duplicates"] = [(_f(b"dup"), 0x40)] * 3 + [(_f(b"dup"), 0x80)] * 2 + [(_f(b"dup"), 0x40)] * 2 + [(_f(P24 + b"dup"), 0x80)] * 3
    g["one name"] = [(_f(b"solo"), 0x40)]
    g["empty"] = []
    g["everything"] = [x for k in sorted(g) for x in g[k]]
    return g


def with_name(rec, field):
    """rec with its name field replaced (l_read_name and block_size follow)"""
    assert 1 <= len(field) <= 255
    body = rec[4:12] + bytes([len(field)]) + rec[13:36] + field + rec[36 + rec[12]:]
    return struct.pack("<I", len(body)) + body


def records(case, seed=1, bare_last=True):
    """the case as records from test_bam_store_gpu's maker: bodies of lengths in turn, so that the names' addresses in a stream take every
    residue modulo 8; with bare_last the last record ends with its name (no CIGAR, no bases: the name is the last bytes of the buffer)"""
    rng = random.Random(seed)
    out = []
    for i, (field, flag) in enumerate(case):
        tid, pos = rng.randrange(3), rng.randrange(1 << 20)
        base = make_record(48 + (i * 5 + seed) % 45, tid, pos, flag, rng.choice(SPANS), seed * 7919 + i)
        if bare_last and i == len(case) - 1:
            base = make_record(36, tid, pos, flag, [], i)
        out.append(with_name(base, field))
    return out


def bulk(n, seed):
    """n records of read pairs in no order: names that share a long prefix, both reads of a pair, some names three times and more"""
    rng = random.Random(seed)
    recs = []
    for i in range(n):
        name = b"SRR062634.%d" % rng.randrange(max(n // 2, 1))
        base = make_record(120 + i % 60, rng.randrange(3), rng.randrange(1 << 24), rng.choice((0x40, 0x80)) | rng.choice((0, 0x10, 0x1)), rng.choice(SPANS), seed + i)
        recs.append(with_name(base, name + b"\0"))
    return recs


def name_of(rec):
    return rec[36:36 + rec[12]].split(b"\0")[0]


def flag_of(rec):
    return struct.unpack_from("<H", rec, 18)[0]


def restated_order(recs):
    return sorted(range(len(recs)), key=lambda i: (name_of(recs[i]), flag_of(recs[i]) & 0xc0, i))


def restated_order_names(names, tie=None):
    return sorted(range(len(names)), key=lambda i: (names[i], tie[i] if tie is not None else 0, i))
