"""Comparison of two decompressed BAM streams (SAM/BAM specification v1, section 4.2), for the golden tests: the reference's files
(tests/golden/<set>/<reads>.bam, written by htslib's bam_hdr_write / bam_write1) against the product's.  The BGZF blocks are not
compared: htslib flushes a block at a record boundary (bgzf_flush_try in bam_write1), the product cuts blocks at fixed offsets, and
the deflate bytes depend on the zlib build.  A difference is reported by record index and by field of the 32-byte core."""
import gzip
import struct

CORE = (("block_size", 0, "<I"), ("refID", 4, "<i"), ("pos", 8, "<i"), ("l_read_name", 12, "<B"), ("mapq", 13, "<B"), ("bin", 14, "<H"),
        ("n_cigar_op", 16, "<H"), ("flag", 18, "<H"), ("l_seq", 20, "<I"), ("next_refID", 24, "<i"), ("next_pos", 28, "<i"), ("tlen", 32, "<i"))


def stream(path):
    with gzip.open(path, "rb") as f:
        return f.read()


def split(raw):
    """(header bytes, [record bytes incl. block_size])"""
    assert raw[:4] == b"BAM\x01", "not a BAM stream"
    off = 8 + struct.unpack_from("<i", raw, 4)[0]
    n_ref = struct.unpack_from("<i", raw, off)[0]
    off += 4
    for _ in range(n_ref):
        off += 8 + struct.unpack_from("<i", raw, off)[0]
    head, recs = raw[:off], []
    while off < len(raw):
        assert off + 4 <= len(raw), "truncated block_size at byte %d" % off
        end = off + 4 + struct.unpack_from("<I", raw, off)[0]
        assert end <= len(raw), "record %d runs past the end of the stream" % len(recs)
        recs.append(raw[off:end])
        off = end
    return head, recs


def first_difference(got, want):
    """None when the two streams are equal, else a message naming the first record and the field that differ."""
    if got == want:
        return None
    gh, gr = split(got)
    wh, wr = split(want)
    if gh != wh:
        i = next((k for k in range(min(len(gh), len(wh))) if gh[k] != wh[k]), min(len(gh), len(wh)))
        return "header differs at byte %d (%d vs %d bytes of header)" % (i, len(gh), len(wh))
    for i, (g, w) in enumerate(zip(gr, wr)):
        if g == w:
            continue
        name = w[36:36 + w[12] - 1] if len(w) > 36 else b"?"
        for field, at, fmt in CORE:
            a, b = (struct.unpack_from(fmt, x, at)[0] if len(x) >= at + struct.calcsize(fmt) else None for x in (g, w))
            if a != b:
                return "record %d (%r): core field %s is %r, the reference's is %r" % (i, name, field, a, b)
        k = next((j for j in range(min(len(g), len(w))) if g[j] != w[j]), min(len(g), len(w)))
        return "record %d (%r): byte %d of the record after the core differs (%r vs the reference's %r)" % (i, name, k - 36, g[k:k + 16], w[k:k + 16])
    return "%d records, the reference has %d (first extra record: %d)" % (len(gr), len(wr), min(len(gr), len(wr)))
