"""The BAM files of `panSVR aln` (its default output, as the reference's) against the reference's own BAM files, record byte for record
byte.  The goldens tests/golden/<set>/<reads>.bam / .ori.bam were written by the reference objects through htslib's bam_hdr_write /
bam_write1 (oracle/ref_harness/ref_aln_main.cpp --bam, tests/golden/gen_aln_golden.py).  Here the results come from the CPU emulation of
the engine (tests/emu), and the product's BamWriter writes both files: the direct encoder (sam_emit.h) and, with --bam-via-text, the SAM
line's fields through BamWriter::encode.  The decompressed streams are compared (tests/bam_stream.py); fx1/crafted holds the records
that hit htslib's corners (FLAG 0x4 with a CIGAR across a bin boundary, the B operator, integer tags at every type boundary, ...)."""
import os
import subprocess
import tempfile

import pytest

import aln_common as ac
import bam_reader
import bam_stream
from test_emu_aln import CASES, EMU

NOT_ORI = [("fx1", "reads150"), ("fx2", "reads150")]
ROUTES = [("direct", []), ("text", ["--bam-via-text"])]


@pytest.fixture(scope="module")
def emu():
    subprocess.check_call(["make", "-s", "-C", os.path.join(ac.HERE, "emu")])
    return EMU


def emu_bam(name, rname, extra):
    w = ac.workdir(name)
    tmp = tempfile.mkdtemp(prefix="psvr_bamg_")
    out = [os.path.join(tmp, f) for f in ("o.bam", "p.bam")]
    r = subprocess.run([EMU, ac.index_dir(name), os.path.join(w, rname + ".fq"), os.path.join(w, "header.sam"), "--no-records", "--sam", os.path.join(tmp, "o.sam"),
                        "--ori-sam", os.path.join(tmp, "p.sam"), "--bam", out[0], "--ori-bam", out[1]] + extra, stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    assert r.returncode == 0, r.stderr.decode()[-1500:]
    return out


def check_files(got_files, name, golden_stem):
    for got, ext in zip(got_files, (".bam", ".ori.bam")):
        want = os.path.join(ac.golden_dir(name), golden_stem + ext)
        bam_reader.check_bgzf(got)
        diff = bam_stream.first_difference(bam_stream.stream(got), bam_stream.stream(want))
        assert diff is None, "%s%s: %s" % (golden_stem, ext, diff)


@pytest.mark.parametrize("route,extra", ROUTES)
@pytest.mark.parametrize("name,rname", CASES)
def test_bam_files_equal_the_reference_bam_files(emu, name, rname, route, extra):
    check_files(emu_bam(name, rname, extra), name, rname)


@pytest.mark.parametrize("route,extra", ROUTES)
@pytest.mark.parametrize("name,rname", NOT_ORI)
def test_not_ori_bam_files_equal_the_reference_bam_files(emu, name, rname, route, extra):
    check_files(emu_bam(name, rname, ["-Q"] + extra), name, rname + ".notori")


def test_crafted_set_reaches_the_corners():
    """the crafted goldens hold what they were made for: FLAG 0x4 records with a CIGAR whose span crosses a 16 kb bin boundary (their
    bin is the one of a 1-base span), B-operator records, and every integer tag type"""
    _, refs, recs = bam_reader.read_bam(os.path.join(ac.golden_dir("fx1"), "crafted.ori.bam"))
    crossing = [r for r in recs if int(r[1]) & 0x4 and r[5] != "*" and
                bam_reader.reg2bin(int(r[3]) - 1, int(r[3]) - 1 + 150) != bam_reader.reg2bin(int(r[3]) - 1, int(r[3]))]
    assert crossing, "no FLAG 0x4 record with a CIGAR across a bin boundary"
    assert any("B" in r[5] for r in recs), "no record with a B operator"
    _, recs_main = bam_stream.split(bam_stream.stream(os.path.join(ac.golden_dir("fx1"), "crafted.ori.bam")))
    types = set()
    for rec in recs_main:
        i = rec.find(b"X0")
        while i >= 0 and i + 2 < len(rec):
            types.add(chr(rec[i + 2]))
            i = rec.find(b"X", i + 3)
    assert {"c", "C", "s", "S", "i", "I"} <= types, types
    assert len(refs) == 32


def test_reader_bin_follows_sam_parse1():
    """bam_reader's bin check takes sam_parse1's span: 1 for a FLAG 0x4 record whatever its CIGAR"""
    assert bam_reader.reg2bin(16284, 16285) == 4681 and bam_reader.reg2bin(16284, 16434) == 585
