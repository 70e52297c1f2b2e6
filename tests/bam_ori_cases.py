"""Inputs and helpers for the tests of the second BAM file's device encoder (tests/test_bam_ori_device.py on the host build of
pansvr_amd/csrc/bam_ori_device.h, tests/test_bam_ori_gpu.py through psvr_bam_emit_ori_*).  The yardstick is the BAM branch of
SamEmitter::ori_pair (sam_emit.h), which tests/tools/bam_ori_device_check.cpp runs on the same text and the same generated results."""
import os
import subprocess
import tempfile

import bam_emit_cases as bc
import fastq_cases as fc

HERE = os.path.dirname(os.path.abspath(__file__))
CHECK_SRC = os.path.join(HERE, "tools", "bam_ori_device_check.cpp")
CLI = fc.CLI
N_HEADER = 30
MFS = 520
LENGTHS = (1, 2, 15, 16, 17, 31, 32, 33, 150)
# the thirteen integers of fx1/crafted's TAG_ sections: every border between two of the BAM integer types
BOUNDARY_INTS = (-129, -128, 127, 128, 255, 256, 65535, 65536, -32769, -32768, 0, -1, -128)
# families in which both a plain and a declining text (or class) exist: states 1 and 2 must occur in each
TWO_SIDED = ("seq", "name", "qual", "comment", "number", "cigar", "tags", "index")


def build_checker(tmp, sanitize):
    exe = os.path.join(tmp, "bam_ori_device_check_asan" if sanitize else "bam_ori_device_check")
    flags = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"] if sanitize else ["-O2"]
    subprocess.check_call(["g++"] + flags + ["-std=c++17", "-Wall", "-o", exe, CHECK_SRC, "-lz", "-lpthread"])
    return exe


def run_checker(exe, text, cls, seed, mfs=MFS, n_header=N_HEADER, timeout=300):
    """(summary dict, out file bytes) of one case; a mismatch with ori_pair or a sanitizer's report fails the call."""
    tmp = tempfile.mkdtemp(prefix="psvr_boc_")
    with open(os.path.join(tmp, "in.fq"), "wb") as f:
        f.write(text)
    r = subprocess.run([exe, "run", os.path.join(tmp, "in.fq"), cls, str(seed), str(mfs), str(n_header), os.path.join(tmp, "out")], stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                       timeout=timeout)
    assert r.returncode == 0 and not r.stderr, "bam_ori_device_check (%s): exit status %d\n%s\n%s" % (cls, r.returncode, r.stdout.decode(), r.stderr.decode()[-4000:])
    w = r.stdout.split()
    assert w[0] == b"class" and w[1].decode() == cls
    summary = {"label": w[2].decode()}
    summary.update({w[i].decode(): int(w[i + 1]) for i in range(3, len(w), 2)})
    return summary, open(os.path.join(tmp, "out"), "rb").read()


def split_out(raw):
    """The checker's out file (the layout of bam_emit_device_check's; the eighth number is the gate's min_filter_score)."""
    out = bc.split_out(raw)
    out["min_filter_score"] = out.pop("n_anchor")
    return out


def comment(chr_id=3, ref_bg=777, flag=b"99", mapq=b"60", cigar=b"50M", mate=(b"3", b"1234", b"300"), tags=(b"NM:i:3",), raw_tail=None):
    """A comment of the `signal` step: the original alignment's tokens, then the FLAG_ / CIGAR_ / MATE_ / TAG_ sections.  raw_tail replaces
    everything from FLAG_ on."""
    head = b"%d_%d_0_280_60_a_b_c_d_FY_STAT_150_200_400_600_" % (chr_id, ref_bg)
    if raw_tail is not None:
        return head + raw_tail
    return head + b"FLAG_%s_%s_CIGAR_%s_MATE_%s_%s_%s_TAG_" % (flag, mapq, cigar, mate[0], mate[1], mate[2]) + b"".join(t + b"_" for t in tags)


def each_pair(n_pairs, make, seq=b"ACGTTGCAAN" * 5):
    """make(i, k) -> the keyword arguments of comment() for read k (1, 2) of pair i; names and lines every encoder takes"""
    return b"".join(fc.read(name=b"o%d/%d" % (i, k), comment=comment(**make(i, k)), seq=seq, qual=b"IIIIIHHHH#" * (len(seq) // 10) + b"5" * (len(seq) % 10)) for i in range(n_pairs) for k in (1, 2))


def one_of(n_pairs, bad, good=None):
    """pairs in which read 1 + i % 2 holds `bad` (keyword arguments of comment()) and the other read `good`"""
    return each_pair(n_pairs, lambda i, k: bad if k == 1 + i % 2 else (good or {}))


def cases(golden=True):
    """[dict(name, family, label, expect, text, cls, seed, mfs)].  label: 'plain' (no pair may be declined) or 'declining' (every pair must
    be).  expect: 'written' (every pair is in state 1), 'nothing' (every pair in state 0) or None."""
    C = []

    def add(name, family, label, text, cls="kept", seed=1, expect=None, mfs=MFS):
        C.append(dict(name=name, family=family, label=label, expect=expect, text=text, cls=cls, seed=seed, mfs=mfs))

    if golden:
        for i, (name, text) in enumerate(fc.golden_fastqs()):
            add("golden " + name, "golden", "plain", text, "mixed", seed=100 + i)
        add("golden fx1/reads150, every pair kept", "golden", "plain", fc.golden_fastqs()[0][1], "kept", seed=99)
        add("golden fx1/crafted, every pair kept", "golden", "plain", dict(fc.golden_fastqs())["fx1/crafted"], "kept", seed=98)
    clean = each_pair(200, lambda i, k: dict(ref_bg=1000 + i))
    # pair counts on both sides of a workgroup (16 pairs) and of the command's chunk
    for n in (1, 255, 256, 257, 4097):
        add("%d pairs" % n, "counts", "plain", each_pair(n, lambda i, k: dict(ref_bg=1 + i, flag=b"83" if (i + k) % 3 else b"163")), "mixed", seed=20 + n)
    # SEQ / QUAL: every length around the group's width on both values of flag & 0x10
    for n in LENGTHS:
        seq = (b"ACGTNacgtnRYKM" * 11)[:n]
        add("reads of %d bases" % n, "seq", "plain", each_pair(4, lambda i, k: dict(flag=b"83" if (i + k) % 2 else b"163"), seq=seq), expect="written")
    add("reads of 0 bases", "seq", "declining", each_pair(4, lambda i, k: dict(flag=b"83" if (i + k) % 2 else b"163"), seq=b""))
    add("a * for the bases", "seq", "declining", b"".join(fc.read(name=b"s%d" % i, comment=comment(), seq=b"*" if k == 1 + i % 2 else b"A", qual=b"I") for i in range(4) for k in (1, 2)))
    add("IUPAC, lower case and other bytes", "seq", "plain", each_pair(6, lambda i, k: dict(flag=b"16" if (i + k) % 2 else b"0"), seq=b"ACGTNacgtnRYKMSWBDHVrykmswbdhv=.*0123U\x01\x7f\xff "), expect="written")
    add("a * for the qualities", "seq", "plain", b"".join(fc.read(name=b"s%d" % i, comment=comment(flag=b"16" if i % 2 else b"0"), seq=b"AC"[:k], qual=b"**"[:k]) for i in range(4) for k in (1, 2)), expect="written")
    # names, qualities
    add("names of 1 and 254 bytes", "name", "plain", b"".join(fc.read(name=b"n" * (1 if (i + k) % 2 else 254), comment=comment()) for i in range(6) for k in (1, 2)), expect="written")
    add("names of 0 bytes", "name", "declining", b"".join(fc.read(name=b"" if k == 1 + i % 2 else b"ok", comment=comment()) for i in range(6) for k in (1, 2)))
    add("names of 255 bytes", "name", "declining", b"".join(fc.read(name=b"n" * (255 if k == 1 + i % 2 else 254), comment=comment()) for i in range(6) for k in (1, 2)))
    for d, label in ((-1, "declining"), (1, "declining"), (0, "plain")):
        add("quality line %+d" % d, "qual", label, b"".join(fc.read(name=b"q%d" % i, comment=comment(), seq=b"ACGT" * 5, qual=b"I" * (20 + (d if k == 1 + i % 2 else 0))) for i in range(6) for k in (1, 2)))
    # the comment: a tab, a NUL, each missing section, numbers the host reads with sscanf
    whole = comment()
    add("a tab in the comment", "comment", "declining", b"".join(fc.read(name=b"t%d" % i, comment=(whole[:3 * i] + b"\t" + whole[3 * i:]) if k == 1 + i % 2 else whole) for i in range(36) for k in (1, 2)))
    add("a NUL in the comment", "comment", "declining", b"".join(fc.read(name=b"z%d" % i, comment=(whole[:3 * i] + b"\0" + whole[3 * i:]) if k == 1 + i % 2 else whole) for i in range(36) for k in (1, 2)))
    add("whole comments", "comment", "plain", clean, expect="written")
    missing = [b"", b"FLA_99_60_CIGAR_50M_MATE_3_1234_300_TAG_NM:i:3_", b"FLAG_99_60_CIGA_50M_MATE_3_1234_300_TAG_NM:i:3_", b"FLAG_99_60_CIGAR_50M", b"FLAG_99_60_CIGAR_50M_", b"FLAG_99_60_CIGAR_50M_MATE",
               b"FLAG_99_60_CIGAR_50M_MATE_3_1234_300_TA_NM:i:3_", b"CIGAR_50M_MATE_3_1234_300_TAG_NM:i:3_FLAG_99_60_", b"FLAG_99_60_CIGAR_50M_MATE_3_1234_300_", b"FLAG_99_60_CIGAR_"]
    add("each missing section", "section", "plain", each_pair(2 * len(missing), lambda i, k: dict(raw_tail=missing[i // 2]) if k == 1 + i % 2 else {}), expect="nothing")
    slow = [dict(flag=b"+99"), dict(flag=b" 99"), dict(flag=b"1234567890"), dict(flag=b"-1"), dict(flag=b""), dict(mapq=b""), dict(mapq=b"x"), dict(mapq=b"1234567890"), dict(mate=(b"+3", b"1", b"1")),
            dict(mate=(b"3", b"", b"1")), dict(mate=(b"3", b"1", b"")), dict(mate=(b"3", b"1", b"--1")), dict(mate=(b"3", b"1234567890", b"1")), dict(mate=(b"x", b"1", b"1")),
            dict(raw_tail=b"FLAG_99_60_CIGAR_50M_MATE_3_1234"), dict(raw_tail=b"FLAG_99x60_CIGAR_50M_MATE_3_1234_300_TAG_NM:i:3_")]
    add("numbers for sscanf", "number", "declining", each_pair(2 * len(slow), lambda i, k: slow[i // 2] if k == 1 + i % 2 else {}))
    plain_numbers = [dict(flag=b"0", mapq=b"0"), dict(flag=b"999999999", mapq=b"999999999"), dict(flag=b"007", mapq=b"000000255"), dict(flag=b"65535", mapq=b"255"), dict(flag=b"65536", mapq=b"256"),
                     dict(flag=b"20", mapq=b"7"), dict(flag=b"4", cigar=b"50M"), dict(flag=b"99", mapq=b"60x")]
    add("plain numbers", "number", "plain", each_pair(2 * len(plain_numbers), lambda i, k: plain_numbers[i // 2] if k == 1 + i % 2 else {}), expect="written")
    mates = [(b"-1", b"1234", b"300"), (b"3", b"-1", b"-300"), (b"3", b"-2", b"0"), (b"3", b"0", b"1"), (b"%d" % N_HEADER, b"5", b"5"), (b"%d" % (N_HEADER - 1), b"5", b"-5"), (b"0", b"999999999", b"-999999999"),
             (b"-999999999", b"-999999999", b"999999999"), (b"-0", b"-0", b"-0")]
    add("MATE_ values", "mate", "plain", each_pair(2 * len(mates), lambda i, k: dict(mate=mates[i // 2]) if k == 1 + i % 2 else {}), expect="written")
    # original alignments the gate or the header turns away
    add("an original chr_id of -1", "gate", "plain", one_of(8, dict(chr_id=-1)), expect="nothing")
    add("original chr_ids outside the header", "skip", "plain", each_pair(12, lambda i, k: dict(chr_id=(N_HEADER, -2, 1 << 30)[i % 3]) if k == 1 + i % 2 or i >= 6 else {}))
    add("original positions at the top", "skip", "plain", each_pair(8, lambda i, k: dict(ref_bg=(0, 0x7ffffffe, 0x7fffffff, 0xffffffff)[(i + k) % 4])), expect="written")
    # CIGAR texts
    ops = b"MIDNSHP=XB"
    good_cigars = [b"*", b"", b"7M", b"3S47M", b"1M" * 16, b"1M" * 17, b"60M5B40M", b"0M", b"0005M", b"268435455M", b"268435456M1D", b"99999999999M2S"] + [b"3M5%c9M" % c for c in ops] + [b"5%c" % c for c in ops]
    add("CIGAR texts", "cigar", "plain", each_pair(2 * len(good_cigars), lambda i, k: dict(cigar=good_cigars[i // 2], flag=b"83" if i % 4 < 2 else b"99") if k == 1 + i % 2 else {}), expect="written")
    add("65535 operators", "cigar", "plain", one_of(2, dict(cigar=b"1M" * 65535)), expect="written")
    add("65536 operators", "cigar", "declining", one_of(2, dict(cigar=b"1M" * 65536)))
    bad_cigars = [b"-5M", b"5Q", b"5M3", b"M", b"5MM", b"**", b"5m", b"5M-", b"5 M", b"3M5-2I", b"5"]
    add("CIGAR texts the host refuses or reads with a sign", "cigar", "declining", each_pair(2 * len(bad_cigars), lambda i, k: dict(cigar=bad_cigars[i // 2]) if k == 1 + i % 2 else {}))
    # TAG_ texts
    ints = tuple(b"X%x:i:%d" % (j, v) for j, v in enumerate(BOUNDARY_INTS))
    good_tags = [dict(raw_tail=b"FLAG_99_60_CIGAR_50M_MATE_3_1234_300_TAG_"), dict(raw_tail=b"FLAG_99_60_CIGAR_50M_MATE_3_1234_300_TAG__"), dict(tags=(b"NM:i:3",)), dict(tags=ints), dict(tags=(b"NM:i:-0", b"X0:i:999999999", b"X1:i:-999999999", b"X2:i:000000001")),
                 dict(tags=(b"XA:Z:c1,+100,50M,0;c2,-7,10S40M,1;", b"NM:i:1")), dict(tags=(b"SA:Z:c1,100,+,50M,60,0;", b"XA:Z:a_b_c,_d:e_f", b"NM:i:1")), dict(tags=(b"XA:Z:with_XY:Z:inside", b"X1:Z:")),
                 dict(tags=(b"XT:A:U", b"XU:A:", b"XV:A:long", b"XH:H:1AE301", b"XI:H:")), dict(tags=(b"XA:Z:x_y:", b"XB:Z:_", b"XC:Z:__:_:_")), dict(tags=(b"", b"NM:i:1", b"X0:A:q")),
                 dict(raw_tail=b"FLAG_99_60_CIGAR_50M_MATE_3_1234_300_TAG_NM:i:33"), dict(raw_tail=b"FLAG_99_60_CIGAR_50M_MATE_3_1234_300_TAG_NM:i:3_X0:Z:ab"), dict(raw_tail=b"FLAG_99_60_CIGAR_50M_MATE_3_1234_300_TAG_NM:i:3_X0:Z:ab_X")]
    add("TAG_ texts", "tags", "plain", each_pair(2 * len(good_tags), lambda i, k: good_tags[i // 2] if k == 1 + i % 2 else {}), expect="written")
    bad_tags = [(b"X0:i:1234567890",), (b"X0:f:1.5",), (b"X0:B:c,1,2",), (b"X0:x:1",), (b"NM:i",), (b"NM:i:3", b"N:i:3"), (b"X0:i:",), (b"X0:i:+1",), (b"X0:i: 1",), (b"X0:i:1x",), (b"X0:i:-",), (b"NMi::3",), (b"NM:i3:",), (b"N",)]
    add("TAG_ texts the host refuses or reads with strtoll / strtof", "tags", "declining", each_pair(2 * len(bad_tags), lambda i, k: dict(tags=bad_tags[i // 2]) if k == 1 + i % 2 else {}))
    # the `proper` rule, branch by branch, on a text that keeps every pair
    add("the gate's score", "proper", "plain", clean, "gate", seed=30, expect="nothing")
    add("max1 / max2 == -1", "proper", "plain", clean, "m1", seed=31, expect="written")
    for cg, expect in ((b"24S26M", "nothing"), (b"25S25M", "written"), (b"12H26M12S", "nothing"), (b"12S25M13H", "written"), (b"24H", "written"), (b"*", "written"), (b"", "written"), (b"26M", "nothing"), (b"30I20M", "nothing")):
        add("max1 / max2 == -2, CIGAR %s" % cg.decode(), "proper", "plain", each_pair(6, lambda i, k: dict(cigar=cg if k == 1 + i % 2 else b"50M")), "m2", seed=32, expect=expect)
    add("candidate I sum 24", "proper", "plain", clean, "i24", seed=33, expect="nothing")
    add("candidate I sum 25", "proper", "plain", clean, "i25", seed=34, expect="written")
    add("candidate n_cigar 0", "proper", "plain", clean, "ncig0", seed=35, expect="written")
    add("mixed results", "proper", "plain", clean, "mixed", seed=36)
    add("MS:i of every integer type", "proper", "plain", clean, "kept", seed=37, expect="written", mfs=70000)
    add("index_edge", "index", "plain", clean, "index_edge", seed=38)
    add("index_bad", "index", "declining", clean, "index_bad", seed=39)
    return C
