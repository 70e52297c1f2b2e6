"""What the tests of `panSVR signal -N --signal-device` share: the two stand-alone checkers (tests/tools/signal_device_check.cpp: the rules of
signal_device.h against SignalStep::pair; tests/tools/signal_device_route_check.cpp: the route over a host-memory backend), crafted records for
every rule edge on top of test_signal's make_pairs, and the base-code count the declined pairs are held to."""
import os
import struct
import subprocess
import tempfile

import numpy as np

import test_signal as ts

ROOT = ts.ROOT
CLI = ts.CLI
FLAG_SETS = [([], 20240), (["-D"], 20241), (["-U"], 20241), (["-D", "-U", "-I", "22"], 20244)]      # test_signal's REF_CASES
REFS = [("chr%d" % (i + 1), 50000000) for i in range(30)]
GOOD_CODES = (1, 2, 4, 8, 15)


def build(src, tmp, sanitize):
    exe = os.path.join(tmp, src + ("_asan" if sanitize else ""))
    flags = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"] if sanitize else ["-O2"]
    subprocess.check_call(["g++"] + flags + ["-std=c++17", "-Wall", "-Wno-unused-function", "-o", exe, os.path.join(ROOT, "tests", "tools", src + ".cpp"), "-lz", "-lpthread"])
    return exe


def run_rules(exe, bam, flags, dump=None):
    """(exit status, summary dict, stderr) of signal_device_check; dump: a prefix for the .tab and .fq files"""
    r = subprocess.run([exe, bam] + flags + (["--dump", dump] if dump else []), stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600)
    w = r.stdout.split()
    s = {w[i].decode(): (int(w[i + 1]) if w[i] != b"fnv" else w[i + 1].decode()) for i in range(0, len(w) - 1, 2)}
    return r.returncode, s, r.stderr.decode()


def read_tab(prefix):
    """[(state, note, bytes, rec1, rec2)] of a dump"""
    return [tuple(int(x) for x in l.split()) for l in open(prefix + ".tab")]


def has_bad_base(rec):
    """does the record (block_size first) hold a base code outside {1, 2, 4, 8, 15}?"""
    l_name, n_cig, l_seq = rec[12], struct.unpack_from("<H", rec, 16)[0], struct.unpack_from("<i", rec, 20)[0]
    s4 = rec[36 + l_name + 4 * n_cig:36 + l_name + 4 * n_cig + (l_seq + 1) // 2]
    return any(((s4[i >> 1] >> (0 if i & 1 else 4)) & 15) not in GOOD_CODES for i in range(l_seq))


def with_raw_aux(rec, raw):
    """the record with `raw` appended to its optional fields"""
    body = rec[4:] + raw
    return struct.pack("<i", len(body)) + body


def q(n, v=50):
    return [v] * n


def seq(n, rng):
    return "".join("ACGT"[x] for x in rng.randint(0, 4, n))


def good_pair(name, rng, L=100, **kw):
    """a pair the filter passes: both mapped with mapq 60 on one chromosome, F/R, 300 apart, no clip, NM 0, high qualities; kw overrides per read
    (keys ending in 1 or 2: flag, tid, pos, mapq, cigar, mtid, mpos, isize, seq, qual, tags)"""
    d = dict(flag1=0x61, flag2=0x91, tid1=0, tid2=0, pos1=10000, pos2=10200, mapq1=60, mapq2=60, cigar1=[(L, "M")], cigar2=[(L, "M")], isize1=300, isize2=-300,
             seq1=seq(L, rng), seq2=seq(L, rng), qual1=q(L), qual2=q(L), tags1=[("NM", "C", 0)], tags2=[("NM", "C", 0)])
    d.update(kw)
    d.setdefault("mtid1", d["tid2"]), d.setdefault("mpos1", d["pos2"]), d.setdefault("mtid2", d["tid1"]), d.setdefault("mpos2", d["pos1"])
    return [ts.record(name, d["flag%d" % k], d["tid%d" % k], d["pos%d" % k], d["mapq%d" % k], d["cigar%d" % k], d["mtid%d" % k], d["mpos%d" % k], d["isize%d" % k], d["seq%d" % k],
                      d["qual%d" % k], d["tags%d" % k]) for k in (1, 2)]


def crafted():
    """[(name, [rec1, rec2], state without flags or None)]: one pair per rule edge, none in an error state"""
    rng = np.random.RandomState(99)
    out = []

    def add(name, pair, state=None):
        out.append((name, pair, state))

    add("good", good_pair("good", rng), 0)
    # each reason bit alone
    add("bit1", good_pair("bit1", rng, mapq1=5, mapq2=9), 1)
    add("bit2", good_pair("bit2", rng, flag2=0x95, cigar2=[], mapq2=0, tags2=[]), 1)
    add("bit4", good_pair("bit4", rng, isize1=1500, isize2=-1500), 1)
    add("bit8", good_pair("bit8", rng, flag2=0x81), 1)
    add("bit16", good_pair("bit16", rng, tags1=[("NM", "C", 8)], tags2=[("NM", "C", 8)]), 1)
    add("bit32", good_pair("bit32", rng, cigar1=[(6, "S"), (94, "M")], cigar2=[(94, "M"), (6, "S")]), 1)
    add("bit64", good_pair("bit64", rng, tid1=25, tid2=25), 1)
    add("bit64b", good_pair("bit64b", rng, tid2=3), 1)
    # CIGAR shapes
    add("nocigar", good_pair("nocigar", rng, cigar1=[], cigar2=[]))
    add("oneS", good_pair("oneS", rng, cigar1=[(100, "S")]), 1)
    add("oneH", good_pair("oneH", rng, cigar2=[(100, "H")]), 1)
    add("ops", good_pair("ops", rng, cigar1=[(3, "H"), (20, "="), (2, "X"), (5, "N"), (1, "P"), (30, "M"), (4, "I"), (40, "M"), (2, "D"), (4, "S")]))
    # NM in each code, absent, as a float; XA; tags in every order
    for t, v in (("c", -3), ("C", 200), ("s", -300), ("S", 60000), ("i", -70000), ("I", 70000)):
        add("nm_" + t, good_pair("nm_" + t, rng, tags1=[("AS", "i", 5), ("NM", t, v)], mapq1=3, mapq2=3))
    add("nm_none", good_pair("nm_none", rng, tags1=[], tags2=[("XX", "A", b"x")], mapq1=3, mapq2=3), 1)
    add("nm_f", good_pair("nm_f", rng, tags1=[("NM", "f", 3.0)], mapq1=3, mapq2=3), 1)
    add("xa_none", good_pair("xa_none", rng, mapq1=0, mapq2=0), 1)
    add("xa_some", good_pair("xa_some", rng, mapq1=0, mapq2=0, tags1=[("XA", "Z", "chr2,+5,100M,1;chr3,-9,100M,2;"), ("NM", "C", 1)],
                             tags2=[("SA", "Z", "chr3,7,-,60S40M,60,0;"), ("MC", "Z", "100M"), ("XA", "Z", ""), ("NM", "s", 2)]), 1)
    add("xa_notZ", good_pair("xa_notZ", rng, mapq1=0, mapq2=0, tags1=[("XA", "i", 5)]), 1)
    # the walk's size rules: an unknown type in front of NM, a Z tag without NUL at the record's end, B arrays
    p = good_pair("aux_unknown", rng, mapq1=3, mapq2=3, tags1=[], tags2=[])
    add("aux_unknown", [with_raw_aux(p[0], b"ZZ?\x01\x02NMC\x07"), with_raw_aux(p[1], b"NMC\x07ZZ?\x01")], 1)
    p = good_pair("aux_open_z", rng, mapq1=3, mapq2=3, tags1=[("NM", "C", 4)], tags2=[])
    add("aux_open_z", [with_raw_aux(p[0], b"XAZchr2,1;"), with_raw_aux(p[1], b"SAZopen")], 1)
    p = good_pair("aux_b", rng, mapq1=3, mapq2=3, tags1=[], tags2=[])
    add("aux_b", [with_raw_aux(p[0], b"BBBs" + struct.pack("<I", 3) + bytes(6) + b"NMC\x05"), with_raw_aux(p[1], b"BBBi" + struct.pack("<I", 1 << 30) + b"NMC\x05")], 1)
    p = good_pair("aux_short", rng, mapq1=3, mapq2=3, tags1=[], tags2=[])
    add("aux_short", [with_raw_aux(p[0], b"NM"), with_raw_aux(p[1], b"NMi\x01\x02")], 1)
    # lengths, both strands (read 1 below 2048; 2048 as read 2)
    for L1, L2 in ((0, 0), (1, 2), (2, 1), (35, 36), (36, 35), (2047, 2048), (101, 100)):
        for rev in (False, True):
            n = "len%d_%d%s" % (L1, L2, "r" if rev else "f")
            add(n, good_pair(n, rng, flag1=0x51 if rev else 0x61, flag2=0xa1 if rev else 0x91, mapq1=3, mapq2=3, cigar1=[(L1, "M")] if L1 else [], cigar2=[(L2, "M")] if L2 else [],
                             seq1=seq(L1, rng), seq2=seq(L2, rng), qual1=list(rng.randint(2, 60, L1)), qual2=list(rng.randint(2, 60, L2))), 1)
    # negative fields
    add("neg", good_pair("neg", rng, pos1=-5, mtid1=-1, mpos1=-1, isize1=-300, isize2=300, tid2=-1, pos2=-1), 1)
    # isize == l_qseq for both reads, R/F and F/R; pos order swapped
    add("isz_rf", good_pair("isz_rf", rng, flag1=0x51, flag2=0xa1, isize1=100, isize2=-100, pos1=10000, pos2=10000))
    add("isz_fr", good_pair("isz_fr", rng, isize1=100, isize2=-100, pos1=10000, pos2=10000))
    add("posswap", good_pair("posswap", rng, pos1=10200, pos2=10000, flag1=0x51, flag2=0xa1, isize1=-300, isize2=300), 0)
    # low qualities above and below the clip
    add("lowq_lt", good_pair("lowq_lt", rng, cigar1=[(12, "S"), (88, "M")], qual1=q(1, 3) + q(99)), 1)
    add("lowq_gt", good_pair("lowq_gt", rng, cigar1=[(12, "S"), (88, "M")], qual1=q(40, 3) + q(60), tags1=[("NM", "C", 9)]), 0)
    # both unmapped; wrong ISIZE
    add("unm", [ts.record("unm", 0x4d, -1, -1, 0, [], -1, -1, 0, seq(50, rng), q(50), []), ts.record("unm", 0x8d, -1, -1, 0, [], -1, -1, 0, seq(50, rng), q(50), [])], 1)
    add("isize_note", good_pair("isize_note", rng, isize1=300, isize2=-250, mapq1=3, mapq2=3), 1)
    # a base code without a letter; a secondary record between the mates
    add("badbase", good_pair("badbase", rng, mapq1=3, mapq2=3, seq2="AC=GT" + seq(95, rng)), 2)
    p = good_pair("between", rng, mapq1=3, mapq2=3)
    add("between", [p[0], ts.record("between", 0x181, 0, 5, 0, [(40, "M")], 0, 5, 0, seq(40, rng), q(40), []), ts.record("other", 0x841, 0, 5, 0, [(40, "M")], 0, 5, 0, seq(40, rng), q(40), []), p[1]], 1)
    return out


def error_pairs():
    """{state: [rec1, rec2]}"""
    rng = np.random.RandomState(7)
    a = good_pair("left", rng, mapq1=3, mapq2=3)
    b = good_pair("right", rng, mapq1=3, mapq2=3)
    return {3: [a[0], b[1]],
            4: good_pair("tmpl", rng, mapq1=3, mapq2=3, flag1=0x21),
            5: good_pair("long", rng, mapq1=3, mapq2=3, cigar1=[(2048, "M")], seq1=seq(2048, rng), qual1=q(2048), isize1=300, isize2=-250)}


def write_bam(path, recs):
    ts.write_bam(path, recs, REFS)


def tmpdir(tag):
    return tempfile.mkdtemp(prefix="psvr_" + tag + "_")


def bam_file(recs, refs=REFS):
    """(the file's bytes, the inflated bytes its header takes) of ts.write_bam's file"""
    d = tmpdir("bam")
    ts.write_bam(os.path.join(d, "x.bam"), recs, refs)
    text = "@HD\tVN:1.6\tSO:queryname\n" + "".join("@SQ\tSN:%s\tLN:%d\n" % r for r in refs)
    return open(os.path.join(d, "x.bam"), "rb").read(), 12 + len(text) + sum(8 + len(n) + 1 for n, _ in refs)


def opt_of(summary, flags):
    """the psvr_signal_opt_t the rules checker ran with (pansvr_amd.signal_step.SignalOpt)"""
    from pansvr_amd import signal_step as ss
    return ss.signal_opt([summary["stat%d" % k] for k in range(4)], summary["isize_min"], summary["isize_max"], not_use_filter="-D" in flags, discard_full_match="-U" in flags,
                         max_tid=int(flags[flags.index("-I") + 1]) if "-I" in flags else 24)


def opt_arg(summary):
    return "%d,%d,%d,%d,%d,%d" % tuple([summary["isize_min"], summary["isize_max"]] + [summary["stat%d" % k] for k in range(4)])
