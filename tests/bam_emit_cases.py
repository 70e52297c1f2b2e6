"""Inputs and helpers for the tests of the BAM record encoder's device route (tests/test_bam_emit_device.py on the host build of
pansvr_amd/csrc/bam_emit_device.h, tests/test_bam_emit_gpu.py through psvr_bam_emit_*).  The yardstick is SamEmitter::main_pair
(sam_emit.h), which tests/tools/bam_emit_device_check.cpp runs on the same text and the same generated results."""
import os
import random
import subprocess
import tempfile

import numpy as np

import fastq_cases as fc

HERE = os.path.dirname(os.path.abspath(__file__))
CHECK_SRC = os.path.join(HERE, "tools", "bam_emit_device_check.cpp")
CLI = fc.CLI
N_HEADER = 30
LENGTHS = (0, 1, 2, 15, 16, 17, 31, 32, 33, 150)
HDR_BYTES, PAIR_BYTES, CAND_BYTES = 48, 24, 48
# families in which both a plain and a declining class (or text) exist: both states must occur in each
TWO_SIDED = ("name", "comment", "qual", "cigar", "sv", "index")


def build_checker(tmp, sanitize):
    exe = os.path.join(tmp, "bam_emit_device_check_asan" if sanitize else "bam_emit_device_check")
    flags = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"] if sanitize else ["-O2"]
    subprocess.check_call(["g++"] + flags + ["-std=c++17", "-Wall", "-o", exe, CHECK_SRC, "-lz", "-lpthread"])
    return exe


def run_checker(exe, text, cls, seed, flags=0, n_header=N_HEADER, anchors=None, timeout=300):
    """(summary dict, out file bytes) of one case; a mismatch with main_pair or a sanitizer's report fails the call.  anchors: None for
    the checker's own table, or [(print_string, vcf_id)] as bytes."""
    tmp = tempfile.mkdtemp(prefix="psvr_bec_")
    with open(os.path.join(tmp, "in.fq"), "wb") as f:
        f.write(text)
    apath = "-"
    if anchors is not None:
        apath = os.path.join(tmp, "anchors.txt")
        with open(apath, "wb") as f:
            f.write(b"".join(a + b"\t" + b + b"\n" for a, b in anchors))
    r = subprocess.run([exe, "run", os.path.join(tmp, "in.fq"), cls, str(seed), str(flags), str(n_header), apath, os.path.join(tmp, "out")], stdout=subprocess.PIPE,
                       stderr=subprocess.PIPE, timeout=timeout)
    assert r.returncode == 0 and not r.stderr, "bam_emit_device_check (%s): exit status %d\n%s\n%s" % (cls, r.returncode, r.stdout.decode(), r.stderr.decode()[-4000:])
    w = r.stdout.split()
    assert w[0] == b"class" and w[1].decode() == cls
    summary = {"label": w[2].decode()}
    summary.update({w[i].decode(): int(w[i + 1]) for i in range(3, len(w), 2)})
    return summary, open(os.path.join(tmp, "out"), "rb").read()


def split_out(raw):
    """The checker's out file: the generated results (raw bytes of each array) and what the encoder must give back."""
    head = [int(x) for x in np.frombuffer(raw, dtype=np.int64, count=8)]
    P, nc, nw, nb = head[:4]
    o = 64
    out = {"P": P, "n_cands": nc, "n_cigar": nw, "n_bytes": nb, "n_records": head[4], "n_written": head[5], "n_declined": head[6], "n_anchor": head[7]}
    for key, size in (("hdr", 2 * P * HDR_BYTES), ("pairs", P * PAIR_BYTES), ("cands", nc * CAND_BYTES), ("cigar", nw * 4), ("state", P), ("pair_off", (P + 1) * 8), ("bytes", nb)):
        out[key] = raw[o:o + size]
        o += size
    assert o == len(raw)
    return out


def comment(rng, chr_id=None, ref_bg=None, flag=None, tail=b"_STAT_150_200_400_600"):
    """chr_refbg_readbg_score_mapq + four tokens + the flag token (parse_ori_mapping_rst), with the values the ORI branch must survive"""
    chr_id = rng.choice([-1, 0, 3, N_HEADER - 1, N_HEADER, 7]) if chr_id is None else chr_id
    ref_bg = rng.choice([0, 1, 100000, 0x7ffffffe, 0x7fffffff, 0xffffffff, 5000]) if ref_bg is None else ref_bg
    score = rng.choice([-32769, -32768, -129, -128, -1, 0, 255, 256, 65535, 65536, 300])
    return b"%d_%d_%d_%d_%d_a_b_c_d_%s" % (chr_id, ref_bg, rng.choice([0, 0, 5, 32768, 70000]), score, rng.choice([0, 60, 255]), flag or rng.choice([b"FN", b"RY", b"FY", b"RN"])) + tail


def crafted(n_pairs, seed, lengths=LENGTHS, alphabet=b"ACGTN", eol=b"\n", **kw):
    """n_pairs pairs of reads whose lengths cycle through `lengths`, with comments of every ORI kind"""
    rng = random.Random(seed)
    out = []
    for i in range(n_pairs):
        for k in (1, 2):
            n = lengths[(i + (k - 1) * 3) % len(lengths)]
            seq = bytes(rng.choice(alphabet) for _ in range(n))
            qual = bytes(33 + rng.randrange(60) for _ in range(n))
            out.append(fc.read(name=b"r%d/%d" % (i, k), comment=comment(rng), seq=seq, qual=qual, eol=eol, **kw))
    return b"".join(out)


def clean(n_pairs, seed):
    """pairs every read of which is written when its results say so: names, comments and lines the direct path takes"""
    rng = random.Random(seed)
    return b"".join(fc.read(name=b"c%d/%d" % (i, k), comment=comment(rng, chr_id=3, ref_bg=1000 + i), seq=b"ACGTTGCAAN" * 5, qual=b"IIIIIHHHH#" * 5) for i in range(n_pairs) for k in (1, 2))


def each_pair(n_pairs, make):
    """make(i, k) -> the FASTQ text of read k of pair i"""
    return b"".join(make(i, k) for i in range(n_pairs) for k in (1, 2))


def cases(golden=True):
    """[dict(name, family, label, text, cls, seed, flags)]: label 'plain' (no pair may be declined) or 'declining' (every pair must be)"""
    C = []

    def add(name, family, label, text, cls, seed=1, flags=0):
        C.append(dict(name=name, family=family, label=label, text=text, cls=cls, seed=seed, flags=flags))

    if golden:
        for i, (name, text) in enumerate(fc.golden_fastqs()):
            add("golden " + name, "golden", "plain", text, "mixed", seed=100 + i)
        add("golden fx1/reads150, every read written", "golden", "plain", fc.golden_fastqs()[0][1], "written", seed=99)
    rng = random.Random(7)
    c = lambda: comment(rng, chr_id=3, ref_bg=777)
    # SEQ / QUAL: every length around the group's width, both strands (the candidates' and the original alignments' directions are drawn)
    add("lengths, written", "seq", "plain", crafted(120, 1), "written")
    add("lengths, mixed", "seq", "plain", crafted(200, 2), "mixed", seed=2)
    add("lower case and IUPAC", "seq", "plain", crafted(60, 3, alphabet=b"ACGTNacgtnRYKMSWBDHVrykmswbdhv=.*0123U"), "written", seed=3)
    add("arbitrary bytes", "seq", "plain", crafted(60, 4, alphabet=bytes(b for b in range(256) if b not in (10, 13))), "written", seed=4)
    add("crlf line ends", "seq", "plain", crafted(40, 5, eol=b"\r\n"), "written", seed=5)
    add("original alignments of every kind", "ori", "plain", crafted(300, 6), "mixed", seed=6)
    add("not_ori", "ori", "plain", crafted(300, 6), "mixed", seed=6, flags=1)
    # names
    add("names of 1 and 254 bytes", "name", "plain", each_pair(12, lambda i, k: fc.read(name=b"n" * (1 if (i + k) % 2 else 254), comment=c())), "written")
    add("names of 0 bytes", "name", "declining", each_pair(8, lambda i, k: fc.read(name=b"" if k == 1 + i % 2 else b"ok", comment=c())), "written")
    add("names of 255 bytes", "name", "declining", each_pair(8, lambda i, k: fc.read(name=b"n" * (255 if k == 1 + i % 2 else 254), comment=c())), "written")
    # comments
    forms = [b"", None, b"3_1000_0", b"_3__1000_0_280_60_a__b_c_d_FY_x", b"3_1000_0_280_60_a_b_c_d_FY_", b"3_1000_0_280_60_a_b_c_d_", b"_____", b"3_1000_0_280_60_a_b_c_d_e_f_g_h_i_j_k_FY_x_y", b"x", b"_",
             b"3_1000_0_280_60_a_b_c_d_FN_0123456789abcdef_", b"3_1000_0_280_6_a_b_c_d_FN_0123456789abcde_"]
    add("comment forms", "comment", "plain", each_pair(2 * len(forms), lambda i, k: fc.read(name=b"f%d" % i, comment=forms[(i + k) % len(forms)])), "written")
    add("comment forms, crlf", "comment", "plain", each_pair(2 * len(forms), lambda i, k: fc.read(name=b"f%d" % i, comment=forms[(i + k) % len(forms)], eol=b"\r\n")), "written")
    add("a tab in the comment", "comment", "declining", each_pair(40, lambda i, k: fc.read(name=b"t%d" % i, comment=(c()[:i] + b"\t" + c()[i:]) if k == 1 + i % 2 else c())), "written")
    add("a NUL in the comment", "comment", "declining", each_pair(40, lambda i, k: fc.read(name=b"z%d" % i, comment=(c()[:i] + b"\0" + c()[i:]) if k == 1 + i % 2 else c())), "written")
    # QUAL against SEQ
    add("quality line shorter", "qual", "declining", each_pair(8, lambda i, k: fc.read(name=b"q%d" % i, comment=c(), seq=b"ACGT" * 5, qual=b"I" * (19 if k == 1 + i % 2 else 20))), "written")
    add("quality line longer", "qual", "declining", each_pair(8, lambda i, k: fc.read(name=b"q%d" % i, comment=c(), seq=b"ACGT" * 5, qual=b"I" * (21 if k == 1 + i % 2 else 20))), "written")
    add("quality line as long", "qual", "plain", each_pair(8, lambda i, k: fc.read(name=b"q%d" % i, comment=c(), seq=b"ACGT" * 5, qual=b"I" * 20)), "written")
    # the results' classes on a text that declines nothing
    text = clean(200, 8)
    add("tag integers", "ints", "plain", text, "ints", seed=8)
    add("cigar_ok", "cigar", "plain", text, "cigar_ok", seed=9)
    add("cigar_bad", "cigar", "declining", text, "cigar_bad", seed=10)
    add("sv_ok", "sv", "plain", text, "sv_ok", seed=11)
    add("sv_bad", "sv", "declining", text, "sv_bad", seed=12)
    add("index_edge", "index", "plain", text, "index_edge", seed=13)
    add("index_bad", "index", "declining", text, "index_bad", seed=14)
    # pair counts on both sides of a workgroup (16 pairs), of a scan tile (2048 counts) and of the command's chunk
    for n in (1, 15, 16, 17, 255, 256, 257, 2047, 2048, 4097):
        add("%d pairs" % n, "counts", "plain", crafted(n, 20 + n, lengths=(33, 16, 150, 1)), "mixed", seed=20 + n)
    return C
