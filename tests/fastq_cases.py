"""Inputs and helpers for the tests of the FASTQ parser's device route (tests/test_fastq_parse.py on the host build of
pansvr_amd/csrc/fastq_device.h, tests/test_fastq_gpu.py through psvr_fastq_parse).  The yardstick is the host parser of fastq_batch.h,
which tests/fastq_check.cpp runs on the same bytes and limits."""
import os
import subprocess
import tempfile

import numpy as np

import aln_common as ac
import datasets

HERE = os.path.dirname(os.path.abspath(__file__))
CHECK_SRC = os.path.join(HERE, "fastq_check.cpp")
CLI = os.path.join(ac.ROOT, "pansvr_amd", "bin", "panSVR")
BIG_PAIRS, BIG_BASES = 1 << 20, 1 << 40
ORI_BYTES = 20
COMMENT = b"3_1000_0_280_60_a_b_c_d_FN_rest"          # eleven tokens; the tenth is the flag token


def build_checker(tmp, sanitize):
    exe = os.path.join(tmp, "fastq_check_asan" if sanitize else "fastq_check")
    flags = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"] if sanitize else ["-O2"]
    subprocess.check_call(["g++"] + flags + ["-std=c++17", "-Wall", "-o", exe, CHECK_SRC, "-lz", "-lpthread"])
    return exe


def constants(exe):
    w = subprocess.run([exe, "constants"], stdout=subprocess.PIPE, check=True).stdout.split()
    return {w[i].decode(): int(w[i + 1]) for i in range(0, len(w), 2)}


def run_checker(exe, text, at_end, max_pairs, max_bases, timeout=600):
    """The checker's out file for one case (bytes); a mismatch with fastq_batch.h or a sanitizer's report fails the call."""
    tmp = tempfile.mkdtemp(prefix="psvr_fqc_")
    with open(os.path.join(tmp, "in"), "wb") as f:
        f.write(text)
    r = subprocess.run([exe, "parse", os.path.join(tmp, "in"), str(int(at_end)), str(max_pairs), str(max_bases), os.path.join(tmp, "out")], stdout=subprocess.PIPE,
                       stderr=subprocess.PIPE, timeout=timeout)
    assert r.returncode == 0 and not r.stderr, "fastq_check: exit status %d\n%s" % (r.returncode, r.stderr.decode()[-4000:])
    return open(os.path.join(tmp, "out"), "rb").read()


def split_out(raw):
    """The checker's out file as the dict FastqParser.download() returns (ori and bases as raw bytes) plus 'info'."""
    head = np.frombuffer(raw, dtype=np.int64, count=5)
    P, total = int(head[0]), int(head[2])
    o = 40
    out = {"info": [int(x) for x in head]}
    for key, dt, cnt in (("line_start", np.uint64, 8 * P + 1), ("name_end", np.uint16, 2 * P), ("base_off", np.int64, 2 * P + 1), ("ori", np.uint8, 2 * P * ORI_BYTES),
                         ("bases", np.uint8, total + 1)):
        out[key] = np.frombuffer(raw, dtype=dt, count=cnt, offset=o)
        o += out[key].nbytes
    assert o == len(raw)
    return out


def read(name=b"r", comment=COMMENT, seq=b"ACGTACGTAC", qual=None, eol=b"\n", sep=b" ", header=None):
    if header is None:
        header = b"@" + name + (sep + comment if comment is not None else b"")
    return header + eol + seq + eol + b"+" + eol + (qual if qual is not None else b"I" * len(seq)) + eol


def pairs(n, **kw):
    return b"".join(read(name=b"p%d/%d" % (i, k), **kw) for i in range(n) for k in (1, 2))


def sixteen_pairs():
    """The text of the cutting case: sixteen pairs with lengths that differ, longer than a tile of the newline pass."""
    return b"".join(read(name=b"cut%d/%d" % (i, k), seq=b"ACGTN"[:1 + (i + k) % 5] * (8 + i), comment=COMMENT + b"_%d" % i) for i in range(16) for k in (1, 2))


def golden_fastqs():
    out = []
    for name in ("fx1", "fx2", "fx3", "fx4", "fx5"):
        w = ac.workdir(name)
        for rname in datasets.DATASETS[name]["reads"]:
            out.append(("%s/%s" % (name, rname), open(os.path.join(w, rname + ".fq"), "rb").read()))
    # the fused set's FASTQ: what `panSVR signal -N -D` writes for the BAM of tests/test_fused_signal.py
    import test_fused_signal as tfs
    tmp = tempfile.mkdtemp(prefix="psvr_fqc_")
    bam = os.path.join(tmp, "in.bam")
    tfs.bam_of("fx1", "reads150", 2000, bam)
    r = subprocess.run([CLI, "signal", "-N", "-D", "-H", os.path.join(tmp, "h.sam"), "-S", os.path.join(tmp, "s.txt"), bam], stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    assert r.returncode == 0 and len(r.stdout) > 100000, r.stderr.decode()[-1000:]
    out.append(("fused/fx1_reads150", r.stdout))
    return out


def cases(T):
    """[(name, text, at_end, max_pairs, max_bases)]; T = bytes per tile of the newline pass (the checker prints it)."""
    C = []

    def add(name, text, at_end=1, max_pairs=BIG_PAIRS, max_bases=BIG_BASES):
        C.append((name, text, at_end, max_pairs, max_bases))

    for name, text in golden_fastqs():
        add(name, text)
    three = pairs(3)
    # line endings
    add("crlf", pairs(3, eol=b"\r\n"))
    add("cr cr lf", pairs(3, eol=b"\r\r\n"))
    add("no final newline, at_end", three[:-1], 1)
    add("no final newline, not at_end", three[:-1], 0)
    # line counts
    add("empty", b"")
    add("empty, not at_end", b"", 0)
    add("seven lines", pairs(1)[:-1].rsplit(b"\n", 1)[0] + b"\n")
    for k in range(1, 8):
        add("8k+%d lines" % k, pairs(2) + b"".join(b"x%d\n" % j for j in range(k)))
    # header forms
    add("empty header", read(header=b"") + read() + pairs(1))
    add("header is only @", read(header=b"@") + read() + pairs(1))
    add("no comment", read(comment=None) + read(comment=None))
    add("tab for the space", pairs(2, sep=b"\t"))
    add("space inside the comment", pairs(1, comment=b"3_1000 7_0_280_60_a_b_c_d_FY_x y"))
    add("space as the first byte", read(header=b" 5_6_7_8_9") + read(header=b"  5_6_7_8_9"))
    # token forms
    add("leading _", pairs(1, comment=b"_" + COMMENT))
    add("__ runs", pairs(1, comment=b"__3__1000___0_280_60_a__b_c_d____FY__"))
    add("nine tokens", pairs(1, comment=b"3_1000_0_280_60_a_b_c_FY"))
    add("ten tokens", pairs(1, comment=b"3_1000_0_280_60_a_b_c_d_FY"))
    add("eleven tokens", pairs(1, comment=b"3_1000_0_280_60_a_b_c_d_e_FY"))
    add("comment ends in _", pairs(1, comment=b"3_1000_0_280_60_a_b_c_d_FY_"))
    add("nine tokens and _", pairs(1, comment=b"3_1000_0_280_60_a_b_c_d_"))
    add("only underscores", pairs(1, comment=b"_____"))
    add("empty comment", pairs(1, comment=b""))
    # number tokens
    add("signs", pairs(1, comment=b"-1_+17_-0_+-3_--4_a_b_c_d_FN"))
    add("leading blanks", pairs(1, comment=b" 12_\t13_\v\f\r14_  -15_ \t16_a_b_c_d_RN"))
    add("trailing letter", pairs(1, comment=b"12x_13M5_1e3_0x10_60q_a_b_c_d_FN"))
    add("wrapping", pairs(1, comment=b"4294967297_4294967296_99999999999999999999_2147483648_300_a_b_c_d_FN"))
    add("mapq 300", pairs(1, comment=b"1_2_3_4_300_a_b_c_d_FN"))
    add("mapq -1", pairs(1, comment=b"1_2_3_4_-1_a_b_c_d_FN"))
    # flag tokens
    for flag in (b"F", b"FY", b"RN", b"R", b"Y", b"YF", b"FYY"):
        add("flag " + flag.decode(), pairs(1, comment=b"1_2_3_4_5_a_b_c_d_" + flag) + pairs(1, comment=b"1_2_3_4_5_a_b_c_d_" + flag + b"_more"))
    add("empty flag token", pairs(1, comment=b"1_2_3_4_5_a_b_c_d__"))
    # sizes
    add("name of 70000 bytes", read(name=b"n" * 70000) + read(name=b"m" * 65535) + read(name=b"k" * 65534) + read(name=b"j" * 65536))
    add("comment of 5000 bytes", pairs(1, comment=COMMENT + b"_XA:Z:" + b"chr1,+100,150M,0;" * 290))
    add("comment of 5000 bytes, few tokens", pairs(1, comment=b"7_8_" + b"x" * 5000))
    add("1600-base read", read(seq=b"ACGTTGCAAN" * 160) + read(seq=b"A" * 1599) + pairs(1))
    add("empty sequence line", read(seq=b"") + read() + read() + read(seq=b""))
    add("all sequences empty", pairs(2, seq=b""))
    # limits
    six = pairs(6)                                        # twenty bases a pair
    add("max_pairs smaller than the text", six, 1, 3)
    add("max_pairs 1", six, 1, 1)
    add("max_pairs 0", six, 1, 0)
    add("max_pairs exactly the text", six, 1, 6)
    for mb in (59, 60, 61, 1, 0, 120, 121, 119):
        add("max_bases %d" % mb, six, 1, BIG_PAIRS, mb)
    add("both limits", six, 1, 4, 61)
    add("limits, no final newline, not at_end", six[:-1], 0, 6, 200)
    # tile boundaries of the newline pass
    for tag, at in (("last byte of a tile", T - 1), ("first byte of a tile", T)):
        hdr_len = len(b"@t1 " + COMMENT)
        add("newline as the " + tag, read(name=b"t1" + b"x" * (at - hdr_len)) + read() + pairs(2))
    add("line spanning three tiles", pairs(1) + read(name=b"s" * (2 * T + 100)) + read() + pairs(1))
    add("sequence line spanning three tiles", pairs(1) + read(seq=b"ACGT" * (T // 2 + 40)) + read() + pairs(1))
    long_text = pairs(T // 50)
    assert len(long_text) > T + 16
    for n in (T - 1, T, T + 1):
        add("text of %d bytes" % n, long_text[:n], 1)
        add("text of %d bytes, not at_end" % n, long_text[:n], 0)
    tiny = b"@r x\nAC\n+\nII\n@s\n"
    for n in range(1, 16):
        add("text of %d bytes" % n, tiny[:n], 1)
        add("text of %d bytes, not at_end" % n, tiny[:n], 0)
    add("newlines only", b"\n" * 37)
    add("sixteen pairs", sixteen_pairs())
    return C
