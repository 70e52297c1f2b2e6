"""Inputs and helpers for the tests of the wavefront-per-member BGZF encoder (tests/test_deflate_wave.py on the host build of
pansvr_amd/csrc/deflate_wave_device.h, tests/test_deflate_wave_gpu.py through psvr_bgzf_compress_members).  zlib is the judge: a member
counts when inflate_cases.oracle() accepts it (header rules, raw inflate to the end of the stream, ISIZE, CRC32)."""
import os
import random
import subprocess
import tempfile

import aln_common as ac
import inflate_cases as ic

HERE = os.path.dirname(os.path.abspath(__file__))
CHECK_SRC = os.path.join(HERE, "tools", "deflate_wave_check.cpp")
EMU = os.path.join(HERE, "emu", "emu_aln")
MEMBER_SIZES = (256, 4096, 0x4000, 0xff00)


def build_checker(tmp, sanitize):
    exe = os.path.join(tmp, "deflate_wave_check_asan" if sanitize else "deflate_wave_check")
    flags = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"] if sanitize else ["-O2"]
    subprocess.check_call(["g++"] + flags + ["-std=c++17", "-Wall", "-o", exe, CHECK_SRC])
    return exe


def host_members(exe, data, member_bytes, timeout=900):
    """The bytes the encoder's host build writes for `data`; the sanitizer's report, if any, fails the call."""
    tmp = tempfile.mkdtemp(prefix="psvr_dfw_")
    with open(os.path.join(tmp, "in"), "wb") as f:
        f.write(data)
    r = subprocess.run([exe, str(member_bytes), os.path.join(tmp, "in"), os.path.join(tmp, "out")], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=timeout)
    assert r.returncode == 0 and not r.stderr, "deflate_wave_check: exit status %d\n%s" % (r.returncode, r.stderr.decode()[-4000:])
    return open(os.path.join(tmp, "out"), "rb").read()


def fx2_records():
    """The BAM records of golden set fx2, made the way tests/test_deflate.py makes records.bam."""
    subprocess.check_call(["make", "-s", "-C", os.path.join(HERE, "emu")])
    w = ac.workdir("fx2")
    tmp = tempfile.mkdtemp(prefix="psvr_dfw_")
    rec = os.path.join(tmp, "records.bam")
    r = subprocess.run([EMU, ac.index_dir("fx2"), os.path.join(w, "reads150.fq"), os.path.join(w, "header.sam"), "--no-records", "--sam", os.path.join(tmp, "o.sam"),
                        "--ori-sam", os.path.join(tmp, "p.sam"), "--bam-records", rec], stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    assert r.returncode == 0, r.stderr.decode()[-1000:]
    return open(rec, "rb").read()


def cases(member_bytes, records):
    """[(name, data)] for one member size."""
    r = random.Random(5)
    block = bytes(r.getrandbits(8) for _ in range(32768))
    # four bits a byte, so that a match shows in the size; the first 300 bytes from an alphabet of their own, so that the table's one entry
    # per hash still points at them 32768 bytes later
    few = bytes(r.choice(b"ACGTNacgtn012345") for _ in range(32768 + 340))
    far = bytes(r.choice(range(128, 144)) for _ in range(300))
    text = b"".join(b"%d bottles of beer on the wall, %d bottles of beer; take one down, pass it around\n" % (i, i) for i in range(99, 0, -1)) * 3
    rnd = bytes(r.getrandbits(8) for _ in range(70000))
    return [
        ("empty", b""),
        ("one byte", b"x"),
        ("whole members", ic.bam_like(3 * member_bytes, 12)),
        ("whole members and a byte", ic.bam_like(3 * member_bytes + 1, 12)),
        ("zeros", b"\0" * 70000),
        ("period 2", b"ab" * 35000),
        ("period 3", b"abc" * 23000),
        ("period 32768", (block * 3)[:100000]),
        ("a match at distance 32768", far + few[300:32768] + far + few[32768 + 300:]),
        ("no match at distance 32768", far + few[300:32768] + far[::-1] + few[32768 + 300:]),
        ("random", rnd),
        ("text", text),
        ("bam-like", ic.bam_like(200000, 21)),
        ("fx2 records", records),
    ]


def check_members(raw, data, member_bytes):
    """raw is exactly ceil(len(data) / member_bytes) members, each accepted by the oracle and inflating to its piece of data; returns them"""
    ms = ic.split_members(raw) if raw else []
    assert len(ms) == (len(data) + member_bytes - 1) // member_bytes
    for i, m in enumerate(ms):
        assert len(m) <= 65536
        assert ic.oracle(m) == data[i * member_bytes:(i + 1) * member_bytes], "member %d" % i
    return ms
