"""The second BAM file's device encoder without a GPU: the host build of pansvr_amd/csrc/bam_ori_device.h (the rules the ori kernels of
bam_emit.hip run, compiled with one "lane") against the BAM branch of SamEmitter::ori_pair, per pair: state and bytes, on every case of
tests/bam_ori_cases.py -- once plain and once under AddressSanitizer + UBSan (tests/tools/bam_ori_device_check.cpp, a program of its own).
Also: the C ABI's new symbols and their answer without a device, and the command's refusal of --ori-device with several devices and with -S."""
import ctypes as C
import os
import struct
import subprocess
import tempfile

import pytest

import bam_ori_cases as oc


@pytest.fixture(scope="module")
def checkers():
    tmp = tempfile.mkdtemp(prefix="psvr_boc_")
    return oc.build_checker(tmp, False), oc.build_checker(tmp, True)


@pytest.fixture(scope="module")
def results(checkers):
    """every case through both builds: [(case, summary, out)]; the two builds must write the same file"""
    out = []
    cases = oc.cases()
    names = [c["name"] for c in cases]
    assert len(set(names)) == len(names)
    for c in cases:
        a, raw_a = oc.run_checker(checkers[0], c["text"], c["cls"], c["seed"], c["mfs"])
        b, raw_b = oc.run_checker(checkers[1], c["text"], c["cls"], c["seed"], c["mfs"])
        assert a == b and raw_a == raw_b, c["name"]
        out.append((c, a, oc.split_out(raw_a)))
    return out


def records(raw):
    """[(flag, l_seq, n_cigar, aux bytes)] of a run of BAM records"""
    out, at = [], 0
    while at < len(raw):
        bs, = struct.unpack_from("<I", raw, at)
        l_name, n_cigar, flag, l_seq = raw[at + 12], struct.unpack_from("<H", raw, at + 16)[0], struct.unpack_from("<H", raw, at + 18)[0], struct.unpack_from("<I", raw, at + 20)[0]
        aux = at + 36 + l_name + 4 * n_cigar + (l_seq + 1) // 2 + l_seq
        out.append((flag, l_seq, n_cigar, raw[aux:at + 4 + bs]))
        at += 4 + bs
    assert at == len(raw)
    return out


def test_host_build_of_the_device_rules_equals_ori_pair_on_every_case(results):
    """(the checker's exit status said so for every case: here, that the cases were not empty and the files hold what the counts say)"""
    for c, s, o in results:
        assert s["pairs"] == o["P"] > 0, c["name"]
        assert s["state0"] + s["state1"] + s["state2"] == s["pairs"], c["name"]
        assert o["n_written"] == s["state1"] and o["n_declined"] == s["state2"] and o["n_bytes"] == s["bytes"] == len(o["bytes"]), c["name"]
        assert (s["bytes"] > 0) == (s["state1"] > 0), c["name"]
        assert o["min_filter_score"] == c["mfs"]


def test_no_plain_case_declines_and_every_declining_case_declines(results):
    for c, s, _ in results:
        if c["label"] == "plain":
            assert s["state2"] == 0, "%s: %d pairs of a plain case were declined" % (c["name"], s["state2"])
        else:
            assert s["state2"] == s["pairs"], "%s: %d of %d pairs of a declining case were declined" % (c["name"], s["state2"], s["pairs"])
        if c["expect"] == "written":
            assert s["state1"] == s["pairs"], "%s: %d of %d pairs were written" % (c["name"], s["state1"], s["pairs"])
        if c["expect"] == "nothing":
            assert s["state0"] == s["pairs"], "%s: %d of %d pairs wrote nothing" % (c["name"], s["state0"], s["pairs"])


def test_golden_sets_decline_nothing_and_write_records(results):
    """a condition, not a measurement: the reference's own comments hold only i tags and the operators the rules take"""
    n = 0
    for c, s, _ in results:
        if c["family"] == "golden":
            assert s["state2"] == 0 and s["state1"] > 0, (c["name"], s)
            n += 1
    assert n >= 16


def test_both_states_occur_in_every_two_sided_family(results):
    fam = {}
    for c, s, _ in results:
        f = fam.setdefault(c["family"], [0, 0, 0])
        for k in range(3):
            f[k] += s["state%d" % k]
    for name in oc.TWO_SIDED:
        assert fam[name][1] > 0 and fam[name][2] > 0, (name, fam[name])
    assert fam["proper"][0] > 0 and fam["proper"][1] > 0 and fam["gate"][0] > 0 and fam["section"][0] > 0 and fam["skip"][0] > 0


def test_cases_reach_both_strands_every_length_and_every_operator(results):
    seen = set()
    for c, _, o in results:
        if c["family"] == "seq":
            seen |= {(l_seq, bool(flag & 0x10)) for flag, l_seq, _, _ in records(o["bytes"])}
    assert seen >= {(n, r) for n in oc.LENGTHS for r in (False, True)}
    o = next(o for c, _, o in results if c["name"] == "CIGAR texts")
    recs = records(o["bytes"])
    assert {n for _, _, n, _ in recs} >= {0, 1, 2, 3, 16, 17}
    assert any(flag & 4 for flag, _, n, _ in recs if n == 0)
    o = next(o for c, _, o in results if c["name"] == "65535 operators")
    assert 65535 in {n for _, _, n, _ in records(o["bytes"])}


def aux_fields(aux):
    """[(tag, type, value bytes)] of a record's aux block"""
    size = {"c": 1, "C": 1, "s": 2, "S": 2, "i": 4, "I": 4, "A": 1}
    out, at = [], 0
    while at < len(aux):
        tag, ty = aux[at:at + 2], chr(aux[at + 2])
        n = size[ty] if ty in size else aux.index(b"\0", at + 3) - (at + 3) + 1
        out.append((tag, ty, aux[at + 3:at + 3 + n]))
        at += 3 + n
    assert at == len(aux)
    return out


def test_boundary_integers_take_the_smallest_type(results):
    code = lambda v: ("c" if v >= -128 else "s" if v >= -32768 else "i") if v < 0 else ("C" if v <= 255 else "S" if v <= 65535 else "I")
    pack = {"c": "b", "C": "B", "s": "h", "S": "H", "i": "i", "I": "I"}
    want = [(b"X%x" % j, code(v), struct.pack("<" + pack[code(v)], v)) for j, v in enumerate(oc.BOUNDARY_INTS)]
    o = next(o for c, _, o in results if c["name"] == "TAG_ texts")
    assert any(aux_fields(aux)[:-1] == want for _, _, _, aux in records(o["bytes"]))
    o = next(o for c, _, o in results if c["name"] == "MS:i of every integer type")
    last = [aux_fields(aux)[-1] for _, _, _, aux in records(o["bytes"])]
    assert all(tag == b"MS" for tag, _, _ in last) and {ty for _, ty, _ in last} >= {"C", "S", "I"}


NEW_SYMBOLS = ("psvr_bam_emit_ori_results", "psvr_bam_emit_ori_engine")


def test_library_exports_the_ori_calls_and_they_need_a_device():
    from pansvr_amd import lib
    import pansvr_amd.emit as pe
    L = lib()
    for n in NEW_SYMBOLS:
        assert hasattr(L, n), n
    assert hasattr(pe.BamEmitter, "emit_ori_results") and hasattr(pe.BamEmitter, "emit_ori_engine")
    if L.psvr_device_count() > 0:
        return
    PSVR_ERR_DEVICE = 3
    info = pe.EmitInfo()
    assert L.psvr_bam_emit_ori_results(None, None, C.c_int64(0), C.c_int64(0), None, None, None, C.c_int64(0), None, C.c_int64(0), C.c_int32(0), C.byref(info)) == PSVR_ERR_DEVICE
    assert b"no HIP device" in L.psvr_last_error()
    assert L.psvr_bam_emit_ori_engine(None, None, None, C.byref(info)) == PSVR_ERR_DEVICE


@pytest.mark.parametrize("other,words", [(["--devices", "0,1"], ("--ori-device", "--devices")), (["-S"], ("--ori-device", "-S"))])
def test_command_refuses_ori_device_with_several_devices_and_with_sam(other, words):
    tmp = tempfile.mkdtemp(prefix="psvr_boc_")
    r = subprocess.run([oc.CLI, "aln", "--ori-device"] + other + [os.path.join(tmp, "no_such_index"), os.path.join(tmp, "no.fq"), os.path.join(tmp, "no.sam")],
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    err = r.stderr.decode()
    assert r.returncode == 1, err[-1000:]
    assert all(w in err for w in words) and err.count("\n") == 1, err
    assert "loading index" not in err and "Open original header" not in err
