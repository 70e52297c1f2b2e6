"""The BAM record encoder's device route without a GPU: the host build of pansvr_amd/csrc/bam_emit_device.h (the rules the kernels of
bam_emit.hip run, compiled with one "lane") against SamEmitter::main_pair's direct BAM branch, per pair: state and bytes, on every case of
tests/bam_emit_cases.py -- once plain and once under AddressSanitizer + UBSan (tests/tools/bam_emit_device_check.cpp, a program of its
own).  Also: the C ABI's new symbols and their answer without a device, and the command's refusal of --emit-device with several devices
and with -S."""
import ctypes as C
import os
import subprocess
import tempfile

import pytest

import bam_emit_cases as bc


@pytest.fixture(scope="module")
def checkers():
    tmp = tempfile.mkdtemp(prefix="psvr_bec_")
    return bc.build_checker(tmp, False), bc.build_checker(tmp, True)


@pytest.fixture(scope="module")
def results(checkers):
    """every case through both builds: [(case, summary)]; the two builds must write the same file"""
    out = []
    cases = bc.cases()
    names = [c["name"] for c in cases]
    assert len(set(names)) == len(names)
    for c in cases:
        a, raw_a = bc.run_checker(checkers[0], c["text"], c["cls"], c["seed"], c["flags"])
        b, raw_b = bc.run_checker(checkers[1], c["text"], c["cls"], c["seed"], c["flags"])
        assert a == b and raw_a == raw_b, c["name"]
        out.append((c, a, bc.split_out(raw_a)))
    return out


def test_host_build_of_the_device_rules_equals_main_pair_on_every_case(results):
    """(the checker's exit status said so for every case: here, that the cases were not empty and the files hold what the counts say)"""
    for c, s, o in results:
        assert s["pairs"] == o["P"] > 0, c["name"]
        assert s["state0"] + s["state1"] + s["state2"] == s["pairs"], c["name"]
        assert o["n_written"] == s["state1"] and o["n_declined"] == s["state2"] and o["n_bytes"] == s["bytes"] == len(o["bytes"]), c["name"]
        assert (s["bytes"] > 0) == (s["state1"] > 0), c["name"]


def test_no_plain_case_declines_and_every_declining_case_declines(results):
    for c, s, _ in results:
        if c["label"] == "plain":
            assert s["state2"] == 0, "%s: %d pairs of a plain case were declined" % (c["name"], s["state2"])
        else:
            assert s["state2"] == s["pairs"], "%s: %d of %d pairs of a declining case were declined" % (c["name"], s["state2"], s["pairs"])
        if c["cls"] != "written":
            assert s["label"] == c["label"], c["name"]           # the checker's own label of a generated class


def test_both_states_occur_in_every_family(results):
    fam = {}
    for c, s, _ in results:
        f = fam.setdefault(c["family"], [0, 0, 0])
        for k in range(3):
            f[k] += s["state%d" % k]
    for name in bc.TWO_SIDED:
        assert fam[name][1] > 0 and fam[name][2] > 0, (name, fam[name])
    for name, f in fam.items():
        assert f[1] > 0, (name, f)
    assert fam["ori"][0] > 0 and fam["golden"][0] > 0 and fam["golden"][1] > 1000


def test_cases_reach_both_strands_and_every_length(results):
    """the records of the 'lengths' case: every l_seq of the list, on both strands (flag 0x10)"""
    import struct
    o = next(o for c, _, o in results if c["name"] == "lengths, written")
    seen, at, raw = set(), 0, o["bytes"]
    while at < len(raw):
        bs, = struct.unpack_from("<I", raw, at)
        flag, l_seq = struct.unpack_from("<H", raw, at + 18)[0], struct.unpack_from("<I", raw, at + 20)[0]
        seen.add((l_seq, bool(flag & 0x10)))
        at += 4 + bs
    assert at == len(raw)
    assert seen == {(n, r) for n in bc.LENGTHS for r in (False, True)}


NEW_SYMBOLS = ("psvr_bam_emit_create", "psvr_bam_emit_results", "psvr_bam_emit_engine", "psvr_bam_emit_download", "psvr_bam_emit_destroy")


def test_library_exports_the_emit_calls_and_they_need_a_device():
    from pansvr_amd import lib
    import pansvr_amd.emit as pe
    L = lib()
    for n in NEW_SYMBOLS:
        assert hasattr(L, n), n
    assert pe.NOT_ORI == 1 and C.sizeof(pe.EmitInfo) == 32
    if L.psvr_device_count() > 0:
        return
    PSVR_ERR_DEVICE = 3
    h = C.c_void_p()
    info = pe.EmitInfo()
    assert L.psvr_bam_emit_create(None, C.byref(h)) == PSVR_ERR_DEVICE and not h.value
    assert b"no HIP device" in L.psvr_last_error()
    assert L.psvr_bam_emit_results(None, None, C.c_int64(0), C.c_int64(0), None, None, None, C.c_int64(0), None, C.c_int64(0), C.c_int32(0), C.byref(info)) == PSVR_ERR_DEVICE
    assert L.psvr_bam_emit_engine(None, None, None, C.c_int32(0), C.byref(info)) == PSVR_ERR_DEVICE
    assert L.psvr_bam_emit_download(None, None, C.c_int64(0), None, None) == PSVR_ERR_DEVICE
    L.psvr_bam_emit_destroy.restype = None
    L.psvr_bam_emit_destroy(None)


@pytest.mark.parametrize("other,words", [(["--devices", "0,1"], ("--emit-device", "--devices")), (["-S"], ("--emit-device", "-S"))])
def test_command_refuses_emit_device_with_several_devices_and_with_sam(other, words):
    tmp = tempfile.mkdtemp(prefix="psvr_bec_")
    r = subprocess.run([bc.CLI, "aln", "--emit-device"] + other + [os.path.join(tmp, "no_such_index"), os.path.join(tmp, "no.fq"), os.path.join(tmp, "no.sam")],
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    err = r.stderr.decode()
    assert r.returncode == 1, err[-1000:]
    assert all(w in err for w in words), err
    assert "loading index" not in err and "Open original header" not in err
