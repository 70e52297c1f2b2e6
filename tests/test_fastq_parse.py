"""The FASTQ parser's device route without a GPU: the host build of pansvr_amd/csrc/fastq_device.h (the rules the kernels of fastq.hip
run, compiled with one "lane") against the host parser of fastq_batch.h, byte for byte, on every case of tests/fastq_cases.py -- once
plain and once under AddressSanitizer + UBSan (tests/fastq_check.cpp, a program of its own).  Also: the C ABI's new symbols and their
answer without a device, and the command's refusal of --parse-device with several devices."""
import ctypes as C
import os
import subprocess
import tempfile

import pytest

import fastq_cases as fc


@pytest.fixture(scope="module")
def checkers():
    tmp = tempfile.mkdtemp(prefix="psvr_fqc_")
    return fc.build_checker(tmp, False), fc.build_checker(tmp, True)


@pytest.fixture(scope="module")
def all_cases(checkers):
    return fc.cases(fc.constants(checkers[0])["tile_bytes"])


def test_constants_are_printed(checkers):
    k = fc.constants(checkers[0])
    assert k == fc.constants(checkers[1])
    assert k["tile_bytes"] >= 256 and k["tile_bytes"] % 16 == 0 and k["group"] >= 1


def test_host_build_of_the_device_rules_equals_fastq_batch_on_every_case(checkers, all_cases):
    plain, asan = checkers
    names = [c[0] for c in all_cases]
    assert len(set(names)) == len(names)
    for name, text, at_end, max_pairs, max_bases in all_cases:
        a = fc.run_checker(plain, text, at_end, max_pairs, max_bases)
        b = fc.run_checker(asan, text, at_end, max_pairs, max_bases)
        assert a == b, name
        out = fc.split_out(a)
        assert out["bases"][-1] == 0, name


def test_cases_reach_what_they_are_meant_to(checkers, all_cases):
    """the limits and the window's end really stop some cases, and every stop reason occurs"""
    stops = {}
    for name, text, at_end, max_pairs, max_bases in all_cases:
        if name.startswith(("max_", "both", "limits", "text of", "empty", "8k+")):
            stops[name] = fc.split_out(fc.run_checker(checkers[0], text, at_end, max_pairs, max_bases))["info"]
    assert stops["max_pairs smaller than the text"][0] == 3 and stops["max_pairs smaller than the text"][4] == 0
    assert stops["max_bases 60"][0] == 3 and stops["max_bases 61"][0] == 4 and stops["max_bases 59"][0] == 3 and stops["max_bases 1"][0] == 1
    assert stops["max_bases 0"][0] == 0 and stops["max_bases 60"][4] == 1
    assert stops["empty"][4] == 2 and stops["8k+3 lines"][:1] == [2] and stops["8k+3 lines"][3] == 19


def test_a_text_cut_at_every_byte_gives_the_whole(checkers):
    tmp = tempfile.mkdtemp(prefix="psvr_fqc_")
    text = fc.sixteen_pairs()
    assert len(text) > fc.constants(checkers[0])["tile_bytes"] + 64
    with open(os.path.join(tmp, "in"), "wb") as f:
        f.write(text)
    for exe in checkers:
        r = subprocess.run([exe, "cut", os.path.join(tmp, "in")], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=900)
        assert r.returncode == 0 and not r.stderr, r.stderr.decode()[-2000:]
        assert r.stdout.split() == [b"cuts", b"%d" % (len(text) + 1), b"pairs", b"16"]


NEW_SYMBOLS = ("psvr_fastq_create", "psvr_fastq_parse", "psvr_fastq_download", "psvr_engine_upload_fastq", "psvr_fastq_destroy")


def test_library_exports_the_fastq_calls_and_they_need_a_device():
    from pansvr_amd import lib
    import pansvr_amd.fastq as pf
    L = lib()
    for n in NEW_SYMBOLS:
        assert hasattr(L, n), n
    if L.psvr_device_count() > 0:
        return
    PSVR_ERR_DEVICE = 3
    h = C.c_void_p()
    info = pf.FastqInfo()
    assert L.psvr_fastq_create(C.c_int(0), C.byref(h)) == PSVR_ERR_DEVICE and not h.value
    assert b"no HIP device" in L.psvr_last_error()
    assert L.psvr_fastq_parse(None, b"@r\n", C.c_int64(3), C.c_int(1), C.c_int64(1), C.c_int64(1), C.byref(info)) == PSVR_ERR_DEVICE
    assert L.psvr_fastq_download(None, None, None, None, None, None) == PSVR_ERR_DEVICE
    assert L.psvr_engine_upload_fastq(None, None, C.c_int64(0), C.c_int64(0)) == PSVR_ERR_DEVICE
    L.psvr_fastq_destroy.restype = None
    L.psvr_fastq_destroy(None)
    with pytest.raises(pf.EngineError if hasattr(pf, "EngineError") else Exception):
        pf.FastqParser()


def test_command_refuses_parse_device_with_several_devices():
    tmp = tempfile.mkdtemp(prefix="psvr_fqc_")
    r = subprocess.run([fc.CLI, "aln", "--parse-device", "--devices", "0,1", os.path.join(tmp, "no_such_index"), os.path.join(tmp, "no.fq"), os.path.join(tmp, "no.sam")],
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    err = r.stderr.decode()
    assert r.returncode == 1, err[-1000:]
    assert "--parse-device" in err and "between devices" in err
    assert "loading index" not in err and "Open original header" not in err
