"""`panSVR aln --mate-device` where no GPU is needed: what the command line refuses or ignores on one line each, the new call under the option,
which answers PSVR_ERR_DEVICE where no device is visible, and its Python view."""
import ctypes as C
import subprocess

import signal_device_cases as sc

PSVR_ERR_ARG, PSVR_ERR_DEVICE = 1, 3


def aln(*args):
    return subprocess.run([sc.CLI, "aln"] + list(args), stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=60)


def said(r, word=b"--mate-device"):
    return [l for l in r.stderr.split(b"\n") if word in l]


def test_a_fastq_name_gets_the_ignored_line():
    r = aln("--mate-device", "no_such_index", "no.fq", "no.sam")
    assert said(r) == [b"[panSVR-amd] --mate-device applies to a *.bam read file: ignored for [no.fq]"]


def test_with_N_the_option_is_refused_on_one_line_that_points_at_bam_device():
    r = aln("-N", "--mate-device", "no_such_index", "no.bam", "no.sam")
    lines = said(r)
    assert len(lines) == 1 and b"aln --mate-device: refused" in lines[0] and b"--bam-device" in lines[0] and b"the host fused route runs" in lines[0]


def test_more_than_one_device_is_a_conflict():
    r = aln("--mate-device", "--devices", "0,1", "no_such_index", "no.bam", "no.sam")
    assert r.returncode == 1
    assert r.stderr.count(b"\n") == 1 and b"--mate-device cannot be combined with more than one entry in --devices" in r.stderr


def test_bam_device_without_N_keeps_its_line_beside_the_new_option():
    r = aln("--bam-device", "--mate-device", "--devices", "0,1", "no_such_index", "no.bam", "no.sam")
    assert r.returncode == 1 and r.stderr.count(b"\n") == 1 and b"--bam-device cannot be combined" in r.stderr
    r = aln("--bam-device", "no_such_index", "no.fq", "no.sam")
    assert said(r) == [] and len(said(r, b"--bam-device")) == 1


def test_block_records_wants_at_least_two():
    for bad in ("1", "0", "-5", "x"):
        r = aln("--block-records", bad, "no_such_index", "no.bam", "no.sam")
        assert r.returncode == 1 and r.stderr == b"--block-records wants a number of at least 2\n"


def test_library_exports_the_add_and_it_needs_a_device():
    from pansvr_amd import lib
    import pansvr_amd.signal_step as ss
    L = lib()
    assert hasattr(L, "psvr_signal_window_add") and hasattr(ss.Signal, "window_add")
    wi, off = ss.SignalWindowInfo(), (C.c_int64 * 1)(0)
    want = PSVR_ERR_ARG if L.psvr_device_count() > 0 else PSVR_ERR_DEVICE                   # (a null object: with a device the argument is what is refused)
    got = L.psvr_signal_window_add(None, None, C.c_int64(0), off, C.c_int64(0), C.c_int32(0), C.byref(wi))
    assert got == want
    if got == PSVR_ERR_DEVICE:
        assert b"no HIP device" in L.psvr_last_error()
