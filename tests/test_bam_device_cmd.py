"""`panSVR aln --bam-device` where no GPU is needed: what the command line refuses or ignores, and the four calls under the option, which answer
PSVR_ERR_DEVICE where no device is visible."""
import ctypes as C
import subprocess

import signal_device_cases as sc

NEW_SYMBOLS = ("psvr_signal_window", "psvr_signal_window_text", "psvr_fastq_parse_signal", "psvr_fastq_text")
PSVR_ERR_ARG, PSVR_ERR_DEVICE = 1, 3


def aln(*args):
    return subprocess.run([sc.CLI, "aln"] + list(args), stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=60)


def test_more_than_one_device_is_a_conflict():
    r = aln("-N", "--bam-device", "--devices", "0,1", "no_such_index", "no.bam", "no.sam")
    assert r.returncode == 1
    assert r.stderr.count(b"\n") == 1 and b"--bam-device cannot be combined with more than one entry in --devices" in r.stderr


def test_a_fastq_name_gets_the_ignored_line():
    r = aln("-N", "--bam-device", "no_such_index", "no.fq", "no.sam")
    assert b"[panSVR-amd] --bam-device applies to a *.bam read file: ignored for [no.fq]\n" in r.stderr
    assert b"aln --bam-device: refused" not in r.stderr


def test_without_N_the_option_is_refused_on_one_line():
    r = aln("--bam-device", "no_such_index", "no.bam", "no.sam")
    said = [l for l in r.stderr.split(b"\n") if b"--bam-device" in l]
    assert len(said) == 1 and b"refused" in said[0] and b"give -N" in said[0] and b"the host fused route runs" in said[0]


def test_signal_device_keeps_its_message_beside_the_new_option():
    r = aln("-N", "--bam-device", "--signal-device", "--devices", "0,1", "no_such_index", "no.bam", "no.sam")
    assert r.returncode == 1 and b"--signal-device is `panSVR signal -N`'s route" in r.stderr


def test_library_exports_the_four_calls_and_they_need_a_device():
    from pansvr_amd import lib
    import pansvr_amd.fastq as fq
    import pansvr_amd.signal_step as ss
    L = lib()
    for n in NEW_SYMBOLS:
        assert hasattr(L, n), n
    assert C.sizeof(ss.SignalWindowInfo) == 24
    assert all(hasattr(ss.Signal, n) for n in ("window", "window_text")) and all(hasattr(fq.FastqParser, n) for n in ("parse_signal", "text"))
    wi, fi, off = ss.SignalWindowInfo(), fq.FastqInfo(), (C.c_int64 * 1)(0)
    calls = (lambda: L.psvr_signal_window(None, None, C.c_int64(0), off, C.c_int64(0), C.byref(wi)), lambda: L.psvr_signal_window_text(None, None, C.c_int64(0), C.c_int64(0)),
             lambda: L.psvr_fastq_parse_signal(None, None, C.c_int64(0), C.c_int64(1), C.c_int64(1), C.byref(fi)), lambda: L.psvr_fastq_text(None, None, C.c_int64(0), C.c_int64(0)))
    want = PSVR_ERR_ARG if L.psvr_device_count() > 0 else PSVR_ERR_DEVICE          # (null objects: with a device the arguments are what is refused)
    for call in calls:
        assert call() == want
        if want == PSVR_ERR_DEVICE:
            assert b"no HIP device" in L.psvr_last_error()
