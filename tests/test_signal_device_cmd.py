"""`panSVR signal --signal-device` and the calls under it where no GPU is: the C ABI's new symbols answer PSVR_ERR_DEVICE, the command says on
one line that it leaves the device route and writes the host route's three files, and the option is refused without -N and with -R."""
import ctypes as C
import os
import struct
import subprocess

import pytest

import signal_device_cases as sc
import test_signal as ts

NEW_SYMBOLS = ("psvr_signal_create", "psvr_signal_run", "psvr_signal_text", "psvr_signal_pairs", "psvr_signal_side", "psvr_signal_pair_records", "psvr_signal_stats", "psvr_signal_destroy",
               "psvr_bam_store_drop", "psvr_bam_store_footprint")
PSVR_ERR_ARG, PSVR_ERR_DEVICE = 1, 3


def test_library_exports_the_signal_calls_and_they_need_a_device():
    from pansvr_amd import lib
    import pansvr_amd.signal_step as ss
    L = lib()
    for n in NEW_SYMBOLS:
        assert hasattr(L, n), n
    assert C.sizeof(ss.SignalOpt) == 60 and C.sizeof(ss.SignalInfo) == 56 and ss.PAIR_DTYPE.itemsize == 40
    h = C.c_void_p()
    opt = ss.signal_opt([100, 1, 2, 3], 1, 500)
    assert L.psvr_signal_create(C.c_int(0), None, C.byref(h)) == PSVR_ERR_ARG and L.psvr_signal_create(C.c_int(0), C.byref(opt), None) == PSVR_ERR_ARG
    if L.psvr_device_count() > 0:
        return
    info, n, b = ss.SignalInfo(), C.c_int64(0), C.c_int64(0)
    assert L.psvr_signal_create(C.c_int(0), C.byref(opt), C.byref(h)) == PSVR_ERR_DEVICE and not h.value
    assert b"no HIP device" in L.psvr_last_error()
    assert L.psvr_signal_run(None, None, C.c_int64(0), C.c_int32(0), C.byref(info)) == PSVR_ERR_DEVICE
    assert L.psvr_signal_text(None, None, C.c_int64(0)) == PSVR_ERR_DEVICE
    assert L.psvr_signal_pairs(None, None, C.c_int64(0)) == PSVR_ERR_DEVICE
    assert L.psvr_signal_side(None, None, C.c_int64(0)) == PSVR_ERR_DEVICE
    assert L.psvr_signal_pair_records(None, None, C.c_int64(0), None, C.c_int64(0), C.byref(n)) == PSVR_ERR_DEVICE
    assert L.psvr_signal_stats(None, None, None) == PSVR_ERR_DEVICE
    assert L.psvr_bam_store_drop(None, C.c_int64(0)) == PSVR_ERR_DEVICE
    assert L.psvr_bam_store_footprint(None, C.byref(n), C.byref(b)) == PSVR_ERR_DEVICE
    L.psvr_signal_destroy.restype = None
    L.psvr_signal_destroy(None)


def run(tmp, bam, flags, tag):
    r = subprocess.run([sc.CLI, "signal"] + flags + ["-H", os.path.join(tmp, tag + ".sam"), "-S", os.path.join(tmp, tag + ".txt"), bam], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120)
    return r, open(os.path.join(tmp, tag + ".sam"), "rb").read(), open(os.path.join(tmp, tag + ".txt"), "rb").read()


@pytest.fixture(scope="module")
def bam():
    recs, refs = ts.make_pairs(20241, 300)
    tmp = sc.tmpdir("sdc")
    ts.write_bam(os.path.join(tmp, "in.bam"), recs, refs)

    def key(i):                                                         # (the position-sorted mode's input, as test_signal orders it)
        tid, pos = struct.unpack_from("<ii", recs[i], 4)
        return (tid if tid >= 0 else 1 << 31, pos, i)
    ts.write_bam(os.path.join(tmp, "pos.bam"), [recs[i] for i in sorted(range(len(recs)), key=key)], refs)
    return tmp, os.path.join(tmp, "in.bam")


def test_without_a_device_the_command_says_so_on_one_line_and_writes_the_host_routes_files(bam):
    from pansvr_amd import lib
    if lib().psvr_device_count() > 0:
        return                                                          # (a device is visible: tests/test_signal_device_gpu.py holds the command there)
    tmp, path = bam
    h = run(tmp, path, ["-N", "-D"], "h")
    d = run(tmp, path, ["-N", "-D", "--signal-device"], "d")
    assert h[0].returncode == 0 and d[0].returncode == 0
    assert d[0].stdout == h[0].stdout and len(d[0].stdout) > 100000 and d[1:] == h[1:]
    said = [l for l in d[0].stderr.split(b"\n") if b"--signal-device" in l]
    assert len(said) == 1 and b"store create failed (no HIP device visible" in said[0] and b"0 pairs are written" in said[0]
    assert d[0].stderr.replace(said[0] + b"\n", b"") == h[0].stderr


@pytest.mark.parametrize("flags,why", [(["-D"], b"give -N"), (["-N", "-D", "-R", "0.5"], b"-R draws rand() per pair")])
def test_refused_up_front_without_N_and_with_R(bam, flags, why):
    tmp, path = bam
    if "-N" not in flags:
        path = os.path.join(tmp, "pos.bam")
    h = run(tmp, path, flags, "h")
    d = run(tmp, path, flags + ["--signal-device"], "d")
    assert h[0].returncode == 0 and d[0].returncode == 0, d[0].stderr.decode()[-1000:]
    assert d[0].stdout == h[0].stdout and len(h[0].stdout) > 10000 and d[1:] == h[1:]
    said = [l for l in d[0].stderr.split(b"\n") if b"--signal-device" in l]
    assert len(said) == 1 and b"refused" in said[0] and why in said[0] and b"the host route runs" in said[0]


def test_aln_says_that_the_option_is_not_its_own():
    r = subprocess.run([sc.CLI, "aln", "--signal-device", "no_such_index", "no.bam", "no.sam"], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=60)
    assert b"--signal-device is `panSVR signal -N`'s route" in r.stderr
