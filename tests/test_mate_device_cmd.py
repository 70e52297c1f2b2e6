"""`panSVR signal --mate-device` and the calls under it where no GPU is: the C ABI's new symbols answer PSVR_ERR_DEVICE, the command says on one
line that it leaves the device route and writes the host route's three files, and the option's refusals are one line each."""
import ctypes as C
import os
import subprocess

import pytest

import signal_mate_cases as mc

NEW_SYMBOLS = ("psvr_signal_run_pos", "psvr_signal_mate_notes", "psvr_signal_left", "psvr_signal_run_left", "psvr_signal_left_errors")
PSVR_ERR_DEVICE = 3


def test_library_exports_the_mate_calls_and_they_need_a_device():
    from pansvr_amd import lib
    import pansvr_amd.signal_step as ss
    L = lib()
    for n in NEW_SYMBOLS:
        assert hasattr(L, n), n
    assert C.sizeof(ss.SignalPosOpt) == 16 and C.sizeof(ss.SignalPosInfo) == 64 and ss.NOTE_DTYPE.itemsize == 280 and C.sizeof(ss.SignalLeftInfo) == 48
    assert C.sizeof(ss.SignalOpt) == 60 and C.sizeof(ss.SignalInfo) == 56 and ss.PAIR_DTYPE.itemsize == 40      # (the earlier structs stay as they are)
    if L.psvr_device_count() > 0:
        return
    info, pi, opt = ss.SignalInfo(), ss.SignalPosInfo(), ss.SignalPosOpt(0, 0)
    assert L.psvr_signal_run_pos(None, None, C.c_int64(0), C.c_int32(0), C.byref(opt), C.byref(info), C.byref(pi)) == PSVR_ERR_DEVICE
    assert b"no HIP device" in L.psvr_last_error()
    assert L.psvr_signal_mate_notes(None, None, C.c_int64(0)) == PSVR_ERR_DEVICE
    assert L.psvr_signal_left(None, None, C.c_int64(0)) == PSVR_ERR_DEVICE
    assert L.psvr_signal_run_left(None, C.c_int64(0), C.c_int64(1), C.byref(info), C.byref(ss.SignalLeftInfo())) == PSVR_ERR_DEVICE
    assert L.psvr_signal_left_errors(None, None, C.c_int64(0)) == PSVR_ERR_DEVICE


@pytest.fixture(scope="module")
def bams():
    tmp = mc.sc.tmpdir("mdc")
    recs, refs = mc.ts.make_pairs(20241, 300)
    mc.ts.write_bam(os.path.join(tmp, "name.bam"), recs, refs)
    mc.ts.write_bam(os.path.join(tmp, "pos.bam"), mc.by_position(recs), refs)
    return tmp, os.path.join(tmp, "pos.bam"), os.path.join(tmp, "name.bam")


def test_without_a_device_the_command_says_so_on_one_line_and_writes_the_host_routes_files(bams):
    from pansvr_amd import lib
    if lib().psvr_device_count() > 0:
        return                                                          # (a device is visible: tests/test_mate_device_gpu.py holds the command there)
    tmp, pos, _ = bams
    h = mc.run_cmd(mc.CLI, tmp, pos, ["-D"], "h")
    d = mc.run_cmd(mc.CLI, tmp, pos, ["-D", "--mate-device"], "d")
    assert h[0].returncode == 0 and d[0].returncode == 0
    assert d[0].stdout == h[0].stdout and len(d[0].stdout) > 100000 and d[1:] == h[1:]
    said = mc.own_lines(d[0].stderr)
    assert len(said) == 1 and b"store create failed (no HIP device visible" in said[0] and b"0 pairs are written" in said[0]
    assert mc.without(d[0].stderr, said) == h[0].stderr


@pytest.mark.parametrize("flags,why", [(["-N", "-D"], b"-N has --signal-device"), (["-D", "-R", "0.5"], b"-R draws rand() per pair"),
                                       (["-D", "--signal-device"], b"give one of the two")])
def test_refusals_are_one_line_each(bams, flags, why):
    tmp, pos, name = bams
    path = name if "-N" in flags else pos
    h = mc.run_cmd(mc.CLI, tmp, path, [f for f in flags if f != "--signal-device"], "h")
    d = mc.run_cmd(mc.CLI, tmp, path, flags + ["--mate-device"], "d")
    assert h[0].returncode == 0 and d[0].returncode == 0, d[0].stderr.decode()[-1000:]
    assert d[0].stdout == h[0].stdout and len(h[0].stdout) > 10000 and d[1:] == h[1:]
    said = mc.own_lines(d[0].stderr)
    assert len(said) == 1 and b"refused" in said[0] and why in said[0] and b"the host route runs" in said[0]


def test_a_build_without_the_route_refuses_on_one_line(bams):
    tmp, pos, _ = bams
    exe = mc.build("signal_device_route_check", tmp)                    # (its signal_main gets no route for the position-sorted mode)
    h = mc.run_cmd(mc.CLI, tmp, pos, ["-D"], "h")
    d = mc.run_cmd(exe, tmp, pos, ["-D", "--mate-device"], "d")
    assert d[0].returncode == 0 and d[0].stdout == h[0].stdout and d[1:] == h[1:]
    said = mc.own_lines(d[0].stderr)
    assert len(said) == 1 and b"refused (this build has no device route)" in said[0]


def test_block_records_wants_two_at_least(bams):
    tmp, pos, _ = bams
    r = subprocess.run([mc.CLI, "signal", "--block-records", "1", pos], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=60)
    assert r.returncode == 1 and b"--block-records wants a number of at least 2" in r.stderr
