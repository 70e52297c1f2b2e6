"""`panSVR sort --sort-device` and psvr_bam_store_append_bgzf as far as they go on any machine: the option is listed and refused with -n, the library
exports the calls, and the command's files are those of `panSVR sort --deflate-device` -- through the device route where a GPU is visible, and
where none is through the fall-back the command names (tests/test_sort_device_gpu.py holds the device route itself)."""
import ctypes as C
import subprocess

import numpy as np

import test_signal as ts

CLI = ts.CLI


def _run(args, **kw):
    return subprocess.run([CLI] + args, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300, **kw)


def _has_device():
    from pansvr_amd import lib
    return lib().psvr_device_count() > 0


def test_usage_lists_the_option():
    r = _run(["sort"])
    assert r.returncode == 1 and "--sort-device" in r.stderr.decode()
    assert "sort --sort-device" in _run([]).stderr.decode()


def test_name_order_is_refused(tmp_path):
    recs, refs = ts.make_pairs(5, 20)
    inp = str(tmp_path / "in.bam")
    ts.write_bam(inp, recs, refs)
    for args in (["-n", "--sort-device"], ["--sort-device", "-n"]):
        r = _run(["sort"] + args + ["-o", str(tmp_path / "o.bam"), inp])
        err = r.stderr.decode().strip().split("\n")
        assert r.returncode == 1 and len(err) == 1 and "name order is not built on the device" in err[0]
    assert not (tmp_path / "o.bam").exists()


def test_the_library_exports_the_calls():
    from pansvr_amd import lib
    L = lib()
    used, bad = C.c_int64(7), C.c_int64(7)
    rc = L.psvr_bam_store_append_bgzf(None, None, C.c_int64(0), C.c_int64(0), C.c_int32(-1), C.byref(used), C.byref(bad))
    rc2 = L.psvr_bam_store_chain_info(None, None)
    assert (rc, rc2) == ((1, 1) if _has_device() else (3, 3))                   # PSVR_ERR_ARG for no store; without a device PSVR_ERR_DEVICE


def test_the_files_are_those_of_deflate_device(tmp_path):
    recs, refs = ts.make_pairs(17, 1500)
    order = np.random.RandomState(3).permutation(len(recs))
    inp = str(tmp_path / "in.bam")
    ts.write_bam(inp, [recs[i] for i in order], refs)
    host, dev = str(tmp_path / "host.bam"), str(tmp_path / "dev.bam")
    rh = _run(["sort", "-t", "3", "--deflate-device", "-o", host, inp])
    rd = _run(["sort", "-t", "3", "--sort-device", "-o", dev, inp])
    assert rh.returncode == 0 and rd.returncode == 0, rd.stderr.decode()
    for ext in ("", ".bai"):
        assert open(dev + ext, "rb").read() == open(host + ext, "rb").read(), ext
    err = rd.stderr.decode()
    if _has_device():
        assert "records kept on the device" in err and "failed" not in err, err
    else:
        assert "sort --sort-device: store create failed" in err and "sorted by the --deflate-device route" in err, err
