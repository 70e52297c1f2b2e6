"""`panSVR sort --nsort-device`, psvr_sort_order_names and psvr_bam_store_order_names as far as they go on any machine: the option is listed
and refused with --sort-device, the library exports the calls, and the command's file is that of `panSVR sort -n --deflate-device` -- through
the device route where a GPU is visible, and where none is through the fall-back the command names (tests/test_nsort_device_gpu.py holds the
device route itself)."""
import ctypes as C
import os
import subprocess

import numpy as np

import test_signal as ts

CLI = ts.CLI


def _run(args, **kw):
    return subprocess.run([CLI] + args, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300, **kw)


def _has_device():
    from pansvr_amd import lib
    return lib().psvr_device_count() > 0


def _shuffled(tmp_path, seed, n):
    recs, refs = ts.make_pairs(seed, n)
    order = np.random.RandomState(seed).permutation(len(recs))
    inp = str(tmp_path / "in.bam")
    ts.write_bam(inp, [recs[i] for i in order], refs)
    return inp


def test_usage_lists_the_option():
    r = _run(["sort"])
    assert r.returncode == 1 and "--nsort-device" in r.stderr.decode()
    assert "sort --nsort-device" in _run([]).stderr.decode()


def test_the_two_device_orders_are_refused_together(tmp_path):
    inp = _shuffled(tmp_path, 5, 20)
    for args in (["--nsort-device", "--sort-device"], ["--sort-device", "--nsort-device"], ["-n", "--sort-device", "--nsort-device"]):
        r = _run(["sort"] + args + ["-o", str(tmp_path / "o.bam"), inp])
        err = r.stderr.decode().strip().split("\n")
        assert r.returncode == 1 and len(err) == 1 and "--nsort-device cannot be combined with --sort-device" in err[0], err
    assert not (tmp_path / "o.bam").exists()


def test_the_library_exports_the_calls():
    from pansvr_amd import lib
    import pansvr_amd.sort as ps
    L = lib()
    rc = L.psvr_sort_order_names(C.c_int(0), C.c_int64(3), None, C.c_int64(0), None, None, None)
    rc2 = L.psvr_bam_store_order_names(None)
    assert (rc, rc2) == ((1, 1) if _has_device() else (3, 3))                   # PSVR_ERR_ARG for null arguments; without a device PSVR_ERR_DEVICE
    assert callable(ps.sort_order_names) and callable(ps.BamStore.order_names)


def test_the_file_is_that_of_name_order_with_deflate_device(tmp_path):
    inp = _shuffled(tmp_path, 17, 1500)
    host, dev = str(tmp_path / "host.bam"), str(tmp_path / "dev.bam")
    rh = _run(["sort", "-n", "-t", "3", "--deflate-device", "-o", host, inp])
    rd = _run(["sort", "-t", "3", "--nsort-device", "-o", dev, inp])
    assert rh.returncode == 0 and rd.returncode == 0, rd.stderr.decode()
    assert open(dev, "rb").read() == open(host, "rb").read()
    assert not os.path.exists(dev + ".bai") and not os.path.exists(host + ".bai")
    err = rd.stderr.decode()
    if _has_device():
        assert "records kept on the device" in err and "name order" in err and "failed" not in err, err
    else:
        assert "sort --nsort-device: store create failed" in err and "sorted by the -n --deflate-device route" in err, err
        assert "(name order)" in err


def test_the_default_output_name(tmp_path):
    inp = _shuffled(tmp_path, 3, 30)
    r = _run(["sort", "--nsort-device", inp])
    assert r.returncode == 0 and os.path.exists(inp + ".nsorted.bam") and not os.path.exists(inp + ".sorted.bam"), r.stderr.decode()


def test_a_truncated_input_ends_as_the_host_route_ends(tmp_path):
    inp = _shuffled(tmp_path, 9, 600)
    data = open(inp, "rb").read()
    cut = str(tmp_path / "cut.bam")
    with open(cut, "wb") as f:
        f.write(data[:len(data) * 2 // 3])
    rh = _run(["sort", "-n", "--deflate-device", "-o", str(tmp_path / "h.bam"), cut])
    rd = _run(["sort", "--nsort-device", "-o", str(tmp_path / "d.bam"), cut])
    eh, ed = rh.stderr.decode().strip().split("\n"), rd.stderr.decode().strip().split("\n")
    assert rh.returncode != 0 and rd.returncode == rh.returncode, (eh, ed)
    assert ed[-1] == eh[-1] and "sort --nsort-device:" in ed[0] and "sorted by the -n --deflate-device route" in ed[0], ed
    assert not os.path.exists(str(tmp_path / "d.bam.bai"))
