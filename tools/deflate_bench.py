#!/usr/bin/env python3
"""BGZF deflate on the device, a wavefront per member (psvr_bgzf_compress_members), beside everything else in the tree that makes BGZF
members, on the BAM-like records of tools/bgzf_bench.py (warm-up first, the arms alternating inside one run, three runs each, the spread
printed).
  python tools/deflate_bench.py call [MB]     from page-locked memory, wall per call with the copies: psvr_bgzf_compress (a lane per 16 KB
                                              block), psvr_bgzf_compress_members at 0xff00 and at 0x4000 bytes per member (and calls of 1024 and of 256 members:
                                              what a writer should gather per call); and BgzfWriter
                                              (bam_writer.h, compiled here into a small timing program) on 1 and 16 threads at zlib level 1,
                                              zlib's default level and with compress_block_fast (16 threads)
  python tools/deflate_bench.py kernel [MB] [--effort N]   two calls of the wavefront entry point (at effort N) and nothing else: the run to put
                                              under `rocprofv3 --kernel-trace --stats`
  python tools/deflate_bench.py effort [MB] [--effort 0,1,2,3] [--parent-lib PATH]
                                              psvr_bgzf_compress_members_effort at 0xff00 bytes per member, time and output size per effort; with
                                              --parent-lib also psvr_bgzf_compress_members of another build's libpsvr_engine.so (the parent commit's:
                                              effort 0 must not pay for the feature).  Every arm is a process of its own (one warm-up call, three
                                              timed ones); one process is discarded, then three rounds with the arms interleaved; median of the
                                              processes' medians and the range of all calls
Every line of results is also appended, as JSON, to the file named by --json."""
import ctypes as C
import json
import os
import shutil
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from pansvr_amd._lib import check, lib  # noqa: E402

HOST = r'''
#include <chrono>
#include "bam_writer.h"
int main(int argc, char **argv)
{
	FILE *f = fopen(argv[1], "rb");
	const int level = atoi(argv[2]), threads = atoi(argv[3]);
	if (!f) return 2;
	fseek(f, 0, SEEK_END);
	std::vector<uint8_t> in((size_t)ftell(f));
	fseek(f, 0, SEEK_SET);
	if (fread(in.data(), 1, in.size(), f) != in.size()) return 2;
	psvr::BgzfWriter w;
	if (!w.open(argv[4], threads, level)) return 3;
	const auto t0 = std::chrono::steady_clock::now();
	w.write(in.data(), in.size());
	if (!w.close()) return 4;
	printf("%.6f\n", std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count());
	return 0;
}
'''


def arg_after(flag):
    return sys.argv[sys.argv.index(flag) + 1] if flag in sys.argv else None


def report(rec):
    print(json.dumps(rec), flush=True)
    fn = arg_after("--json")
    if fn:
        with open(fn, "a") as f:
            f.write(json.dumps(rec) + "\n")


def spread(ts):
    return {"runs_s": [round(t, 4) for t in ts], "median_s": round(sorted(ts)[len(ts) // 2], 4), "spread_s": round(max(ts) - min(ts), 4)}


def records(mb):
    """tools/bgzf_bench.py's records: fixed fields, a name, 75 bytes of 4-bit sequence, 150 quality values from a small alphabet, text tags"""
    rng = np.random.RandomState(3)
    rec, size, i = [], 0, 0
    while size < mb << 20:
        r = (np.uint32(400).tobytes() + rng.randint(0, 1 << 20, size=8).astype(np.uint32).tobytes() + b"read%08d\0" % i + rng.randint(0, 256, size=75, dtype=np.uint8).tobytes()
             + (rng.randint(0, 6, size=150) * 5 + 10).astype(np.uint8).tobytes() + b"ASC\x2aOSC\x20OAZ3,%d,0,60,M;\0RCZ3_%d_0_280_60_150M\0" % (rng.randint(1 << 27), rng.randint(1 << 27)))
        rec.append(r)
        size += len(r)
        i += 1
    return b"".join(rec)


def effort_arm(data_fn, lib_path, effort):
    """one process of `effort`: a warm-up call and three timed ones from page-locked memory; effort None: psvr_bgzf_compress_members of lib_path"""
    data = open(data_fn, "rb").read()
    n = len(data)
    L = C.CDLL(lib_path)
    L.psvr_bgzf_members_bound.restype = C.c_int64
    L.psvr_host_alloc.restype = C.c_void_p
    L.psvr_host_alloc.argtypes = [C.c_size_t]
    L.psvr_last_error.restype = C.c_char_p
    cap = L.psvr_bgzf_members_bound(C.c_int64(n), C.c_int32(0xff00))
    pin_in, pin_out = L.psvr_host_alloc(n), L.psvr_host_alloc(cap)
    assert pin_in and pin_out
    C.memmove(pin_in, data, n)
    got = C.c_int64(0)
    args = (0, C.c_void_p(pin_in), C.c_int64(n), C.c_int32(0xff00), C.c_void_p(pin_out), C.c_int64(cap), C.byref(got), None, C.c_int64(0), None)
    ts = []
    for _ in range(4):
        t0 = time.perf_counter()
        rc = L.psvr_bgzf_compress_members(*args) if effort is None else L.psvr_bgzf_compress_members_effort(*args, C.c_int32(effort))
        ts.append(time.perf_counter() - t0)
        assert rc == 0, L.psvr_last_error()
    import zlib
    assert zlib.decompress(C.string_at(pin_out, 65536), 31) == data[:0xff00]
    print(json.dumps({"calls_s": ts[1:], "out": got.value}))


def effort_main(mb):
    efforts = [int(e) for e in (arg_after("--effort") or "0,1,2,3").split(",")]
    parent = arg_after("--parent-lib")
    data = records(mb)
    tmp = tempfile.mkdtemp(prefix="psvr_deflate_bench_", dir="/dev/shm" if os.path.isdir("/dev/shm") else None)
    data_fn = os.path.join(tmp, "in.bin")
    open(data_fn, "wb").write(data)
    own = os.path.join(ROOT, "pansvr_amd", "libpsvr_engine.so")
    arms = ([("parent build", parent, None)] if parent else []) + [("effort %d" % e, own, e) for e in efforts]

    def run(lib_path, effort):
        cmd = [sys.executable, os.path.abspath(__file__), "effort-arm", data_fn, lib_path, "parent" if effort is None else str(effort)]
        return json.loads(subprocess.check_output(cmd, timeout=600).decode().strip().split("\n")[-1])
    run(own, efforts[0])                                                       # the discarded process
    calls, meds, size = {a[0]: [] for a in arms}, {a[0]: [] for a in arms}, {}
    for _ in range(3):
        for name, lib_path, effort in arms:
            r = run(lib_path, effort)
            calls[name] += r["calls_s"]
            meds[name].append(sorted(r["calls_s"])[1])
            size[name] = r["out"]
    for name, _, _ in arms:
        m = sorted(meds[name])[1]
        report({"level": "call", "arm": name, "input_mb": len(data) / 1e6, "output_mb": size[name] / 1e6, "ratio": round(len(data) / size[name], 3), "process_medians_s": [round(t, 4) for t in meds[name]],
                "median_s": round(m, 4), "min_s": round(min(calls[name]), 4), "max_s": round(max(calls[name]), 4), "gb_per_s": round(len(data) / m / 1e9, 3)})
    shutil.rmtree(tmp, ignore_errors=True)


def main(mb, kernel_only):
    data = records(mb)
    n = len(data)
    L = lib()
    L.psvr_bgzf_bound.restype = C.c_int64
    L.psvr_bgzf_members_bound.restype = C.c_int64
    L.psvr_host_alloc.restype = C.c_void_p
    L.psvr_host_alloc.argtypes = [C.c_size_t]
    cap = max(L.psvr_bgzf_bound(C.c_int64(n)), L.psvr_bgzf_members_bound(C.c_int64(n), C.c_int32(0x4000)))
    pin_in, pin_out = L.psvr_host_alloc(n), L.psvr_host_alloc(cap)
    assert pin_in and pin_out
    C.memmove(pin_in, data, n)
    got, nm = C.c_int64(0), C.c_int64(0)
    offs = np.zeros(n // 0x4000 + 2, dtype=np.int64)

    def lane_per_block():
        t0 = time.perf_counter()
        check(L.psvr_bgzf_compress(0, C.c_void_p(pin_in), C.c_int64(n), C.c_void_p(pin_out), C.c_int64(cap), C.byref(got)))
        return time.perf_counter() - t0, got.value

    def wave(member_bytes, n=n):
        t0 = time.perf_counter()
        check(L.psvr_bgzf_compress_members(0, C.c_void_p(pin_in), C.c_int64(n), C.c_int32(member_bytes), C.c_void_p(pin_out), C.c_int64(cap), C.byref(got),
                                           offs.ctypes.data_as(C.c_void_p), C.c_int64(len(offs) - 1), C.byref(nm)))
        return time.perf_counter() - t0, got.value
    if kernel_only and arg_after("--effort"):
        def wave(member_bytes, n=n):  # noqa: F811  (the same call at an effort)
            check(L.psvr_bgzf_compress_members_effort(0, C.c_void_p(pin_in), C.c_int64(n), C.c_int32(member_bytes), C.c_void_p(pin_out), C.c_int64(cap), C.byref(got),
                                                      offs.ctypes.data_as(C.c_void_p), C.c_int64(len(offs) - 1), C.byref(nm), C.c_int32(int(arg_after("--effort")))))
    wave(0xff00)
    if kernel_only:
        wave(0xff00)
        return
    import gzip
    assert gzip.decompress(C.string_at(pin_out, int(offs[3]))) == data[:3 * 0xff00]
    tmp = tempfile.mkdtemp(prefix="psvr_deflate_bench_", dir="/dev/shm" if os.path.isdir("/dev/shm") else None)
    bindir = tempfile.mkdtemp(prefix="psvr_deflate_bench_")                     # (a memory file system may not run programs)
    exe = os.path.join(bindir, "h")
    open(os.path.join(bindir, "h.cpp"), "w").write(HOST)
    open(os.path.join(tmp, "in.bin"), "wb").write(data)
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-I" + os.path.join(ROOT, "pansvr_amd", "csrc"), "-o", exe, os.path.join(bindir, "h.cpp"), "-lz", "-lpthread"])

    def host(level, threads):
        out = os.path.join(tmp, "out.bgzf")
        dt = float(subprocess.check_output([exe, os.path.join(tmp, "in.bin"), str(level), str(threads), out]).decode())
        return dt, os.path.getsize(out) - 28
    arms = [("lane-per-block-16KB (psvr_bgzf_compress)", lane_per_block), ("wave-per-member-0xff00", lambda: wave(0xff00)), ("wave-per-member-0x4000", lambda: wave(0x4000)),
            ("wave-per-member-0xff00, 1024 members a call", lambda: wave(0xff00, 1024 * 0xff00)), ("wave-per-member-0xff00, 256 members a call", lambda: wave(0xff00, 256 * 0xff00)),
            ("zlib-1-16-threads", lambda: host(1, 16)), ("zlib-default-16-threads", lambda: host(-1, 16)), ("compress_block_fast-16-threads", lambda: host(-2, 16)),
            ("zlib-1-1-thread", lambda: host(1, 1)), ("zlib-default-1-thread", lambda: host(-1, 1))]
    lane_per_block(), wave(0x4000), host(1, 16)                                 # warm-up
    res = {name: [] for name, _ in arms}
    size = {}
    for _ in range(3):
        for name, fn in arms:
            dt, size[name] = fn()
            res[name].append(dt)
    for name, _ in arms:
        n_in = int(name.split(", ")[1].split()[0]) * 0xff00 if ", " in name else n
        rec = {"level": "call", "arm": name, "input_mb": n_in / 1e6, "output_mb": size[name] / 1e6, "ratio": round(n_in / size[name], 3)}
        rec.update(spread(res[name]))
        rec["gb_per_s"] = round(n_in / rec["median_s"] / 1e9, 3)
        report(rec)
    shutil.rmtree(tmp, ignore_errors=True), shutil.rmtree(bindir, ignore_errors=True)


if __name__ == "__main__":
    mode = sys.argv[1] if len(sys.argv) > 1 else "call"
    if mode == "effort-arm":
        effort_arm(sys.argv[2], sys.argv[3], None if sys.argv[4] == "parent" else int(sys.argv[4]))
        sys.exit(0)
    skip = {i + 1 for i, a in enumerate(sys.argv) if a in ("--effort", "--json", "--parent-lib")}
    num = [a for i, a in enumerate(sys.argv) if i >= 2 and i not in skip and a.isdigit()]
    if mode == "effort":
        effort_main(int(num[0]) if num else 192)
        sys.exit(0)
    assert lib().psvr_device_count() > 0, "no HIP device: nothing is measured without one"
    main(int(num[0]) if num else 192, mode == "kernel")
