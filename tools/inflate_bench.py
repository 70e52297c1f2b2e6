#!/usr/bin/env python3
"""BGZF inflate on the device, measured at two levels (warm-up first, the arms alternating inside one process, three runs each, the spread printed).
  python tools/inflate_bench.py call [MB]        psvr_bgzf_decompress on >= MB (default 1024) inflated of level-6 BAM-like members from
                                                 page-locked memory: wall per call, copies included, beside zlib on 1 and on 16 threads
                                                 over the same members in this process
  python tools/inflate_bench.py kernel [MB]      two calls and nothing else: the run to put under `rocprofv3 --kernel-trace --stats`
  python tools/inflate_bench.py cmd [PAIRS] [--parent DIR]
                                                 `panSVR sort` and `panSVR signal -N` on a generated BAM of 2 x PAIRS records (default 1 000 000
                                                 pairs); arms: the parent commit's binary (DIR/bin/panSVR, if given), this build's default route,
                                                 --inflate-threads 16, --inflate-device (also at 4 MiB and 64 MiB chunks)
Every line of results is also appended, as JSON, to the file named by --json."""
import ctypes as C
import json
import os
import subprocess
import sys
import tempfile
import time
import zlib
from concurrent.futures import ThreadPoolExecutor

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import inflate_cases as ic  # noqa: E402
from pansvr_amd._lib import check, lib  # noqa: E402

CLI = os.path.join(ROOT, "pansvr_amd", "bin", "panSVR")


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


def call_level(mb, kernel_only):
    data = b"".join(ic.bam_like_big(min(64, mb - k) << 20, 31 + k) for k in range(0, mb, 64))      # (in pieces: the generator's temporaries stay small)
    members = ic.members_of(data)
    comp = b"".join(members)
    L = lib()
    L.psvr_host_alloc.restype = C.c_void_p
    L.psvr_host_alloc.argtypes = [C.c_size_t]
    pin_in, pin_out = L.psvr_host_alloc(len(comp)), L.psvr_host_alloc(len(data))
    assert pin_in and pin_out
    C.memmove(pin_in, comp, len(comp))
    used, total, nm, bad = C.c_int64(0), C.c_int64(0), C.c_int64(0), C.c_int64(-1)

    def device():
        t0 = time.perf_counter()
        check(L.psvr_bgzf_decompress(0, C.c_void_p(pin_in), C.c_int64(len(comp)), C.byref(used), C.c_void_p(pin_out), C.c_int64(len(data)), C.byref(total), None, C.c_int64(0),
                                     C.byref(nm), C.byref(bad)))
        return time.perf_counter() - t0
    device()
    assert total.value == len(data) and C.string_at(pin_out, 1 << 20) == data[:1 << 20] and C.string_at(pin_out + len(data) - 4096, 4096) == data[-4096:]
    if kernel_only:
        device()
        return
    payloads = [m[18:-8] for m in members]

    def host(threads):
        t0 = time.perf_counter()
        if threads == 1:
            n = sum(len(zlib.decompress(p, -15)) for p in payloads)
        else:
            with ThreadPoolExecutor(threads) as ex:
                n = sum(ex.map(lambda p: len(zlib.decompress(p, -15)), payloads))
        assert n == len(data)
        return time.perf_counter() - t0
    host(16)
    arms = {"device": [], "zlib-16-threads": [], "zlib-1-thread": []}
    for _ in range(3):
        arms["device"].append(device())
        arms["zlib-16-threads"].append(host(16))
        arms["zlib-1-thread"].append(host(1))
    for name, ts in arms.items():
        rec = {"level": "call", "arm": name, "inflated_mb": len(data) / 1e6, "compressed_mb": len(comp) / 1e6, "members": len(members)}
        rec.update(spread(ts))
        rec["gb_per_s_inflated"] = round(len(data) / rec["median_s"] / 1e9, 3)
        report(rec)


def make_bam(path, pairs):
    """A name-sorted BAM of 2 x pairs primary records (+ a few secondary ones): tests/test_signal.py's generator for 20 000 pairs, repeated
    (a repeat lies megabytes behind its first copy, far outside DEFLATE's window, so the members compress like unrepeated ones)."""
    import test_signal as ts
    recs, refs = ts.make_pairs(12, 20000)
    body = b"".join(recs)
    text = "@HD\tVN:1.6\tSO:queryname\n" + "".join("@SQ\tSN:%s\tLN:%d\n" % r for r in refs)
    h = b"BAM\x01" + np.int32(len(text)).tobytes() + text.encode() + np.int32(len(refs)).tobytes()
    for n, l in refs:
        h += np.int32(len(n) + 1).tobytes() + n.encode() + b"\0" + np.int32(l).tobytes()
    raw = h + body * ((pairs + 19999) // 20000)
    with open(path, "wb") as f:
        f.write(b"".join(ic.members_of(raw)) + ic.wrap(ic.deflate(b""), b""))
    return len(raw), len(recs) * ((pairs + 19999) // 20000)


def cmd_level(pairs, parent):
    tmp = tempfile.mkdtemp(prefix="psvr_inflate_bench_")
    bam = os.path.join(tmp, "in.bam")
    raw_bytes, n_rec = make_bam(bam, pairs)
    arms = []
    if parent:
        arms.append(("parent", os.path.join(parent, "bin", "panSVR"), [], None))
    arms += [("default", CLI, [], None), ("inflate-threads-16", CLI, ["--inflate-threads", "16"], None), ("inflate-device", CLI, ["--inflate-device"], None),
             ("inflate-device-4MiB", CLI, ["--inflate-device"], str(4 << 20)), ("inflate-device-64MiB", CLI, ["--inflate-device"], str(64 << 20))]
    for what in ("sort", "signal -N"):
        def run(exe, extra, batch):
            env = dict(os.environ)
            env.pop("PSVR_INFLATE_BATCH", None)
            if batch:
                env["PSVR_INFLATE_BATCH"] = batch
            if what == "sort":
                cmd = [exe, "sort", "-t", "16", "-o", os.path.join(tmp, "out.bam")] + extra + [bam]
            else:
                cmd = [exe, "signal", "-N"] + extra + ["-H", os.path.join(tmp, "h.sam"), "-S", os.path.join(tmp, "s.txt"), bam]
            t0 = time.perf_counter()
            r = subprocess.run(cmd, env=env, stdout=subprocess.DEVNULL, stderr=subprocess.PIPE, timeout=600)
            dt = time.perf_counter() - t0
            assert r.returncode == 0, r.stderr.decode()[-1000:]
            assert "host threads" not in r.stderr.decode() or "--inflate-device" not in extra, r.stderr.decode()[-1000:]
            return dt
        run(CLI, [], None)                                        # warm-up: the file in the page cache, the binaries loaded
        times = {a[0]: [] for a in arms}
        for _ in range(3):
            for name, exe, extra, batch in arms:
                times[name].append(run(exe, extra, batch))
        for name, ts in times.items():
            rec = {"level": "command", "command": what, "arm": name, "records": n_rec, "inflated_mb": raw_bytes / 1e6, "bam_mb": os.path.getsize(bam) / 1e6}
            rec.update(spread(ts))
            report(rec)


if __name__ == "__main__":
    mode = sys.argv[1] if len(sys.argv) > 1 else "call"
    num = [a for a in sys.argv[2:] if a.isdigit()]
    assert lib().psvr_device_count() > 0, "no HIP device: nothing is measured without one"
    if mode in ("call", "kernel"):
        call_level(int(num[0]) if num else 1024, mode == "kernel")
    else:
        cmd_level(int(num[0]) if num else 1000000, arg_after("--parent"))
