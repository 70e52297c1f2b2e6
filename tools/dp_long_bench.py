#!/usr/bin/env python3
"""Long-shape benchmark of the DP kernels through the device-pointer C ABI (psvr_dp_plan_*): n problems of qlen = tlen = L
(~5 % divergence) at band width w, with or without CIGAR; reports the kernel the planner picked and the rate in IN-BAND cells/s
(the cells of [st0, en0] on every anti-diagonal, what the recurrence computes; a band w holds ~ (2 w + 1) L of the L^2 cells).
Usage: python tools/dp_long_bench.py [L:w:n[:s] ...]   (s: score only; default: the shapes of the long-route report)"""
import ctypes as C
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from ksw_cases import mat5  # noqa: E402
from pansvr_amd import ksw  # noqa: E402
from pansvr_amd._lib import check, lib  # noqa: E402

DEFAULT = ["8000:200:512", "20000:200:512", "8000:132:512", "20000:132:512", "8000:1000:128", "20000:1000:64",
           "8000:-1:16", "20000:-1:4", "100000:200:16:s"]


def in_band_cells(ql, tl, w):
    w = max(ql, tl) if w < 0 else w
    r = np.arange(ql + tl - 1, dtype=np.int64)
    st = np.maximum.reduce([np.zeros_like(r), r - ql + 1, (r - w + 1) >> 1])
    en = np.minimum.reduce([np.full_like(r, tl - 1), r, (r + w) >> 1])
    return int(np.maximum(en - st + 1, 0).sum())


def run(L, w, n, score_only):
    rng = np.random.RandomState(L + w)
    t = rng.randint(0, 4, size=n * L).astype(np.uint8)
    q = t.copy()
    m = rng.random_sample(q.size) < 0.05
    q[m] = (q[m] + 1 + rng.randint(3, size=int(m.sum()))) % 4
    qlen = np.full(n, L, np.int32)
    off = (np.arange(n) * L).astype(np.int64)
    dev = torch.device("cuda:0")
    dq, dt, doff = torch.from_numpy(q).to(dev), torch.from_numpy(t).to(dev), torch.from_numpy(off).to(dev)
    ez_host = np.zeros(n, dtype=np.dtype([("f", "<i4", 12), ("cigar_off", "<i8")]))
    ez_host["cigar_off"] = np.arange(n) * (2 * L + 2)
    dez = torch.from_numpy(ez_host.view(np.uint8).reshape(-1)).to(dev)
    dcig = torch.zeros(n * (2 * L + 2) + 16, dtype=torch.int32, device=dev)
    p = ksw.make_params(5, mat5(2, 12), 16, 1, 32, 0, w, 400, -1, 1 if score_only else 0)
    L_ = lib()
    plan = C.c_void_p()
    check(L_.psvr_dp_plan_create(0, C.c_int64(n), qlen.ctypes.data_as(C.c_void_p), qlen.ctypes.data_as(C.c_void_p), C.byref(p), 0, C.byref(plan)))
    L_.psvr_dp_plan_workspace_bytes.restype = C.c_int64
    ws = torch.empty(int(L_.psvr_dp_plan_workspace_bytes(plan)) + 256, dtype=torch.uint8, device=dev)
    buf = C.create_string_buffer(4096)
    L_.psvr_dp_plan_describe(plan, buf, 4096)

    def once():
        check(L_.psvr_dp_plan_launch(plan, C.c_void_p(dq.data_ptr()), C.c_void_p(doff.data_ptr()), C.c_void_p(dt.data_ptr()), C.c_void_p(doff.data_ptr()),
                                     C.c_void_p(dez.data_ptr()), C.c_void_p(dcig.data_ptr()), C.c_void_p(ws.data_ptr()), None))
    once()
    torch.cuda.synchronize()
    reps, t0 = 0, time.time()
    while reps < 3 and (reps == 0 or time.time() - t0 < 5):
        once()
        torch.cuda.synchronize()
        reps += 1
    dt_ = (time.time() - t0) / reps
    cells = in_band_cells(L, L, w) * n
    print("L=%-6d w=%-5d n=%-4d %-10s %10.2f ms  %8.2f G in-band cells/s  workspace %7.1f MB  [%s]"
          % (L, w, n, "score only" if score_only else "CIGAR", dt_ * 1e3, cells / dt_ / 1e9, ws.numel() / 1e6, buf.value.decode().strip()), flush=True)
    L_.psvr_dp_plan_destroy(plan)


for spec in sys.argv[1:] or DEFAULT:
    f = spec.split(":")
    run(int(f[0]), int(f[1]), int(f[2]), len(f) > 3 and f[3] == "s")
