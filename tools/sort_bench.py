"""psvr_sort_order_u64 timed with the host clock around the call (copies included: keys in, order out) on samtools coordinate keys
(25 references, positions up to 2^28, 2 % unplaced), checked against numpy's stable argsort, whose time is printed beside it.
    python tools/sort_bench.py [--n 2000000 50000000] [--reps 5] [--device 0]
One JSON line per size.  Kernel times: run it under `rocprofv3 --kernel-trace --stats` in a run of its own."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from pansvr_amd.sort import sort_order  # noqa: E402


def coord_keys(n, seed=4):
    rng = np.random.RandomState(seed)
    tid = rng.randint(0, 25, n).astype(np.uint64)
    pos = rng.randint(-1, 1 << 28, n).astype(np.uint64) + np.uint64(1)
    keys = tid << np.uint64(32) | pos << np.uint64(1) | rng.randint(0, 2, n).astype(np.uint64)
    un = rng.random_sample(n) < 0.02
    keys[un] = np.uint64(0xFFFFFFFF) << np.uint64(32)
    return keys


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, nargs="+", default=[2000000, 50000000])
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--device", type=int, default=0)
    a = ap.parse_args()
    for n in a.n:
        keys = coord_keys(n)
        got = sort_order(keys, a.device)                    # warm-up (code objects, stream) and the result that is checked
        t0 = time.perf_counter()
        want = np.argsort(keys, kind="stable")
        t_np = time.perf_counter() - t0
        assert np.array_equal(got.astype(np.int64), want), "device order differs from numpy's stable argsort"
        ts = []
        for _ in range(a.reps):
            t0 = time.perf_counter()
            sort_order(keys, a.device)
            ts.append(time.perf_counter() - t0)
        print(json.dumps({"n": n, "device_s_median": float(np.median(ts)), "device_s_min": min(ts), "device_s_max": max(ts), "reps": a.reps,
                          "numpy_stable_argsort_s": t_np}), flush=True)


if __name__ == "__main__":
    main()
