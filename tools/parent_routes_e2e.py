"""The device-resident routes of this build against the parent commit's (parent_bin/panSVR, git-ignored, with its own engine library beside it), on the
1 M-pair bench batch as tools/sort_cmd_device_e2e.py prepares it (10 000 anchors, seed 11; reads seed 13; RAM-backed storage, -t 16):
    sort --sort-device | aln --sort-device | aln --stream-device
One discarded process, then --reps repetitions in which the two builds alternate on every route, every command in a fresh child under a time
limit; the wall is the host clock around the child.  The two builds' files are compared byte for byte.  With --kernel-stats DIR, afterwards one
`rocprofv3 --kernel-trace --stats` run of each build for every route (runs of their own: tracing slows the
host); the six kernel tables go to DIR, and for the kernels named in KERNELS the new build's average is set beside the parent run's own
minimum and maximum.  A refactor's check: the new wall range overlaps the parent's, the new average lies inside the parent's spread.
    python tools/parent_routes_e2e.py OUT.json [--pairs 1000000] [--reps 3] [--kernel-stats DIR]"""
import argparse
import csv
import glob
import hashlib
import json
import os
import shutil
import statistics
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
BUILDS = (("parent", os.path.join(ROOT, "parent_bin", "panSVR")), ("new", os.path.join(ROOT, "pansvr_amd", "bin", "panSVR")))
HEADER = "@SQ\tSN:chr1\tLN:250000000\n@SQ\tSN:chr2\tLN:250000000\n"
KERNELS = ("k_store_count", "k_store_fill", "k_store_copy", "k_store_gather", "k_chain_guess", "k_chain_settle", "k_bs_append", "k_be_size", "k_be_write")
LIMIT = 180                                                # seconds per command: a run takes a few


def sha(fn):
    return hashlib.sha256(open(fn, "rb").read()).hexdigest()


def run(cmd, traced=False):
    t = time.perf_counter()
    r = subprocess.run(cmd, stdout=subprocess.DEVNULL, stderr=subprocess.PIPE, timeout=LIMIT)
    t = time.perf_counter() - t
    if r.returncode != 0:
        raise SystemExit("%s: exit status %d\n%s" % (" ".join(cmd), r.returncode, r.stderr.decode()[-2000:]))
    err = r.stderr.decode()
    if "failed" in err and not traced:                     # (the profiler's own lines are not the command's)
        raise SystemExit("%s left the device route:\n%s" % (" ".join(cmd), err[-2000:]))
    return t


def kernel_table(fn):
    return {row["Name"].split("(")[0].split("::")[-1]: row for row in csv.DictReader(open(fn))}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("out")
    ap.add_argument("--pairs", type=int, default=1000000)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--kernel-stats")
    a = ap.parse_args()
    for name, exe in BUILDS:
        if not os.path.exists(exe):
            raise SystemExit("no %s build at %s" % (name, exe))
    import bench_data
    t = str(a.threads)
    tmp = tempfile.mkdtemp(prefix="psvr_routes_", dir="/dev/shm" if os.path.isdir("/dev/shm") else None)
    try:
        anc = bench_data.make_anchors(10000, seed=11)
        bench_data.write_index_dir(bench_data.build_index_cli(anc, dense=False), os.path.join(tmp, "idx"))
        bases, base_off, ori, isize = bench_data.make_reads(anc, a.pairs, seed=13)
        fq = os.path.join(tmp, "block.fq")
        bench_data.write_fastq(fq, bases, base_off, ori, isize, procs=16)
        del bases, base_off, ori, isize
        with open(os.path.join(tmp, "header.sam"), "w") as f:
            f.write(HEADER)
        inp, out, ori_out = (os.path.join(tmp, x) for x in ("in.bam", "out.bam", "ori.bam"))
        pos = [os.path.join(tmp, "idx"), fq, os.path.join(tmp, "header.sam")]
        run([BUILDS[1][1], "aln", "-t", t, "--deflate-device", "-o", inp, "-p", ori_out] + pos)
        print("input ready: %d bytes" % os.path.getsize(inp), flush=True)
        routes = (("sort_sort_device", ["sort", "-t", t, "--sort-device", "-o", out, inp], (out, out + ".bai")),
                  ("aln_sort_device", ["aln", "-t", t, "--sort-device", "-o", out, "-p", ori_out] + pos, (out, out + ".bai", ori_out)),
                  ("aln_stream_device", ["aln", "-t", t, "--stream-device", "-o", out, "-p", ori_out] + pos, (out, ori_out)))
        res = {"pairs": a.pairs, "threads": a.threads, "reps": a.reps, "input_bytes": os.path.getsize(inp), "runs": {r[0]: {b[0]: [] for b in BUILDS} for r in routes}}
        run([BUILDS[0][1]] + routes[0][1])                                   # the discarded first process
        digest = {}
        for rep in range(a.reps):
            for route, args, files in routes:
                for build, exe in BUILDS:
                    for fn in (out, out + ".bai", ori_out):
                        if os.path.exists(fn):
                            os.remove(fn)
                    wall = run([exe] + args)
                    res["runs"][route][build].append(round(wall, 4))
                    digest.setdefault(route, set()).add(tuple(sha(fn) for fn in files))
                    print(rep, route, build, "%.3f" % wall, flush=True)
        res["same_files"] = {route: len(d) == 1 for route, d in digest.items()}
        res["summary"] = {route: {b: {"median": statistics.median(v), "min": min(v), "max": max(v)} for b, v in runs.items()} for route, runs in res["runs"].items()}
        res["ranges_overlap"] = {route: s["new"]["min"] <= s["parent"]["max"] and s["parent"]["min"] <= s["new"]["max"] for route, s in res["summary"].items()}
        if a.kernel_stats:
            os.makedirs(a.kernel_stats, exist_ok=True)
            res["kernels"] = {}
            for route, args, _ in routes:
                tables = {}
                for build, exe in BUILDS:
                    d = os.path.join(tmp, "prof_%s_%s" % (route, build))
                    run(["rocprofv3", "--kernel-trace", "--stats", "-d", d, "-o", "run", "--output-format", "csv", "--", exe] + args, traced=True)
                    got = glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True)
                    if not got:
                        raise SystemExit("rocprofv3 left no kernel_stats.csv under " + d)
                    dst = os.path.join(a.kernel_stats, "kernel_stats_%s_%s.csv" % (route, build))
                    shutil.copy(got[0], dst)
                    tables[build] = kernel_table(dst)
                    print("traced", route, build, flush=True)
                rows = {}
                for k in KERNELS:
                    p, n = tables["parent"].get(k), tables["new"].get(k)
                    if p and n:
                        rows[k] = {"calls": [int(p["Calls"]), int(n["Calls"])], "parent_avg_ns": round(float(p["AverageNs"])), "parent_min_ns": int(p["MinNs"]), "parent_max_ns": int(p["MaxNs"]),
                                   "new_avg_ns": round(float(n["AverageNs"])), "new_min_ns": int(n["MinNs"]), "new_max_ns": int(n["MaxNs"]),
                                   "inside_parent_spread": int(p["MinNs"]) <= float(n["AverageNs"]) <= int(p["MaxNs"])}
                res["kernels"][route] = rows
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1, sort_keys=True)
            f.write("\n")
        print(json.dumps(res["summary"]), res["same_files"], res["ranges_overlap"], json.dumps(res.get("kernels")))
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


if __name__ == "__main__":
    main()
