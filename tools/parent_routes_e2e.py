"""The device-resident routes of this build against the parent commit's (parent_bin/panSVR, git-ignored, with its own engine library beside it), on the
1 M-pair bench batch as tools/sort_cmd_device_e2e.py prepares it (10 000 anchors, seed 11; reads seed 13; RAM-backed storage, -t 16):
    sort --sort-device | aln --sort-device | aln --stream-device
and the signal step's device routes on the same reads as tools/bam_device_e2e.py writes them into a BAM (name order, and coordinate order by
`panSVR sort`; -D as there: every read keeps its original alignment, so the filter would pass next to nothing):
    signal -N --signal-device | signal --mate-device | aln -N --bam-device --stream-device | aln --mate-device --stream-device
--routes a,b,... runs only the named rows (and prepares only what they read).  One discarded process, then --reps repetitions in which the two builds alternate on every route, every command in a fresh child under a time
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


def run(cmd, traced=False, stdout=None):
    """the wall of one fresh child; stdout: the file its standard output goes to"""
    t = time.perf_counter()
    with open(stdout or os.devnull, "wb") as f:
        r = subprocess.run(cmd, stdout=f, stderr=subprocess.PIPE, timeout=LIMIT)
    t = time.perf_counter() - t
    if r.returncode != 0:
        raise SystemExit("%s: exit status %d\n%s" % (" ".join(cmd), r.returncode, r.stderr.decode()[-2000:]))
    err = r.stderr.decode()
    # (the profiler's own lines are not the command's; "Mate failed" is the position-sorted mode's note about a record, not about the route)
    if not traced and any("failed" in l and ": Mate failed, index:" not in l for l in err.split("\n")):
        raise SystemExit("%s left the device route:\n%s" % (" ".join(cmd), err[-2000:]))
    run.summary = [l[l.index("[panSVR-amd]"):] for l in err.split("\n") if "[panSVR-amd]" in l and " pairs, " in l]   # a signal route's own line
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
    ap.add_argument("--routes")
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
        fq, named, placed, sig_fq, sig_h, sig_s = (os.path.join(tmp, x) for x in ("block.fq", "named.bam", "placed.bam", "signal.fq", "signal.sam", "signal.txt"))
        inp, out, ori_out = (os.path.join(tmp, x) for x in ("in.bam", "out.bam", "ori.bam"))
        pos = [os.path.join(tmp, "idx"), fq, os.path.join(tmp, "header.sam")]
        signal = ["-D", "-H", sig_h, "-S", sig_s]
        fused = ["aln", "-t", t, "-D", "--stream-device", "-o", out, "-p", ori_out]
        routes = (("sort_sort_device", ["sort", "-t", t, "--sort-device", "-o", out, inp], (out, out + ".bai")),
                  ("aln_sort_device", ["aln", "-t", t, "--sort-device", "-o", out, "-p", ori_out] + pos, (out, out + ".bai", ori_out)),
                  ("aln_stream_device", ["aln", "-t", t, "--stream-device", "-o", out, "-p", ori_out] + pos, (out, ori_out)),
                  ("signal_signal_device", ["signal", "-N", "--signal-device"] + signal + [named], (sig_fq, sig_h, sig_s)),
                  ("signal_mate_device", ["signal", "--mate-device"] + signal + [placed], (sig_fq, sig_h, sig_s)),
                  ("aln_bam_device_stream", fused + ["-N", "--bam-device", pos[0], named, sig_h], (out, ori_out)),
                  ("aln_mate_device_stream", fused + ["--mate-device", pos[0], placed, sig_h], (out, ori_out)))
        if a.routes:
            unknown = set(a.routes.split(",")) - {r[0] for r in routes}
            if unknown:
                raise SystemExit("no such route: " + ", ".join(sorted(unknown)))
            routes = tuple(r for r in routes if r[0] in a.routes.split(","))
        reads = {x for r in routes for x in r[1]}
        if fq in reads or inp in reads:
            bench_data.write_fastq(fq, bases, base_off, ori, isize, procs=16)
            with open(os.path.join(tmp, "header.sam"), "w") as f:
                f.write(HEADER)
            run([BUILDS[1][1], "aln", "-t", t, "--deflate-device", "-o", inp, "-p", ori_out] + pos)
        if named in reads or placed in reads:
            import bam_device_e2e
            bam_device_e2e.write_bam(named, bases, base_off, ori, isize, min(16, os.cpu_count() or 1))
        if placed in reads:                                                  # coordinate order, by the command's own sort
            run([BUILDS[1][1], "sort", "-t", t, "-o", placed, named])
        del bases, base_off, ori, isize
        sizes = {os.path.basename(x): os.path.getsize(x) for x in (inp, named, placed) if os.path.exists(x)}
        print("input ready: %s" % sizes, flush=True)
        res = {"pairs": a.pairs, "threads": a.threads, "reps": a.reps, "input_bytes": sizes, "runs": {r[0]: {b[0]: [] for b in BUILDS} for r in routes}}
        run([BUILDS[0][1]] + routes[0][1])                                   # the discarded first process
        digest = {}
        for rep in range(a.reps):
            for route, args, files in routes:
                for build, exe in BUILDS[::-1] if rep & 1 else BUILDS:       # (neither build always runs behind the other)
                    for fn in (out, out + ".bai", ori_out, sig_fq, sig_h, sig_s):
                        if os.path.exists(fn):
                            os.remove(fn)
                    wall = run([exe] + args, stdout=sig_fq if args[0] == "signal" else None)
                    res["runs"][route][build].append(round(wall, 4))
                    if run.summary:
                        res.setdefault("lines", {}).setdefault(route, {}).setdefault(build, []).append(run.summary[-1])
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
