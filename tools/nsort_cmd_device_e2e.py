"""`panSVR sort` in name order four ways on the BAM that `panSVR aln --deflate-device` makes from the bench batch (as tools/sort_cmd_device_e2e.py
prepares it: 10 000 anchors, seed 11; 1 M pairs, seed 13) in RAM-backed storage, -t 16:
    sort -n --deflate-device | sort -n --inflate-threads 16 --deflate-device     the parent commit's binary (parent_bin/bin/panSVR beside its library,
                                                                                  git-ignored): the order on one host thread
    sort -n --deflate-device                                                      this build's: the order from psvr_sort_order_names
    sort --nsort-device                                                           this build's: the records kept in GPU memory
Without a parent binary the first two routes are left out and the result says so.  One discarded process, then --reps interleaved repetitions,
every command in a fresh child under a time limit; the wall is the host clock around the child.  The routes' files are compared byte for byte.
Median and range per route and the --nsort-device route's own phase times go to OUT.  With --kernel-stats FILE, afterwards one
`rocprofv3 --kernel-trace --stats` run of `sort --nsort-device` (a run of its own, no counters: tracing slows the host), its kernel table copied
to FILE.
    python tools/nsort_cmd_device_e2e.py OUT.json [--pairs 1000000] [--reps 3] [--kernel-stats FILE.csv]"""
import argparse
import glob
import hashlib
import json
import os
import re
import shutil
import statistics
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
NEW = os.path.join(ROOT, "pansvr_amd", "bin", "panSVR")
PARENT = os.path.join(ROOT, "parent_bin", "bin", "panSVR")
HEADER = "@SQ\tSN:chr1\tLN:250000000\n@SQ\tSN:chr2\tLN:250000000\n"
LIMIT = 180                                                # seconds per command: a run takes a few


def sha(fn):
    return hashlib.sha256(open(fn, "rb").read()).hexdigest()


def run(cmd, env=None):
    t = time.perf_counter()
    r = subprocess.run(cmd, stdout=subprocess.DEVNULL, stderr=subprocess.PIPE, timeout=LIMIT, env=dict(os.environ, **(env or {})))
    t = time.perf_counter() - t
    if r.returncode != 0:
        raise SystemExit("%s: exit status %d\n%s" % (" ".join(cmd), r.returncode, r.stderr.decode()[-2000:]))
    return t, r.stderr.decode()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("out")
    ap.add_argument("--pairs", type=int, default=1000000)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--kernel-stats")
    a = ap.parse_args()
    import bench_data
    t = str(a.threads)
    routes = []
    if os.path.exists(PARENT):
        routes += [("parent_n_deflate_device", PARENT, ["-n", "--deflate-device"]), ("parent_n_inflate_threads", PARENT, ["-n", "--inflate-threads", t, "--deflate-device"])]
    routes += [("n_deflate_device", NEW, ["-n", "--deflate-device"]), ("nsort_device", NEW, ["--nsort-device"])]
    tmp = tempfile.mkdtemp(prefix="psvr_nsortcmd_", dir="/dev/shm" if os.path.isdir("/dev/shm") else None)
    try:
        anc = bench_data.make_anchors(10000, seed=11)
        bench_data.write_index_dir(bench_data.build_index_cli(anc, dense=False), os.path.join(tmp, "idx"))
        bases, base_off, ori, isize = bench_data.make_reads(anc, a.pairs, seed=13)
        fq = os.path.join(tmp, "block.fq")
        bench_data.write_fastq(fq, bases, base_off, ori, isize, procs=16)
        del bases, base_off, ori, isize
        with open(os.path.join(tmp, "header.sam"), "w") as f:
            f.write(HEADER)
        inp = os.path.join(tmp, "in.bam")
        run([NEW, "aln", "-t", t, "--deflate-device", "-o", inp, "-p", os.path.join(tmp, "ori.bam"), os.path.join(tmp, "idx"), fq, os.path.join(tmp, "header.sam")])
        os.remove(fq)
        print("input ready: %d bytes" % os.path.getsize(inp), flush=True)
        res = {"pairs": a.pairs, "threads": a.threads, "reps": a.reps, "input_bytes": os.path.getsize(inp), "parent_binary": os.path.exists(PARENT), "runs": {k: [] for k, _, _ in routes}}
        out = os.path.join(tmp, "out.bam")
        run([routes[0][1], "sort", "-t", t] + routes[0][2] + ["-o", out, inp])   # the discarded first process
        digest, last_err = {}, ""
        for rep in range(a.reps):
            for name, exe, flags in routes:
                if os.path.exists(out):
                    os.remove(out)
                wall, err = run([exe, "sort", "-t", t] + flags + ["-o", out, inp])
                res["runs"][name].append(round(wall, 4))
                digest.setdefault(name, sha(out))
                if name == "n_deflate_device" and "name order, ordered on the device" not in err:
                    raise SystemExit("sort -n did not order on the device:\n" + err[-2000:])
                if name == "nsort_device":
                    if "failed" in err or "records kept on the device" not in err:
                        raise SystemExit("--nsort-device left the device route:\n" + err[-2000:])
                    last_err = err
                    res.setdefault("nsort_device_phases", []).append({k: float(v) for k, v in re.findall(r"(append|order|write) ([0-9.]+) s", err)})
                print(rep, name, "%.3f" % wall, flush=True)
        res["same_files"] = len(set(digest.values())) == 1
        res["summary"] = {k: {"median": statistics.median(v), "min": min(v), "max": max(v)} for k, v in res["runs"].items()}
        line = [l for l in last_err.split("\n") if "sort --nsort-device:" in l][-1]
        res["nsort_device_line"] = line.split("sort --nsort-device: ", 1)[1]
        if a.kernel_stats:
            d = os.path.join(tmp, "prof")
            wall, err = run(["rocprofv3", "--kernel-trace", "--stats", "-d", d, "-o", "nsort", "--output-format", "csv", "--", NEW, "sort", "-t", t, "--nsort-device", "-o", out, inp])
            got = glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True)
            if not got:
                raise SystemExit("rocprofv3 left no kernel_stats.csv under " + d)
            os.makedirs(os.path.dirname(os.path.abspath(a.kernel_stats)), exist_ok=True)
            shutil.copy(got[0], a.kernel_stats)
            res["traced_wall_s"] = round(wall, 4)
            print("traced", flush=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1, sort_keys=True)
            f.write("\n")
        print(json.dumps(res["summary"]), res["same_files"], res["nsort_device_line"])
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


if __name__ == "__main__":
    main()
