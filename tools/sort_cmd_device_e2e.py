"""`panSVR sort` four ways on the BAM that `panSVR aln --deflate-device` makes from the bench batch (as tools/aln_parent_e2e.py prepares it: 10 000
anchors, seed 11; 1 M pairs, seed 13) in RAM-backed storage, -t 16:
    sort --deflate-device | sort --inflate-device --deflate-device | sort --inflate-threads 16 --deflate-device     the parent commit's binary (parent_bin/panSVR,
                                                                                                                     git-ignored; this build's when it is absent)
    sort --sort-device                                                                                               this build's
One discarded process, then --reps interleaved repetitions, every command in a fresh child under a time limit; the wall is the host clock around
the child.  The four routes' files are compared byte for byte.  Median and range per route, the --sort-device route's own phase times and the
chain finder's counters on that file go to OUT.  With --kernel-stats DIR, afterwards one `rocprofv3 --kernel-trace --stats` run each of
`sort --sort-device` with segments of 16 KiB and of 64 KiB (runs of their own: tracing slows the host), their kernel tables copied to
DIR/kernel_stats_seg<bytes>.csv.
With --efforts 1,2,3 the same interleaved repetitions also run `sort --sort-device --deflate-effort N` for every N (this build's) and, when
parent_bin/ is there, the parent commit's `sort --sort-device` (what this build's effort 0 is held to); every route's file size is recorded
beside the size of the file plain `sort` writes with zlib's default level (one run, not timed).
    python tools/sort_cmd_device_e2e.py OUT.json [--pairs 1000000] [--reps 3] [--kernel-stats DIR] [--efforts 1,2,3]"""
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
PARENT = os.path.join(ROOT, "parent_bin", "panSVR")
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
    ap.add_argument("--efforts", default="")
    a = ap.parse_args()
    import bench_data
    old = PARENT if os.path.exists(PARENT) else NEW
    t = str(a.threads)
    routes = (("deflate_device", old, ["--deflate-device"]), ("inflate_device", old, ["--inflate-device", "--deflate-device"]),
              ("inflate_threads", old, ["--inflate-threads", t, "--deflate-device"]), ("sort_device", NEW, ["--sort-device"]))
    efforts = [int(e) for e in a.efforts.split(",") if e]
    if efforts and old == PARENT:
        routes += (("sort_device_parent", PARENT, ["--sort-device"]),)
    routes += tuple(("sort_device_effort%d" % e, NEW, ["--sort-device", "--deflate-effort", str(e)]) for e in efforts)
    tmp = tempfile.mkdtemp(prefix="psvr_sortcmd_", dir="/dev/shm" if os.path.isdir("/dev/shm") else None)
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
        res = {"pairs": a.pairs, "threads": a.threads, "reps": a.reps, "input_bytes": os.path.getsize(inp), "first_three_routes_binary": "parent" if old == PARENT else "this build",
               "runs": {k: [] for k, _, _ in routes}}
        out = os.path.join(tmp, "out.bam")
        run([old, "sort", "-t", t, "--deflate-device", "-o", out, inp])       # the discarded first process
        digest, last_err = {}, ""
        for rep in range(a.reps):
            for name, exe, flags in routes:
                for fn in (out, out + ".bai"):
                    if os.path.exists(fn):
                        os.remove(fn)
                wall, err = run([exe, "sort", "-t", t] + flags + ["-o", out, inp])
                res["runs"][name].append(round(wall, 4))
                if "effort" not in name:
                    digest.setdefault(name, (sha(out), sha(out + ".bai")))
                res.setdefault("file_bytes", {})[name] = os.path.getsize(out)
                if name.startswith("sort_device"):
                    if "failed" in err or "records kept on the device" not in err:
                        raise SystemExit("--sort-device left the device route:\n" + err[-2000:])
                    if name != "sort_device":
                        res.setdefault(name + "_phases", []).append({k: float(v) for k, v in re.findall(r"(append|order|write) ([0-9.]+) s", err)})
                        print(rep, name, "%.3f" % wall, flush=True)
                        continue
                    last_err = err
                    res.setdefault("sort_device_phases", []).append({k: float(v) for k, v in re.findall(r"(append|order|write) ([0-9.]+) s", err)})
                print(rep, name, "%.3f" % wall, flush=True)
        res["same_files"] = len(set(digest.values())) == 1
        if efforts:
            run([NEW, "sort", "-t", t, "-o", out, inp])
            res["file_bytes"]["zlib_default_level"] = os.path.getsize(out)
        res["summary"] = {k: {"median": statistics.median(v), "min": min(v), "max": max(v)} for k, v in res["runs"].items()}
        line = [l for l in last_err.split("\n") if "sort --sort-device:" in l][-1]
        res["sort_device_line"] = line.split("sort --sort-device: ", 1)[1]
        if a.kernel_stats:
            os.makedirs(a.kernel_stats, exist_ok=True)
            for seg in (16384, 65536):
                d = os.path.join(tmp, "prof%d" % seg)
                wall, err = run(["rocprofv3", "--kernel-trace", "--stats", "-d", d, "-o", "sort", "--output-format", "csv", "--", NEW, "sort", "-t", t, "--sort-device", "-o", out, inp],
                                env={"PSVR_BAM_STORE_SEG_BYTES": str(seg)})
                got = glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True)
                if not got:
                    raise SystemExit("rocprofv3 left no kernel_stats.csv under " + d)
                shutil.copy(got[0], os.path.join(a.kernel_stats, "kernel_stats_seg%d.csv" % seg))
                res.setdefault("traced_wall_s", {})[str(seg)] = round(wall, 4)
                print("traced seg", seg, flush=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1, sort_keys=True)
            f.write("\n")
        print(json.dumps(res["summary"]), res["same_files"], res["sort_device_line"])
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


if __name__ == "__main__":
    main()
