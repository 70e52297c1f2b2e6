"""The coordinate-sorted main file two ways on the bench batch written as FASTQ (bench.py's workload: 10 000 anchors, seed 11; the
reads of rank 0, seed 13): `panSVR aln` then `panSVR sort`, against `panSVR aln --sort`.  Each command runs in a child of its own;
its wall is the host clock around it and its peak memory the child's ru_maxrss (what `time -v` reports as the maximum resident set
size).  The two routes alternate `--reps` times and their files are compared byte for byte.  One JSON line.
    python tools/aln_sort_e2e.py [--pairs 1000000] [--threads 16] [--reps 2]"""
import argparse
import json
import os
import shutil
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
CLI = os.path.join(ROOT, "pansvr_amd", "bin", "panSVR")
HEADER = "@SQ\tSN:chr1\tLN:250000000\n@SQ\tSN:chr2\tLN:250000000\n"
RUN = ("import resource, subprocess, sys, time\n"
       "t = time.perf_counter(); r = subprocess.run(sys.argv[1:], stdout=subprocess.DEVNULL, stderr=subprocess.PIPE); t = time.perf_counter() - t\n"
       "sys.stderr.buffer.write(r.stderr)\n"
       "print('%d %.4f %d' % (r.returncode, t, resource.getrusage(resource.RUSAGE_CHILDREN).ru_maxrss))\n")


def run(cmd):
    """(wall s, max RSS MB, e2e_json dict or None) of one command, in a fresh child so that ru_maxrss is its own"""
    r = subprocess.run([sys.executable, "-c", RUN] + cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    rc, wall, rss = r.stdout.decode().split()
    err = r.stderr.decode()
    if int(rc) != 0:
        raise SystemExit("%s failed:\n%s" % (" ".join(cmd[:2]), err[-2000:]))
    j = [l for l in err.split("\n") if "e2e_json" in l]
    return float(wall), int(rss) / 1024.0, (json.loads(j[-1].split("e2e_json ", 1)[1]) if j else None)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=1000000)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--reps", type=int, default=2)
    ap.add_argument("--deflate-device", action="store_true")
    a = ap.parse_args()
    import bench_data
    tmp = tempfile.mkdtemp(prefix="psvr_alnsort_", dir="/dev/shm" if os.path.isdir("/dev/shm") else None)
    try:
        anc = bench_data.make_anchors(10000, seed=11)
        bench_data.write_index_dir(bench_data.build_index_cli(anc, dense=False), os.path.join(tmp, "idx"))
        bases, base_off, ori, isize = bench_data.make_reads(anc, a.pairs, seed=13)
        fq = os.path.join(tmp, "block.fq")
        bench_data.write_fastq(fq, bases, base_off, ori, isize, procs=min(16, os.cpu_count() or 1))
        del bases, base_off, ori, isize
        with open(os.path.join(tmp, "header.sam"), "w") as f:
            f.write(HEADER)
        pos = [os.path.join(tmp, "idx"), fq, os.path.join(tmp, "header.sam")]
        t = str(a.threads)
        res = {"pairs": a.pairs, "threads": a.threads, "two_step": [], "aln_sort": []}
        for _ in range(a.reps):
            for f in os.listdir(tmp):
                if f.endswith(".bam") or f.endswith(".bai"):
                    os.remove(os.path.join(tmp, f))
            o, p, s = (os.path.join(tmp, x) for x in ("o.bam", "p.bam", "s.bam"))
            w1, m1, j1 = run([CLI, "aln", "-t", t, "-o", o, "-p", p] + pos)
            w2, m2, _ = run([CLI, "sort", "-t", t, "-o", s, o])
            res["two_step"].append({"aln_wall_s": round(w1, 3), "aln_e2e_wall_s": j1["wall_s"], "aln_index_s": j1["index_s"], "sort_wall_s": round(w2, 3),
                                    "total_wall_s": round(w1 + w2, 3), "aln_max_rss_mb": round(m1), "sort_max_rss_mb": round(m2), "out_bytes": os.path.getsize(s)})
            o2, p2 = os.path.join(tmp, "o2.bam"), os.path.join(tmp, "p2.bam")
            w3, m3, j3 = run([CLI, "aln", "--sort", "-t", t, "-o", o2, "-p", p2] + pos)
            res["aln_sort"].append({"wall_s": round(w3, 3), "e2e_wall_s": j3["wall_s"], "index_s": j3["index_s"], "sort_s": j3["sort_s"], "write_s": j3["write_s"],
                                    "max_rss_mb": round(m3), "out_bytes": os.path.getsize(o2)})
            same = all(open(x, "rb").read() == open(y, "rb").read() for x, y in ((s, o2), (s + ".bai", o2 + ".bai"), (p, p2)))
            res.setdefault("identical", []).append(same)
            if a.deflate_device:
                import gzip
                o3, p3, s3 = (os.path.join(tmp, x) for x in ("o3.bam", "p3.bam", "s3.bam"))
                w4, m4, j4 = run([CLI, "aln", "--sort", "--deflate-device", "-t", t, "-o", o3, "-p", p3] + pos)
                res.setdefault("aln_sort_deflate_device", []).append({"wall_s": round(w4, 3), "e2e_wall_s": j4["wall_s"], "index_s": j4["index_s"], "sort_s": j4["sort_s"],
                                                                      "write_s": j4["write_s"], "max_rss_mb": round(m4), "out_bytes": os.path.getsize(o3)})
                w5, m5, _ = run([CLI, "sort", "--deflate-device", "-t", t, "-o", s3, o])
                res.setdefault("sort_deflate_device", []).append({"sort_wall_s": round(w5, 3), "sort_max_rss_mb": round(m5), "out_bytes": os.path.getsize(s3)})
                # the unsorted route: the same option, and the fastest host route, beside two_step's default `aln`
                for key, flags in (("aln_deflate_device", ["--deflate-device"]), ("aln_bgzf_fast", ["--bgzf-fast"])):
                    o4, p4 = os.path.join(tmp, "o4.bam"), os.path.join(tmp, "p4.bam")
                    w6, m6, j6 = run([CLI, "aln"] + flags + ["-t", t, "-o", o4, "-p", p4] + pos)
                    res.setdefault(key, []).append({"wall_s": round(w6, 3), "e2e_wall_s": j6["wall_s"], "write_s": j6["write_s"], "max_rss_mb": round(m6), "out_bytes": os.path.getsize(o4)})
                ref = gzip.open(s, "rb").read()
                res.setdefault("deflate_device_same_payload", []).append(all(gzip.open(x, "rb").read() == ref for x in (o3, s3)))
        print(json.dumps(res), flush=True)
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


if __name__ == "__main__":
    main()
