"""`panSVR aln` end to end with the record encoder on the host threads and on the device, on the bench batch written as FASTQ (bench.py's
workload: 10 000 anchors, seed 11; the reads of rank 0, seed 13) in RAM-backed storage.  The routes --deflate-device,
--parse-device --deflate-device, --emit-device --deflate-device and --stream-device, the first three with --sort, and --sort-device, run interleaved
`--reps` times (--routes: only the named ones), each command in a child of its own; wall_s, read_parse_s, engine_s, format_s and write_s come from the command's e2e_json line.  The unsorted
routes' inflated payloads are compared with the first route's, the sorted routes' files (BAM and .bai, byte for byte) with the first sorted route's.  One JSON line.
With --efforts 1,2,3 every named route also runs with `--deflate-effort N` for each N (arm <route>_effortN) and, when parent_bin/panSVR is there,
as the parent commit's binary runs it (arm <route>_parent: what this build's effort 0 is held to); those arms' files are held to the route's
inflated payload, and every arm's main file size is recorded (file_bytes).
    python tools/emit_device_e2e.py [--efforts 1,2,3] [--pairs 1000000] [--threads 16] [--reps 3] [--routes a,b,...] [--profile-dir DIR] [--profile-route emit_device]
--profile-dir: one more run of one route (--profile-route) under `rocprofv3 --kernel-trace --stats` (kernel times only, no counters), its
files left in DIR."""
import argparse
import gzip
import json
import os
import shutil
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
CLI = os.path.join(ROOT, "pansvr_amd", "bin", "panSVR")
PARENT = os.path.join(ROOT, "parent_bin", "panSVR")
HEADER = "@SQ\tSN:chr1\tLN:250000000\n@SQ\tSN:chr2\tLN:250000000\n"
ROUTES = (("deflate_device", ["--deflate-device"]), ("parse_device", ["--parse-device", "--deflate-device"]), ("emit_device", ["--emit-device", "--deflate-device"]),
          ("stream_device", ["--stream-device"]),
          ("deflate_device_sort", ["--deflate-device", "--sort"]), ("parse_device_sort", ["--parse-device", "--deflate-device", "--sort"]),
          ("emit_device_sort", ["--emit-device", "--deflate-device", "--sort"]), ("sort_device", ["--sort-device"]))
KEYS = ("wall_s", "read_parse_s", "engine_s", "format_s", "write_s", "sort_s", "sort_order_s", "sorter", "sort_device_bytes", "sort_host_bytes", "sort_records", "sort_members", "emitter", "emit_device_pairs", "emit_declined_pairs", "parser", "pieces", "streamer", "stream_device_bytes",
        "stream_host_bytes", "stream_members")


def run(cmd, timeout):
    r = subprocess.run(cmd, stdout=subprocess.DEVNULL, stderr=subprocess.PIPE, timeout=timeout)
    err = r.stderr.decode()
    if r.returncode != 0:
        raise SystemExit("%s failed (%d):\n%s" % (" ".join(cmd[:3]), r.returncode, err[-2000:]))
    j = json.loads([l for l in err.split("\n") if "e2e_json" in l][-1].split("e2e_json ", 1)[1])
    return {k: j[k] for k in KEYS}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=1000000)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--profile-dir", default=None)
    ap.add_argument("--routes", default=None)
    ap.add_argument("--profile-route", default="emit_device")
    ap.add_argument("--efforts", default="")
    a = ap.parse_args()
    # an arm: (name, the route it belongs to, its --deflate-effort or None, the binary, the route's flags)
    arms = []
    for n, f in ROUTES:
        if a.routes is not None and n not in a.routes.split(","):
            continue
        arms.append((n, n, None, CLI, f))
        if a.efforts and os.path.exists(PARENT):
            arms.append((n + "_parent", n, None, PARENT, f))
        arms += [("%s_effort%s" % (n, e), n, int(e), CLI, f + ["--deflate-effort", e]) for e in a.efforts.split(",") if e]
    import bench_data
    tmp = tempfile.mkdtemp(prefix="psvr_emit_", dir="/dev/shm" if os.path.isdir("/dev/shm") else None)
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
        res = {"pairs": a.pairs, "threads": a.threads, "fastq_bytes": os.path.getsize(fq)}
        print("data ready", file=sys.stderr, flush=True)
        ref = ref_sorted = None
        base_payload = {}
        for rep in range(a.reps):
            for name, route, effort, exe, flags in arms:
                o, p = os.path.join(tmp, "o.bam"), os.path.join(tmp, "p.bam")
                res.setdefault(name, []).append(run([exe, "aln", "-t", str(a.threads), "-o", o, "-p", p] + flags + pos, 600))
                print(name, res[name][-1], file=sys.stderr, flush=True)
                res.setdefault("file_bytes", {})[name] = os.path.getsize(o)
                if rep > 0:
                    continue
                if effort is not None:                     # other members, the same data: held to its route's inflated payload
                    res.setdefault("same_payload_as_effort_0", []).append(gzip.open(o, "rb").read() == base_payload[route])
                    continue
                base_payload[route] = gzip.open(o, "rb").read()
                if "--sort" in flags or "--sort-device" in flags:
                    files = (open(o, "rb").read(), open(o + ".bai", "rb").read())
                    ref_sorted = files if ref_sorted is None else ref_sorted
                    res.setdefault("same_sorted_files", []).append(files == ref_sorted)
                else:
                    ref = base_payload[route] if ref is None else ref
                    res.setdefault("same_payload", []).append(base_payload[route] == ref)
        if a.profile_dir:
            os.makedirs(a.profile_dir, exist_ok=True)
            subprocess.run(["rocprofv3", "--kernel-trace", "--stats", "-d", a.profile_dir, "-o", a.profile_route, "--output-format", "csv", "--", CLI, "aln", "-t", str(a.threads),
                            "-o", os.path.join(tmp, "o.bam"), "-p", os.path.join(tmp, "p.bam")] + dict(ROUTES)[a.profile_route] + pos, stdout=subprocess.DEVNULL,
                           stderr=subprocess.DEVNULL, timeout=600, check=True)
        print(json.dumps(res), flush=True)
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


if __name__ == "__main__":
    main()
