"""`panSVR aln` of this tree against the parent commit's build of the command (parent_bin/panSVR, git-ignored: the parent's cli_main.cpp
compiled against the same library) on the bench batch written as FASTQ (as tools/emit_device_e2e.py prepares it) in RAM-backed storage,
-t 16: -S, default BAM and --deflate-device, parent and new alternately, five runs each, every command in a fresh child under a time
limit; wall_s and the stage times come from the e2e_json line, the two files of each mode's first run are compared.  The raw runs and,
per mode, the medians and whether the new median wall_s is within the parent's median + the parent's own spread (max - min) go to OUT.
    python tools/aln_parent_e2e.py OUT.json"""
import hashlib
import json
import os
import shutil
import statistics
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
BIN = {"parent": os.path.join(ROOT, "parent_bin", "panSVR"), "new": os.path.join(ROOT, "pansvr_amd", "bin", "panSVR")}
MODES = (("sam", ["-S"]), ("bam", []), ("deflate_device", ["--deflate-device"]))
KEYS = ("wall_s", "read_parse_s", "engine_s", "format_s", "write_s", "pieces", "batches", "pairs")
HEADER = "@SQ\tSN:chr1\tLN:250000000\n@SQ\tSN:chr2\tLN:250000000\n"
PAIRS, THREADS, REPS = 1000000, 16, 5
import bench_data
tmp = tempfile.mkdtemp(prefix="psvr_e2e_", dir="/dev/shm" if os.path.isdir("/dev/shm") else None)
try:
    anc = bench_data.make_anchors(10000, seed=11)
    bench_data.write_index_dir(bench_data.build_index_cli(anc, dense=False), os.path.join(tmp, "idx"))
    bases, base_off, ori, isize = bench_data.make_reads(anc, PAIRS, seed=13)
    fq = os.path.join(tmp, "block.fq")
    bench_data.write_fastq(fq, bases, base_off, ori, isize, procs=16)
    del bases, base_off, ori, isize
    with open(os.path.join(tmp, "header.sam"), "w") as f:
        f.write(HEADER)
    pos = [os.path.join(tmp, "idx"), fq, os.path.join(tmp, "header.sam")]
    print("data ready", flush=True)
    res = {"pairs": PAIRS, "threads": THREADS, "reps": REPS, "runs": {}, "same_output": {}}
    for mode, flags in MODES:
        digest = {}
        for rep in range(REPS):
            for tag in ("parent", "new"):
                o, p = os.path.join(tmp, "o.out"), os.path.join(tmp, "p.out")
                r = subprocess.run([BIN[tag], "aln", "-t", str(THREADS), "-o", o, "-p", p] + flags + pos, stdout=subprocess.DEVNULL, stderr=subprocess.PIPE, timeout=120)
                err = r.stderr.decode()
                if r.returncode != 0:
                    print(tag, mode, "exit status", r.returncode, err[-2000:], flush=True)
                    sys.exit(r.returncode if r.returncode > 0 else 1)
                j = json.loads([l for l in err.split("\n") if "e2e_json" in l][-1].split("e2e_json ", 1)[1])
                res["runs"].setdefault(mode, {}).setdefault(tag, []).append({k: j[k] for k in KEYS})
                if rep == 0:
                    digest[tag] = [hashlib.sha256(open(f, "rb").read()).hexdigest() for f in (o, p)]
                print(mode, tag, res["runs"][mode][tag][-1], flush=True)
        res["same_output"][mode] = digest["parent"] == digest["new"]
    res["summary"] = {}
    for mode, _ in MODES:
        w = {t: [x["wall_s"] for x in res["runs"][mode][t]] for t in BIN}
        res["summary"][mode] = {"parent_median_wall_s": statistics.median(w["parent"]), "new_median_wall_s": statistics.median(w["new"]), "parent_spread_s": max(w["parent"]) - min(w["parent"]),
                                "within": statistics.median(w["new"]) <= statistics.median(w["parent"]) + max(w["parent"]) - min(w["parent"])}
        for k in ("read_parse_s", "engine_s", "format_s", "write_s"):
            for t in BIN:
                res["summary"][mode]["%s_median_%s" % (t, k)] = statistics.median(x[k] for x in res["runs"][mode][t])
    with open(sys.argv[1], "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res["summary"], indent=1), json.dumps(res["same_output"]), flush=True)
finally:
    shutil.rmtree(tmp, ignore_errors=True)
