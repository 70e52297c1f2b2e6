"""`panSVR signal -N -D -U` four ways on a name-sorted BAM of PAIRS pairs in RAM-backed storage, stdout written to a file in the same storage:
    signal -N | --inflate-threads 16 | --inflate-device        the parent commit's binary (parent_bin/bin/panSVR beside its library, git-ignored)
    signal -N --signal-device                                   this build's: the records inflated, paired, judged and formatted in GPU memory
Without a parent binary the first three routes run this build's binary and the result says so (their code is the parent's unchanged).
The input is tools/inflate_bench.py's generated BAM (tests/test_signal.py's generator for 20 000 pairs, repeated: about 2.2 records per pair,
the input of DESIGN.md section 4 (5)'s figures).  `aln`'s own output cannot serve: its second reads do not carry flag 0x80, and `signal -N`
ends at the first pair of such a file on every route.
One discarded process, then --reps interleaved repetitions, every command in a fresh child under a time limit; the wall is the host clock
around the child.  The four files are compared byte for byte.  Median and range per route and the device route's statistics line go to OUT.
With --kernel-stats FILE, afterwards one `rocprofv3 --kernel-trace --stats` run of the device route (a run of its own, no counters: tracing
slows the host), its kernel table copied to FILE.
    python tools/signal_device_e2e.py OUT.json [--pairs 1000000] [--reps 3] [--kernel-stats FILE.csv]"""
import argparse
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
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "tools")]
NEW = os.path.join(ROOT, "pansvr_amd", "bin", "panSVR")
PARENT = os.path.join(ROOT, "parent_bin", "bin", "panSVR")
LIMIT = 300                                                # seconds per command: a run takes a few


def sha(fn):
    h = hashlib.sha256()
    with open(fn, "rb") as f:
        for b in iter(lambda: f.read(1 << 24), b""):
            h.update(b)
    return h.hexdigest()


def run(cmd, out):
    env = dict(os.environ)
    env.pop("PSVR_INFLATE_BATCH", None)
    t = time.perf_counter()
    with open(out, "wb") as f:
        r = subprocess.run(cmd, stdout=f, stderr=subprocess.PIPE, timeout=LIMIT, env=env)
    t = time.perf_counter() - t
    if r.returncode != 0:
        raise SystemExit("%s: exit status %d\n%s" % (" ".join(cmd), r.returncode, r.stderr.decode()[-2000:]))
    return t, r.stderr.decode(errors="replace")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("out")
    ap.add_argument("--pairs", type=int, default=1000000)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--kernel-stats")
    a = ap.parse_args()
    import inflate_bench
    old = PARENT if os.path.exists(PARENT) else NEW
    routes = [("serial", old, []), ("inflate_threads_16", old, ["--inflate-threads", "16"]), ("inflate_device", old, ["--inflate-device"]), ("signal_device", NEW, ["--signal-device"])]
    tmp = tempfile.mkdtemp(prefix="psvr_signalcmd_", dir="/dev/shm" if os.path.isdir("/dev/shm") else None)
    try:
        inp = os.path.join(tmp, "in.bam")
        raw_bytes, n_rec = inflate_bench.make_bam(inp, a.pairs)
        print("input ready: %d bytes, %d records" % (os.path.getsize(inp), n_rec), flush=True)
        res = {"pairs": a.pairs, "records": n_rec, "inflated_bytes": raw_bytes, "reps": a.reps, "input_bytes": os.path.getsize(inp), "parent_binary": os.path.exists(PARENT),
               "flags": "-N -D -U", "runs": {k: [] for k, _, _ in routes}}
        out = os.path.join(tmp, "out.fq")

        def cmd(exe, flags):
            return [exe, "signal", "-N", "-D", "-U"] + flags + ["-H", os.path.join(tmp, "h.sam"), "-S", os.path.join(tmp, "s.txt"), inp]
        run(cmd(routes[0][1], routes[0][2]), out)              # the discarded first process
        digest, last_err = {}, ""
        for rep in range(a.reps):
            for name, exe, flags in routes:
                wall, err = run(cmd(exe, flags), out)
                res["runs"][name].append(round(wall, 4))
                digest.setdefault(name, sha(out))
                if name == "signal_device":
                    if "failed" in err or "refused" in err or "signal --signal-device:" not in err:
                        raise SystemExit("--signal-device left the device route:\n" + err[-2000:])
                    last_err = err
                print(rep, name, "%.3f" % wall, flush=True)
        res["output_bytes"] = os.path.getsize(out)
        res["same_files"] = len(set(digest.values())) == 1
        res["summary"] = {k: {"median": statistics.median(v), "min": min(v), "max": max(v)} for k, v in res["runs"].items()}
        res["signal_device_line"] = [l for l in last_err.split("\n") if "signal --signal-device:" in l][-1].split("signal --signal-device: ", 1)[1]
        if a.kernel_stats:
            d = os.path.join(tmp, "prof")
            wall, err = run(["rocprofv3", "--kernel-trace", "--stats", "-d", d, "-o", "signal", "--output-format", "csv", "--"] + cmd(NEW, ["--signal-device"]), out)
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
        print(json.dumps(res["summary"]), res["same_files"], res["signal_device_line"])
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


if __name__ == "__main__":
    main()
