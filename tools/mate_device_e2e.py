"""`panSVR signal -D -U` four ways on a position-sorted BAM of PAIRS pairs in RAM-backed storage, stdout written to a file in the same storage:
    signal | --inflate-threads 16 | --inflate-device        the parent commit's binary (parent_bin/bin/panSVR beside its library, git-ignored)
    signal --mate-device                                    this build's: the blocks inflated, mated, judged and formatted in GPU memory
Without a parent binary the first three routes run this build's binary and the result says so (their code is the parent's unchanged).
The input is tools/inflate_bench.py's generated BAM (the input of tools/signal_device_e2e.py) with the names of every repeat made its own, put
into coordinate order by `panSVR sort`.
One discarded process, then --reps interleaved repetitions, every command in a fresh child under a time limit; the wall is the host clock
around the child.  The four files are compared byte for byte.  Median and range per route and the device route's summary line go to OUT.
With --kernel-stats FILE, afterwards one `rocprofv3 --kernel-trace --stats` run of the device route (a run of its own, no counters: tracing
slows the host), its kernel table copied to FILE.
    python tools/mate_device_e2e.py OUT.json [--pairs 1000000] [--reps 3] [--kernel-stats FILE.csv]"""
import argparse
import glob
import json
import os
import shutil
import statistics
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "tools")]
from signal_device_e2e import NEW, PARENT, LIMIT, run, sha  # noqa: E402

TAG = "signal --mate-device:"


def make_bam(path, pairs):
    """tools/inflate_bench.py's generated BAM (tests/test_signal.py's generator for 20 000 pairs, repeated) with the names of every repeat made
    its own ("pairNNNNN" -> "pRRRNNNNN"): in coordinate order the copies of a record lie side by side, and equal names there are not a
    pair's but a damaged file's, which the host loop ends on.  Returns (inflated bytes, records)."""
    import numpy as np
    import inflate_cases as ic
    import test_signal as ts
    recs, refs = ts.make_pairs(12, 20000)
    assert all(r[36:40] == b"pair" for r in recs)
    text = "@HD\tVN:1.6\tSO:queryname\n" + "".join("@SQ\tSN:%s\tLN:%d\n" % r for r in refs)
    h = b"BAM\x01" + np.int32(len(text)).tobytes() + text.encode() + np.int32(len(refs)).tobytes()
    for n, l in refs:
        h += np.int32(len(n) + 1).tobytes() + n.encode() + b"\0" + np.int32(l).tobytes()
    reps = (pairs + 19999) // 20000
    raw = h + b"".join(b"".join(r[:36] + b"p%03d" % k + r[40:] for r in recs) for k in range(reps))
    with open(path, "wb") as f:
        f.write(b"".join(ic.members_of(raw)) + ic.wrap(ic.deflate(b""), b""))
    return len(raw), len(recs) * reps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("out")
    ap.add_argument("--pairs", type=int, default=1000000)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--kernel-stats")
    a = ap.parse_args()
    old = PARENT if os.path.exists(PARENT) else NEW
    routes = [("serial", old, []), ("inflate_threads_16", old, ["--inflate-threads", "16"]), ("inflate_device", old, ["--inflate-device"]), ("mate_device", NEW, ["--mate-device"])]
    tmp = tempfile.mkdtemp(prefix="psvr_matecmd_", dir="/dev/shm" if os.path.isdir("/dev/shm") else None)
    try:
        by_name, inp = os.path.join(tmp, "name.bam"), os.path.join(tmp, "in.bam")
        raw_bytes, n_rec = make_bam(by_name, a.pairs)
        r = subprocess.run([NEW, "sort", "-t", "16", "--inflate-threads", "16", "-o", inp, by_name], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=LIMIT)
        if r.returncode != 0:
            raise SystemExit("panSVR sort: exit status %d\n%s" % (r.returncode, r.stderr.decode()[-2000:]))
        os.remove(by_name)
        print("input ready: %d bytes, %d records" % (os.path.getsize(inp), n_rec), flush=True)
        res = {"pairs": a.pairs, "records": n_rec, "inflated_bytes": raw_bytes, "reps": a.reps, "input_bytes": os.path.getsize(inp), "parent_binary": os.path.exists(PARENT),
               "flags": "-D -U", "runs": {k: [] for k, _, _ in routes}}
        out = os.path.join(tmp, "out.fq")

        def cmd(exe, flags):
            return [exe, "signal", "-D", "-U"] + flags + ["-H", os.path.join(tmp, "h.sam"), "-S", os.path.join(tmp, "s.txt"), inp]
        run(cmd(routes[0][1], routes[0][2]), out)              # the discarded first process
        digest, last_err = {}, ""
        for rep in range(a.reps):
            for name, exe, flags in routes:
                wall, err = run(cmd(exe, flags), out)
                res["runs"][name].append(round(wall, 4))
                digest.setdefault(name, sha(out))
                if name == "mate_device":
                    if "failed" in err or "refused" in err or TAG not in err:
                        raise SystemExit("--mate-device left the device route:\n" + err[-2000:])
                    last_err = err
                print(rep, name, "%.3f" % wall, flush=True)
        res["output_bytes"] = os.path.getsize(out)
        res["same_files"] = len(set(digest.values())) == 1
        res["summary"] = {k: {"median": statistics.median(v), "min": min(v), "max": max(v)} for k, v in res["runs"].items()}
        res["mate_device_line"] = [l for l in last_err.split("\n") if TAG in l][-1].split(TAG + " ", 1)[1]
        if a.kernel_stats:
            d = os.path.join(tmp, "prof")
            wall, err = run(["rocprofv3", "--kernel-trace", "--stats", "-d", d, "-o", "signal", "--output-format", "csv", "--"] + cmd(NEW, ["--mate-device"]), out)
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
        print(json.dumps(res["summary"]), res["same_files"], res["mate_device_line"])
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


if __name__ == "__main__":
    main()
