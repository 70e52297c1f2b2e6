"""`panSVR aln` on a BAM end to end -- by default `aln -N` on a name-sorted one, the host fused routes against `--bam-device`, on the bench batch (bench.py's workload: 10 000
anchors, seed 11; the reads of rank 0, seed 13) written as a BAM by tests/test_fused_signal.py's rule -- every read keeps its original
alignment, second reads carry 0x80 -- once, outside any timed region, into RAM-backed storage.  Routes:
    parent_serial, parent_threads16     aln -N -D in.bam --deflate-device [--inflate-threads 16]        the parent commit's binary
    parent_two_steps                    signal -N -D --signal-device > fq, then aln --stream-device fq   the parent's; the sum of the two walls
    parent_sort                         aln -N -D --sort --deflate-device in.bam                         the parent's
    bam_device, bam_device_stream, bam_device_sort       --bam-device with --deflate-device | --stream-device | --sort-device    this build's
The parent's binary is parent_bin/bin/panSVR beside its library (git-ignored); without it the tool refuses: a build is never its own baseline.
One discarded process, then --reps interleaved repetitions, every command in a fresh child under its own time limit; the wall is the host
clock around the child (for two steps: the sum), the stage times come from the command's e2e_json line.  The files of corresponding routes
are compared byte for byte (the unsorted routes by their inflated payloads: the member cuts differ between the host writer and the stream).
    python tools/bam_device_e2e.py OUT.json [--pairs 1000000] [--threads 16] [--reps 3] [--kernel-stats FILE.csv] [--order position]
--order position: the same for `panSVR aln` without -N and `--mate-device`.  The BAM is put in coordinate order by `panSVR sort` outside every
timed region; the parent's two steps are signal -D --mate-device > fq, then aln --stream-device fq; the new routes are mate_device,
mate_device_stream and mate_device_sort.  One further run of each new route at --block-records 8192 reports the blocks, the windows offered
and the pieces (many small blocks put together into few windows)."""
import argparse
import glob
import gzip
import json
import os
import shutil
import statistics
import struct
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
NEW = os.path.join(ROOT, "pansvr_amd", "bin", "panSVR")
PARENT = os.path.join(ROOT, "parent_bin", "bin", "panSVR")
LIMIT = 300
KEYS = ("wall_s", "read_parse_s", "engine_s", "format_s", "write_s", "sort_s", "parser", "emitter", "streamer", "sorter", "pieces")
REFS = [("chr1", 250000000), ("chr2", 250000000)]
COMP = bytes.maketrans(b"ACGTNacgtn", b"TGCANtgcan")


def _records(args):
    """the BAM records of pairs [p0, p1): bam_of's rule on bench_data's fields (its FASTQ comment says the same)"""
    bases, base_off, ori, isize, p0, p1 = args
    out = []
    cigar = struct.pack("<II", 40 << 4 | 4, 110 << 4 | 0)
    for p in range(p0, p1):
        name = b"r%07d\0" % p
        for k in range(2):
            r = 2 * p + k
            o, mate = ori[r], ori[2 * p + 1 - k]
            fw = bool(o["direction"])
            flag = (0x40 if k == 0 else 0x80) | 0x1 | (0 if fw else 0x10) | (0x20 if fw else 0)
            s = bases[base_off[r]:base_off[r + 1]].tobytes().upper()
            if not fw:                                                   # BAM stores the reference strand
                s = s.translate(COMP)[::-1]
            codes = s.translate(bytes.maketrans(b"ACGTN", bytes([1, 2, 4, 8, 15])))
            if len(codes) & 1:
                codes += b"\0"
            s4 = bytes(a << 4 | b for a, b in zip(codes[0::2], codes[1::2]))
            tid = int(o["chr_id"])
            body = struct.pack("<iiBBHHHiiii", tid if tid <= 24 else 29, int(o["ref_bg"]), len(name), 20, 0, 2, flag, len(s), 0, int(mate["ref_bg"]), int(isize[p]) if fw else -int(isize[p]))
            body += name + cigar + s4 + bytes([40]) * len(s) + b"NMi" + struct.pack("<i", 3)
            out.append(struct.pack("<i", len(body)) + body)
    return b"".join(out)


def write_bam(path, bases, base_off, ori, isize, procs):
    import multiprocessing as mp
    import test_signal as ts
    P = (len(base_off) - 1) // 2
    n = max(1, min(procs, P // 20000 + 1))
    jobs = [(bases, base_off, ori, isize, P * i // n, P * (i + 1) // n) for i in range(n)]
    with mp.get_context("fork").Pool(n) as pool:
        parts = pool.map(_records, jobs)
    text = "@HD\tVN:1.6\tSO:queryname\n" + "".join("@SQ\tSN:%s\tLN:%d\n" % r for r in REFS)
    h = b"BAM\x01" + struct.pack("<i", len(text)) + text.encode() + struct.pack("<i", len(REFS))
    for name, length in REFS:
        h += struct.pack("<i", len(name) + 1) + name.encode() + b"\0" + struct.pack("<i", length)
    data = h + b"".join(parts)
    del parts
    cuts = list(range(0, len(data), 0xff00 * 256))
    with mp.get_context("fork").Pool(n) as pool:
        blobs = pool.map(_members, [data[c:c + 0xff00 * 256] for c in cuts])
    with open(path, "wb") as f:
        for b in blobs:
            f.write(b)
        f.write(ts.bgzf(b""))                                            # the end-of-file member
    return len(data)


def _members(data):
    import test_signal as ts
    return ts.bgzf(data)[:-28]                                           # (without the end-of-file member)


def child(cmd, stdout=None):
    env = dict(os.environ)
    env.pop("PSVR_INFLATE_BATCH", None)
    t = time.perf_counter()
    r = subprocess.run(cmd, stdout=stdout or subprocess.DEVNULL, stderr=subprocess.PIPE, timeout=LIMIT, env=env)
    t = time.perf_counter() - t
    err = r.stderr.decode(errors="replace")
    if r.returncode != 0:
        raise SystemExit("%s: exit status %d\n%s" % (" ".join(cmd), r.returncode, err[-2000:]))
    return t, err


def stages(err):
    lines = [l for l in err.split("\n") if "e2e_json" in l]
    j = json.loads(lines[-1].split("e2e_json ", 1)[1]) if lines else {}
    return {k: j[k] for k in KEYS if k in j}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("out")
    ap.add_argument("--pairs", type=int, default=1000000)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--kernel-stats")
    ap.add_argument("--order", choices=("name", "position"), default="name")
    a = ap.parse_args()
    if not os.path.exists(PARENT):
        raise SystemExit("no parent binary at %s: the build under test is never its own baseline" % PARENT)
    import bench_data
    tmp = tempfile.mkdtemp(prefix="psvr_bamdev_", dir="/dev/shm" if os.path.isdir("/dev/shm") else None)
    try:
        anc = bench_data.make_anchors(10000, seed=11)
        bench_data.write_index_dir(bench_data.build_index_cli(anc, dense=False), os.path.join(tmp, "idx"))
        bases, base_off, ori, isize = bench_data.make_reads(anc, a.pairs, seed=13)
        inp = os.path.join(tmp, "in.bam")
        raw = write_bam(inp, bases, base_off, ori, isize, min(16, os.cpu_count() or 1))
        del bases, base_off, ori, isize
        pos = a.order == "position"
        option, key, sig = ("--mate-device", "mate_device", ("-D",)) if pos else ("--bam-device", "bam_device", ("-N", "-D"))
        if pos:                                                          # coordinate order, by the command's own sort
            child([NEW, "sort", "-t", str(a.threads), "-o", os.path.join(tmp, "sorted.bam"), inp])
            os.remove(inp)
            inp = os.path.join(tmp, "sorted.bam")
        print("input ready: %d bytes (%d inflated)" % (os.path.getsize(inp), raw), flush=True)
        idx, hdr, t = os.path.join(tmp, "idx"), os.path.join(tmp, "h.sam"), ["-t", str(a.threads)]

        def aln(exe, tag, flags, reads=inp, signal_flags=sig):
            return [exe, "aln"] + t + list(signal_flags) + ["-o", os.path.join(tmp, tag + ".bam"), "-p", os.path.join(tmp, tag + ".ori.bam")] + flags + [idx, reads, hdr]

        def two_steps(tag):
            fq = os.path.join(tmp, "two.fq")
            with open(fq, "wb") as f:
                w1, _ = child([PARENT, "signal"] + list(sig) + ["--mate-device" if pos else "--signal-device", "-H", os.path.join(tmp, "h2.sam"), "-S", os.path.join(tmp, "s2.txt"), inp], f)
            hdr2 = os.path.join(tmp, "h2.sam")
            w2, err = child([PARENT, "aln"] + t + ["-o", os.path.join(tmp, tag + ".bam"), "-p", os.path.join(tmp, tag + ".ori.bam"), "--stream-device", idx, fq, hdr2])
            return w1 + w2, err, {"signal_wall_s": round(w1, 4), "aln_wall_s": round(w2, 4)}

        routes = [("parent_serial", lambda: child(aln(PARENT, "parent_serial", ["--deflate-device"]))),
                  ("parent_threads16", lambda: child(aln(PARENT, "parent_threads16", ["--deflate-device", "--inflate-threads", "16"]))),
                  ("parent_two_steps", lambda: two_steps("parent_two_steps")),
                  ("parent_sort", lambda: child(aln(PARENT, "parent_sort", ["--sort", "--deflate-device"]))),
                  (key, lambda: child(aln(NEW, key, [option, "--deflate-device"]))),
                  (key + "_stream", lambda: child(aln(NEW, key + "_stream", [option, "--stream-device"]))),
                  (key + "_sort", lambda: child(aln(NEW, key + "_sort", [option, "--sort-device"])))]
        res = {"order": a.order, "pairs": a.pairs, "threads": a.threads, "reps": a.reps, "input_bytes": os.path.getsize(inp), "inflated_bytes": raw, "runs": {k: [] for k, _ in routes}, "stages": {}, "lines": {}}
        def route_line(err):
            """the device route's summary line; a route that was left or refused ends the measurement"""
            line = [l for l in err.split("\n") if "aln %s:" % option in l]
            if not line or " failed (" in line[-1] or "refused" in line[-1]:
                raise SystemExit("%s left the device route:\n" % option + err[-2000:])
            return line[-1].split("aln %s: " % option, 1)[1]

        routes[0][1]()                                                   # the discarded first process
        for rep in range(a.reps):
            for name, fn in routes:
                got = fn()
                res["runs"][name].append(round(got[0], 4))
                res["stages"].setdefault(name, []).append(dict(stages(got[1]), **(got[2] if len(got) > 2 else {})))
                if name.startswith(key):
                    res["lines"][name] = route_line(got[1])
                print(rep, name, "%.3f" % got[0], flush=True)

        def payload(tag, ext):
            return gzip.open(os.path.join(tmp, tag + ext), "rb").read()
        ref = [payload("parent_serial", e) for e in (".bam", ".ori.bam")]
        res["same_payload"] = {k: [payload(k, e) for e in (".bam", ".ori.bam")] == ref for k in ("parent_threads16", "parent_two_steps", key, key + "_stream")}
        del ref
        res["same_sorted_files"] = all(open(os.path.join(tmp, key + "_sort" + e), "rb").read() == open(os.path.join(tmp, "parent_sort" + e), "rb").read() for e in (".bam", ".bam.bai", ".ori.bam"))
        res["summary"] = {k: {"median": statistics.median(v), "min": min(v), "max": max(v)} for k, v in res["runs"].items()}
        if pos:                                                          # many small blocks: what becomes of them
            res["block_records_8192"] = {}
            for name, flags in ((key, ["--deflate-device"]), (key + "_stream", ["--stream-device"]), (key + "_sort", ["--sort-device"])):
                wall, err = child(aln(NEW, name + "_8192", [option, "--block-records", "8192"] + flags))
                line = route_line(err)
                w = line.replace(",", "").split()
                res["block_records_8192"][name] = {"wall_s": round(wall, 4), "blocks": int(w[w.index("blocks") - 1]), "windows": int(w[w.index("windows") - 1]),
                                                   "pieces": stages(err).get("pieces"), "line": line}
                print("8192", name, "%.3f" % wall, flush=True)
        if a.kernel_stats:
            d = os.path.join(tmp, "prof")
            wall, _ = child(["rocprofv3", "--kernel-trace", "--stats", "-d", d, "-o", "bamdev", "--output-format", "csv", "--"] + aln(NEW, "traced", [option, "--stream-device"]))
            found = glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True)
            if not found:
                raise SystemExit("rocprofv3 left no kernel_stats.csv under " + d)
            os.makedirs(os.path.dirname(os.path.abspath(a.kernel_stats)), exist_ok=True)
            shutil.copy(found[0], a.kernel_stats)
            res["traced_wall_s"] = round(wall, 4)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1, sort_keys=True)
            f.write("\n")
        print(json.dumps(res["summary"]), res["same_payload"], res["same_sorted_files"])
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


if __name__ == "__main__":
    main()
