"""`panSVR aln` with and without --ori-device on two command lines, on the bench batch (bench.py's workload: 10 000 anchors, seed 11; the reads
of rank 0, seed 13) in RAM-backed storage: the input of tools/emit_device_e2e.py (FASTQ) and of tools/bam_device_e2e.py --order position (the
same reads as a BAM, put in coordinate order by `panSVR sort` outside every timed region).  Arms:
    stream            aln --stream-device reads.fq                  stream_ori           ... --ori-device
    mate_stream       aln -D --mate-device --stream-device in.bam   mate_stream_ori      ... --ori-device
One discarded process, then --reps interleaved repetitions, every command in a fresh child under its own time limit; the wall is the host
clock around the child, format_s, engine_s, d2h_bytes and the option's own fields come from the command's e2e_json line.  The inflated
payloads of both files of an arm with the option are held to those of the arm without it.  Median and range per arm go to OUT.
    python tools/ori_device_e2e.py OUT.json [--pairs 1000000] [--threads 16] [--reps 3]"""
import argparse
import gzip
import json
import os
import shutil
import statistics
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "tools")]
from bam_device_e2e import NEW, child, write_bam  # noqa: E402
from emit_device_e2e import HEADER  # noqa: E402

KEYS = ("wall_s", "read_parse_s", "engine_s", "format_s", "write_s", "d2h_bytes", "pieces", "parser", "emitter", "streamer", "ori_emitter", "ori_device_pairs", "ori_declined_pairs",
        "ori_spliced_pairs", "resident_pieces", "text_d2h_bytes")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("out")
    ap.add_argument("--pairs", type=int, default=1000000)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--reps", type=int, default=3)
    a = ap.parse_args()
    import bench_data
    tmp = tempfile.mkdtemp(prefix="psvr_oridev_", dir="/dev/shm" if os.path.isdir("/dev/shm") else None)
    try:
        anc = bench_data.make_anchors(10000, seed=11)
        idx = os.path.join(tmp, "idx")
        bench_data.write_index_dir(bench_data.build_index_cli(anc, dense=False), idx)
        bases, base_off, ori, isize = bench_data.make_reads(anc, a.pairs, seed=13)
        fq, by_name, bam = os.path.join(tmp, "block.fq"), os.path.join(tmp, "name.bam"), os.path.join(tmp, "sorted.bam")
        procs = min(16, os.cpu_count() or 1)
        print("index and reads ready", flush=True)
        bench_data.write_fastq(fq, bases, base_off, ori, isize, procs=procs)
        print("FASTQ ready", flush=True)
        write_bam(by_name, bases, base_off, ori, isize, procs)
        del bases, base_off, ori, isize
        print("BAM ready", flush=True)
        child([NEW, "sort", "-t", str(a.threads), "-o", bam, by_name])
        os.remove(by_name)
        hdr = os.path.join(tmp, "header.sam")
        with open(hdr, "w") as f:
            f.write(HEADER)
        print("input ready: %d bytes of FASTQ, %d of BAM" % (os.path.getsize(fq), os.path.getsize(bam)), flush=True)

        def aln(tag, flags, reads, header):
            return [NEW, "aln", "-t", str(a.threads), "-o", os.path.join(tmp, tag + ".bam"), "-p", os.path.join(tmp, tag + ".ori.bam")] + flags + [idx, reads, header]
        arms = [("stream", ["--stream-device"], fq, hdr), ("stream_ori", ["--stream-device", "--ori-device"], fq, hdr),
                ("mate_stream", ["-D", "--mate-device", "--stream-device"], bam, os.path.join(tmp, "h.sam")),
                ("mate_stream_ori", ["-D", "--mate-device", "--stream-device", "--ori-device"], bam, os.path.join(tmp, "h.sam"))]
        res = {"pairs": a.pairs, "threads": a.threads, "reps": a.reps, "fastq_bytes": os.path.getsize(fq), "bam_bytes": os.path.getsize(bam), "runs": {k: [] for k, _, _, _ in arms}, "stages": {}}
        child(aln(*arms[0]))                                             # the discarded first process
        for rep in range(a.reps):
            for arm in arms:
                wall, err = child(aln(*arm))
                if "failed" in err or "refused" in err:
                    raise SystemExit("%s left a device route:\n%s" % (arm[0], err[-2000:]))
                j = json.loads([l for l in err.split("\n") if "e2e_json" in l][-1].split("e2e_json ", 1)[1])
                res["runs"][arm[0]].append(round(wall, 4))
                res["stages"].setdefault(arm[0], []).append({k: j[k] for k in KEYS if k in j})
                print(rep, arm[0], "%.3f" % wall, res["stages"][arm[0]][-1], flush=True)

        def payload(tag):
            return [gzip.open(os.path.join(tmp, tag + e), "rb").read() for e in (".bam", ".ori.bam")]
        res["same_payload"] = {k + "_ori": payload(k + "_ori") == payload(k) for k in ("stream", "mate_stream")}
        res["ori_file_bytes"] = len(payload("stream")[1])
        res["summary"] = {k: {"wall": {"median": statistics.median(v), "min": min(v), "max": max(v)}} for k, v in res["runs"].items()}
        for k, runs in res["stages"].items():
            for key in ("format_s", "engine_s", "read_parse_s", "d2h_bytes", "text_d2h_bytes", "resident_pieces", "pieces"):
                v = [r[key] for r in runs if key in r]
                if v:
                    res["summary"][k][key] = {"median": statistics.median(v), "min": min(v), "max": max(v)}
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1, sort_keys=True)
            f.write("\n")
        print(json.dumps(res["summary"]), res["same_payload"], res["ori_file_bytes"])
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


if __name__ == "__main__":
    main()
