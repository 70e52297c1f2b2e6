#!/usr/bin/env python3
"""Regenerates tests/golden/prefix_sha256.json: the length and SHA-256 of both SAM files the REFERENCE's `fc_aln` objects
(oracle/_ref/ref_aln -t 1 -S) write for the prefixes that tests/test_stream_gpu.py and tests/test_cfg3_gpu.py compare the command's
output with -- too large to store, so their bytes are pinned by digest.  BUILD CONTAINER ONLY; needs the built CLI and oracle/_ref."""
import hashlib
import json
import os
import shutil
import subprocess
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path[:0] = [ROOT, os.path.dirname(HERE)]
import test_cfg3_gpu as tc  # noqa: E402
import test_stream_gpu as ts  # noqa: E402

REF = os.path.join(ROOT, "oracle", "_ref", "ref_aln")


def digest(data):
    return {"bytes": len(data), "sha256": hashlib.sha256(data).hexdigest()}


def body_of(data):
    """A SAM file without its header lines."""
    at = 0
    while data[at:at + 1] == b"@":
        at = data.index(b"\n", at) + 1
    return data[at:]


def ref_aln(args, tmp):
    subprocess.run([REF, "-t", "1", "-S", "-o", os.path.join(tmp, "ref.sam"), "-p", os.path.join(tmp, "ref.ori.sam")] + args + ["--quiet"],
                   stdout=subprocess.DEVNULL, check=True)
    return {ext: open(os.path.join(tmp, "ref" + ext), "rb").read() for ext in (".sam", ".ori.sam")}


def main():
    shm = "/dev/shm" if os.path.isdir("/dev/shm") else None
    out = {}
    # test_stream_gpu: the first PREFIX pairs of its input (all within the first part), whole files with their header lines
    tmp = tempfile.mkdtemp(prefix="psvr_prefixg_", dir=shm)
    try:
        base = ts.write_inputs(tmp, 1, dense=True)
        files = ref_aln(["-R", str(ts.PREFIX)] + base, tmp)
        out["stream"] = dict({"pairs": ts.PREFIX}, **{ext: digest(d) for ext, d in files.items()})
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
    # test_cfg3_gpu: the first PREFIX pairs generated on their own, the files' bodies
    tmp = tempfile.mkdtemp(prefix="psvr_prefixg_", dir=shm)
    try:
        t = tc.build_tools()
        idx, hdr = tc.write_index(t, tmp)
        pre = os.path.join(tmp, "prefix.fq")
        with open(pre, "wb") as f:
            subprocess.check_call([t["gen_signal_fastq"], "reads", str(tc.N_ANCHORS), str(tc.ANCHOR_SEED), str(tc.PREFIX), str(tc.READ_SEED), "8"], stdout=f)
        files = ref_aln([idx, pre, hdr], tmp)
        out["cfg3"] = dict({"pairs": tc.PREFIX}, **{ext: digest(body_of(d)) for ext, d in files.items()})
        shutil.rmtree(os.path.dirname(t["sam_check"]), ignore_errors=True)
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
    with open(os.path.join(HERE, "prefix_sha256.json"), "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
