"""`panSVR aln --ori-device` in the pipeline, without a GPU: the PRODUCT's pansvr_amd/csrc/aln_pipeline.h over the emulated engine with a driver
whose two encoders are the host builds of the device rules (tests/tools/aln_ori_pipeline_check.cpp).  Both files must be the plain
pipeline's; a piece of which neither encoder declined a pair must stay resident (its results not downloaded, its poisoned text never
fetched or read), every other piece must be fetched and downloaded; --records fetches everything; a failing ori call falls back with its
one line and identical files."""
import gzip
import json
import os
import subprocess
import tempfile

import pytest

import aln_common as ac
import test_aln_pipeline as tap
from test_bam_emit_gpu import _with_tabs

SRC = os.path.join(ac.HERE, "tools", "aln_ori_pipeline_check.cpp")
FAIL_LINE = "[panSVR-amd] ori BAM records on the device failed (injected failure of the ori encode): formatting the second file on the host threads from here on"


@pytest.fixture(scope="module")
def checker():
    tmp = tempfile.mkdtemp(prefix="psvr_aoc_")
    exe = os.path.join(tmp, "aln_ori_pipeline_check")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-DPSVR_EMU_SPARSE_HASH", "-DPSVR_NO_ENGINE_LIB", "-Wall", "-Wno-unused-variable", "-Wno-maybe-uninitialized", "-o", exe, SRC, tap.KSW,
                           "-lz", "-lpthread"])
    return exe


def run(exe, fq, args):
    """(stderr, the counters of the last line, the inflated payload of both files)"""
    w = ac.workdir("fx1")
    tmp = tempfile.mkdtemp(prefix="psvr_aoc_")
    fn = [os.path.join(tmp, f) for f in ("o.bam", "p.bam")]
    r = subprocess.run([exe, "-t", "4", "-o", fn[0], "-p", fn[1]] + list(args) + [ac.index_dir("fx1"), fq, os.path.join(w, "header.sam")], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600)
    err = r.stderr.decode()
    assert r.returncode == 0, "aln_ori_pipeline_check %s: exit status %d\n%s" % (" ".join(args), r.returncode, err[-3000:])
    last = err.strip().split("\n")[-1].split()
    assert last[0] == "ori_pipeline"
    return err, {last[i]: int(last[i + 1]) for i in range(1, len(last), 2)}, [gzip.decompress(open(f, "rb").read()) for f in fn]


@pytest.fixture(scope="module")
def reads():
    return os.path.join(ac.workdir("fx1"), "reads150.fq")


@pytest.fixture(scope="module")
def tabs():
    """6000 pairs; three of the last 1800 hold a tab in a comment (pairs whose records go to the second file: tests/golden/fx1/reads150.ori.sam.gz
    names r0000206, r0000208 and r0000210), so both encoders decline them"""
    tmp = tempfile.mkdtemp(prefix="psvr_aoc_")
    fq = os.path.join(tmp, "tabs.fq")
    with open(fq, "wb") as f:
        f.write(_with_tabs(open(os.path.join(ac.workdir("fx1"), "reads150.fq"), "rb").read() * 3, (4206, 4208, 4210)))
    return fq


@pytest.mark.parametrize("args", [[], ["--sub-batch", "31"], ["-Q", "--sub-batch", "700"]])
def test_both_files_are_the_plain_pipelines_and_every_piece_stays_resident(checker, reads, args):
    _, _, want = run(checker, reads, args)
    err, n, got = run(checker, reads, args + ["--ori-device"])
    assert got[0] == want[0] and got[1] == want[1] and len(got[1]) > 100000
    assert n["pieces"] == (1 if not args else 65 if "31" in args else 3)
    assert n["resident"] == n["pieces"] and n["text_fetches"] == 0 and n["downloads"] == 0, n
    assert n["ori_device_pairs"] == n["ori_spliced_pairs"] == 2000 and n["ori_declined_pairs"] == 0 and n["ori_host_pieces"] == 0
    assert "failed" not in err and '"d2h_bytes":0,' in err


def test_a_piece_with_declined_pairs_is_fetched_and_the_others_stay_resident(checker, tabs):
    """--sub-batch 4200: a piece of two chunks that stays resident, then the piece with the three tab-comment pairs"""
    herr, _, want = run(checker, tabs, ["--sub-batch", "4200"])
    err, n, got = run(checker, tabs, ["--sub-batch", "4200", "--ori-device"])
    assert got[0] == want[0] and got[1] == want[1]
    assert n["pieces"] == 2 and n["resident"] == 1 and n["text_fetches"] == 1 and n["downloads"] == 1, n
    assert n["ori_declined_pairs"] == 3 and n["ori_device_pairs"] == 5997 and n["ori_spliced_pairs"] == 4200, n
    j = json.loads([l for l in err.split("\n") if "e2e_json" in l][-1].split("e2e_json", 1)[1])
    assert j["emit_declined_pairs"] <= 3 and j["emit_spliced_pairs"] >= 4200 and j["emit_device_pairs"] + j["emit_declined_pairs"] == 6000    # (a pair without gain is nothing to the main file)
    assert sorted(l for l in err.split("\n") if "ERROR" in l) == sorted(l for l in herr.split("\n") if "ERROR" in l)


def test_records_fetch_every_piece(checker, reads):
    tmp = tempfile.mkdtemp(prefix="psvr_aoc_")
    _, _, want = run(checker, reads, ["--sub-batch", "500", "--records", os.path.join(tmp, "plain.jsonl")])
    _, n, got = run(checker, reads, ["--sub-batch", "500", "--ori-device", "--records", os.path.join(tmp, "rec.jsonl")])
    assert got == want
    assert n["pieces"] == 4 and n["resident"] == 0 and n["text_fetches"] == 3 and n["downloads"] == 4, n      # (the first piece's text comes with it)
    rec = open(os.path.join(tmp, "rec.jsonl"), "rb").read()
    assert rec == open(os.path.join(tmp, "plain.jsonl"), "rb").read() and rec.count(b"\n") == 2000


def test_a_failing_ori_call_falls_back_with_its_line_and_identical_files(checker, reads):
    _, _, want = run(checker, reads, ["--sub-batch", "500"])
    err, n, got = run(checker, reads, ["--sub-batch", "500", "--ori-device", "--fail-ori", "3"])
    assert got == want
    assert [l for l in err.split("\n") if "failed" in l] == [FAIL_LINE]
    assert n["pieces"] == 4 and n["resident"] == 2 and n["ori_pieces"] == 2 and n["ori_host_pieces"] == 2 and n["text_fetches"] == 2 and n["downloads"] == 2, n
    assert n["ori_device_pairs"] == 1000
