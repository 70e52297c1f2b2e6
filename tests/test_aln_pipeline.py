"""The pipeline of `panSVR aln` without a GPU: the PRODUCT's pansvr_amd/csrc/aln_pipeline.h (the four stages on their threads, the pieces
that end where the reference's batches end, the three short first pieces, -R, the slot ring, the block split over several engines and
the draw-order exchange, the order of what reaches the two files, the statistics) instantiated over the CPU emulation of the engine
(tests/tools/aln_pipeline_check.cpp: a driver over EngineCore<CpuBE>, tests/emu/cpu_backend.h).  Both SAM files against the reference's
own (tests/golden/<set>/<reads>.sam.gz / .ori.sam.gz, as tests/test_sam_golden.py), the progress lines, e2e_json's keys, the piece rule
on its own -- and the same program under AddressSanitizer + UBSan and under ThreadSanitizer.  The device routes (--parse-device,
--emit-device) and the real engine behind the same pipeline are what the CLI-level GPU tests witness."""
import gzip
import json
import os
import subprocess
import tempfile

import pytest

import aln_common as ac

SRC = os.path.join(ac.HERE, "tools", "aln_pipeline_check.cpp")
KSW = os.path.join(ac.ROOT, "oracle", "ksw_oracle.c")
SETS = [("fx1", "reads150"), ("fx2", "reads150"), ("fx3", "ragged")]
# the whole input as one piece; batches of 97; a piece that ends where a batch ends; batches cut by bases
SPLITS = [[], ["--batch", "97"], ["--batch", "211", "--sub-batch", "97"], ["--batch-bases", "60000"]]
# today's format string of the statistics line, key by key
E2E_KEYS = ["pairs", "batches", "pieces", "devices", "threads", "wall_s", "index_s", "index_first_s", "index_clone_s", "read_parse_s", "engine_s", "exchange_s",
            "rebase_iterations", "format_s", "write_s", "sort_s", "sort_order_s", "d2h_bytes", "hbm_used_first", "hbm_used_last", "dropped", "teardown_s", "parser",
            "emitter", "emit_device_pairs", "emit_declined_pairs", "emit_spliced_pairs"]


def build(tmp, tag, flags):
    exe = os.path.join(tmp, "aln_pipeline_check" + tag)
    subprocess.check_call(["g++"] + flags + ["-std=c++17", "-DPSVR_EMU_SPARSE_HASH", "-DPSVR_NO_ENGINE_LIB", "-Wall", "-Wno-unused-variable", "-Wno-maybe-uninitialized",
                                             "-o", exe, SRC, KSW, "-lz", "-lpthread"])
    return exe


@pytest.fixture(scope="module")
def tmpdir():
    return tempfile.mkdtemp(prefix="psvr_apc_")


@pytest.fixture(scope="module")
def checker(tmpdir):
    return build(tmpdir, "", ["-O2"])


_runs = {}


def run(exe, name, rname, args, records=False):
    """One run of the checker (kept: several tests look at the same run): stderr text, both files, the --records file."""
    key = (exe, name, rname, tuple(args), records)
    if key not in _runs:
        w = ac.workdir(name)
        tmp = tempfile.mkdtemp(prefix="psvr_apc_")
        fn = [os.path.join(tmp, f) for f in ("o.sam", "p.sam", "rec.jsonl")]
        r = subprocess.run([exe, "-S", "-o", fn[0], "-p", fn[1]] + (["--records", fn[2]] if records else []) + list(args) +
                           [ac.index_dir(name), os.path.join(w, rname + ".fq"), os.path.join(w, "header.sam")], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)
        err = r.stderr.decode()
        assert r.returncode == 0, "aln_pipeline_check %s: exit status %d\n%s" % (" ".join(args), r.returncode, err[-3000:])
        _runs[key] = (err, open(fn[0], "rb").read(), open(fn[1], "rb").read(), open(fn[2], "rb").read() if records else None)
    return _runs[key]


def golden(name, rname, ext):
    with gzip.open(os.path.join(ac.golden_dir(name), rname + ext), "rb") as f:
        return f.read()


def assert_reference_files(res, name, rname, exts=(".sam.gz", ".ori.sam.gz")):
    for got, ext in zip(res[1:3], exts):
        want = golden(name, rname, ext)
        if got != want:
            gl, wl = got.split(b"\n"), want.split(b"\n")
            first = next((i for i, (a, b) in enumerate(zip(wl, gl)) if a != b), min(len(gl), len(wl)))
            raise AssertionError("%s differs from the reference's file at line %d (%d vs %d lines)\nref: %r\ngot: %r"
                                 % (ext, first, len(wl), len(gl), wl[first][:600] if first < len(wl) else None, gl[first][:600] if first < len(gl) else None))


def e2e(err):
    line = [l for l in err.split("\n") if l.startswith("[panSVR-amd] e2e_json ")]
    assert len(line) == 1, err[-2000:]
    return json.loads(line[0][len("[panSVR-amd] e2e_json "):], object_pairs_hook=lambda kv: kv)


def pair_lengths(name, rname):
    """bases of every pair of the FASTQ, and the first read's name of every pair"""
    lines = open(os.path.join(ac.workdir(name), rname + ".fq"), "rb").read().split(b"\n")
    n = len(lines) // 8
    return [len(lines[8 * p + 1]) + len(lines[8 * p + 5]) for p in range(n)], [lines[8 * p][1:].split()[0] for p in range(n)]


def reference_batches(lens, batch_pairs=2000000, batch_bases=100000000):
    """load_reads' batches: a batch ends with the pair that brings it to batch_pairs pairs or to batch_bases bases (rr.cpp:24,109,126)"""
    out, pairs, bases = [], 0, 0
    for n in lens:
        pairs, bases = pairs + 1, bases + n
        if pairs >= batch_pairs or bases >= batch_bases:
            out.append(pairs)
            pairs = bases = 0
    return out + ([pairs] if pairs else [])


@pytest.mark.parametrize("threads", [1, 4])
@pytest.mark.parametrize("split", SPLITS, ids=lambda s: " ".join(s) or "one piece")
@pytest.mark.parametrize("name,rname", SETS)
def test_pipeline_writes_the_reference_sam_files(checker, name, rname, split, threads):
    res = run(checker, name, rname, split + ["-t", str(threads)])
    assert_reference_files(res, name, rname)
    assert golden(name, rname, ".sam.gz").count(b"\n") > 40


def test_not_ori_option_matches_the_reference(checker):
    assert_reference_files(run(checker, "fx2", "reads150", ["-Q"]), "fx2", "reads150", (".notori.sam.gz", ".notori.ori.sam.gz"))
    assert golden("fx2", "reads150", ".notori.sam.gz").count(b"\n") < golden("fx2", "reads150", ".sam.gz").count(b"\n")


@pytest.mark.parametrize("split", [[], ["--batch", "211"]], ids=["one batch", "--batch 211"])
@pytest.mark.parametrize("devices", [2, 3])
def test_several_engines_split_every_piece_in_input_order(checker, devices, split):
    """what test_gpu_cli_devices_split_every_batch_in_input_order asserts with --devices 0,0 and 0,0,0: the files and the records of one
    engine, and the draw-order exchange really moved a block (without that it was not exercised)"""
    res = run(checker, "fx2", "reads150", split + ["--devices", str(devices)], records=True)
    assert_reference_files(res, "fx2", "reads150")
    one = run(checker, "fx2", "reads150", split, records=True)
    assert len(one[3]) > 100000 and res[3] == one[3]
    st = dict(e2e(res[0]))
    assert st["devices"] == devices and st["rebase_iterations"] >= 1 and st["pairs"] == 1500
    assert dict(e2e(one[0]))["rebase_iterations"] == 0


def test_max_use_read_takes_the_first_pairs(checker):
    n = 250
    res = run(checker, "fx2", "reads150", ["-R", str(n)])
    _, names = pair_lengths("fx2", "reads150")
    assert len(names) > n
    first = set(names[:n])
    assert not first & set(names[n:])
    want = [l for l in golden("fx2", "reads150", ".sam.gz").split(b"\n") if l and (l[:1] == b"@" or l.split(b"\t")[0] in first)]
    got = [l for l in res[1].split(b"\n") if l]
    assert got == want and sum(1 for l in got if l[:1] != b"@") > n
    assert dict(e2e(res[0]))["pairs"] == n


@pytest.mark.parametrize("split", SPLITS, ids=lambda s: " ".join(s) or "one piece")
@pytest.mark.parametrize("name,rname", SETS)
def test_progress_lines_are_the_reference_sized_batches(checker, name, rname, split):
    err = run(checker, name, rname, split + ["-t", "4"])[0]
    lens, _ = pair_lengths(name, rname)
    opt = dict(zip(split[::2], (int(v) for v in split[1::2])))
    want = reference_batches(lens, opt.get("--batch", 2000000), opt.get("--batch-bases", 100000000))
    got = [l.split() for l in err.split("\n") if l.startswith("Processing ") and " reads, at block ID " in l]
    assert [int(w[1]) for w in got] == want and sum(want) == len(lens)
    assert [int(w[-1]) for w in got] == list(range(len(want)))
    st = dict(e2e(err))
    assert st["batches"] == len(want) and st["pairs"] == len(lens) and st["pieces"] >= len(want)
    if "--sub-batch" in opt:
        assert st["pieces"] == sum((b + opt["--sub-batch"] - 1) // opt["--sub-batch"] for b in want) > len(want)


def pieces(checker, batch_pairs, sub_pairs, max_use_read, input_pairs):
    out = subprocess.run([checker, "pieces", str(batch_pairs), str(sub_pairs), str(max_use_read), str(input_pairs)], stdout=subprocess.PIPE, check=True).stdout.decode()
    return [(w[0], int(w[1])) for w in (l.split() for l in out.split("\n") if l)]


def test_piece_rule_on_its_own(checker):
    # the three short first pieces, then -R cuts the fourth; the input ends there
    assert pieces(checker, 2000000, 65536, 100000, 10 ** 9) == [("piece", 8192), ("piece", 16384), ("piece", 32768), ("piece", 42656), ("end", 100000)]
    assert pieces(checker, 2000000, 0, 100000, 10 ** 9)[0] == ("piece", 100000)
    # pieces end where a batch ends; the first-piece counter keeps counting across batches (the third would be capped at 32768, not smaller than 20000)
    assert pieces(checker, 20000, 65536, 0x7fffffff, 40000) == [("piece", 8192), ("piece", 11808), ("batch", 20000), ("piece", 20000), ("batch", 20000), ("end", 0)]


def test_e2e_json_keys_and_their_order(checker):
    kv = e2e(run(checker, "fx1", "reads150", ["-t", "4"])[0])
    assert [k for k, _ in kv] == E2E_KEYS
    st = dict(kv)
    assert st["parser"] == "host" and st["emitter"] == "host" and st["pairs"] == 2000 and st["threads"] == 4 and st["devices"] == 1


def assert_clean_and_equal(exe, checker, name, rname, args):
    err, main, ori, _ = run(exe, name, rname, args)
    assert "Sanitizer" not in err and "runtime error" not in err, err[-4000:]
    plain = run(checker, name, rname, args)
    assert (main, ori) == plain[1:3]
    assert_reference_files(plain, name, rname)


@pytest.fixture(scope="module")
def asan(tmpdir):
    return build(tmpdir, "_asan", ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"])


def test_pipeline_under_address_and_ub_sanitizers(asan, checker):
    assert_clean_and_equal(asan, checker, "fx2", "reads150", ["--devices", "2", "--batch", "211", "-t", "4"])


@pytest.fixture(scope="module")
def tsan(tmpdir):
    return build(tmpdir, "_tsan", ["-O1", "-g", "-fsanitize=thread"])


@pytest.mark.parametrize("args", [["--sub-batch", "97", "-t", "4"], ["--devices", "2"]], ids=lambda a: " ".join(a))
def test_pipeline_under_thread_sanitizer(tsan, checker, args):
    assert_clean_and_equal(tsan, checker, "fx1", "reads150", args)
