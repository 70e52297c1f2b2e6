"""The by-name mode of the sorted writer over a store its caller filled (pansvr_amd/csrc/sorted_bam.h: finish_sorted_store(..., by_name), what
`panSVR sort --nsort-device` ends with) without a GPU: tests/tools/nsort_sink_check.cpp drives it over a backend that keeps store and stream in
host memory and has a store_order_names().  The file is write_sorted_bam(..., by_name = true)'s for the same records, byte for byte, there is
no .bai, and a failing backend call is named and answered with -1.  The plain and the sanitizer build (stand-alone programs) run the same cases."""
import gzip
import os
import subprocess
import tempfile

import pytest

import name_cases as nc

HERE = os.path.dirname(os.path.abspath(__file__))
CHECK_SRC = os.path.join(HERE, "tools", "nsort_sink_check.cpp")
FAILS = ("order", "info", "meta", "stream create", "stream append", "stream", "take", "the last take")


def build_checker(tmp, sanitize):
    exe = os.path.join(tmp, "nsort_sink_check_asan" if sanitize else "nsort_sink_check")
    flags = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"] if sanitize else ["-O2"]
    subprocess.check_call(["g++"] + flags + ["-std=c++17", "-Wall", "-Wno-unused-function", "-o", exe, CHECK_SRC, "-lz", "-lpthread"])
    return exe


@pytest.fixture(scope="module")
def checkers():
    tmp = tempfile.mkdtemp(prefix="psvr_nss_")
    return build_checker(tmp, False), build_checker(tmp, True)


bulk = nc.bulk


def _read(fn):
    return open(fn, "rb").read() if os.path.exists(fn) else None


def run(exe, recs, take_members, fail="none"):
    tmp = tempfile.mkdtemp(prefix="psvr_nss_")
    inp, out, ref = (os.path.join(tmp, n) for n in ("records", "out.bam", "ref.bam"))
    with open(inp, "wb") as f:
        f.write(b"".join(recs))
    r = subprocess.run([exe, inp, out, ref, str(take_members), fail], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)
    err = r.stderr.decode()
    assert r.returncode == 0 and "Sanitizer" not in err and "runtime error" not in err, err[-4000:]
    w = r.stdout.decode().split()
    counts = {w[i]: int(w[i + 1]) for i in range(0, len(w), 2)}
    return counts, err, _read(out), _read(ref), os.path.exists(out + ".bai") or os.path.exists(ref + ".bai")


def records_of(bam):
    """(header text, the records in file order) of a BAM file with the three references of the check"""
    raw = gzip.decompress(bam)
    l_text = int.from_bytes(raw[4:8], "little")
    at = 8 + l_text
    n_ref = int.from_bytes(raw[at:at + 4], "little")
    at += 4
    for _ in range(n_ref):
        at += 8 + int.from_bytes(raw[at:at + 4], "little")
    recs = []
    while at < len(raw):
        n = 4 + int.from_bytes(raw[at:at + 4], "little")
        recs.append(raw[at:at + n])
        at += n
    return raw[8:8 + l_text], recs


@pytest.mark.parametrize("what,take_members", [("empty", 1), ("one", 1), ("cases", 1), ("bulk", 1), ("bulk", 3)])
def test_the_file_is_the_name_sorted_writers(checkers, what, take_members):
    recs = {"empty": [], "one": nc.records(nc.groups()["one name"]), "cases": nc.records(nc.groups()["everything"]), "bulk": bulk(3000, 11)}[what]
    results = [run(exe, recs, take_members) for exe in checkers]
    for c, err, got, want, bai in results:
        assert c["rc"] == 0 and not err, err
        assert got is not None and got == want and not bai
        assert c["records"] == len(recs)
        assert c["members"] == (len(gzip.decompress(want)) + 0xff00 - 1) // 0xff00
    text, out = records_of(results[0][2])
    assert text.startswith(b"@HD\tVN:1.6\tSO:queryname\n")
    # the yardstick itself is those records in the restated order (the bin recomputed: bytes 14-15 are not compared)
    order = nc.restated_order(recs)
    assert [r[:14] + r[16:] for r in out] == [recs[i][:14] + recs[i][16:] for i in order]
    if what == "bulk":
        assert results[0][0]["members"] >= 5 and results[0][0]["calls"] > 8 // take_members


@pytest.mark.parametrize("take_members", [1, 3])
def test_a_failing_call_is_named_and_answered_with_minus_one(checkers, take_members):
    recs = bulk(3000, 12)
    for exe in checkers:
        for fail in FAILS:
            c, err, got, want, bai = run(exe, recs, take_members, fail)
            lines = [l for l in err.split("\n") if l]
            assert c["rc"] == -1, (fail, err)
            assert len(lines) == 1 and "record store on the device failed" in lines[0] and "stand-in failure in %s)" % fail in lines[0], (fail, err)
            assert "the input is read again" in lines[0] and not bai and c["records"] == 0, (fail, err)
