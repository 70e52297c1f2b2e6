"""The writer of `panSVR aln --stream-device`'s main file (pansvr_amd/csrc/bgzf_stream_sink.h) without a GPU: tests/tools/bgzf_stream_sink_check.cpp
drives it over a stand-in backend that keeps the stream in host memory and makes the members with the encoder's host build.  Whatever the
chunks are and whichever backend call fails, the file inflates to the header and the chunks in order, every member but the last holds
0xff00 bytes, and the EOF block is last; a stream that cannot be recovered ends the run with a non-zero status instead of a file with bytes
missing.  The plain and the sanitizer build run the same cases.  Then the command's option rules, through the real binary."""
import os
import struct
import subprocess
import tempfile

import pytest

import aln_common as ac
import inflate_cases as ic
import test_signal as ts

CLI = ts.CLI
CHECK_SRC = os.path.join(ac.HERE, "tools", "bgzf_stream_sink_check.cpp")
SCENARIOS = ("device", "host", "alternating", "empty", "boundary")
EOF_BLOCK = bytes([0x1f, 0x8b, 8, 4, 0, 0, 0, 0, 0, 0xff, 6, 0, 0x42, 0x43, 2, 0, 0x1b, 0, 3, 0, 0, 0, 0, 0, 0, 0, 0, 0])
MB = 0xff00


def build_checker(tmp, sanitize):
    """as deflate_wave_cases.build_checker builds its tool"""
    exe = os.path.join(tmp, "bgzf_stream_sink_check_asan" if sanitize else "bgzf_stream_sink_check")
    flags = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"] if sanitize else ["-O2"]
    subprocess.check_call(["g++"] + flags + ["-std=c++17", "-Wall", "-o", exe, CHECK_SRC, "-lz", "-lpthread"])
    return exe


@pytest.fixture(scope="module")
def checkers():
    tmp = tempfile.mkdtemp(prefix="psvr_bss_")
    return build_checker(tmp, False), build_checker(tmp, True)


def run(exe, scenario, fail_at=0, fail_recover=0):
    """(exit status, the printed counts, stderr, the file's bytes, the payload it must hold)"""
    tmp = tempfile.mkdtemp(prefix="psvr_bss_")
    out, pay = os.path.join(tmp, "out.bam"), os.path.join(tmp, "payload")
    r = subprocess.run([exe, scenario, out, pay, str(fail_at), str(fail_recover)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)
    w = r.stdout.decode().split()
    counts = {w[i]: int(w[i + 1]) for i in range(0, len(w), 2)}
    err = r.stderr.decode()
    assert "Sanitizer" not in err and "runtime error" not in err, err[-4000:]
    return r.returncode, counts, err, open(out, "rb").read(), open(pay, "rb").read()


def check_file(raw, payload, what):
    """the members inflate to the payload in order; every member but the last holds 0xff00 bytes; no empty member; the EOF block is last"""
    assert raw[-28:] == EOF_BLOCK, what
    ms = ic.split_members(raw[:-28]) if len(raw) > 28 else []
    pieces = [ic.oracle(m) for m in ms]
    assert all(p is not None for p in pieces), what
    assert b"".join(pieces) == payload, what
    assert all(len(p) == MB for p in pieces[:-1]) and (not pieces or 0 < len(pieces[-1]) <= MB), (what, [len(p) for p in pieces])
    return len(ms)


@pytest.mark.parametrize("scenario", SCENARIOS)
def test_the_file_holds_the_chunks_in_order(checkers, scenario):
    plain, asan = checkers
    rc, c, err, raw, payload = run(plain, scenario)
    assert rc == 0 and not err, err
    nm = check_file(raw, payload, scenario)
    assert c["left"] == 0 and c["members"] == nm and c["device_bytes"] + c["host_bytes"] == len(payload)
    if scenario in ("device", "boundary"):
        assert c["host_chunks"] == 0 and c["device_chunks"] == 5                 # a piece's adjacent device chunks are one range
        assert c["host_bytes"] < 200                                           # (the BAM header)
    if scenario == "host":
        assert c["device_chunks"] == 0 and c["device_bytes"] == 0
    if scenario == "alternating":
        assert c["device_chunks"] > 5 and c["host_chunks"] > 5
    if scenario == "boundary":
        assert len(payload) % MB == 0 and nm == len(payload) // MB               # no empty member at the end
    rc2, c2, err2, raw2, payload2 = run(asan, scenario)
    assert rc2 == 0 and not err2 and raw2 == raw and payload2 == payload and c2 == c, err2


@pytest.mark.parametrize("scenario", ("alternating", "device", "empty"))
def test_any_failing_call_leaves_a_complete_file_in_order(checkers, scenario):
    """the k-th backend call fails, for every k of the run: appends, appends from an emitter, the waits after a piece, takes and the last take"""
    plain, asan = checkers
    rc, c, err, raw, payload = run(plain, scenario)
    n_calls = c["calls"]
    assert n_calls >= 10
    kinds = {plain: set(), asan: set()}
    for k in range(1, n_calls + 1):
        for exe in (plain, asan):                                               # the same cases through the sanitizer build, every one
            rc, c, err, raw, payload = run(exe, scenario, fail_at=k)
            what = "%s, call %d fails" % (scenario, k)
            assert rc == 0, (what, err)
            lines = [l for l in err.split("\n") if l]
            assert len(lines) == 1 and "BGZF stream on the device failed" in lines[0] and "stand-in failure in" in lines[0], (what, err)
            kinds[exe].add(lines[0].split("stand-in failure in ")[1].split(")")[0])
            assert c["left"] == 1, what                                        # the route is reported as left
            check_file(raw, payload, what)
            assert c["device_bytes"] + c["host_bytes"] == len(payload), what
    want = {"append", "pending", "take", "the last take"} | ({"append_emit"} if scenario != "host" else set())
    assert want <= kinds[plain] and want <= kinds[asan], kinds             # every kind of call was made to fail, under the sanitizers too


def test_a_failing_recover_ends_with_a_status_and_the_message(checkers):
    plain, asan = checkers
    n_calls = run(plain, "alternating")[1]["calls"]
    for exe in (plain, asan):
        for k in range(1, n_calls + 1):
            rc, c, err, raw, payload = run(exe, "alternating", fail_at=k, fail_recover=1)
            assert rc == 3, (k, err)
            assert "could not be recovered" in err and "bytes missing" in err, err
            assert raw[-28:] != EOF_BLOCK                                       # what was written does not pass for a whole file
            got = b"".join(ic.oracle(m) for m in ic.split_members(raw)) if raw else b""
            assert payload.startswith(got)                                      # ... and holds nothing out of order


# ---- the command's option rules ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("flags,name", [(["--sort"], "--sort"), (["-S"], "-S"), (["--devices", "0,0"], "more than one entry in --devices"),
                                        (["--bgzf-fast"], "--bgzf-fast"), (["--compress-level", "1"], "--compress-level")])
def test_stream_device_refuses_conflicting_options(tmp_path, flags, name):
    missing = [str(tmp_path / "no_idx"), str(tmp_path / "no_reads.fq"), str(tmp_path / "no_header.sam")]
    for first in (["--stream-device"] + flags, flags + ["--stream-device"]):
        r = subprocess.run([CLI, "aln"] + first + ["-o", str(tmp_path / "o.bam"), "-p", str(tmp_path / "p.bam")] + missing, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=60)
        err = r.stderr.decode()
        assert r.returncode == 1, err
        assert "--stream-device cannot be combined with %s" % name in err, err
        assert "loading index" not in err and not os.path.exists(str(tmp_path / "o.bam")) and not os.path.exists(str(tmp_path / "p.bam"))


def test_usage_lists_stream_device():
    r = subprocess.run([CLI, "aln"], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=60)
    assert r.returncode == 1 and "--stream-device" in r.stderr.decode()
    r = subprocess.run([CLI], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=60)
    assert r.returncode == 1 and "--stream-device" in r.stderr.decode()
