"""The writer of `panSVR aln --sort-device`'s main file (pansvr_amd/csrc/sort_store_sink.h) without a GPU: tests/tools/sort_store_sink_check.cpp
drives it over a stand-in backend that keeps the record store and the BGZF stream in host memory and makes the members with the encoder's host
build.  Whatever the chunks are and whichever backend call fails, the sorted BAM and its .bai are write_sorted_bam's for the same records, byte
for byte; a store that cannot be downloaded ends the run with status 2 and no .bai.  The plain and the sanitizer build run the same cases.  Then
the one .bai builder over both of its views, the command's option rules through the real binary, and the store's C entry points without a device."""
import ctypes as C
import gzip
import os
import struct
import subprocess
import tempfile

import pytest

import aln_common as ac
import test_signal as ts

CLI = ts.CLI
CHECK_SRC = os.path.join(ac.HERE, "tools", "sort_store_sink_check.cpp")
SCENARIOS = ("device", "host", "alternating", "empty")
KINDS = {"append", "append_emit", "info", "order", "meta", "stream", "take", "the last take", "stream create", "stream append"}


def build_checker(tmp, sanitize):
    exe = os.path.join(tmp, "sort_store_sink_check_asan" if sanitize else "sort_store_sink_check")
    flags = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"] if sanitize else ["-O2"]
    subprocess.check_call(["g++"] + flags + ["-std=c++17", "-Wall", "-Wno-unused-function", "-o", exe, CHECK_SRC, "-lz", "-lpthread"])
    return exe


@pytest.fixture(scope="module")
def checkers():
    tmp = tempfile.mkdtemp(prefix="psvr_sss_")
    return build_checker(tmp, False), build_checker(tmp, True)


def _read(fn):
    return open(fn, "rb").read() if os.path.exists(fn) else None


def run(exe, scenario, fail_at=0, fail_download=0):
    """(exit status, the printed counts, stderr, (out.bam, out.bam.bai), (ref.bam, ref.bam.bai))"""
    tmp = tempfile.mkdtemp(prefix="psvr_sss_")
    out, ref = os.path.join(tmp, "out.bam"), os.path.join(tmp, "ref.bam")
    r = subprocess.run([exe, scenario, out, ref, str(fail_at), str(fail_download)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)
    w = r.stdout.decode().split()
    counts = {w[i]: (w[i + 1] if w[i] == "sorter" else int(w[i + 1])) for i in range(0, len(w), 2)}
    err = r.stderr.decode()
    assert "Sanitizer" not in err and "runtime error" not in err, err[-4000:]
    return r.returncode, counts, err, (_read(out), _read(out + ".bai")), (_read(ref), _read(ref + ".bai"))


def keys_of(bam):
    """samtools' key of every record of a BAM file, in file order (a restatement, not the writer's code)"""
    raw = gzip.decompress(bam)
    l_text, = struct.unpack_from("<i", raw, 4)
    at = 8 + l_text
    n_ref, = struct.unpack_from("<i", raw, at)
    at += 4
    for _ in range(n_ref):
        l_name, = struct.unpack_from("<i", raw, at)
        at += 8 + l_name
    keys = []
    while at < len(raw):
        bs, tid, pos = struct.unpack_from("<Iii", raw, at)
        flag, = struct.unpack_from("<H", raw, at + 18)
        keys.append(((tid & 0xffffffff) << 32) | (((pos + 1) & 0x7fffffff) << 1) | ((flag >> 4) & 1))
        at += 4 + bs
    return keys, raw[:8 + l_text]


@pytest.mark.parametrize("scenario", SCENARIOS)
def test_the_files_are_the_sorted_writers(checkers, scenario):
    plain, asan = checkers
    rc, c, err, got, want = run(plain, scenario)
    assert rc == 0 and not err, err
    assert got[0] is not None and got == want
    keys, head = keys_of(want[0])
    assert keys == sorted(keys) and len(keys) == c["records"] and b"SO:coordinate" in head      # the yardstick itself is a sorted file of those records
    assert c["left"] == 0 and c["sorter"] == "device"
    assert c["members"] == (len(gzip.decompress(want[0])) + 0xff00 - 1) // 0xff00
    assert c["device_bytes"] + c["host_bytes"] == len(gzip.decompress(want[0]))
    if scenario == "device":
        assert c["host_chunks"] == 0 and c["device_chunks"] == 5 and c["host_bytes"] < 300       # (the BAM header)
        assert c["members"] > 4                                                                  # several windows of two members
    if scenario == "host":
        assert c["device_chunks"] == 0 and c["device_bytes"] == 0
    if scenario == "alternating":
        assert c["device_chunks"] > 5 and c["host_chunks"] > 5
    rc2, c2, err2, got2, want2 = run(asan, scenario)
    assert rc2 == 0 and not err2 and got2 == got and want2 == want and c2 == c, err2


@pytest.mark.parametrize("scenario", SCENARIOS)
def test_any_failing_call_leaves_the_same_files(checkers, scenario):
    """the k-th backend call fails, for every k of the run and every kind of call"""
    plain, asan = checkers
    rc, c, err, got, want = run(plain, scenario)
    n_calls = c["calls"]
    assert n_calls >= 10
    kinds = {plain: set(), asan: set()}
    for k in range(1, n_calls + 1):
        for exe in (plain, asan):                                               # the same cases through the sanitizer build, every one
            rc, c, err, got, want = run(exe, scenario, fail_at=k)
            what = "%s, call %d fails" % (scenario, k)
            assert rc == 0, (what, err)
            lines = [l for l in err.split("\n") if l]
            assert len(lines) == 1 and "record store on the device failed" in lines[0] and "stand-in failure in" in lines[0], (what, err)
            kinds[exe].add(lines[0].split("stand-in failure in ")[1].split(")")[0])
            assert c["left"] == 1 and c["sorter"] == "device+host", what
            assert got[0] is not None and got == want, what
            assert c["device_bytes"] == 0 and c["members"] == 0, what           # every record came to the host after all
    want_kinds = set(KINDS)
    if scenario == "host":
        want_kinds.discard("append_emit")
    if scenario == "device":
        want_kinds.discard("append")
    if scenario == "empty":
        want_kinds.discard("take")                                              # (too few records for a window that is not the last)
    assert want_kinds <= kinds[plain] and want_kinds <= kinds[asan], (kinds, want_kinds)


def test_a_failing_download_ends_with_status_2_and_no_index(checkers):
    plain, asan = checkers
    n_calls = run(plain, "alternating")[1]["calls"]
    for exe in (plain, asan):
        for k in range(1, n_calls + 1):
            rc, c, err, got, want = run(exe, "alternating", fail_at=k, fail_download=1)
            assert rc == 2, (k, err)
            assert "could not be downloaded" in err and "records missing" in err and "stand-in failure in download" in err, err
            assert got[1] is None, k                                            # no .bai, partial or otherwise


def test_the_bai_builder_over_meta_equals_the_one_over_the_records(checkers):
    for exe in checkers:
        r = subprocess.run([exe, "bai", "20000"], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)
        assert r.returncode == 0 and b"equal" in r.stdout and not r.stderr, (r.stdout, r.stderr)


# ---- the command's option rules ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("flags,name", [(["-S"], "-S"), (["--devices", "0,0"], "more than one entry in --devices"), (["--stream-device"], "--stream-device"),
                                        (["--bgzf-fast"], "--bgzf-fast"), (["--compress-level", "1"], "--compress-level"), (["--bgzf-device"], "--bgzf-device")])
def test_sort_device_refuses_conflicting_options(tmp_path, flags, name):
    missing = [str(tmp_path / "no_idx"), str(tmp_path / "no_reads.fq"), str(tmp_path / "no_header.sam")]
    for first in (["--sort-device"] + flags, flags + ["--sort-device"]):
        r = subprocess.run([CLI, "aln"] + first + ["-o", str(tmp_path / "o.bam"), "-p", str(tmp_path / "p.bam")] + missing, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=60)
        err = r.stderr.decode()
        assert r.returncode == 1, err
        assert err.startswith("--sort-device cannot be combined with %s" % name), err
        assert "loading index" not in err and not os.path.exists(str(tmp_path / "o.bam")) and not os.path.exists(str(tmp_path / "p.bam"))


def test_usage_lists_sort_device():
    r = subprocess.run([CLI, "aln"], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=60)
    assert r.returncode == 1 and "--sort-device" in r.stderr.decode()
    r = subprocess.run([CLI], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=60)
    assert r.returncode == 1 and "--sort-device" in r.stderr.decode()


# ---- the C entry points ------------------------------------------------------------------------------------------------------------------------------
NEW_SYMBOLS = ("psvr_bam_store_create", "psvr_bam_store_append", "psvr_bam_store_append_emit", "psvr_bam_store_info", "psvr_bam_store_order", "psvr_bam_store_meta",
               "psvr_bam_store_stream", "psvr_bam_store_download", "psvr_bam_store_destroy")


def test_library_exports_the_store_and_it_needs_a_device():
    from pansvr_amd import lib
    import pansvr_amd.sort as ps
    L = lib()
    for n in NEW_SYMBOLS:
        assert hasattr(L, n), n
    assert C.sizeof(ps.RecMeta) == 32 and C.sizeof(ps.StoreInfo) == 24
    if L.psvr_device_count() > 0:
        return
    h = C.c_void_p()
    assert L.psvr_bam_store_create(C.c_int(0), C.byref(h)) == 3 and not h.value      # PSVR_ERR_DEVICE
    assert b"no HIP device" in L.psvr_last_error()
    L.psvr_bam_store_destroy.restype = None
    L.psvr_bam_store_destroy(None)
    with pytest.raises(ps.EngineError):
        ps.BamStore()
