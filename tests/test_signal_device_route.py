"""`panSVR signal -N --signal-device` without a GPU: pansvr_amd/csrc/signal_device_route.h over a backend that keeps the store in host memory and
runs the rules of signal_device.h with one lane (tests/tools/signal_device_route_check.cpp, built with AddressSanitizer + UBSan), against the
command's host route: stdout, the header file, the status file, the messages and the exit status."""
import os
import re
import subprocess

import pytest

import signal_device_cases as sc
import test_signal as ts

CALLS = ("store_create", "store_append_bgzf", "store_footprint", "store_drop", "store_chain_info", "signal_create", "signal_run", "signal_pairs", "signal_text",
         "signal_side", "signal_stats", "host_alloc")
STAT_LINE = re.compile(rb"signal --signal-device: (\d+) pairs, (\d+) written on the device, (\d+) declined to the host, (\d+) runs, (\d+) text bytes, peak footprint (\d+) chunks \((\d+) bytes\)")
LEFT_LINE = re.compile(rb"signal --signal-device: (.*) failed \((.*)\): (\d+) pairs are written, the host route reads the file from its beginning, silent up to there\n")


@pytest.fixture(scope="module")
def route():
    return sc.build("signal_device_route_check", sc.tmpdir("sdr"), True)


def run(exe, tmp, bam, flags, tag, env=None, device=True):
    e = dict(os.environ)
    for k in ("PSVR_INFLATE_BATCH", "PSVR_CHECK_FAIL", "PSVR_CHECK_CHUNK"):
        e.pop(k, None)
    e.update(env or {})
    r = subprocess.run([exe, "signal", "-N"] + (["--signal-device"] if device else []) + flags + ["-H", os.path.join(tmp, tag + ".sam"), "-S", os.path.join(tmp, tag + ".txt"), bam],
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=e, timeout=300)
    files = [open(os.path.join(tmp, tag + x), "rb").read() if os.path.exists(os.path.join(tmp, tag + x)) else None for x in (".sam", ".txt")]
    return r, files


def last_status(err):
    at = err.rindex(b"BAM/CRAM status: ave_read_depth")
    return err[at:err.index(b"\n", at)]


def held_to_host(route, tmp, recs, flags, env=None, bam=None):
    """the route's run, after its files and its last line have been held to the command's host route"""
    if bam is None:
        bam = os.path.join(tmp, "in.bam")
        sc.write_bam(bam, recs)
    h, hf = run(sc.CLI, tmp, bam, flags, "h", device=False)
    d, df = run(route, tmp, bam, flags, "d", env)
    assert h.returncode == 0 and d.returncode == 0, d.stderr.decode()[-3000:]
    assert d.stdout == h.stdout and df == hf
    assert last_status(d.stderr) == last_status(h.stderr)
    assert d.stdout.count(b"STAT_") == (1 if d.stdout else 0)
    return d


@pytest.mark.parametrize("piece", [1000, 70000, None])
@pytest.mark.parametrize("flags,seed", sc.FLAG_SETS)
def test_route_writes_the_host_routes_files(route, tmp_path, flags, seed, piece):
    recs, _ = ts.make_pairs(seed, 600)                                  # (secondary and supplementary records between mates, also at piece boundaries)
    d = held_to_host(route, str(tmp_path), recs, flags, {"PSVR_INFLATE_BATCH": str(piece)} if piece else None)
    m = STAT_LINE.search(d.stderr)
    assert m and not LEFT_LINE.search(d.stderr), d.stderr.decode()[-2000:]
    pairs, written, declined, runs, text_bytes, chunks, _ = (int(x) for x in m.groups())
    assert pairs == 600 and declined > 0 and written > 300 and 0 < text_bytes < len(d.stdout) and chunks == 1
    assert runs == 1 if piece is None else runs >= 2
    assert d.stderr.count(b"Wrong base!") >= declined


def test_odd_primary_count_header_only_one_pair_and_crafted_edges(route, tmp_path):
    recs, _ = ts.make_pairs(20241, 50)
    tmp = str(tmp_path)
    held_to_host(route, tmp, recs + recs[:1], ["-D"], {"PSVR_INFLATE_BATCH": "3000"})
    d = held_to_host(route, tmp, [], ["-D"])
    assert d.stdout == b"" and STAT_LINE.search(d.stderr).group(1) == b"0"
    pair = sc.crafted()[1][1]
    assert held_to_host(route, tmp, pair, []).stdout.count(b"\n") == 8
    d = held_to_host(route, tmp, [r for _, p, _ in sc.crafted() for r in p], [])
    assert d.stderr.count(b" wrong ISIZE: 300  -250 \n") == 1


def test_stat_occurs_once_also_when_the_first_written_pair_is_declined(route, tmp_path):
    cases = {n: p for n, p, _ in sc.crafted()}
    recs = cases["good"] + cases["badbase"] + cases["bit1"] + cases["bit4"]
    d = held_to_host(route, str(tmp_path), recs, [])
    names = d.stdout.split(b"\n")[0:-1:4]
    assert b"_STAT_" in names[0] and names[0].startswith(b"@badbase ") and sum(b"_STAT_" in l for l in names) == 1 and len(names) == 6
    assert STAT_LINE.search(d.stderr).group(3) == b"1"


@pytest.fixture(scope="module")
def long_file():
    recs, _ = ts.make_pairs(20241, 1200)
    tmp = sc.tmpdir("sdr")
    bam = os.path.join(tmp, "in.bam")
    sc.write_bam(bam, recs)
    return tmp, bam


@pytest.mark.parametrize("call", CALLS)
def test_every_backend_call_failing_leaves_the_host_routes_output(route, long_file, call):
    """on the first piece and on a later one (pieces of 70 000 bytes: at least one whole member each)"""
    tmp, bam = long_file
    once = call in ("store_create", "signal_create", "store_chain_info", "signal_stats")
    for nth in (1,) if once else (1, 3):
        d = held_to_host(route, tmp, None, ["-D"], {"PSVR_INFLATE_BATCH": "70000", "PSVR_CHECK_FAIL": "%s:%d" % (call, nth)}, bam)
        m = LEFT_LINE.search(d.stderr)
        assert m, (call, nth, d.stderr.decode()[-2000:])
        assert call.replace("store_", "").replace("signal_", "").replace("_", " ") in m.group(1).decode().replace("_", " "), m.group(1)
        assert b"injected failure of " + call.encode() in m.group(2)
        assert not STAT_LINE.search(d.stderr)
        done = int(m.group(3))
        if call == "host_alloc":                                        # (the two piece buffers, then the first piece's text buffer)
            assert done == 0
        elif call in ("store_chain_info", "signal_stats"):
            assert done == 1200
        else:
            assert (done > 0) == (nth > 1 or call == "store_drop"), (call, nth, done)


def test_damage_in_mid_file_is_named_and_the_host_route_takes_over(route, long_file):
    tmp, bam = long_file
    data = open(bam, "rb").read()
    members, at = [], 0
    while at < len(data):
        members.append(at)
        at += int.from_bytes(data[at + 16:at + 18], "little") + 1
    assert len(members) >= 6
    # a payload byte of the fourth member flipped (its CRC32 says so); the file cut inside a member; cut between members, inside a record
    broken = bytearray(data)
    broken[members[3] + 200] ^= 0x55
    for name, blob, why in (("corrupt", bytes(broken), b"corrupt BGZF block"), ("cut_member", data[:members[4] - 100], b"truncated BGZF block"),
                            ("cut_record", data[:members[4]], b"truncated BAM stream")):
        other = os.path.join(tmp, name + ".bam")
        open(other, "wb").write(blob)
        d = held_to_host(route, tmp, None, ["-D"], {"PSVR_INFLATE_BATCH": "70000", "PSVR_CHECK_ROUTE_INPUT": other}, bam)
        m = LEFT_LINE.search(d.stderr)
        assert m and why in m.group(2), (name, d.stderr.decode()[-2000:])
        assert 0 < int(m.group(3)) < 1200, name


def test_a_damaged_input_ends_with_the_host_routes_status_and_message(route, tmp_path):
    recs, _ = ts.make_pairs(20241, 300)
    tmp = str(tmp_path)
    data, _ = sc.bam_file(recs)
    second = int.from_bytes(data[16:18], "little") + 1
    broken = bytearray(data)
    broken[second + 200] ^= 0x55
    for name, blob in (("corrupt", bytes(broken)), ("cut", data[:second + 5000])):
        bam = os.path.join(tmp, name + ".bam")
        open(bam, "wb").write(blob)
        h, hf = run(sc.CLI, tmp, bam, ["-D"], "h", device=False)
        d, df = run(route, tmp, bam, ["-D"], "d")
        assert h.returncode == d.returncode == 1 and d.stdout == h.stdout and df == hf, name
        assert d.stderr == h.stderr and b"[panSVR-amd] signal: " in h.stderr, name


@pytest.mark.parametrize("state", [3, 4, 5])
def test_error_states_return_their_code_behind_the_right_prefix(route, tmp_path, state):
    front = [r for _, pair, _ in sc.crafted()[:6] for r in pair]
    tmp = str(tmp_path)
    bam, short = os.path.join(tmp, "in.bam"), os.path.join(tmp, "front.bam")
    sc.write_bam(bam, front + sc.error_pairs()[state] + front)
    sc.write_bam(short, front)
    flags = ["-D", "--isize", "100,300,500"]                            # (STAT_'s numbers given: the two files' first records differ)
    want, _ = run(sc.CLI, tmp, short, flags, "w", device=False)
    h, _ = run(sc.CLI, tmp, bam, flags, "h", device=False)
    d, _ = run(route, tmp, bam, flags, "d")
    assert want.returncode == 0 and h.returncode == -6 and d.returncode == 30 + state   # (the host loop aborts; the route returns the state)
    assert d.stdout == want.stdout and d.stdout.count(b"\n") == 6 * 8
    assert b"route returned state %d behind 6 pairs\n" % state in d.stderr
    msg = [l for l in h.stderr.split(b"\n") if l.startswith(b"[panSVR-amd] signal: ")]
    assert len(msg) == 1 and msg[0] + b"\n" in d.stderr
    assert d.stderr.count(b" wrong ISIZE: ") == h.stderr.count(b" wrong ISIZE: ") == (1 if state == 5 else 0)


def test_peak_footprint_stays_at_the_bound_when_the_chunk_is_small(route, tmp_path):
    recs, _ = ts.make_pairs(20244, 1200)
    chunk = 80000
    d = held_to_host(route, str(tmp_path), recs, ["-D", "-U", "-I", "22"], {"PSVR_INFLATE_BATCH": "20000", "PSVR_CHECK_CHUNK": str(chunk)})
    pairs, _, _, runs, _, chunks, nbytes = (int(x) for x in STAT_LINE.search(d.stderr).groups())
    assert pairs == 1200 and runs >= 5 and 2 <= chunks <= 3 and nbytes == chunks * chunk
