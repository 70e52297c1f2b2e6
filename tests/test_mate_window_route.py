"""`panSVR aln --mate-device`'s route without a GPU: signal_mate_route (pansvr_amd/csrc/signal_device_route.h) in window mode over the host-memory
backend of the position-sorted mode, the kept window grown run by run by the host build of signal_window_device.h's add rule, with a reader
that takes every offered window in pieces and prints what it took (tests/tools/mate_window_route_check.cpp, built with AddressSanitizer +
UBSan).  The printed text must be `panSVR signal`'s stdout -- whole when the route runs to its end, and also when any call on either side
fails and the host route takes over, silent for the pairs that were handed over -- and the header file, the status file and the host loop's
own lines must be the host route's, whatever the flags, the block size, the window's pair threshold and the reader's piece are."""
import os
import re

import pytest

import signal_device_cases as sc
import signal_mate_cases as mc

WORD = b"[panSVR-amd] aln --mate-device"
STAT_LINE = re.compile(rb"aln --mate-device: (\d+) pairs, (\d+) formatted on the device, (\d+) formatted by the host, (\d+) paired by name, (\d+) blocks, (\d+) windows offered, (\d+) window bytes, peak")
LEFT_LINE = re.compile(rb"aln --mate-device: (.*) failed \((.*)\): (\d+) pairs are handed over, the host fused route reads the file from its beginning, silent up to there\n")
READER_LINE = re.compile(rb"the reader was offered (\d+) windows and took (\d+) pieces\n")
HOST_LOOP_LINES = (b"NUM:", b"WARNING, too many", b"phase 2:", b"Sort all unpaired", b"Read Pairing error")
BLOCKS = [["--block-records", "2"], ["--block-records", "3"], ["--block-records", "64"], []]


def sorted_crafted():
    """the position-sorted signal_device_cases.crafted() without its two pairs with a read of 2047 / 2048 bases"""
    cases = [c for c in sc.crafted() if not c[0].startswith("len2047")]
    assert len(cases) == len(sc.crafted()) - 2
    return mc.by_position([r for _, pair, _ in cases for r in pair])


@pytest.fixture(scope="module")
def env():
    tmp = sc.tmpdir("mwr")
    files = {"crafted": mc.write(os.path.join(tmp, "crafted.bam"), mc.crafted()), "fails": mc.write(os.path.join(tmp, "fails.bam"), mc.many_failures()),
             "decreasing": mc.write(os.path.join(tmp, "decreasing.bam"), mc.decreasing())}
    files["rules"] = os.path.join(tmp, "rules.bam")
    sc.write_bam(files["rules"], sorted_crafted())
    return tmp, files, sc.build("mate_window_route_check", tmp, True), {}


def host(env, name, flags):
    """the command's host route, once per input and flags"""
    tmp, files, _, cache = env
    key = (name, tuple(flags))
    if key not in cache:
        cache[key] = mc.run_cmd(mc.CLI, tmp, files[name], flags, "h")
        assert cache[key][0].returncode == 0 and cache[key][1] and cache[key][2]
    return cache[key]


def route(env, name, flags, window_pairs=1 << 20, piece_pairs=1 << 20, inflate=1000, **more):
    tmp, files, exe, _ = env
    e = {"PSVR_CHECK_WINDOW_PAIRS": str(window_pairs), "PSVR_CHECK_PIECE_PAIRS": str(piece_pairs), "PSVR_INFLATE_BATCH": str(inflate)}
    e.update(more)
    return mc.run_cmd(exe, tmp, files[name], flags + ["--mate-device"], "d", env=e)


def host_loop_lines(stderr):
    return [l for l in stderr.split(b"\n") if l.startswith(HOST_LOOP_LINES)]


def held_to_host(h, d):
    assert d[0].returncode == 0, d[0].stderr.decode()[-3000:]
    assert d[0].stdout == h[0].stdout and d[1] == h[1] and d[2] == h[2]
    assert b"signal --mate-device" not in d[0].stderr


def ran_to_its_end(h, d):
    """the numbers of the route's summary line, and of the reader's"""
    held_to_host(h, d)
    assert host_loop_lines(d[0].stderr) == host_loop_lines(h[0].stderr)
    own = mc.own_lines(d[0].stderr, WORD)
    m = STAT_LINE.search(d[0].stderr)
    assert len(own) == 1 and m, own
    pairs, on_device, by_host, by_name, blocks, windows, window_bytes = (int(x) for x in m.groups())
    offers, pieces = (int(x) for x in READER_LINE.search(d[0].stderr).groups())
    assert window_bytes == len(h[0].stdout) and offers == windows and pieces >= windows
    assert on_device + by_host == h[0].stdout.count(b"\n") // 8
    return pairs, on_device, by_host, by_name, blocks, windows, pieces


@pytest.mark.parametrize("flags", mc.FLAG_SETS)
@pytest.mark.parametrize("name", ["crafted", "fails", "rules"])
def test_windows_and_pieces_are_the_host_routes_text(env, name, flags, ):
    for block in BLOCKS:
        h = host(env, name, flags + block)
        for window_pairs in (1, 7, 1 << 20):
            for piece_pairs in (1, 7):
                d = route(env, name, flags + block, window_pairs, piece_pairs)
                pairs, on_device, by_host, _, _, windows, pieces = ran_to_its_end(h, d)
                written = on_device + by_host
                if window_pairs == 1 << 20:
                    assert windows == (1 if written else 0)
                else:
                    # (a window is offered as soon as it holds window_pairs pairs: a run more at the most, and the last one may hold fewer)
                    assert windows <= written // window_pairs + 1 and (written < window_pairs or windows >= 1)
                assert pieces >= (written + piece_pairs - 1) // piece_pairs


def test_the_crafted_rule_pairs_in_blocks_and_in_slices(env):
    """50 pairs; -D writes every one, the pair with a base code that has no letter through the host formatter: met in a block (by default the
    file is three blocks), and in a slice of the by-name pass (34 blocks of three records mate nobody)"""
    assert len(sorted_crafted()) == 2 * 50 + 2                            # (one pair has a secondary and a supplementary record between its mates)
    for block, want_blocks, want_by_name in ([], 3, None), (["--block-records", "3"], 34, 50):
        d = route(env, "rules", ["-D"] + block, 7, 7)
        pairs, on_device, by_host, by_name, blocks, _, _ = ran_to_its_end(host(env, "rules", ["-D"] + block), d)
        assert (pairs, on_device, by_host, blocks) == (50, 49, 1, want_blocks)
        assert by_name == want_by_name if want_by_name is not None else by_name < 50
        assert d[0].stderr.count(b"Wrong base!") >= 1
    # by default the pair is mated in its block
    d = route(env, "rules", ["-D"], 1, 1)
    assert b"badbase" in d[0].stdout
    stat = [int(x) for x in STAT_LINE.search(d[0].stderr).groups()]
    assert stat[3] < 50


def test_every_thousandth_mate_failed_line(env):
    d = route(env, "fails", ["-D"], 7, 7)
    ran_to_its_end(host(env, "fails", ["-D"]), d)
    assert b"NUM: [1000]: Mate failed" in d[0].stderr and b"NUM: [2000]: Mate failed" in d[0].stderr


def test_decreasing_positions_leave_the_route_on_one_line(env):
    h = host(env, "decreasing", ["-D"])
    d = route(env, "decreasing", ["-D"], 7, 7)
    held_to_host(h, d)
    own = mc.own_lines(d[0].stderr, WORD)
    m = LEFT_LINE.search(d[0].stderr)
    assert len(own) == 1 and m and m.group(1) == b"signal run_pos" and b"positions decrease" in m.group(2) and int(m.group(3)) == 0


@pytest.mark.parametrize("part", [3, 8])
def test_a_window_is_offered_before_an_add_would_take_it_to_the_byte_limit(env, part):
    """the 2^32 rule at a size a test can reach, a part of the whole text: no window reaches the limit and every pair still arrives (blocks of
    three records: every run is small); a run that alone reaches the limit is the add's to refuse, and the route is left"""
    ended = 0
    for block in (["--block-records", "3"], ["--block-records", "64"], []):
        h = host(env, "crafted", ["-D"] + block)
        limit = len(h[0].stdout) // part
        d = route(env, "crafted", ["-D"] + block, 1 << 20, 7, PSVR_CHECK_WINDOW_BYTES=str(limit))
        m = LEFT_LINE.search(d[0].stderr)
        if m:
            held_to_host(h, d)
            assert block != ["--block-records", "3"] and m.group(1) == b"signal window_add" and b"a window of" in m.group(2)
        else:
            assert ran_to_its_end(h, d)[5] > part
            ended += 1
    assert ended >= 1


CALLS = ["store_create:1", "store_append_bgzf:1", "store_append_bgzf:2", "store_footprint:1", "store_footprint:3", "store_drop:1", "store_drop:3", "store_chain_info:1", "signal_create:1",
         "signal_run_pos:1", "signal_run_pos:2", "signal_run_pos:4", "signal_pairs:1", "signal_pairs:2", "signal_side:1", "signal_side:2", "signal_stats:1", "signal_run_left:1",
         "signal_run_left:2", "signal_left_errors:1", "signal_left_errors:2", "signal_mate_notes:1", "host_alloc:1", "signal_window_add:1", "signal_window_add:2", "signal_window_add:5",
         "window_parse:1", "window_parse:2", "window_parse:5"]


@pytest.mark.parametrize("call", CALLS)
def test_every_call_failing_on_either_side_leaves_the_host_routes_text(env, call):
    # (the records of a pair come back for the host formatter and for the wrong-ISIZE line: the rule pairs have both)
    name = "fails" if call.startswith("signal_mate_notes") else "rules" if call.startswith("signal_side") else "crafted"
    # (20: several blocks, and the by-name pass takes several slices; 3: the two rule pairs come in slices of their own)
    flags = ["-D", "--block-records", "2000" if name == "fails" else "3" if name == "rules" else "20"]
    h = host(env, name, flags)
    for window_pairs, piece_pairs in ((7, 7), (1 << 20, 1)):
        d = route(env, name, flags, window_pairs, piece_pairs, PSVR_CHECK_FAIL=call)
        held_to_host(h, d)
        m = LEFT_LINE.findall(d[0].stderr)
        assert len(m) == 1 and len(mc.own_lines(d[0].stderr, WORD)) == 1, (call, d[0].stderr.decode()[-2000:])
        said, why, done = m[0][0].decode(), m[0][1], int(m[0][2])
        assert b"injected failure of " + call.split(":")[0].encode() in why and not STAT_LINE.search(d[0].stderr)
        if call.startswith("window_parse"):
            # -D: every pair is written, so the pairs handed over are the pieces the reader printed before its n-th one failed
            assert said == "taking a window" and done == piece_pairs * (int(call.split(":")[1]) - 1)
        elif window_pairs == 1 << 20 and not call.startswith(("signal_stats", "window_parse")):
            assert done == 0                                             # (one window, behind the last slice: nothing was handed over before)
        assert done <= h[0].stdout.count(b"\n") // 8


def test_no_text_comes_back_in_window_mode(env):
    """signal_text is never called: a failure injected into it is never met"""
    d = route(env, "crafted", ["-D"], 7, 7, PSVR_CHECK_FAIL="signal_text:1")
    ran_to_its_end(host(env, "crafted", ["-D"]), d)
