"""`panSVR signal --mate-device` without a GPU: the route of signal_device_route.h over a host-memory backend that runs the mate rules with
one lane (tests/tools/signal_pos_route_check.cpp), against the command's host route: stdout, header file, status file and stderr less the
route's own lines are the host route's, whatever the flags, the block size and the piece size; when a backend call fails the files and the
exit status still are.  The inputs the host loop aborts on are held here only."""
import os

import pytest

import signal_mate_cases as mc


@pytest.fixture(scope="module")
def env():
    tmp = mc.sc.tmpdir("spr")
    files = {"crafted": mc.write(os.path.join(tmp, "crafted.bam"), mc.crafted()), "fails": mc.write(os.path.join(tmp, "fails.bam"), mc.many_failures())}
    recs, refs = mc.make_pairs_sorted(20241, 300)
    mc.ts.write_bam(os.path.join(tmp, "pairs.bam"), recs, refs)
    files["pairs"] = os.path.join(tmp, "pairs.bam")
    return tmp, files, mc.build("signal_pos_route_check", tmp)


def both(env, name, flags, envvars=None):
    tmp, files, exe = env
    h = mc.run_cmd(mc.CLI, tmp, files[name], flags, "h")
    d = mc.run_cmd(exe, tmp, files[name], flags + ["--mate-device"], "d", env=envvars)
    return h, d


def same(h, d, summary=True):
    assert h[0].returncode == 0 and d[0].returncode == 0, d[0].stderr.decode()[-2000:]
    assert d[0].stdout == h[0].stdout and d[1] == h[1] and d[2] == h[2] and h[1] and h[2]
    own = mc.own_lines(d[0].stderr)
    assert len(own) == 1 and (not summary or b"written on the device" in own[0]), own
    assert mc.without(d[0].stderr, own) == h[0].stderr
    return own[0]


@pytest.mark.parametrize("name", ["crafted", "pairs"])
@pytest.mark.parametrize("flags", mc.FLAG_SETS)
def test_flag_sets(env, name, flags):
    h, d = both(env, name, flags)
    same(h, d)
    assert name != "crafted" or flags != ["-D"] or len(h[0].stdout) > 5000


@pytest.mark.parametrize("name", ["crafted", "pairs"])
@pytest.mark.parametrize("block", [2, 3, 64, 65])
def test_block_records(env, name, block):
    h, d = both(env, name, ["-D", "--block-records", str(block)])
    line = same(h, d)
    w = line.split()
    assert block > 2 or w[w.index(b"pairs,") - 1] == w[w.index(b"paired") - 1]    # (a block of two records mates nobody: every pair is the by-name pass's)


def test_a_block_spans_many_appends(env):
    h, d = both(env, "pairs", ["-D"], {"PSVR_INFLATE_BATCH": "1000"})
    same(h, d)
    h, d = both(env, "crafted", ["-D", "-U", "--block-records", "64"], {"PSVR_INFLATE_BATCH": "1000"})
    same(h, d)


def test_every_thousandth_mate_failed_line(env):
    h, d = both(env, "fails", ["-D"])
    same(h, d)
    assert b"NUM: [1000]: Mate failed" in d[0].stderr and b"NUM: [2000]: Mate failed" in d[0].stderr


CALLS = ["store_create:1", "store_append_bgzf:1", "store_append_bgzf:2", "store_footprint:1", "store_footprint:3", "store_drop:1", "store_drop:3", "store_chain_info:1", "signal_create:1",
         "signal_run_pos:1", "signal_run_pos:2", "signal_run_pos:4", "signal_pairs:1", "signal_pairs:2", "signal_text:1", "signal_text:2", "signal_side:1", "signal_stats:1", "signal_run_left:1",
         "signal_run_left:2", "signal_left_errors:1", "signal_left_errors:3", "signal_mate_notes:1", "host_alloc:1", "host_alloc:2", "host_alloc:3"]


@pytest.mark.parametrize("call", CALLS)
def test_a_failing_backend_call_leaves_the_host_routes_files_and_status(env, call):
    name = "fails" if call.startswith("signal_mate_notes") else "pairs"
    flags = ["-D", "--block-records", "2000" if name == "fails" else "20" if "left" in call else "100"]   # (20: the by-name pass takes several slices)
    h, d = both(env, name, flags, {"PSVR_CHECK_FAIL": call, "PSVR_INFLATE_BATCH": "20000"})
    assert h[0].returncode == 0 and d[0].returncode == 0, d[0].stderr.decode()[-2000:]
    assert d[0].stdout == h[0].stdout and d[1] == h[1] and d[2] == h[2] and len(h[0].stdout) > 10000
    own = mc.own_lines(d[0].stderr)
    assert len(own) == 1 and b"failed (injected failure of " + call.split(":")[0].encode() in own[0] and b"the host route reads the file from its beginning" in own[0], own


def test_the_host_loops_aborts(env):
    tmp, files, exe = env
    rng = mc.np.random.RandomState(3)
    good = []
    for k in range(6):
        good += [mc.rec("k%d" % k, 0x61, 0, 100 + 40 * k, 0, 110 + 40 * k, rng), mc.rec("k%d" % k, 0x91, 0, 110 + 40 * k, 0, 100 + 40 * k, rng)]
    good.sort(key=lambda r: mc.struct.unpack_from("<i", r, 8)[0])
    # not first / second in template, found in a block: k2's first read carries 0x80 as well as its mate
    bad = list(good)
    i = [j for j, r in enumerate(bad) if r[36:38] == b"k2" and not mc.struct.unpack_from("<H", r, 18)[0] & 0x80][0]
    bad[i] = bad[i][:18] + mc.struct.pack("<H", 0x21) + bad[i][20:]
    # an odd number of left-overs: a record whose mate is not in the file
    odd = good + [mc.rec("lone", 0x41, 0, 5000, 3, 5, rng), mc.rec("tail", 0x41, 0, 6000, 3, 5, rng), mc.rec("tail", 0x81, 0, 6001, 3, 5, rng)]
    # equal names with flags 0xc0 and 0x00: the by-name order has the record with 0x40 first (name_tie_key's flag & 0xc0 would have it
    # second), and the pair ends the loop because its second record lacks 0x80
    tie = good + [mc.rec("tie", 0x00, 0, 5000, 3, 5, rng), mc.rec("tie", 0xc1, 0, 6000, 3, 5, rng)]
    for name, recs, status, said in (("tmpl", bad, 34, b"are not first/second in template"), ("tie", tie, 34, b"records of [tie] are not first/second in template")):
        path = mc.write(os.path.join(tmp, name + ".bam"), recs)
        h = mc.run_cmd(mc.CLI, tmp, path, ["-D"], "h")
        d = mc.run_cmd(exe, tmp, path, ["-D", "--mate-device"], "d")
        assert h[0].returncode == -6 and d[0].returncode == status, (h[0].returncode, d[0].returncode, d[0].stderr[-1000:])
        assert said in h[0].stderr and d[1] == h[1] and d[2] == h[2]
        own = [l for l in d[0].stderr.split(b"\n") if b"route returned state" in l]
        assert mc.without(d[0].stderr, own) == h[0].stderr               # the messages up to the abort are the host loop's
        assert d[0].stdout.startswith(h[0].stdout)                       # (abort() drops what the host loop had not flushed)
    # an odd number of left-overs: the call declines, the host route reads the file again and ends as the host loop does
    path = mc.write(os.path.join(tmp, "odd.bam"), odd)
    h = mc.run_cmd(mc.CLI, tmp, path, ["-D"], "h")
    d = mc.run_cmd(exe, tmp, path, ["-D", "--mate-device"], "d")
    assert h[0].returncode == -6 and d[0].returncode == -6 and b"an odd number of records found no mate" in h[0].stderr and d[1] == h[1] and d[2] == h[2]
    own = mc.own_lines(d[0].stderr)
    assert len(own) == 1 and b"signal run_left failed (an odd number of records found no mate" in own[0] and b"6 pairs are written" in own[0]
    # (what the route had printed for its blocks stands in front of its line; behind it the host route's messages, all of them)
    assert d[0].stderr.endswith(own[0] + b"\n" + h[0].stderr[h[0].stderr.index(b"WARNING"):]) and d[0].stdout == h[0].stdout
