"""The mate rules of pansvr_amd/csrc/signal_mate_device.h (host build, one lane) against SignalStep::run_pos_sorted: tests/tools/signal_mate_check.cpp
runs both over a file and compares the FASTQ text and the stderr byte for byte.  Built plain and with the sanitizers; the sanitizer build is a
stand-alone program and is run directly."""
import os
import subprocess

import pytest

import signal_mate_cases as mc


@pytest.fixture(scope="module")
def env():
    tmp = mc.sc.tmpdir("smr")
    files = {"crafted": mc.write(os.path.join(tmp, "crafted.bam"), mc.crafted()), "fails": mc.write(os.path.join(tmp, "fails.bam"), mc.many_failures())}
    recs, refs = mc.make_pairs_sorted(20241, 300)
    mc.ts.write_bam(os.path.join(tmp, "pairs.bam"), recs, refs)
    files["pairs"] = os.path.join(tmp, "pairs.bam")
    return tmp, files, {False: mc.build("signal_mate_check", tmp, False), True: mc.build("signal_mate_check", tmp, True)}


def check(exe, bam, flags):
    r = subprocess.run([exe, bam] + flags, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)
    w = r.stdout.split()
    return r, {w[i].decode(): int(w[i + 1]) for i in range(0, len(w) - 1, 2)}


@pytest.mark.parametrize("sanitize", [False, True])
@pytest.mark.parametrize("block", [None, 2, 3, 64, 65])
def test_crafted_file_pairs_as_the_host_loop_pairs_it(env, block, sanitize):
    tmp, files, exe = env
    r, s = check(exe[sanitize], files["crafted"], ["-D"] + (["--block-records", str(block)] if block else []))
    assert r.returncode == 0, (r.stdout, r.stderr[-3000:])
    assert s["same_text"] == 1 and s["same_stderr"] == 1 and s["text_bytes"] > 5000
    if block is None:
        # five blocks; the two triples, the unmapped triple and the record with the wrong mate position are what the replay walks or what fails
        assert s["blocks"] == 5 and s["left"] == 24 and s["left_pairs"] == 10 and s["pair_errors"] == 4 and s["replayed"] >= 9 and s["fails"] >= 5


@pytest.mark.parametrize("flags", [[], ["-U"], ["-D", "-U"]])
def test_crafted_file_under_the_filter_flags(env, flags):
    tmp, files, exe = env
    r, s = check(exe[False], files["crafted"], flags)
    assert r.returncode == 0 and s["same_text"] == 1 and s["same_stderr"] == 1, (r.stdout, r.stderr[-3000:])


@pytest.mark.parametrize("block", [None, 64, 65])
def test_make_pairs_in_coordinate_order(env, block):
    tmp, files, exe = env
    r, s = check(exe[True], files["pairs"], ["-D"] + (["--block-records", str(block)] if block else []))
    assert r.returncode == 0 and s["same_text"] == 1 and s["same_stderr"] == 1 and s["pairs"] + s["left_pairs"] == 300, (r.stdout, r.stderr[-3000:])


def test_every_thousandth_failed_turn_is_noted_where_the_host_loop_prints_it(env):
    tmp, files, exe = env
    for block in (None, 2000):
        r, s = check(exe[True], files["fails"], ["-D"] + (["--block-records", str(block)] if block else []))
        assert r.returncode == 0 and s["same_text"] == 1 and s["same_stderr"] == 1, (r.stdout, r.stderr[-3000:])
        assert block or s["fails"] > 2000                               # (the counter runs across the smaller blocks: the thousandth turn lies in a later one)


def test_a_block_with_decreasing_positions_is_declined(env):
    tmp, files, exe = env
    r, s = check(exe[False], mc.write(os.path.join(tmp, "dec.bam"), mc.decreasing()), ["-D"])
    assert r.returncode == 2 and r.stdout.split() == [b"declined", b"1"]
