"""The per-pair rules of `panSVR signal -N --signal-device` without a GPU: the host build of pansvr_amd/csrc/signal_device.h (what the kernels of
signal.hip run, compiled with one "lane") against SignalStep::pair, pair by pair: state, note and text -- once plain and once under
AddressSanitizer + UBSan (tests/tools/signal_device_check.cpp, a program of its own; the checker's exit status says that every pair agreed)."""
import gzip
import os

import pytest

import signal_device_cases as sc
import test_signal as ts


@pytest.fixture(scope="module")
def checkers():
    tmp = sc.tmpdir("sdr")
    return sc.build("signal_device_check", tmp, False), sc.build("signal_device_check", tmp, True)


def both(checkers, bam, flags, dump=None):
    """the summary both builds agree on"""
    rc_a, a, err_a = sc.run_rules(checkers[0], bam, flags, dump)
    rc_b, b, err_b = sc.run_rules(checkers[1], bam, flags)
    assert rc_a == 0 and rc_b == 0, (err_a[-3000:], err_b[-3000:])
    assert a == b and a["mismatches"] == 0
    return a


@pytest.mark.parametrize("flags,seed", sc.FLAG_SETS)
def test_rules_equal_pair_on_generated_pairs_and_decline_exactly_the_odd_base_codes(checkers, tmp_path, flags, seed):
    recs, refs = ts.make_pairs(seed, 600)
    bam, dump = str(tmp_path / "in.bam"), str(tmp_path / "dump")
    ts.write_bam(bam, recs, refs)
    s = both(checkers, bam, flags, dump)
    assert s["pairs"] == 600 and s["first_error"] == -1 and s["stat_pairs"] == 1
    assert s["state0"] + s["state1"] + s["state2"] == 600
    tab = sc.read_tab(dump)
    assert len(tab) == 600
    # the declined pairs are exactly the written pairs with a base code outside the five in either read, counted here
    odd = [st in (1, 2) and (sc.has_bad_base(recs[r1]) or sc.has_bad_base(recs[r2])) for st, _, _, r1, r2 in tab]
    assert [st == 2 for st, _, _, _, _ in tab] == odd
    assert 0 < sum(odd) == s["state2"] < s["state1"]
    assert all(nb == 0 for st, _, nb, _, _ in tab if st != 1) and sum(nb for _, _, nb, _, _ in tab) == s["bytes"] == os.path.getsize(dump + ".fq")


def test_rules_equal_pair_on_every_crafted_edge(checkers, tmp_path):
    cases = sc.crafted()
    assert len({n for n, _, _ in cases}) == len(cases)
    bam = str(tmp_path / "in.bam")
    sc.write_bam(bam, [r for _, pair, _ in cases for r in pair])
    dump = str(tmp_path / "dump")
    s = both(checkers, bam, [], dump)
    assert s["pairs"] == len(cases) and s["first_error"] == -1
    tab = sc.read_tab(dump)
    for (name, _, want), (st, note, _, _, _) in zip(cases, tab):
        if want is not None:
            assert st == want, name
        assert (note == 1) == (name == "isize_note"), name
    assert s["notes"] == 1 and s["state2"] == 1
    for flags in (["-D"], ["-U"], ["-D", "-U", "-I", "22"]):
        s = both(checkers, bam, flags)
        assert s["pairs"] == len(cases)
        if "-U" not in flags:
            assert s["state0"] == 0


@pytest.mark.parametrize("state", [3, 4, 5])
def test_error_states_end_the_walk_where_the_host_aborts(checkers, tmp_path, state):
    front = [r for n, pair, _ in sc.crafted()[:6] for r in pair]
    bam = str(tmp_path / "in.bam")
    sc.write_bam(bam, front + sc.error_pairs()[state] + front)
    s = both(checkers, bam, ["-D"])
    assert s["first_error"] == 6 and s["pairs"] == 7 and s["state%d" % state] == 1
    assert s["state1"] == 6


def test_a_lone_last_record_and_a_file_without_records(checkers, tmp_path):
    pair = sc.crafted()[1][1]
    bam = str(tmp_path / "in.bam")
    sc.write_bam(bam, pair + pair[:1])
    assert both(checkers, bam, ["-D"])["pairs"] == 1
    sc.write_bam(bam, [])
    assert both(checkers, bam, ["-D"])["pairs"] == 0


def test_written_text_equals_the_reference_functions(checkers, tmp_path):
    """tests/golden/signal/*.fq.gz under test_signal's exemptions: a record without CIGAR (the reference reads unset soft-clip lengths) is
    compared by name; a pair with a '=' base is declined here and not in the text at all"""
    flags, seed = ["-D"], 20241
    recs, refs = ts.make_pairs(seed, 600)
    bam, dump = str(tmp_path / "in.bam"), str(tmp_path / "dump")
    ts.write_bam(bam, recs, refs)
    both(checkers, bam, flags, dump)
    with gzip.open(os.path.join(ts.ROOT, "tests", "golden", "signal", "pairs%d_D.fq.gz" % seed), "rb") as f:
        want = f.read().split(b"\n")
    got = open(dump + ".fq", "rb").read().split(b"\n")
    assert got[-1] == b"" and (len(got) - 1) % 8 == 0
    by_name = {want[k].split(b" ")[0]: want[k:k + 8] for k in range(0, len(want) - 1, 8)}
    exact = undefined = 0
    for k in range(0, len(got) - 1, 8):
        pa, pb = got[k:k + 8], by_name[got[k].split(b" ")[0]]
        if any(b"CIGAR__" in l for l in (pb[0], pb[4])):
            undefined += 1
            assert pa[4].split(b" ")[0] == pb[4].split(b" ")[0] and pa[3] == pb[3] and pa[7] == pb[7]
            continue
        assert pa == pb, "pair at line %d differs:\n%r\n%r" % (k, pa, pb)
        exact += 1
    assert exact > 4 * undefined and exact > 350
