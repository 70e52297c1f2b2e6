"""The seeding filter's addressing rule on the host (pansvr_amd/csrc/aln_device.h: rc20, bloom_slot, kmer_maybe_present,
seed_pair_half), through the stand-alone checker tests/tools/seed_filter_check.cpp: the word of a 20-mer is that of its canonical
form, so one word answers both strands of a read, and the bits are the orientation's own, so the filter still has no false
negative for a k-mer as indexed and passes about as few absent k-mers as the rule it replaced."""
import os
import re
import subprocess
import tempfile

import pytest

import aln_common as ac

SRC = os.path.join(ac.HERE, "tools", "seed_filter_check.cpp")


def build_tool():
    exe = os.path.join(tempfile.mkdtemp(prefix="psvr_sfc_"), "seed_filter_check")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-Wno-unused-function", "-o", exe, SRC])
    return exe


@pytest.fixture(scope="module")
def tool():
    return build_tool()


def run(tool, *args):
    r = subprocess.run([tool] + list(args), stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    out = r.stdout.decode()
    print(out)
    assert r.returncode == 0, out + r.stderr.decode()
    return out


def test_reverse_complement_shares_the_word(tool):
    out = run(tool, "rc20")
    assert re.search(r"rc20: \d+ k-mers, 0 failures", out)


@pytest.mark.parametrize("name", ["fx1", "fx2", "fx3"])
def test_host_built_filter_has_no_false_negative(tool, name):
    out = run(tool, "index", ac.index_dir(name))
    m = re.search(r"index: (\d+) indexed 20-mers, (\d+) words, shift (\d+), false negatives (\d+)", out)
    assert m and int(m.group(1)) > 20000 and int(m.group(4)) == 0


def test_absent_kmers_pass_no_more_often_than_twice_the_replaced_rule(tool):
    """800 k random keys at the engine's sizing rule; the share of random absent k-mers, and of the keys' reverse complements, that
    pass is at most 2 x the share the replaced rule passes (restated in the tool, same keys and queries) + 1e-3."""
    out = run(tool, "rates")
    m = re.search(r"absent_canonical (\S+) absent_parent (\S+) revcomp_canonical (\S+) revcomp_parent (\S+)", out)
    an, ao, rn, ro = (float(x) for x in m.groups())
    assert re.search(r"false_negatives 0\b", out)
    assert 0 < ao < 0.05 and 0 < ro < 0.05                  # the baseline is a working filter
    assert an <= 2 * ao + 1e-3, (an, ao)
    assert rn <= 2 * ro + 1e-3, (rn, ro)


def test_lane_pair_masks_equal_the_per_strand_filter(tool):
    """lengths 20, 24, 25, 100, 150, 250, 339: two "lanes", each running seed_pair_half on its own strand's packed words and
    handing the other half to its neighbour, hold bit for bit what kmer_maybe_present says per strand and offset (lengths whose
    offsets do not mirror keep the per-strand loop)."""
    out = run(tool, "pair")
    m = re.search(r"pair: (\d+) answers \((\d+) pass, \d+ of palindromes\), (\d+) of (\d+) reads by the lane pair, (\d+) strands differ", out)
    assert m and int(m.group(5)) == 0 and int(m.group(3)) == 1500 and int(m.group(4)) == 2100
    assert 0 < int(m.group(2)) < int(m.group(1))
