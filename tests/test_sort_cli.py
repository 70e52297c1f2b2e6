"""`panSVR aln --sort` refuses the options that shape the unsorted main file (-S, --compress-level, --bgzf-fast, --bgzf-device) as a
usage error before it reads anything; `panSVR sort`'s coordinate order against a plain Python stable sort of the decoded records
(on a machine without a GPU the host order, with one the device order)."""
import os
import subprocess

import numpy as np
import pytest

import bam_reader
import test_signal as ts

CLI = ts.CLI


@pytest.mark.parametrize("flags,name", [(["-S"], "-S"), (["--compress-level", "1"], "--compress-level"), (["--bgzf-fast"], "--bgzf-fast"),
                                        (["--bgzf-device"], "--bgzf-device")])
def test_aln_sort_refuses_conflicting_options(tmp_path, flags, name):
    # none of the positional files exists: a check that came after the header or the index load would end the run differently
    missing = [str(tmp_path / "no_idx"), str(tmp_path / "no_reads.fq"), str(tmp_path / "no_header.sam")]
    r = subprocess.run([CLI, "aln", "--sort"] + flags + ["-o", str(tmp_path / "o.bam"), "-p", str(tmp_path / "p.bam")] + missing,
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=60)
    err = r.stderr.decode()
    assert r.returncode == 1, err
    assert "--sort cannot be combined with %s" % name in err, err
    assert "loading index" not in err and not os.path.exists(str(tmp_path / "o.bam")) and not os.path.exists(str(tmp_path / "p.bam"))


def test_aln_usage_lists_sort():
    r = subprocess.run([CLI, "aln"], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=60)
    assert r.returncode == 1 and "--sort" in r.stderr.decode()


def python_order(recs, refs):
    """samtools' coordinate order of decoded SAM fields: reference id as unsigned ('*' last), position, strand; stable"""
    tid_of = {n: i for i, (n, _) in enumerate(refs)}
    return sorted(recs, key=lambda f: (tid_of[f[2]] if f[2] != "*" else 1 << 40, int(f[3]) - 1, int(f[1]) & 16))


def check_sort_against_python(tmp_path, n_pairs, seed):
    recs, refs = ts.make_pairs(seed, n_pairs)
    rng = np.random.RandomState(seed)
    order = rng.permutation(len(recs))
    inp, out = str(tmp_path / "in.bam"), str(tmp_path / "sorted.bam")
    ts.write_bam(inp, [recs[i] for i in order], refs)
    r = subprocess.run([CLI, "sort", "-t", "3", "-o", out, inp], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600)
    assert r.returncode == 0, r.stderr.decode()
    _, refs0, recs0 = bam_reader.read_bam(inp, check_bin=False)
    text, refs1, recs1 = bam_reader.read_bam(out)
    assert refs1 == refs0 and "SO:coordinate" in text.split("\n")[0]
    want = python_order(recs0, refs0)
    assert len(recs1) == len(want)
    bad = [i for i, (a, b) in enumerate(zip(want, recs1)) if a != b]
    assert not bad, "%d records out of place, first at %d" % (len(bad), bad[0])
    return r.stderr.decode()


def test_sort_matches_a_python_stable_sort(tmp_path):
    check_sort_against_python(tmp_path, 3000, 91)
