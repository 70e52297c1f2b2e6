"""What the tests of psvr_signal_window share (tests/test_signal_window_rules.py without a GPU, tests/test_signal_window_gpu.py with one): BAM
files whose pairs are in chosen states, with names of 1 to 17 bytes so that the segments of a window start on every residue modulo 16, and
what the command's host route makes of such a file: the text, the per-pair table and the text of the state-2 pairs cut out of it."""
import os
import subprocess

import numpy as np

import signal_device_cases as sc

TILE = 16384                                                             # kSwTileBytes of pansvr_amd/csrc/signal_window_device.h


def pair_in_state(state, name, rng, L=100, xa=None):
    """a pair that `signal -N` (no flags) leaves out (0), writes (1) or writes with a base code that has no letter (2: the host formats it)"""
    kw = {} if state == 0 else {"mapq1": 3, "mapq2": 3}
    if state == 2:
        kw["seq2"] = "AC=GT" + sc.seq(L - 5, rng)
    if xa is not None:
        kw["tags1"] = [("XA", "Z", xa), ("NM", "C", 0)]
    return sc.good_pair(name, rng, L=L, **kw)


def records(states, seed=5, error=None):
    """(all records, those in front of the error pair) for pairs in these states, named "a", "bb", ... (1 to 17 bytes, then again); error: a
    state 3, 4 or 5 pair behind them and two more pairs behind that one -- and reads of one length, so that the file and its front have one
    STAT_ field"""
    rng = np.random.RandomState(seed)
    front = []
    for k, st in enumerate(states):
        # (a pair's text is even without the XA string, which the text holds once: it makes the lengths odd and even)
        front += pair_in_state(st, chr(ord("a") + k % 26) * (1 + k % 17), rng, L=100 if error else 20 + (k * 7) % 90, xa="y" * (k % 7))
    if error is None:
        return front, front
    return front + sc.error_pairs()[error] + pair_in_state(1, "behind", rng) + pair_in_state(2, "behind2", rng), front


ISIZE = ["--isize", "100,300,500"]                                       # STAT_'s insert sizes given: a file and its front agree on them


def expected(recs, front, tmp, checker):
    """(summary, table, text): the rules checker's table of the whole file (it ends with the first error pair) and the text the command's
    host route writes for the pairs in front of that pair (the command aborts on the pair itself and loses what it has buffered: the front
    goes through it as a file of its own)"""
    bam = os.path.join(tmp, "whole.bam")
    sc.write_bam(bam, recs)
    rc, s0, err = sc.run_rules(checker, bam, [])
    assert rc == 0, err[-2000:]
    rc, s, err = sc.run_rules(checker, bam, ["--opt", "1,650,%d,100,300,500" % s0["stat0"]], os.path.join(tmp, "dump"))
    assert rc == 0, err[-2000:]
    out, err, status, _ = host_route(front, tmp, ISIZE)
    assert status == 0, err[-2000:]
    if out:
        assert b"STAT_%d_100_300_500_" % s0["stat0"] in out.split(b"\n")[0]
    return s, sc.read_tab(os.path.join(tmp, "dump")), out


PATTERNS = {                                                             # name: (states, error state)
    "no_host_pair": ([1, 0, 1, 1, 0, 1] * 6, None),
    "every_pair_host": ([2] * 40, None),
    "host_first_last_adjacent": ([2, 1, 1, 2, 2, 1, 0, 2, 2, 2, 1, 2] * 4 + [2], None),
    "alternating": ([1, 2, 1, 1, 2, 1, 2] * 16, None),
    "zeros_in_between": ([0, 1, 0, 0, 2, 0, 1, 2, 0] * 5, None),
    "error_pair": ([1, 2, 0, 1, 2, 1] * 3, 5),
    "error_pair_first": ([], 3),
    "empty_run": ([], None),
    "only_zeros": ([0] * 7, None),
}


def host_route(recs, tmp, flags=()):
    """(stdout, stderr, exit status) of `panSVR signal -N` on a BAM of these records, and the file's path"""
    bam = os.path.join(tmp, "in.bam")
    sc.write_bam(bam, recs)
    r = subprocess.run([sc.CLI, "signal", "-N"] + list(flags) + ["-H", os.path.join(tmp, "h.sam"), "-S", os.path.join(tmp, "s.txt"), bam], stdout=subprocess.PIPE,
                       stderr=subprocess.PIPE, timeout=300)
    return r.stdout, r.stderr, r.returncode, bam


def cut_by_table(stdout, tab):
    """[(state, text)] of the pairs in front of the first error pair: a state-1 pair has the table's bytes, a state-2 pair its eight lines"""
    out, at = [], 0
    for st, _, nb, _, _ in tab:
        if st >= 3:
            break
        end = at
        if st == 1:
            end = at + nb
        elif st == 2:
            for _ in range(8):
                end = stdout.index(b"\n", end) + 1
        out.append((st, stdout[at:end]))
        at = end
    assert at == len(stdout)
    return out


def sized_records(n_fill):
    """81 pairs in states 1, 1, 2, 0, ...; the last one's first read carries an XA string of n_fill bytes, which the text repeats once: the
    host text of sized_records(n) has n bytes more than that of sized_records(0)"""
    rng = np.random.RandomState(11)
    recs = []
    for k in range(80):
        recs += pair_in_state([1, 1, 2, 0][k % 4], "q%d" % k + "x" * (k % 17), rng, L=60 + k % 41)
    return recs + pair_in_state(1, "fill", np.random.RandomState(12), L=50, xa="x" * n_fill)
