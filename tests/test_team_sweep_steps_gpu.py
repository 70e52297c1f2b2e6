"""-m gpu: the team sweep (extd2_team_kernel) at the places where a value that one step hands to the next can be dropped, stored twice
or stored from the wrong lane.  A step of the sweep stores what the step BEFORE computed -- its direction bytes, and in the lean
instantiation its strip-boundary dword or its last-column H -- together with the loads for the step after, and whatever the last step
of a strip left is flushed behind the loop.  So: queries so short that the flush carries everything, every strip count with the
boundary hand-over in both ping-pong directions and its absence in the last strip, the last target column owned by the team's first or
second lane, wavefronts whose lanes reach their last row in different steps, batches that do not fill a wavefront, the largest shapes,
N bases, every flag the kernel implements, score-only runs (the cluster has no direction-byte store) and z-drops that cut the rules
short.  Every case is held to the oracle field by field and CIGAR word by word, and to ksw_regimes.route: none may pass by running in
another kernel.  The whole list runs through the full instantiation and, with the aln path's parameters, through the lean one."""
import numpy as np
import pytest

import ksw_regimes as kr
from ksw_cases import DEF, case, mat5, mutate, rand_seq
from ksw_ref import EZ_FIELDS, run_oracle
from test_oracle_ksw import diff

pytestmark = pytest.mark.gpu

FLAGS = [0, 0x40, 0x80, 0xC0, 0x01]
ZDROPS = [400, 30, 10, 3]
LEAN_SKIP = ("max", "max_q", "max_t")


def run_gpu(cases, variant="extd2"):
    from pansvr_amd import ksw
    groups = {}
    for i, c in enumerate(cases):
        key = (c["m"], c["match"], c["mismatch"], c["q"], c["e"], c["q2"], c["e2"], c["w"], c["zdrop"], c["end_bonus"], c["flag"])
        groups.setdefault(key, []).append(i)
    out = [None] * len(cases)
    for key, ids in groups.items():
        m, match, mismatch, q, e, q2, e2, w, zdrop, end_bonus, flag = key
        p = ksw.make_params(m, mat5(match, mismatch), q, e, q2, e2, w, zdrop, end_bonus, flag)
        res = ksw.ext_batch([cases[i]["query"] for i in ids], [cases[i]["target"] for i in ids], p, variant)
        for i, r in zip(ids, res):
            out[i] = r
    return out


def shape_list():
    """(qlen, tlen), every one with max(qlen, tlen) > 16 (smaller problems are the thread-per-alignment kernel's)"""
    shapes = [(ql, tl) for ql in (1, 2, 3, 4) for tl in (17, 18, 23, 24, 25, 31, 32, 33, 47, 48, 49)]   # main loop of 0, 1, 2 iterations
    shapes += [(ql, tl) for ql in range(17, 41) for tl in (1, 7, 8, 9, 15, 16)]                        # one strip
    shapes += [(ql, tl) for ql in (5, 18, 41) for tl in range(17, 33)]                                 # two strips, every tlen mod 16
    shapes += [(ql, tl) for ql in (5, 18, 41) for tl in range(33, 49)]                                 # three strips
    shapes += [(ql, tl) for ql in (190, 199, 200) for tl in (17, 33, 150, 201)]                        # the largest
    assert all(max(ql, tl) > 16 for ql, tl in shapes)
    return shapes


def pair(rng, ql, tl):
    """a query and a target that is related to it two times in three, both with an occasional N"""
    q = rand_seq(rng, ql)
    if rng.randint(3):
        t = (mutate(rng, q, 0.04, 0.02, 0.02) + rand_seq(rng, tl))[:tl]
    else:
        t = rand_seq(rng, tl)
    t = [int(x) for x in t]
    if rng.randint(6) == 0:
        t[rng.randint(tl)] = 4
    if rng.randint(6) == 0:
        q[rng.randint(ql)] = 4
    return q, t


def assert_team(c):
    p = kr.pset("team_sweep_steps", **{k: c[k] for k in DEF if k != "flag"})
    assert kr.route(p, c["flag"], "extd2", len(c["query"]), len(c["target"])) == "extd2_team_kernel", (c["flag"], len(c["query"]), len(c["target"]))


def mismatches(cases, got, skip=()):
    """field by field, CIGAR word by word, against the oracle (computed once per case)"""
    bad = []
    for i, (c, g) in enumerate(zip(cases, got)):
        want = c.setdefault("_want", run_oracle({k: v for k, v in c.items() if k != "_want"}, "extd2"))
        wrong = [f for f in EZ_FIELDS if f not in skip and g[f] != want[f]]
        if len(g["cigar"]) != len(want["cigar"]) or any(a != b for a, b in zip(g["cigar"], want["cigar"])):
            wrong.append("cigar")
        if wrong:
            bad.append((i, c["flag"], c["zdrop"], len(c["query"]), len(c["target"]), wrong, diff(want, g)))
    return bad


def full_cases():
    rng = np.random.RandomState(51017)
    cases = []
    for rep in range(3):
        for ql, tl in shape_list():
            q, t = pair(rng, ql, tl)
            cases.append(case(q, t, flag=int(rng.choice(FLAGS)), zdrop=int(rng.choice(ZDROPS))))
    return cases


def lean_cases():
    rng = np.random.RandomState(51018)
    return [case(*pair(rng, ql, tl)) for rep in range(3) for ql, tl in shape_list()]     # ksw_cases.DEF: the aln path's parameters


def wavefront_batches(rng, **kw):
    """batches that share one parameter set, so each is planned on its own: 32 alignments of one strip class whose queries run from 17 to
    48 rows (one wavefront, whose lanes reach their last row in different steps) at four, three and two strips; 45 alignments (a full
    wavefront and a partial one); a single alignment"""
    out = []
    for tl in (56, 40, 24):
        out.append([case(*pair(rng, ql, tl), **kw) for ql in rng.permutation(np.arange(17, 49))])
    out.append([case(*pair(rng, ql, 40), **kw) for ql in rng.permutation(np.arange(17, 62))])
    out.append([case(*pair(rng, 29, 40), **kw)])
    return out


def test_gpu_full_team_kernel_steps_match_oracle():
    cases = full_cases()
    assert {c["flag"] for c in cases} == set(FLAGS) and {c["zdrop"] for c in cases} == set(ZDROPS)
    for c in cases:
        assert_team(c)
    bad = mismatches(cases, run_gpu(cases))
    assert not bad, "%d/%d mismatches, first: %r" % (len(bad), len(cases), bad[:3])


def test_gpu_full_team_kernel_mixed_wavefronts_match_oracle():
    rng = np.random.RandomState(51019)
    n = 0
    for flag in FLAGS:
        for zdrop in (400, 10):
            for batch in wavefront_batches(rng, flag=flag, zdrop=zdrop):
                for c in batch:
                    assert_team(c)
                bad = mismatches(batch, run_gpu(batch))
                assert not bad, "flag %#x zdrop %d batch of %d: %d mismatches, first: %r" % (flag, zdrop, len(batch), len(bad), bad[:3])
                n += len(batch)
    assert n == 10 * (3 * 32 + 45 + 1)


def test_gpu_lean_team_kernel_steps_match_oracle(monkeypatch):
    """PSVR_DP_FORCE_LEAN routes psvr_extd2_batch through the instantiation the engine's own launches run: it keeps no per-anti-diagonal
    maximum, so max / max_q / max_t are not produced; every other field and the CIGAR are the oracle's."""
    monkeypatch.setenv("PSVR_DP_FORCE_LEAN", "1")
    cases = lean_cases()
    for c in cases:
        assert_team(c)
    bad = mismatches(cases, run_gpu(cases), skip=LEAN_SKIP)
    assert all(c["_want"]["zdropped"] == 0 for c in cases)            # what makes the lean instantiation legal
    assert not bad, "%d/%d mismatches, first: %r" % (len(bad), len(cases), bad[:3])


def test_gpu_lean_team_kernel_mixed_wavefronts_match_oracle(monkeypatch):
    monkeypatch.setenv("PSVR_DP_FORCE_LEAN", "1")
    rng = np.random.RandomState(51020)
    for rep in range(3):
        for batch in wavefront_batches(rng):
            for c in batch:
                assert_team(c)
            bad = mismatches(batch, run_gpu(batch), skip=LEAN_SKIP)
            assert all(c["_want"]["zdropped"] == 0 for c in batch)
            assert not bad, "batch of %d: %d mismatches, first: %r" % (len(batch), len(bad), bad[:3])
