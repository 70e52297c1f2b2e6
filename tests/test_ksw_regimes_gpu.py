"""-m gpu: seam B2 (psvr_extd2_batch / psvr_extz2_batch) over the regime-directed sweep of tests/ksw_regimes.py against the oracle
(which tests/test_oracle_ksw.py holds to the reference library over the same sweep): every result field and the CIGAR.

The sweep is one batch per (parameter set, flag combination, variant) -- parameter sets on both sides of every routing predicate
(tests/test_ksw_regimes.py asserts that on the CPU) -- with ksw_regimes.CAP problems each, drawn from shapes x sequence kinds, plus
the problems of over 8000 bases.  Nothing is filtered out: skip-regime sets must return what the reference returns right after
ksw_reset_extz.  The test reads every batch's plan (psvr_dp_plan_describe), holds it to the restated planner (ksw_regimes.route)
and asserts at the end that every kernel family ran.

Size: 66 parameter sets x 19 flag combinations x 2 variants x CAP = 12 problems, plus 11 problems of over 8000 bases: 30 107 problems.
Measured on the MI355X in a run of the whole GPU suite (145 tests, 433 s): this sweep 11.5 s (the oracle's answers included).  The
ten tests of tests/test_ksw_gpu.py were not timed on their own: none is among that run's 25 slowest tests, the last of which took
3.70 s, so the file takes under 37 s.  CAP = 12 was set before any measurement, from an estimate (about 2 500 batches of a few
milliseconds each and a millisecond of oracle per problem), and was kept when the sweep came out at 11.5 s, below that file's bound.
Kernel families of that run (problems): extd2_lds_kernel 10458, extz2_lds_kernel 14364, extd2_reg_kernel<1,lds> 2173 (the skip
regime's answers among them), <2,lds> 41, <1,hbm> 93, <2,hbm> 49, <3,hbm> 49, <4,hbm> 306, <5,hbm> 313, extd2_team_kernel 1325,
extd2_tiny_kernel 593, extd2_ring_kernel<3> 94, <4> 240, extd2_ring1_kernel<3> 2, <4> 2, extd2_hbm_kernel 2, extz2_hbm_kernel 3; zero
mismatches, every plan as the restated planner says.  extd2_reg_kernel<3..5,lds> cannot be planned (ksw_regimes.KERNEL_NAMES)"""
import ctypes as C
import json
import os
import re
import subprocess
import sys
import time

import numpy as np
import pytest

import ksw_regimes as kr
from ksw_ref import run_oracle
from test_oracle_ksw import diff

pytestmark = pytest.mark.gpu


def describe(cases, variant):
    """kernel name -> problems, from the plan of this batch"""
    from pansvr_amd._lib import check, lib
    L = lib()
    par = kr.ksw_params(cases[0])
    qa, ta = np.array([len(c["query"]) for c in cases], np.int32), np.array([len(c["target"]) for c in cases], np.int32)
    plan = C.c_void_p()
    check(L.psvr_dp_plan_create(0, C.c_int64(len(cases)), qa.ctypes.data_as(C.c_void_p), ta.ctypes.data_as(C.c_void_p), C.byref(par), kr.VARIANTS.index(variant), C.byref(plan)))
    buf = C.create_string_buffer(4096)
    check(L.psvr_dp_plan_describe(plan, buf, 4096))
    L.psvr_dp_plan_destroy(plan)
    out = {}
    for name, count in re.findall(r"(\S+?)\[lds=\d+\] x(\d+); ", buf.value.decode()):
        out[name] = out.get(name, 0) + int(count)
    return out


def predicted(p, cases, variant):
    out = {}
    for c in cases:
        name = kr.route(p, c["flag"], variant, len(c["query"]), len(c["target"]))
        out[name] = out.get(name, 0) + 1
    return out


def run_batch(cases, variant):
    from pansvr_amd import ksw
    return ksw.ext_batch([c["query"] for c in cases], [c["target"] for c in cases], kr.ksw_params(cases[0]), variant)


def test_regime_sweep_matches_oracle_on_every_kernel_family():
    t0 = time.time()
    seen, bad, misrouted, n = {}, [], [], 0
    for b in kr.batches():
        _, p, flag, variant = b
        cases = kr.batch_cases(b)
        plan = describe(cases, variant)
        if plan != predicted(p, cases, variant):
            misrouted.append((p["tag"], flag, variant, plan, predicted(p, cases, variant)))
        for name, count in plan.items():
            seen[name] = seen.get(name, 0) + count
        for c, g in zip(cases, run_batch(cases, variant)):
            want = run_oracle(c, variant)
            n += 1
            if g != want:
                bad.append((p["tag"], flag, variant, len(c["query"]), len(c["target"]), kr.route(p, flag, variant, len(c["query"]), len(c["target"])), diff(want, g)))
    for tag, variant, c in kr.special_cases():
        p = dict(kr.pset("special"), w=c["w"])
        plan = describe([c], variant)
        if plan != predicted(p, [c], variant):
            misrouted.append((tag, c["flag"], variant, plan, predicted(p, [c], variant)))
        for name, count in plan.items():
            seen[name] = seen.get(name, 0) + count
        want = run_oracle(c, variant, cap=len(c["query"]) + len(c["target"]) + 16)
        g = run_batch([c], variant)[0]
        n += 1
        if g != want:
            bad.append((tag, c["flag"], variant, len(c["query"]), len(c["target"]), sorted(plan), diff(want, g)))
    print("regime sweep: %d problems in %.1f s; kernel families: %s" % (n, time.time() - t0, ", ".join("%s x%d" % kv for kv in sorted(seen.items()))))
    assert not bad, "%d/%d mismatches, first: %r" % (len(bad), n, bad[:3])
    assert not misrouted, "%d batches planned otherwise than the restated planner says, first: %r" % (len(misrouted), misrouted[:2])
    assert set(seen) == set(kr.KERNEL_NAMES), (sorted(set(kr.KERNEL_NAMES) - set(seen)), sorted(set(seen) - set(kr.KERNEL_NAMES)))
    assert n == sum(seen.values()) == len(kr.batches()) * kr.CAP + len(kr.special_cases())


def test_named_int8_wrap_case_matches_oracle():
    """kr.int8_wrap_case (17+0k | 16+1k, 200 N against 201): the reference's int8 lanes wrap, so the problem must not be planned on the
    team kernel (which returned -65 for the reference's -66 while nowrap_ok was the int8 bound alone) and must return the oracle's record."""
    for flag in (0, 0x01, 0x80):
        c = kr.int8_wrap_case(flag)
        assert sorted(describe([c], "extd2")) == ["extd2_reg_kernel<4,hbm>"]
        want = run_oracle(c, "extd2")
        assert want["score"] == -66
        got = run_batch([c], "extd2")[0]
        assert got == want, diff(want, got)


def test_lean_team_variant_matches_oracle_in_both_pair_orders():
    """The team kernel's LEAN variant (no per-diagonal maximum; what the engine's own DP launches run when dp_zdrop_inert holds) through
    PSVR_DP_FORCE_LEAN in a child process, on parameter sets the library calls inert: pairs in plain order and swapped, thresholds at
    the rule's edge and far from it.  It does not produce ez.max / max_q / max_t; every other field and the CIGAR are the oracle's, and
    the oracle must not z-drop on any of these (the variant could not say so)."""
    sets = kr.lean_sets()
    assert {kr.regime(p, "extd2")["swapped"] for p in sets} == {0, 1}
    assert all(kr.library_regime(p, "extd2")["zdrop_inert"] for p in sets)
    r = subprocess.run([sys.executable, os.path.join(os.path.dirname(os.path.abspath(__file__)), "ksw_regimes.py")], stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                       env=dict(os.environ, PSVR_DP_FORCE_LEAN="1"))
    assert r.returncode == 0, r.stderr.decode()[-2000:]
    got = json.loads(r.stdout.decode())
    cases = kr.lean_cases()
    assert len(got) == len(cases) == len(sets) * len(kr.LEAN_FLAGS) * len(kr.LEAN_SHAPES)
    skip = ("max", "max_q", "max_t")
    bad, dropped = [], []
    for i, (c, g) in enumerate(zip(cases, got)):
        assert kr.route(c, c["flag"], "extd2", len(c["query"]), len(c["target"])) == "extd2_team_kernel"
        want = run_oracle(c, "extd2")
        if want["zdropped"]:
            dropped.append((i, {k: c[k] for k in ("q", "e", "q2", "e2", "zdrop")}))
        if {k: v for k, v in want.items() if k not in skip} != {k: v for k, v in g.items() if k not in skip}:
            bad.append((i, {k: c[k] for k in ("q", "e", "q2", "e2", "zdrop", "flag")}, len(c["query"]), len(c["target"]), diff(want, g)))
    assert not dropped, "the oracle z-drops under parameters dp_zdrop_inert accepts: %r" % dropped[:3]
    assert not bad, "%d/%d mismatches, first: %r" % (len(bad), len(cases), bad[:3])
