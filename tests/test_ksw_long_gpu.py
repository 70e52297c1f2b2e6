"""-m gpu: seam B2 on sequences longer than 8000 bases (the ring kernels with long images, extd2_ring1_kernel, extd2_hbm_kernel,
the host form's grouping under a workspace budget) against the reference kswlib (oracle/_ref/libref_ksw.so), or the oracle
restatement where that library was not built."""
import ctypes as C

import numpy as np
import pytest

from ksw_cases import case, mat5, mutate, rand_seq
from ksw_ref import ref_available, run_oracle, run_ref
from test_ksw_gpu import run_gpu
from test_oracle_ksw import diff, load_kat

pytestmark = pytest.mark.gpu

FC_SV = dict(match=2, mismatch=10, q=24, e=2, q2=32, e2=1, w=132, zdrop=132)
LONG = [7999, 8000, 8001, 8192, 12000, 20000]


def expect(c, variant="extd2"):
    if ref_available():
        return run_ref(c, variant)
    return run_oracle(c, variant, cap=len(c["query"]) + len(c["target"]) + 16)


def check(cases, variant="extd2"):
    got = run_gpu(cases, variant)
    bad = []
    for i, (c, g) in enumerate(zip(cases, got)):
        want = expect(c, variant)
        if g != want:
            bad.append((i, c["w"], c["flag"], len(c["query"]), len(c["target"]), diff(want, g)))
    assert not bad, "%d/%d mismatches, first: %r" % (len(bad), len(cases), bad[:3])
    return got


def pair(rng, ql, tl, diverge=False, n_bases=False):
    q = rand_seq(rng, ql)
    t = mutate(rng, q, 0.03, 0.01, 0.01, maxindel=20)
    t = (t + rand_seq(rng, tl))[:tl] if len(t) < tl else t[:tl]
    if diverge:          # a diverged stretch in the middle: z-drop fires there
        a = min(ql, tl) // 2
        t[a:a + 600] = rand_seq(rng, len(t[a:a + 600]))
    if n_bases:
        for _ in range(20):
            q[int(rng.randint(ql))] = 4
            t[int(rng.randint(tl))] = 4
    return q, t


def describe(ql, tl, variant=0, **kw):
    from pansvr_amd import ksw
    from pansvr_amd._lib import check as ok, lib
    k = dict(w=200, zdrop=400, flag=0)
    k.update(kw)
    p = ksw.make_params(5, mat5(2, 12), 16, 1, 32, 0, k["w"], k["zdrop"], -1, k["flag"])
    L = lib()
    plan = C.c_void_p()
    qa, ta = np.array([ql], np.int32), np.array([tl], np.int32)
    ok(L.psvr_dp_plan_create(0, C.c_int64(1), qa.ctypes.data_as(C.c_void_p), ta.ctypes.data_as(C.c_void_p), C.byref(p), variant, C.byref(plan)))
    buf = C.create_string_buffer(1024)
    L.psvr_dp_plan_describe(plan, buf, 1024)
    L.psvr_dp_plan_destroy(plan)
    return buf.value.decode()


def test_long_problems_are_planned_on_the_long_routes():
    assert "extd2_ring_kernel<4>" in describe(12000, 12000)
    assert "extd2_ring1_kernel<4>" in describe(20000, 20000)
    assert "extd2_ring1_kernel<3>" in describe(20000, 20000, w=132)
    assert "extd2_hbm_kernel" in describe(20000, 20000, w=-1)
    assert "extd2_hbm_kernel" in describe(100000, 100000, flag=1)
    assert "extz2_hbm_kernel" in describe(9000, 9000, variant=1)
    assert "extd2_hbm_kernel" in describe(9000, 9000, flag=0x08)
    # 8000 bases and fewer: the kinds they had
    assert "extd2_lds_kernel" in describe(8000, 8000, w=-1)
    assert "extd2_ring_kernel<4>" in describe(8000, 8000)


def test_lengths_across_the_old_limit():
    rng = np.random.RandomState(8001)
    cases = []
    for L in LONG:
        for ql, tl in ((L, L + int(rng.randint(-50, 50))), (L, 300), (300, L), (L, 40)):
            q, t = pair(rng, ql, tl)
            cases.append(case(q, t))                     # the `aln` parameters at w = 200
            cases.append(case(q, t, **FC_SV))
    check(cases)


def test_bands_zdrop_and_n_bases():
    rng = np.random.RandomState(20000)
    cases = []
    for ql, tl, w in ((12000, 12100, 500), (20000, 19900, 500), (12000, 11950, 1000), (20000, 20000, 1000), (9000, 9050, -1), (12000, 12000, -1), (8500, 3000, -1)):
        q, t = pair(rng, ql, tl, n_bases=True)
        cases.append(case(q, t, w=w))
    for zdrop in (400, 100, -1):
        for ql, w in ((15000, 200), (10000, 1000), (9000, -1)):
            q, t = pair(rng, ql, ql + 37, diverge=True)
            cases.append(case(q, t, w=w, zdrop=zdrop))
        q, t = pair(rng, 16000, 16020, diverge=True, n_bases=True)
        cases.append(case(q, t, zdrop=zdrop, **{k: v for k, v in FC_SV.items() if k != "zdrop"}))
    check(cases)


@pytest.mark.parametrize("variant", ["extd2", "extz2"])
def test_every_kat_flag(variant):
    flags = sorted(set(r["flag"] for r in load_kat()))
    assert len(flags) >= 11
    rng = np.random.RandomState(4242)
    cases = []
    for flag in flags:
        q, t = pair(rng, 9000, 9100, diverge=flag % 3 == 0)
        cases.append(case(q, t, flag=flag, zdrop=200))
        q, t = pair(rng, 8100, 8050)
        cases.append(case(q, t, flag=flag, w=-1))
    check(cases, variant)


@pytest.mark.parametrize("w", [200, 1000])
def test_mixed_batch_short_results_unchanged(w):
    """Short problems of every existing kernel family with long ones in one call: all equal the reference, and the short
    ones are identical to a call without the long ones."""
    from pansvr_amd import ksw
    rng = np.random.RandomState(77 + w)
    short = [(10, 12), (6, 6), (100, 130), (180, 181), (250, 300), (300, 320), (1500, 1530), (3100, 3000), (7000, 7100), (8000, 8000)]
    cases = []
    for k in range(60):
        ql, tl = short[k % len(short)]
        cases.append(case(*pair(rng, ql, tl), w=w))
    long_ids = []
    for ql, tl in ((8001, 8100), (20000, 20050), (12000, 300), (9000, 9000)):
        long_ids.append(len(cases))
        cases.append(case(*pair(rng, ql, tl), w=w))
    order = rng.permutation(len(cases))
    cases = [cases[i] for i in order]
    got = check(cases)
    is_long = set(int(np.where(order == i)[0][0]) for i in long_ids)
    p = ksw.make_params(5, mat5(2, 12), 16, 1, 32, 0, w, 400, -1, 0)
    short_ids = [i for i in range(len(cases)) if i not in is_long]
    alone = ksw.ext_batch([cases[i]["query"] for i in short_ids], [cases[i]["target"] for i in short_ids], p)
    assert [got[i] for i in short_ids] == alone


def test_score_only_100k():
    rng = np.random.RandomState(100000)
    q = rand_seq(rng, 100000)
    t = [x if rng.random_sample() > 0.04 else (x + 1) % 4 for x in q]   # substitutions only: the path stays in the band to the end
    got = check([case(q, t, flag=1)])
    assert got[0]["score"] > 0 and not got[0]["zdropped"] and got[0]["n_cigar"] == 0


def test_workspace_beyond_the_budget():
    """Six 20 000 x 20 000 unbanded problems with CIGAR: 4.8 GB of direction bytes, more than the host form's 4 GiB budget,
    run in groups and return the reference's answers."""
    from pansvr_amd import ksw
    rng = np.random.RandomState(6)
    q, t = pair(rng, 20000, 20000)
    c = case(q, t, w=-1)
    want = expect(c)
    p = ksw.make_params(5, mat5(2, 12), 16, 1, 32, 0, -1, 400, -1, 0)
    got = ksw.ext_batch([q] * 6, [t] * 6, p)
    bad = [(i, diff(want, g)) for i, g in enumerate(got) if g != want]
    assert not bad, bad[:2]
