"""The host planner of seam B2 (dp_plan_host, dp_plan.h) without a device: the plans of the regime sweep -- the batches
tests/test_ksw_regimes_gpu.py plans, the problems of over 8000 bases included -- held to the restated planner (ksw_regimes.route) and
to the restated sizes below.  Per problem the kernel is the restated one; the id list is a permutation; inside a team launch the query
length never increases and equal lengths keep ascending id; the slab offsets are the running sum of the slab sizes in problem order;
the scratch is the sum over the team launches."""
import os
import subprocess
import tempfile

import numpy as np
import pytest

import aln_common as ac
import ksw_regimes as kr

TEAM, TINY = 12, 11
SCORE_ONLY = 0x01


def p_bytes(ql, tl, w):
    return ((ql + tl - 1) * kr.n_col(ql, tl, w) + 1) * 16


def r256(x):
    return (x + 255) & ~255


def slab_bytes(name, ql, tl, w, v, with_cigar):
    """the slab slice of a problem the planner sends to kernel `name`: its direction bytes (a long problem without a CIGAR has none),
    for extd2_hbm_kernel also the flat image (8 or 6 arrays of T bytes and the query, 16-aligned, then 4 T bytes of H)"""
    is_long = ql > 8000 or tl > 8000
    dirs = r256(p_bytes(ql, tl, w)) if with_cigar or not is_long else 0
    if name.endswith("hbm_kernel"):
        T, QL = (tl + 15) // 16 * 16, (ql + 15) // 16 * 16
        return dirs + r256((((8 if v == 0 else 6) * T + QL + 16 + 15) & ~15) + 4 * T)
    if ",hbm>" in name or "ring" in name or name.endswith("lds_kernel"):
        return dirs
    return 0


def team_class_ws(cls, count, qmax):
    """scratch of a team class: wavefronts of 32 alignments (2 lanes each, 8 columns per lane), each with a slice for the class's
    longest query: 64 x 8 direction bytes per step and strip, 20 bytes per row / diagonal and alignment"""
    strips, q = cls + 1, max(qmax, 1)
    return (count * 2 + 63) // 64 * (512 * strips * (q + 15) + 32 * 20 * (q + 16 * strips + 1))


def plans_of(batches):
    """batches: (parameter set, flag, variant index, [(qlen, tlen)]) -> per batch (rc, slab, ws, launches, idx, poff)"""
    exe = os.path.join(tempfile.mkdtemp(prefix="psvr_hostplan_"), "dp_host_plan_check")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-Wno-unused-variable", "-Wno-unused-function", "-o", exe, os.path.join(ac.HERE, "tools", "dp_host_plan_check.cpp")])
    return parse_plans(batches, subprocess.run([exe], input=tool_input(batches).encode(), stdout=subprocess.PIPE, check=True).stdout.decode())


def tool_input(batches):
    text = []
    for p, flag, v, shapes in batches:
        text.append("%d %d %d %d %d %d %d %d %d %d %d" % (v, p["m"], p["q"], p["e"], p["q2"], p["e2"], p["w"], p["zdrop"], p["end_bonus"], flag, len(shapes)))
        text.append(" ".join(str(int(x)) for x in p["mat"]))
        text.append(" ".join("%d %d" % s for s in shapes))
    return "\n".join(text)


def parse_plans(batches, out):
    out = out.split("\n")
    plans, at = [], 0
    for _ in batches:
        head = out[at].split()
        assert head[0] == "plan"
        rc, slab, ws, m = (int(x) for x in head[1:])
        launches = [l.split() for l in out[at + 1:at + 1 + m]]
        launches = [tuple(int(x) for x in l[:5]) + (l[5],) for l in launches]
        idx, poff = out[at + 1 + m].split(), out[at + 2 + m].split()
        assert idx[0] == "idx" and poff[0] == "poff"
        plans.append((rc, slab, ws, launches, [int(x) for x in idx[1:]], [int(x) for x in poff[1:]]))
        at += m + 3
    return plans


def check_plan(p, flag, v, shapes, plan):
    rc, slab, ws, launches, idx, poff = plan
    n, w = len(shapes), p["w"]
    assert rc == 0
    assert sorted(idx) == list(range(n)), "the id list is not a permutation"
    # the launches tile the id list; a problem's kernel is its launch's
    assert launches[0][2] == 0 if n else not launches
    assert all(a[2] + a[3] == b[2] for a, b in zip(launches, launches[1:])) and (not n or launches[-1][2] + launches[-1][3] == n)
    assert len({(L[0], L[1]) for L in launches}) == len(launches)
    name = [None] * n
    want_ws = 0
    for kind, cls, first, count, qmax, kernel in launches:
        ids = idx[first:first + count]
        assert count > 0
        for i in ids:
            name[i] = kernel
        if kind != TEAM:
            assert qmax == 0
            continue
        # inside a team launch the query length never increases, and equal lengths keep ascending id
        key = [(-shapes[i][0], i) for i in ids]
        assert key == sorted(key), (p["tag"], flag, cls)
        assert all((shapes[i][1] + 15) // 16 - 1 == cls for i in ids) and qmax == max(shapes[i][0] for i in ids)
        want_ws += team_class_ws(cls, count, qmax)
    team = [L for L in launches if L[0] == TEAM]
    assert launches[len(launches) - len(team):] == team, "the team launches are not last"
    assert name == [kr.route(p, flag, kr.VARIANTS[v], ql, tl) for ql, tl in shapes], (p["tag"], flag, v)
    # slab offsets: the running sum of the routed slab sizes in problem order (a problem without a slice has offset 0)
    acc = 0
    for i, (ql, tl) in enumerate(shapes):
        b = slab_bytes(name[i], ql, tl, w, v, not (flag & SCORE_ONLY))
        assert b % 256 == 0 and poff[i] == (acc if b else 0) and poff[i] % 256 == 0, (p["tag"], flag, v, i, name[i], b, poff[i], acc)
        acc += b
    assert slab == acc
    assert ws == want_ws, "the plan's scratch is not the sum over its team launches"
    return name


def sweep_batches():
    """every batch of the regime sweep (shapes only: the plan does not read the sequences), the problems of over 8000 bases one per
    batch as the GPU sweep plans them, and larger mixed batches: many ties, queries beyond 200 bases with no band and a wide one"""
    batches = [(p, flag, kr.VARIANTS.index(variant), [s for s, _ in kr.batch_picks(b)[1]]) for b in kr.batches() for _, p, flag, variant in [b]]
    n_sweep = len(batches)
    for tag, ql, tl, w, flags, variants in kr.SPECIAL:
        for flag in flags:
            for variant in variants:
                batches.append((dict(kr.pset("special"), w=w), flag, kr.VARIANTS.index(variant), [(ql, tl)]))
    n_special = len(batches) - n_sweep
    rng = np.random.RandomState(kr.SEED + 7)
    sets = {p["tag"]: p for p in kr.param_sets()}
    for tag in ("plain", "w-1", "ring_w223", "ring_w224", "w16", "w15", "skip_35"):
        for flag in (0, SCORE_ONLY, 0x02):
            for v in (0, 1):
                shapes = [(int(rng.randint(0, 260)), int(rng.randint(0, 215))) for _ in range(300)]
                shapes += [(int(rng.randint(200, 3000)), int(rng.randint(1, 209))) for _ in range(40)]       # no band: the team kernel at any query length
                shapes += [(int(rng.choice((50, 120, 250))), int(rng.randint(17, 49))) for _ in range(60)]    # ties inside a class
                shapes += [(int(rng.randint(300, 700)), int(rng.randint(300, 700))) for _ in range(20)]
                shapes += [(9000, 9050), (150, 17000), (0, 9000), (20000, 20000)]
                batches.append((sets[tag], flag, v, shapes))
    return batches, n_sweep, n_special


@pytest.fixture(scope="module")
def sweep():
    batches, n_sweep, n_special = sweep_batches()
    return batches, plans_of(batches), n_sweep, n_special


def test_every_plan_is_what_the_restated_planner_says(sweep):
    batches, plans, n_sweep, n_special = sweep
    assert n_sweep == len(kr.param_sets()) * len(kr.FLAGS) * 2 and n_special == len(kr.special_cases())
    seen = {}
    for k, ((p, flag, v, shapes), plan) in enumerate(zip(batches, plans)):
        for nm in check_plan(p, flag, v, shapes, plan):
            if k < n_sweep + n_special:
                seen[nm] = seen.get(nm, 0) + 1
    # the sweep reaches every kernel family (as the GPU sweep asserts of the plans it reads back)
    assert set(seen) == set(kr.KERNEL_NAMES), (sorted(set(kr.KERNEL_NAMES) - set(seen)), sorted(set(seen) - set(kr.KERNEL_NAMES)))
    assert sum(seen.values()) == n_sweep * kr.CAP + n_special


def test_team_order_is_a_stable_sort_beyond_200_bases(sweep):
    """the mixed batches hold what the sweep's twelve problems a batch cannot: team classes with ties in the query length, and with no
    band (w < 0) or a wide one (w > 200) queries longer than the engine's 200 bins"""
    batches, plans, n_sweep, n_special = sweep
    ties = long_q = 0
    for (p, flag, v, shapes), plan in zip(batches[n_sweep + n_special:], plans[n_sweep + n_special:]):
        for kind, cls, first, count, qmax, kernel in plan[3]:
            if kind == TEAM:
                q = [shapes[i][0] for i in plan[4][first:first + count]]
                ties += len(q) - len(set(q))
                long_q += sum(1 for x in q if x > 200)
    assert ties > 0 and long_q > 0, (ties, long_q)


def test_empty_batch():
    (rc, slab, ws, launches, idx, poff), = plans_of([(kr.pset("plain"), 0, 0, [])])
    assert rc == 0 and not launches and not idx and not poff and slab == ws == 0
