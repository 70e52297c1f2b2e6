"""The order in which the engine's device planner lays out a round's DP problems (dp_plan_bucket / dp_plan_starts, engine_core.h),
computed on the host from a histogram: the team kernel's classes come longest first, inside a class the query length never
increases, and every problem has exactly one place."""
import os
import subprocess
import tempfile

import numpy as np

import aln_common as ac

TEAM, TINY = 12, 11
KIND_ORDER = [0, 14, 13, 10, 9, 8, 7, 6, 5, 4, 3, 2, 1, 11]


def starts_of(rows):
    exe = os.path.join(tempfile.mkdtemp(prefix="psvr_plan_"), "dp_plan_order_check")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-Wno-unused-variable", "-Wno-unused-function", "-DPSVR_NO_ENGINE_LIB", "-o", exe,
                           os.path.join(ac.HERE, "tools", "dp_plan_order_check.cpp"), "-lpthread"])
    text = "".join("%d %d %d %d\n" % r for r in rows)
    out = subprocess.run([exe], input=text.encode(), stdout=subprocess.PIPE, check=True).stdout.decode().split("\n")
    got = [tuple(int(x) for x in l.split()) for l in out[:len(rows)]]
    assert out[len(rows)].startswith("total ")
    return got, int(out[len(rows)].split()[1])


def histogram(seed):
    rng = np.random.RandomState(seed)
    rows = []
    for cls in range(13):                                        # team kernel: every class, a few hundred query lengths with gaps, 1 and 200 included
        qs = set(rng.randint(1, 201, size=40).tolist()) | {1, 200}
        rows += [(TEAM, cls, q, int(rng.randint(1, 50))) for q in sorted(qs)]
    for kind in KIND_ORDER:
        for cls in rng.choice(13, size=4, replace=False):
            rows.append((kind, int(cls), int(rng.randint(1, 1600)), int(rng.randint(1, 1000))))
    rng.shuffle(rows)
    return [tuple(int(x) for x in r) for r in rows]


def test_every_problem_has_one_place_and_the_order_holds():
    rows = histogram(3)
    got, total = starts_of(rows)
    assert total == sum(r[3] for r in rows)
    assert len({b for b, _ in got}) == len(rows), "two (kind, class, qlen) share a bucket"
    # the ranges [start, start + count) tile [0, total): every problem exactly once
    spans = sorted((st, st + r[3]) for (b, st), r in zip(got, rows))
    assert spans[0][0] == 0 and spans[-1][1] == total
    assert all(a[1] == b[0] for a, b in zip(spans, spans[1:]))
    by_start = sorted(zip((st for _, st in got), rows))
    seq = [r for _, r in by_start]
    # the wavefront / tiny kernels first, kind by kind in their launch order with the classes largest first; then the team kernel
    other = [r for r in seq if r[0] != TEAM]
    team = [r for r in seq if r[0] == TEAM]
    assert seq == other + team
    keys = [(KIND_ORDER.index(r[0]), -r[1]) for r in other]
    assert keys == sorted(keys)
    # team kernel: classes longest first, the query length never increases inside a class
    assert [r[1] for r in team] == sorted((r[1] for r in team), reverse=True)
    for cls in range(13):
        q = [r[2] for r in team if r[1] == cls]
        assert len(q) >= 2 and all(a > b for a, b in zip(q, q[1:])), (cls, q)


def test_bins_of_width_one():
    """Neighbouring query lengths of a class never share a bucket, the shortest and the longest included."""
    rows = [(TEAM, cls, q, 1) for cls in (0, 5, 12) for q in range(1, 201)]
    got, total = starts_of(rows)
    assert total == len(rows) and len({b for b, _ in got}) == len(rows)
    for cls_i, cls in enumerate((0, 5, 12)):
        st = [s for _, s in got[cls_i * 200:(cls_i + 1) * 200]]
        assert st == sorted(st, reverse=True)                      # longer query, earlier place
