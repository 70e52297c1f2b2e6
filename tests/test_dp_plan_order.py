"""The order in which the engine's device planner lays out a round's DP problems (dp_plan_bucket / dp_plan_starts, dp_plan.h),
computed on the host from a histogram: the team kernel's classes come longest first, inside a class the query length never
increases, and every problem has exactly one place.  And the launch lists both planners build from the same counts
(dp_launch_list): they tile that order, with the tiny kernel's classes merged (the engine) or a launch per class (seam B2), the
team kernel's classes last, and the scratch the planners reserve for them is what TeamLaunch::add hands out."""
import os
import subprocess
import tempfile

import numpy as np

import aln_common as ac
from ksw_regimes import LDS_CLASSES
from pansvr_amd.build import HIPCC

TEAM, TINY = 12, 11
KIND_ORDER = [0, 14, 13, 10, 9, 8, 7, 6, 5, 4, 3, 2, 1, 11]
TINY_SMALL_LDS = 4096
_exe = []


def run_tool(rows):
    """every line of the tool's output, as lists of words"""
    if not _exe:      # host code only: the tool includes ksw_launch.h (TeamLaunch), which needs the HIP headers, and calls nothing on a device
        exe = os.path.join(tempfile.mkdtemp(prefix="psvr_plan_"), "dp_plan_order_check")
        subprocess.check_call([HIPCC, "--offload-host-only", "-O1", "-std=c++17", "-Wall", "-Wno-unused-variable", "-Wno-unused-function", "-o", exe,
                               os.path.join(ac.HERE, "tools", "dp_plan_order_check.cpp")])
        _exe.append(exe)
    text = "".join("%d %d %d %d\n" % r for r in rows)
    return [l.split() for l in subprocess.run([_exe[0]], input=text.encode(), stdout=subprocess.PIPE, check=True).stdout.decode().split("\n")]


def starts_of(rows):
    out = run_tool(rows)
    got = [tuple(int(x) for x in l) for l in out[:len(rows)]]
    assert out[len(rows)][0] == "total"
    return got, int(out[len(rows)][1])


def launches_of(rows):
    """(bucket, start) per row, total, {"merged": [...], "plain": [...]} of (kind, class, first, count, qmax), the scratch sums"""
    out = run_tool(rows)
    got, total = starts_of(rows)
    at, lists = len(rows) + 1, {}
    for name in ("merged", "plain"):
        assert out[at][:2] == ["launches", name]
        m = int(out[at][2])
        lists[name] = [tuple(int(x) for x in l) for l in out[at + 1:at + 1 + m]]
        at += 1 + m
    assert out[at][:2] == ["ws", "shared"] and out[at + 1][:2] == ["ws", "next"]
    return got, total, lists, int(out[at][2]), int(out[at + 1][2])


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


def check_launch_lists(rows):
    got, total, lists, ws_shared, ws_next = launches_of(rows)
    start = {(r[0], r[1], r[2]): st for (b, st), r in zip(got, rows)}
    populated = sorted({(r[0], r[1]) for r in rows})
    count = {kc: sum(r[3] for r in rows if (r[0], r[1]) == kc) for kc in populated}
    first = {kc: min(st for (k, c, q), st in start.items() if (k, c) == kc) for kc in populated}
    for name, ls in lists.items():
        # the launches tile [0, total) in slot order: each begins where its first class's ids begin and where the one before it ended
        assert ls[0][2] == 0 and ls[-1][2] + ls[-1][3] == total, name
        assert all(a[2] + a[3] == b[2] for a, b in zip(ls, ls[1:])), name
        assert all(L[2] == first[(L[0], L[1])] for L in ls), name
        # the team launches come last, most strips first, each with its class's longest query
        team = [L for L in ls if L[0] == TEAM]
        assert ls[len(ls) - len(team):] == team and [L[1] for L in team] == sorted((c for k, c in populated if k == TEAM), reverse=True)
        for L in team:
            assert L[3] == count[(TEAM, L[1])] and L[4] == max(r[2] for r in rows if r[0] == TEAM and r[1] == L[1])
        assert all(L[4] == 0 for L in ls if L[0] != TEAM)
    # without the merge flag: one launch per populated (kind, class), in slot order
    plain = lists["plain"]
    assert sorted((L[0], L[1]) for L in plain) == populated and len(plain) == len(populated)
    assert all(L[3] == count[(L[0], L[1])] for L in plain)
    keys = [(KIND_ORDER.index(L[0]), -L[1]) for L in plain if L[0] != TEAM]
    assert keys == sorted(keys)
    # with it: the same launches but for the tiny kernel's, which are at most two, split at 4096 B, each at its largest populated class
    merged = lists["merged"]
    assert [L for L in merged if L[0] != TINY] == [L for L in plain if L[0] != TINY]
    tiny_cls = sorted((c for k, c in populated if k == TINY), reverse=True)
    want = []
    for side in ([c for c in tiny_cls if LDS_CLASSES[c] > TINY_SMALL_LDS], [c for c in tiny_cls if LDS_CLASSES[c] <= TINY_SMALL_LDS]):
        if side:
            want.append((TINY, side[0], first[(TINY, side[0])], sum(count[(TINY, c)] for c in side), 0))
    assert [L for L in merged if L[0] == TINY] == want and len(want) <= 2
    # the scratch the planners reserve (the shared function, class by class) is what TeamLaunch::add hands out
    assert ws_shared == ws_next > 0
    return lists


def test_launch_lists_tile_the_order():
    rows = histogram(3)
    check_launch_lists(rows)
    # tiny classes on both sides of the split, the two at the split among them (classes 1 and 2: 4096 and 6144 B); counts at which a
    # team class ends in a part-filled wavefront, fills one exactly and is a single problem
    rows = [(TINY, c, 5, n) for c, n in ((0, 7), (1, 300), (2, 11), (5, 2), (12, 1))] + [(0, 3, 900, 4), (6, 0, 60, 9), (14, 9, 700, 2)]
    rows += [(TEAM, 12, 200, 33), (TEAM, 12, 1, 1), (TEAM, 4, 77, 32), (TEAM, 0, 9, 1)]
    lists = check_launch_lists(rows)
    assert [(L[1], L[3]) for L in lists["merged"] if L[0] == TINY] == [(12, 14), (1, 307)]
    # one side only
    check_launch_lists([(TINY, 0, 3, 5), (TINY, 1, 3, 6), (TEAM, 3, 50, 10)])
    check_launch_lists([(TINY, 7, 3, 5), (TEAM, 3, 50, 10)])
