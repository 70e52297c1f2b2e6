"""CPU checks of the regime-directed DP sweep (tests/ksw_regimes.py) and of the rule that lets the engine run the lean team kernel:
(1) the sweep's restated predicates equal the library's own (psvr_dp_regime) on every parameter set;
(2) the sweep holds parameter sets on both sides of every routing predicate, and problems for every kernel family;
(3) whatever parameter set the library's dp_zdrop_inert accepts, the reference never z-drops on adversarial inputs."""
import numpy as np
import pytest

import ksw_regimes as kr
from ksw_cases import mutate, rand_seq
from ksw_ref import ref_available, run_oracle, run_ref


def test_restated_predicates_equal_the_librarys():
    n = 0
    for p in kr.param_sets() + [kr.lean_swapped_400()]:
        for variant in kr.VARIANTS:
            mine, lib = kr.regime(p, variant), kr.library_regime(p, variant)
            for k in ("skip", "swapped", "nowrap_ok", "long_thres", "qe_shift"):
                assert mine[k] == lib[k], (p["tag"], variant, k, mine, lib)
            n += 1
    assert n >= 100


def test_sweep_holds_both_sides_of_every_predicate():
    S = {p["tag"]: p for p in kr.param_sets()}
    R = {t: kr.regime(p, "extd2") for t, p in S.items()}
    L = {t: kr.library_regime(p, "extd2") for t, p in S.items()}
    # nowrap_ok: the bound at 125, 126, 127 | 128, 129 through each of the four routes, and the predicate flips exactly between 127 and 128
    for route in ("bound_match_", "bound_mismatch_", "bound_pair2_", "bound_pair1_"):
        got = {kr.int8_bound(p): L[t]["nowrap_ok"] for t, p in S.items() if t.startswith(route)}
        assert got == {125: 1, 126: 1, 127: 1, 128: 0, 129: 0}, (route, got)
    assert all(R[t]["swapped"] == (1 if t.startswith("bound_pair1_") else 0) for t in S if t.startswith("bound_"))
    # the swap: plain, swapped, equal sums (no swap) in both orders, e == e2 (long_thres = 0) in both orders
    assert (R["plain"]["swapped"], R["swapped"]["swapped"], R["equal_sums"]["swapped"], R["equal_sums_other_order"]["swapped"]) == (0, 1, 0, 0)
    assert S["equal_sums"]["q"] + S["equal_sums"]["e"] == S["equal_sums"]["q2"] + S["equal_sums"]["e2"]
    # (e == e2 starts long_thres at 0 instead of dividing by e - e2; the step after it makes it 1, the second pair still costing more)
    assert all(S[t]["e"] == S[t]["e2"] for t in ("e_eq_e2", "e_eq_e2_swapped"))
    assert (R["e_eq_e2"]["long_thres"], R["e_eq_e2_swapped"]["long_thres"], R["e_eq_e2_swapped"]["swapped"]) == (1, 1, 1)
    assert R["plain"]["long_thres"] > 0
    # nowrap_ok's second condition, with the int8 bound far away: e > e2 | e == e2 (q2 > q: off; same pairs: on) | e < e2
    for t, want in (("plain", 1), ("swapped", 1), ("equal_sums", 1), ("same_pairs", 1), ("e_eq_e2", 0), ("e_eq_e2_swapped", 0), ("e_lt_e2", 0), ("e_lt_e2_swapped", 0),
                    ("equal_sums_other_order", 0)):
        assert kr.int8_bound(S[t]) <= 127 and (R[t]["boundary_ok"], L[t]["nowrap_ok"]) == (want, want), t
    # e2 == 0 after the swap: zdrop at 2 q2 - 1 | 2 q2 | 2 q2 + shift - 1 | 2 q2 + shift; the library's rule accepts the last only
    for stem, zs in (("inert_plain_z", (63, 64)), ("inert_swapped_z", (63, 64, 78, 79)), ("inert_swapped_small_z", (39, 40, 47, 48))):
        r = R[stem + str(zs[0])]
        q2, shift = r["post"][2], r["qe_shift"]
        assert r["post"][3] == 0 and sorted(set((2 * q2 - 1, 2 * q2, 2 * q2 + shift - 1, 2 * q2 + shift))) == list(zs)
        assert [L[stem + str(z)]["zdrop_inert"] for z in zs] == [int(z >= 2 * q2 + shift) for z in zs], stem
        assert (shift > 0) == ("swapped" in stem) == bool(r["swapped"])
    assert L["zdrop_off"]["zdrop_inert"] == 1 and L["zdrop_10"]["zdrop_inert"] == 0 and L["e_eq_e2"]["zdrop_inert"] == 0
    # the skip rule: -min_sc = 2(q+e) | 2(q+e) + 1
    for edge, over in (("skip_edge_34", "skip_35"), ("skip_edge_small_10", "skip_small_11")):
        q, e = R[edge]["post"][:2]
        assert S[edge]["mismatch"] == 2 * (q + e) and S[over]["mismatch"] == 2 * (q + e) + 1
        assert (L[edge]["skip"], L[over]["skip"]) == (0, 1)
    assert L["skip_edge_small_10"]["nowrap_ok"] == 1
    # alphabet sizes for both variants, band widths, N score, end bonus
    assert {p["m"] for p in S.values()} == {0, 1, 2, 5}
    assert [kr.library_regime(S["m%d" % m], v)["skip"] for m in (0, 1, 2) for v in kr.VARIANTS] == [1, 1, 1, 0, 0, 0]
    assert {p["w"] for p in S.values()} >= {-1, 0, 1, 15, 16, 17, 200, 159, 160, 223, 224}
    assert {p["mat"][24] for p in S.values() if p["m"] == 5} >= {0, -3, 1}
    assert {p["end_bonus"] for p in S.values()} == {-1, 0, 5}


def test_default_parameters_stay_lean():
    """the `aln` path's defaults (2/-12, 16+1k | 32+0k, zdrop 400): the engine's DP launches keep the lean team kernel"""
    r = kr.library_regime(kr.pset("defaults"), "extd2")
    assert r["zdrop_inert"] == 1 and r["nowrap_ok"] == 1 and r["skip"] == 0 and r["swapped"] == 0 and r["qe_shift"] == 0
    assert kr.route(kr.pset("defaults"), 0, "extd2", 150, 180) == "extd2_team_kernel"
    # the extension-only flag stops at the z-drop, so the rule is refused there
    assert kr.library_regime(dict(kr.pset("defaults"), flag=0x40), "extd2")["zdrop_inert"] == 0


def test_sweep_reaches_every_kernel_family_flag_shape_and_kind():
    names, flags_by_name = set(), {}
    shapes, kinds, n = set(), set(), 0
    for b in kr.batches():
        _, p, flag, variant = b
        for (ql, tl), kind in kr.batch_picks(b)[1]:
            name = kr.route(p, flag, variant, ql, tl)
            names.add(name)
            flags_by_name.setdefault(name, set()).add(flag)
            shapes.add((ql, tl)), kinds.add(kind)
            n += 1
    for tag, variant, c in kr.special_cases():
        names.add(kr.route(dict(kr.pset("special"), w=c["w"]), c["flag"], variant, len(c["query"]), len(c["target"])))
    assert names == set(kr.KERNEL_NAMES), (sorted(set(kr.KERNEL_NAMES) - names), sorted(names - set(kr.KERNEL_NAMES)))
    assert shapes == set(kr.STD_SHAPES + kr.RING_SHAPES) and kinds == set(kr.KINDS)
    assert n == len(kr.param_sets()) * len(kr.FLAGS) * 2 * kr.CAP
    # the flags a family implements all reach it
    for name in ("extd2_tiny_kernel", "extd2_team_kernel", "extd2_reg_kernel<5,hbm>", "extd2_ring_kernel<3>", "extd2_ring_kernel<4>"):
        assert flags_by_name[name] == {0, 0x01, 0x40, 0x80, 0xC0}, (name, flags_by_name[name])
    for name in ("extd2_lds_kernel", "extz2_lds_kernel"):
        assert flags_by_name[name] >= set(kr.FLAGS) - ({0, 0x01, 0x40, 0x80, 0xC0} if name == "extd2_lds_kernel" else set()), name
    # extd2_reg_kernel<3..5,lds> cannot be planned: more than 128 target columns always pass PSVR_DP_PG_THRESHOLD
    assert min(kr.reg_lds_need(ql, 129, w) for ql in (1, 2, 17) for w in (-1, 0, 1, 200)) > 4096
    # the lean cases sit on the team kernel, on parameter sets of both pair orders that the library calls inert
    sets = kr.lean_sets()
    assert {kr.regime(p, "extd2")["swapped"] for p in sets} == {0, 1} and all(kr.library_regime(p, "extd2")["zdrop_inert"] for p in sets)
    assert all(kr.route(p, f, "extd2", ql, tl) == "extd2_team_kernel" for p in sets for f in kr.LEAN_FLAGS for ql, tl in kr.LEAN_SHAPES)


def test_reference_wraps_int8_on_the_named_case_and_nowrap_ok_refuses_it():
    """nowrap_ok is the licence for the team and tiny kernels, whose arithmetic does not wrap.  On kr.int8_wrap_case the reference's does:
    it scores -66 where unbounded integers give -65, with the int8 bound at 65.  The library must refuse the set (it accepted it while
    nowrap_ok was the bound alone, and extd2_team_kernel returned -65)."""
    c = kr.int8_wrap_case()
    judge = run_ref if ref_available() else run_oracle
    assert kr.int8_bound(c) == 65
    assert (judge(c, "extd2")["score"], kr.unbounded_score(c)) == (-66, -65)
    assert kr.library_regime(c, "extd2")["nowrap_ok"] == 0
    assert kr.route(c, 0, "extd2", 200, 201) == "extd2_reg_kernel<4,hbm>"


def test_no_int8_wrap_where_the_library_says_nowrap_ok():
    """Random gap pairs and scores under the int8 bound, in both pair orders, e > e2, e == e2 and e < e2: wherever the library's
    nowrap_ok holds, the judge's score equals the recurrences in unbounded integers on the longest shapes of the team kernel (where
    an excess has the most columns to accumulate over); and the sample holds sets that the predicate refuses where it does not."""
    judge = run_ref if ref_available() else run_oracle
    rng = np.random.RandomState(424242)
    n_ok, refused_and_wraps, bad = 0, 0, []
    for k in range(160):
        a, b, a2, b2 = int(rng.randint(1, 20)), int(rng.randint(0, 4)), int(rng.randint(1, 30)), int(rng.randint(0, 4))
        if k % 4 == 0:
            b2 = b
        p = kr.pset("wrap%d" % k, q=a, e=b, q2=a2, e2=b2, match=int(rng.randint(1, 4)), mismatch=int(rng.randint(1, 2 * min(a + b, a2 + b2) + 1)), zdrop=-1)
        if kr.int8_bound(p) > 127:
            continue
        ok = kr.library_regime(p, "extd2")["nowrap_ok"]
        ql, tl = ((200, 201), (120, 201))[k % 2]
        c = kr.make_case(p, 0, *kr.make_pair(rng, kr.KINDS[int(rng.randint(len(kr.KINDS)))], ql, tl, kr.regime(p, "extd2")["long_thres"]))
        same = judge(c, "extd2")["score"] == kr.unbounded_score(c)
        n_ok += ok
        refused_and_wraps += (not ok) and (not same)
        if ok and not same:
            bad.append({x: p[x] for x in ("match", "mismatch", "q", "e", "q2", "e2")})
    assert n_ok >= 30 and refused_and_wraps >= 3
    assert not bad, "the reference wraps under parameters nowrap_ok accepts: %r" % bad[:3]


def adversarial_pairs(rng, n):
    """unrelated, diverging after a shared prefix, indel-rich, homopolymer; every second pair with N bases; qlen <= 200, tlen <= 201"""
    out = []
    for k in range(n):
        ql = int(rng.randint(20, 201))
        q = rand_seq(rng, ql)
        kind = k % 4
        if kind == 0:
            t = rand_seq(rng, int(rng.randint(20, 202)))
        elif kind == 1:
            a = int(rng.randint(0, ql))
            t = (q[:a] + rand_seq(rng, 201))[:int(rng.randint(max(a, 20), 202))]
        elif kind == 2:
            t = (mutate(rng, q, 0.05, 0.12, 0.12, maxindel=30) + rand_seq(rng, 30))[:201] or [0]
        else:
            q, t = [k % 3] * ql, [3] * int(rng.randint(20, 202))
        if (k // 4) % 2:
            for _ in range(1 + int(rng.randint(6))):
                q[int(rng.randint(len(q)))] = 4
                t[int(rng.randint(len(t)))] = 4
        out.append((q, t))
    return out


def inert_candidates(rng, n):
    """parameter sets with e2 == 0 after the swap, in both pair orders, z-drop thresholds from 2 q2 - 1 to past the rule's edge"""
    out = []
    for k in range(n):
        a, b = int(rng.randint(2, 24)), int(rng.randint(0, 4))             # the pair with an extension cost
        big = a + b + int(rng.randint(0, 24))                              # the pair without: costs at least as much to open
        match = int(rng.randint(1, 5))
        mismatch = int(rng.randint(1, 2 * (a + b) + 1))                    # never the skip regime
        sc_n = int(rng.choice([0, 0, -1, -3]))
        swapped = k % 2 == 1 and big > a + b
        p = kr.pset("prop%d" % k, match=match, mismatch=mismatch, sc_n=sc_n, w=200,
                    **(dict(q=big, e=0, q2=a, e2=b) if swapped else dict(q=a, e=b, q2=big, e2=0)))
        shift = big - (a + b) if swapped else 0
        for z in sorted(set([2 * big - 1, 2 * big, 2 * big + 1, 2 * big + shift - 1, 2 * big + shift, 2 * big + shift + 2])):
            out.append(dict(p, zdrop=z))
    return out


def test_zdrop_never_fires_where_the_library_calls_it_inert():
    """dp_zdrop_inert is the licence for the lean team kernel, which cannot report a z-drop.  For every parameter set the library's
    predicate accepts -- e2 == 0 after the swap, pairs in plain and in swapped order, thresholds at the rule's edge -- the judge
    (the reference library where it was built, else the oracle) reports zdropped == 0 on inputs made to drop: unrelated, diverging,
    indel-rich and homopolymer pairs, with and without N.  The rule as it stood (zdrop >= 2 q2 whatever the order) fails here on
    swapped pairs: the reference charges the first cell with the pre-swap q + e."""
    judge = run_ref if ref_available() else run_oracle
    rng = np.random.RandomState(8675309)
    cands = inert_candidates(rng, 300)
    accepted = [p for p in cands if kr.library_regime(p, "extd2")["zdrop_inert"]]
    by_order = {s: [p for p in accepted if kr.regime(p, "extd2")["swapped"] == s] for s in (0, 1)}
    assert len(by_order[0]) >= 300 and len(by_order[1]) >= 150 and len(accepted) < len(cands)
    # the edge itself is among the accepted thresholds, in both orders
    for s in (0, 1):
        assert any(p["zdrop"] == 2 * kr.regime(p, "extd2")["post"][2] + kr.regime(p, "extd2")["qe_shift"] for p in by_order[s])
    dropped, n = [], 0
    for p in accepted:
        for flag, (q, t) in zip((0, 0x01, 0x80, 0, 0x01, 0x80, 0, 0, 0x81, 0, 0x01, 0x80), adversarial_pairs(rng, 12)):
            got = judge(kr.make_case(p, flag, q, t), "extd2")
            n += 1
            if got["zdropped"]:
                dropped.append(({k: p[k] for k in ("match", "mismatch", "q", "e", "q2", "e2", "zdrop")}, flag, len(q), len(t)))
    assert not dropped, "%d/%d problems z-drop under parameters dp_zdrop_inert accepts, first: %r" % (len(dropped), n, dropped[:3])
