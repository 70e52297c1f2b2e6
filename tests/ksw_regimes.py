"""Regime-directed DP cases (inputs only): parameter sets enumerated by the predicates that route a problem to a kernel family, the
flags, shapes and sequence kinds at which those kernels have corners.  Shared by tests/test_ksw_regimes.py (CPU),
tests/test_ksw_regimes_gpu.py, tests/test_oracle_ksw.py and tests/golden/gen_ksw_kat.py.

The predicates are restated here from pansvr_amd/csrc/dp_plan.h (make_dp_params, dp_tiny_ok, dp_band_never_binds, dp_route);
tests/test_ksw_regimes.py holds regime() to the library's own psvr_dp_regime, tests/test_dp_host_plan.py holds route() to the host
planner's plans on the CPU and the GPU sweep holds it to the plans' descriptions.  dp_zdrop_inert is NOT restated: its only source is the library."""
import numpy as np

from ksw_cases import DEF, rand_seq

SEED = 20261017
FAST_FLAGS = 0x01 | 0x40 | 0x80
# every flag combination of the KAT list (tests/ksw_cases.fixed_cases) and seven more
FLAGS = [0, 0x01, 0x02, 0x04, 0x08, 0x18, 0x40, 0x80, 0xC0, 0x42, 0x82, 0x09] + [0x06, 0x0C, 0x44, 0x48, 0x58, 0x1E, 0xDE]
VARIANTS = ["extd2", "extz2"]
CAP = 12                       # problems per (parameter set, flag, variant) batch; test_ksw_regimes_gpu.py records how it was set and the wall time
REGIME_KAT_PER_BATCH = 2       # problems per batch whose reference answers are committed (tests/golden/ksw_regime_kat.json.gz)
MAX_LDS = 160 * 1024
LDS_CLASSES = [2048, 4096, 6144, 8192, 12288, 16384, 24576, 32768, 49152, 65536, 98304, 131072, MAX_LDS]


def mat_m(m, match, mismatch, sc_n=0):
    """m x m scoring matrix in 25 bytes, the last row and column the ambiguous base's (ksw_gen_mat_D for m = 5)."""
    out = []
    for l in range(m):
        for k in range(m):
            out.append(sc_n if l == m - 1 or k == m - 1 else (match if l == k else -mismatch))
    return out + [0] * (25 - len(out))


def pset(tag, shapes="std", sc_n=0, **kw):
    p = dict(DEF)
    p.pop("flag")
    p.update(kw)
    p["mat"] = mat_m(p["m"], p["match"], p["mismatch"], sc_n)
    p["tag"], p["shapes"] = tag, shapes
    return p


def int8_bound(p):
    """the quantity make_dp_params compares with 127 (extd2's pairs)"""
    m, mat = p["m"], p["mat"]
    sc = mat[1:m * m] if m * m > 1 else []
    min_sc, max_sc = min([mat[1]] + sc), max([mat[0]] + sc)
    return max_sc + 3 * max(p["q"] + p["e"], p["q2"] + p["e2"]) + max(-min_sc, 0)


def regime(p, variant):
    """make_dp_params, as a dict with the fields of psvr_dp_regime_t except zdrop_inert"""
    v = VARIANTS.index(variant) if variant in VARIANTS else variant
    m, mat = p["m"], p["mat"]
    q, e, q2, e2 = p["q"], p["e"], p["q2"], p["e2"]
    r = dict(skip=0, swapped=0, nowrap_ok=0, long_thres=0, qe_shift=0)
    qe_pre = q + e
    if v == 0:
        if m <= 1:
            return dict(r, skip=1)
        if q2 + e2 < q + e:
            q, e, q2, e2 = q2, e2, q, e
            r["swapped"] = 1
    else:
        if m <= 0:
            return dict(r, skip=1)
        q2, e2 = q, e
    sc = mat[1:m * m] if m * m > 1 else []
    min_sc, max_sc = min([mat[1]] + sc), max([mat[0]] + sc)
    if -min_sc > 2 * (q + e):
        return dict(r, skip=1, swapped=0)
    r["boundary_ok"] = int(e > e2 or (e == e2 and q == q2))     # the first row / column cost what the recurrences charge inside
    r["nowrap_ok"] = int(max_sc + 3 * max(q + e, q2 + e2) + max(-min_sc, 0) <= 127 and min(q, e, q2, e2) >= 0 and r["boundary_ok"])
    if v == 0:
        lt = int((q2 - q) / (e - e2)) - 1 if e != e2 else 0        # C division truncates
        if q2 + e2 + lt * e2 > q + e + lt * e:
            lt += 1
        r["long_thres"] = lt
    r["qe_shift"] = qe_pre - (q + e)
    r["post"] = (q, e, q2, e2)
    return r


def band_never_binds(ql, tl, w):
    return ql <= w and tl <= w + 1


def n_col(ql, tl, w):
    w = max(ql, tl) if w < 0 else w
    return (min(ql, tl, w + 1) + 15) // 16 + 1


def reg_lds_need(ql, tl, w):
    return ((ql + 16 + 15) & ~15) + (ql + tl - 1) * n_col(ql, tl, w) * 16 + 16


def lds_kernel_need(ql, tl, v):
    T, QL = (tl + 15) // 16 * 16, (ql + 15) // 16 * 16
    img = (7 if v == 0 else 5) * T + T + QL + 16
    return ((img + 15) & ~15) + 4 * T


def route(p, flag, variant, ql, tl):
    """the kernel name psvr_dp_plan_describe prints for this problem (dp_route + dp_kind_name)"""
    v = VARIANTS.index(variant)
    r = regime(p, v)
    w = p["w"]
    fast_ok = v == 0 and (flag & ~FAST_FLAGS) == 0
    tiny_ok = fast_ok and r["nowrap_ok"] and not r["skip"] and (w < 0 or w >= 16)
    wf = max(ql, tl) if w < 0 else w
    span = min(wf, min(ql, tl) - 1) + 33
    general = "extd2_lds_kernel" if v == 0 else "extz2_lds_kernel"
    if ql <= 8000 and tl <= 8000:
        if ql <= 0 or tl <= 0 or r["skip"]:
            return "extd2_reg_kernel<1,lds>"
        if tiny_ok and ql <= 16 and tl <= 16:
            return "extd2_tiny_kernel"
        if tiny_ok and band_never_binds(ql, tl, wf) and tl <= 16 * 13:
            return "extd2_team_kernel"
        T = (tl + 15) // 16 * 16
        if fast_ok and T <= 320:
            return "extd2_reg_kernel<%d,%s>" % ((T + 63) // 64, "lds" if reg_lds_need(ql, tl, w) <= 4096 else "hbm")
        if fast_ok and span <= 256:
            return "extd2_ring_kernel<%d>" % (3 if span <= 192 else 4)
        assert lds_kernel_need(ql, tl, v) <= MAX_LDS
        return general
    if r["skip"]:
        return "extd2_reg_kernel<1,lds>"
    ring_need = ((ql + 16 + 15) & ~15) + ((tl + 15) & ~15) + 16
    if fast_ok and span <= 256 and ring_need <= MAX_LDS:
        four = next(c for c in LDS_CLASSES if c >= ring_need) * 4 <= MAX_LDS
        return "extd2_ring%s_kernel<%d>" % ("" if four else "1", 3 if span <= 192 else 4)
    return "extd2_hbm_kernel" if v == 0 else "extz2_hbm_kernel"


# every name dp_kind_name can produce for a plan of the host planner.  extd2_reg_kernel<3..5,lds> are not among them: a target of more
# than 128 columns has (qlen + tlen - 1) * n_col * 16 >= 129 * 2 * 16 = 4128 bytes of direction bytes, over PSVR_DP_PG_THRESHOLD
# (test_ksw_regimes.py checks that arithmetic)
KERNEL_NAMES = (["extd2_reg_kernel<1,lds>", "extd2_reg_kernel<2,lds>"] + ["extd2_reg_kernel<%d,hbm>" % k for k in range(1, 6)] +
                ["extd2_tiny_kernel", "extd2_team_kernel", "extd2_ring_kernel<3>", "extd2_ring_kernel<4>", "extd2_ring1_kernel<3>", "extd2_ring1_kernel<4>",
                 "extd2_lds_kernel", "extz2_lds_kernel", "extd2_hbm_kernel", "extz2_hbm_kernel"])


def param_sets():
    S = []
    # --- nowrap_ok: the int8 bound max_sc + 3 max(q+e, q2+e2) + |min_sc| at 125, 126, 127 | 128, 129, reached through the match score,
    # the mismatch score, the second gap pair (plain order) and the first one (swapped)
    for match in (17, 18, 19, 20, 21):
        S.append(pset("bound_match_%d" % match, match=match))
    for mis in (27, 28, 29, 30, 31):
        S.append(pset("bound_mismatch_%d" % mis, mismatch=mis))
    for g, mis in ((37, 12), (37, 13), (37, 14), (38, 12), (38, 13)):
        S.append(pset("bound_pair2_%d_%d" % (g, mis), mismatch=mis, q=14, e=2, q2=g - 1, e2=1))
        S.append(pset("bound_pair1_%d_%d" % (g, mis), mismatch=mis, q=g - 1, e=1, q2=14, e2=2))
    # --- the swap q+e > q2+e2: plain (the defaults), swapped, equal sums either way, e == e2 (long_thres = 0) in both orders
    S.append(pset("plain"))
    S.append(pset("swapped", q=32, e=0, q2=16, e2=1))
    S.append(pset("equal_sums", q=16, e=1, q2=17, e2=0))
    S.append(pset("equal_sums_other_order", q=17, e=0, q2=16, e2=1))
    S.append(pset("e_eq_e2", q=16, e=1, q2=32, e2=1))
    S.append(pset("e_eq_e2_swapped", q=32, e=1, q2=16, e2=1))
    # --- the boundary costs against the recurrences' (nowrap_ok's second condition): the sets above with e == e2 and q2 > q and
    # "equal_sums_other_order" (e < e2) are on the far side, as are these two; identical pairs are on the near side
    S.append(pset("e_lt_e2", q=6, e=1, q2=24, e2=2))
    S.append(pset("e_lt_e2_swapped", q=24, e=2, q2=6, e2=1))
    S.append(pset("same_pairs", q=6, e=2, q2=6, e2=2, match=1, mismatch=2))
    # --- e2 == 0 after the swap, zdrop at 2 q2 - 1 | 2 q2 and, for swapped pairs, 2 q2 + shift - 1 | 2 q2 + shift with
    # shift = pre-swap q+e minus post-swap q+e; zdrop < 0 switches the rule off
    for z in (63, 64):
        S.append(pset("inert_plain_z%d" % z, zdrop=z))
    for z in (63, 64, 78, 79):
        S.append(pset("inert_swapped_z%d" % z, q=32, e=0, q2=16, e2=1, zdrop=z))
    for z in (39, 40, 47, 48):
        S.append(pset("inert_swapped_small_z%d" % z, q=20, e=0, q2=10, e2=2, zdrop=z))
    S.append(pset("inert_plain_small_z20", q=4, e=2, q2=10, e2=0, zdrop=20))
    S.append(pset("zdrop_off", zdrop=-1))
    S.append(pset("zdrop_10", zdrop=10))
    # --- the skip rule -min_sc > 2(q+e): 2(q+e) | 2(q+e) + 1, at the defaults' pairs and at small ones (where the int8 bound holds)
    S.append(pset("skip_edge_34", mismatch=34))
    S.append(pset("skip_35", mismatch=35))
    S.append(pset("skip_edge_small_10", mismatch=10, q=4, e=1, q2=8, e2=0))
    S.append(pset("skip_small_11", mismatch=11, q=4, e=1, q2=8, e2=0))
    # --- alphabet sizes (extd2 skips m <= 1, extz2 m <= 0), a non-zero N score, end bonus
    for m in (0, 1, 2):
        S.append(pset("m%d" % m, m=m))
    S.append(pset("n_score_minus3", sc_n=-3))
    S.append(pset("n_score_plus1", sc_n=1))
    for eb in (0, 5):
        S.append(pset("end_bonus_%d" % eb, end_bonus=eb))
    # --- band widths: none, 0, 1, and 15 | 16 | 17 (dp_tiny_ok wants w >= 16; 200 is the defaults')
    for w in (-1, 0, 1, 15, 16, 17):
        S.append(pset("w%d" % w, w=w))
    S.append(pset("w16_not_int8", w=16, mismatch=30))
    # --- matrices wider than 320 columns: band widths either side of the ring kernels' limits (w + 33 <= 192: 159 | 160; <= 256: 223 | 224)
    # and the second user's parameters (contig re-alignment: 2/-10, 24+2k | 32+1k, w = zdrop = 132)
    for w in (159, 160, 200, 223, 224):
        S.append(pset("ring_w%d" % w, shapes="ring", w=w))
    S.append(pset("ring_sv", shapes="ring", match=2, mismatch=10, q=24, e=2, q2=32, e2=1, w=132, zdrop=132))
    assert len(set(p["tag"] for p in S)) == len(S)
    return S


# lengths 1, 2, 15-17, 31-33; 63-65, 200 / 201 and 320 / 321 columns
STD_SHAPES = [(1, 1), (1, 2), (2, 1), (2, 2), (15, 16), (16, 16), (16, 17), (17, 15), (31, 32), (32, 33), (33, 31), (1, 33), (33, 1), (2, 201), (2, 100),
              (40, 63), (64, 64), (70, 65), (100, 130), (200, 201), (201, 200), (150, 201), (250, 320), (300, 321), (321, 320)]
RING_SHAPES = [(321, 321), (340, 500), (500, 340), (400, 420), (640, 641), (200, 201), (250, 320), (16, 16)]
KINDS = ["unrelated", "homopolymer", "indel_at_long_thres", "long_gap_then_matches", "all_n", "n_opposite_n"]
# problems of their own, default scoring: (tag, qlen, tlen, w, flags, variants).  Sequences over 8000 bases take the long routes: the
# one-wavefront ring kernels when the query + target image passes a quarter of LDS, and extd2_hbm_kernel<0 / 1> when the general
# kernel's LDS image (12 / 10 bytes per target column + the query) passes PSVR_DP_MAX_LDS
SPECIAL = [("ring1_4", 20000, 20000, 200, (0, 0x80), ("extd2",)), ("ring1_3", 20000, 20010, 132, (0, 0x40), ("extd2",)),
           ("ring_long", 9000, 9050, 200, (0,), ("extd2",)),
           ("beyond_lds", 200, 17000, 200, (0x02, 0x08), ("extd2", "extz2")), ("long_no_band", 150, 17000, -1, (0,), ("extd2", "extz2"))]


def to_alphabet(seq, m):
    """codes 0..3 + N (4) -> the alphabet of size m (its last code is the ambiguous base)"""
    if m >= 5:
        return seq
    if m <= 1:
        return [0] * len(seq)
    return [m - 1 if x == 4 else x % (m - 1) for x in seq]


def make_pair(rng, kind, ql, tl, long_thres):
    q = rand_seq(rng, ql)
    if kind == "unrelated":
        t = rand_seq(rng, tl)
    elif kind == "homopolymer":
        a = int(rng.randint(4))
        q, t = [a] * ql, [(a + 1 + int(rng.randint(3))) % 4] * tl
    elif kind == "indel_at_long_thres":      # identical but for one insertion or deletion of long_thres - 1, long_thres or long_thres + 1 bases
        g = max(1, long_thres + int(rng.randint(-1, 2)))
        k = ql // 2
        t = q[:k] + rand_seq(rng, g) + q[k:] if rng.randint(2) else q[:k] + q[k + g:]
        t = (t + rand_seq(rng, tl))[:tl]
    elif kind == "long_gap_then_matches":
        g = max(1, min(tl // 2, 20 + int(rng.randint(60))))
        t = (rand_seq(rng, g) + q + rand_seq(rng, tl))[:tl] if rng.randint(2) else (q[g:] + rand_seq(rng, tl))[:tl]
    elif kind == "all_n":
        q, t = [4] * ql, [4] * tl
    else:                                    # N opposite N, and a few N opposite a base
        t = (list(q) + rand_seq(rng, tl))[:tl]
        for i in range(min(ql, tl)):
            if rng.randint(6) == 0:
                q[i] = t[i] = 4
        t[int(rng.randint(tl))] = 4
    if kind in ("unrelated", "indel_at_long_thres", "long_gap_then_matches") and rng.randint(4) == 0:
        q[int(rng.randint(ql))] = 4
        t[int(rng.randint(tl))] = 4
    return q, t


def make_case(p, flag, q, t):
    c = {k: p[k] for k in ("m", "match", "mismatch", "mat", "q", "e", "q2", "e2", "w", "zdrop", "end_bonus")}
    c["flag"] = flag
    c["query"], c["target"] = to_alphabet([int(x) for x in q], p["m"]), to_alphabet([int(x) for x in t], p["m"])
    return c


def batches():
    """one batch per (parameter set, flag, variant): (index, parameter set, flag, variant); its problems come from batch_cases"""
    out = []
    for p in param_sets():
        for flag in FLAGS:
            for variant in VARIANTS:
                out.append((len(out), p, flag, variant))
    return out


def batch_picks(b):
    """the (shape, kind) combinations of a batch: CAP of them, drawn without replacement from the batch's own seeded stream"""
    idx, p = b[0], b[1]
    shapes = STD_SHAPES if p["shapes"] == "std" else RING_SHAPES
    combos = [(s, k) for s in shapes for k in KINDS]
    rng = np.random.RandomState(SEED + idx)
    return rng, [combos[i] for i in rng.choice(len(combos), CAP, replace=False)]


def batch_cases(b, limit=None):
    idx, p, flag, variant = b
    rng, picks = batch_picks(b)
    lt = regime(p, variant)["long_thres"]
    return [make_case(p, flag, *make_pair(rng, kind, ql, tl, lt)) for (ql, tl), kind in picks[:limit]]


def special_cases():
    """(tag, variant, case) of the SPECIAL problems: related sequences with a diverged stretch and N bases"""
    from ksw_cases import mutate
    rng = np.random.RandomState(SEED - 1)
    p = pset("special")
    out = []
    for tag, ql, tl, w, flags, variants in SPECIAL:
        q = rand_seq(rng, ql)
        t = mutate(rng, q, 0.03, 0.01, 0.01, maxindel=20)
        t = (t + rand_seq(rng, tl))[:tl]
        q[int(rng.randint(ql))] = 4
        t[int(rng.randint(tl))] = 4
        for flag in flags:
            for variant in variants:
                out.append((tag, variant, make_case(dict(p, w=w), flag, q, t)))
    return out


# ---- the lean team variant (PSVR_DP_FORCE_LEAN): parameter sets the library calls z-drop inert, plain and swapped, on the team kernel's shapes
LEAN_TAGS = ["plain", "inert_plain_z64", "zdrop_off", "inert_plain_small_z20", "inert_swapped_z79", "inert_swapped_small_z48", "equal_sums"]
LEAN_FLAGS = [0, 0x01, 0x80, 0x81]          # the flags the team kernel implements, less the extension-only one (dp_zdrop_inert refuses it)
LEAN_SHAPES = [(ql, tl) for ql, tl in STD_SHAPES if ql <= 200 and tl <= 201 and (ql > 16 or tl > 16)] + [(17, 1), (3, 40), (190, 150), (64, 193), (199, 17)]


def lean_swapped_400():
    return pset("lean_swapped_z400", q=32, e=0, q2=16, e2=1, zdrop=400)


def lean_sets():
    return [p for p in param_sets() if p["tag"] in LEAN_TAGS] + [lean_swapped_400()]


def lean_cases():
    rng = np.random.RandomState(SEED + 99991)
    out = []
    for p in lean_sets():
        lt = regime(p, 0)["long_thres"]
        for flag in LEAN_FLAGS:
            for ql, tl in LEAN_SHAPES:
                kind = KINDS[int(rng.randint(len(KINDS)))]
                out.append(make_case(p, flag, *make_pair(rng, kind, ql, tl, lt)))
    return out


def unbounded_score(c):
    """extd2's end-to-end score of a problem from the same difference recurrences as the reference (z = min(z, sc_mch) included) in
    unbounded integers, with no band and no z-drop rule: what the reference returns wherever none of its int8 lanes wraps, which is
    what nowrap_ok promises the team and tiny kernels.  (m = 5; H of the last cell = H above the last column + its v's.)"""
    r = regime(c, 0)
    (q, e, q2, e2), lt, mat = r["post"], r["long_thres"], c["mat"]
    long_diff = lt * (e - e2) - (q2 - q) - e2
    sc_n = mat[24] if mat[24] else -e2

    def ur(k):
        return -(q + e) if k == 0 else -e if k < lt else long_diff if k == lt else -e2
    tl = len(c["target"])
    U, Y, Y2 = [ur(t) for t in range(tl)], [-(q + e)] * tl, [-(q2 + e2)] * tl
    h = -(c["q"] + c["e"]) + sum(ur(t) for t in range(1, tl))
    for i, qb in enumerate(c["query"]):
        v1, x1, x21 = ur(i), -(q + e), -(q2 + e2)
        for t, tb in enumerate(c["target"]):
            sc = sc_n if qb == 4 or tb == 4 else mat[0] if qb == tb else mat[1]
            a, b, a2, b2 = x1 + v1, Y[t] + U[t], x21 + v1, Y2[t] + U[t]
            z = min(max(sc, a, b, a2, b2), mat[0])
            u, v = z - v1, z - U[t]
            x1, Y[t] = max(a - z + q, 0) - q - e, max(b - z + q, 0) - q - e
            x21, Y2[t] = max(a2 - z + q2, 0) - q2 - e2, max(b2 - z + q2, 0) - q2 - e2
            U[t], v1 = u, v
        h += v1
    return h


def int8_wrap_case(flag=0):
    """A named problem on which the reference's int8 lanes wrap although the int8 bound (65) is far from 127: gap pairs 17+0k | 16+1k
    (no swap, e < e2: the boundary overcharges and z = min(z, sc_mch) cuts), 200 N bases against 201.  The reference scores it -66,
    the same recurrences in unbounded integers -65 (unbounded_score)."""
    return make_case(pset("int8_wrap", q=17, e=0, q2=16, e2=1), flag, [4] * 200, [4] * 201)


def ksw_params(c):
    from pansvr_amd import ksw
    return ksw.make_params(c["m"], c["mat"], c["q"], c["e"], c["q2"], c["e2"], c["w"], c["zdrop"], c["end_bonus"], c.get("flag", 0))


def library_regime(p, variant):
    """psvr_dp_regime: the library's own predicates for a parameter set (no device needed)"""
    import ctypes as C
    from pansvr_amd._lib import check, lib

    class Regime(C.Structure):
        _fields_ = [(n, C.c_int32) for n in ("skip", "swapped", "nowrap_ok", "zdrop_inert", "long_thres", "qe_shift")]
    r = Regime()
    par = ksw_params(p)
    check(lib().psvr_dp_regime(C.byref(par), VARIANTS.index(variant) if variant in VARIANTS else variant, C.byref(r)))
    return {n: int(getattr(r, n)) for n, _ in Regime._fields_}


if __name__ == "__main__":
    # child process of test_ksw_regimes_gpu.py: the lean cases through psvr_extd2_batch, results as JSON on stdout
    import json
    import os
    import sys
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    from pansvr_amd import ksw
    assert os.environ.get("PSVR_DP_FORCE_LEAN")
    cases = lean_cases()
    res = [None] * len(cases)
    groups = {}
    for i, c in enumerate(cases):
        groups.setdefault((tuple(c["mat"]),) + tuple(c[k] for k in ("m", "q", "e", "q2", "e2", "w", "zdrop", "end_bonus", "flag")), []).append(i)
    for ids in groups.values():
        for i, r in zip(ids, ksw.ext_batch([cases[i]["query"] for i in ids], [cases[i]["target"] for i in ids], ksw_params(cases[ids[0]]))):
            res[i] = r
    json.dump(res, sys.stdout)
