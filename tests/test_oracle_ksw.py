"""The oracle restatement of the DP (oracle/ksw_oracle.c) is pinned against
(1) the committed known-answer vectors produced by the reference kswlib itself, and
(2) that library's committed answers for seeded random cases (tests/golden/ksw_random_kat.json.gz), and
(3) its committed answers for a seeded subset of the regime-directed sweep (tests/golden/ksw_regime_kat.json.gz: parameter sets on
both sides of every routing predicate, every flag combination, both variants), all three written by tests/golden/gen_ksw_kat.py."""
import gzip
import json
import os

import pytest

from ksw_cases import random_cases
from ksw_ref import run_oracle

HERE = os.path.dirname(os.path.abspath(__file__))


def load_kat():
    with gzip.open(os.path.join(HERE, "golden", "ksw_kat.json.gz"), "rt") as f:
        recs = json.load(f)
    for r in recs:
        r["query"] = ["ACGTN".index(ch) for ch in r["query"]]
        r["target"] = ["ACGTN".index(ch) for ch in r["target"]]
    return recs


def diff(a, b):
    return {k: (a[k], b[k]) for k in a if a[k] != b[k]}


@pytest.mark.parametrize("kind", ["extd2", "extz2"])
def test_oracle_matches_reference_kat(kind):
    recs = load_kat()
    assert len(recs) >= 600
    bad = []
    for i, r in enumerate(recs):
        got = run_oracle(r, kind)
        if got != r[kind]:
            bad.append((i, r["flag"], len(r["query"]), len(r["target"]), diff(r[kind], got)))
    assert not bad, "%d mismatches, first: %r" % (len(bad), bad[:3])


@pytest.mark.parametrize("kind", ["extd2", "extz2"])
def test_oracle_matches_live_reference_random(kind):
    with gzip.open(os.path.join(HERE, "golden", "ksw_random_kat.json.gz"), "rt") as f:
        kat = json.load(f)
    cases = random_cases(kat["seed"], kat["n"], kat["maxlen"])
    assert len(cases) == len(kat[kind]) == 1500
    bad = []
    for i, (c, a) in enumerate(zip(cases, kat[kind])):
        b = run_oracle(c, kind)
        if a != b:
            bad.append((i, len(c["query"]), len(c["target"]), diff(a, b)))
    assert not bad, "%d mismatches, first: %r" % (len(bad), bad[:3])


def test_oracle_matches_reference_on_the_regime_sweep():
    """The judge of tests/test_ksw_regimes_gpu.py over the space that sweep covers: scoring at the int8 bound, swapped and equal gap
    pairs, z-drop at the inert rule's edges, the skip rule, alphabets of 0, 1, 2 and 5 codes, bands from none to 224, a non-zero N
    score, end bonuses; 19 flag combinations; extd2 and extz2; and the problems of over 8000 bases."""
    import ksw_regimes as kr
    with gzip.open(os.path.join(HERE, "golden", "ksw_regime_kat.json.gz"), "rt") as f:
        kat = json.load(f)
    assert kat["seed"] == kr.SEED and kat["per_batch"] == kr.REGIME_KAT_PER_BATCH
    batches = kr.batches()
    assert len(batches) == len(kat["batches"]) >= 2000
    bad, n = [], 0
    for b, answers in zip(batches, kat["batches"]):
        cases = kr.batch_cases(b, kat["per_batch"])
        assert len(cases) == len(answers) == kat["per_batch"]
        for c, a in zip(cases, answers):
            got = run_oracle(c, b[3])
            n += 1
            if got != a:
                bad.append((b[1]["tag"], c["flag"], b[3], len(c["query"]), len(c["target"]), diff(a, got)))
    special = kr.special_cases()
    assert len(special) == len(kat["special"])
    for (tag, variant, c), a in zip(special, kat["special"]):
        got = run_oracle(c, variant, cap=len(c["query"]) + len(c["target"]) + 16)
        n += 1
        if got != a:
            bad.append((tag, c["flag"], variant, len(c["query"]), len(c["target"]), diff(a, got)))
    assert not bad, "%d/%d mismatches, first: %r" % (len(bad), n, bad[:3])
