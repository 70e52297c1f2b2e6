#!/usr/bin/env python3
"""Generates tests/golden/ksw_kat.json.gz: inputs from tests/ksw_cases.fixed_cases() and the
outputs of the REFERENCE kswlib itself (oracle/_ref/libref_ksw.so, compiled from
/root/reference/src/kswlib by oracle/Makefile), and tests/golden/ksw_random_kat.json.gz: the same
library's outputs for the seeded tests/ksw_cases.random_cases() of tests/test_oracle_ksw.py (inputs
are regenerated from the seed), and tests/golden/ksw_regime_kat.json.gz: its outputs for a seeded subset of the regime-directed
sweep of tests/ksw_regimes.py -- the first REGIME_KAT_PER_BATCH problems of every (parameter set, flag, variant) batch and the
problems of their own (inputs regenerated from the seed as well).  Run in the build container only."""
import gzip
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
from ksw_cases import fixed_cases, random_cases  # noqa: E402
from ksw_ref import ref_available, run_ref  # noqa: E402
import ksw_regimes as kr  # noqa: E402

assert ref_available(), "build oracle/_ref first: make -C oracle"
out = []
for c in fixed_cases():
    rec = {k: v for k, v in c.items() if k not in ("query", "target")}
    rec["query"] = "".join("ACGTN"[x] for x in c["query"])
    rec["target"] = "".join("ACGTN"[x] for x in c["target"])
    rec["extd2"] = run_ref(c, "extd2")
    c2 = dict(c)
    rec["extz2"] = run_ref(c2, "extz2")
    out.append(rec)
with gzip.open(os.path.join(HERE, "ksw_kat.json.gz"), "wt") as f:
    json.dump(out, f, separators=(",", ":"))
print("wrote", len(out), "cases")

seed, n, maxlen = 4242, 1500, 220
cases = random_cases(seed, n, maxlen)
rnd = {"seed": seed, "n": n, "maxlen": maxlen, "extd2": [run_ref(c, "extd2") for c in cases], "extz2": [run_ref(dict(c), "extz2") for c in cases]}
with gzip.GzipFile(os.path.join(HERE, "ksw_random_kat.json.gz"), "wb", mtime=0) as f:
    f.write(json.dumps(rnd, separators=(",", ":")).encode())
print("wrote", n, "random cases")

reg = {"seed": kr.SEED, "per_batch": kr.REGIME_KAT_PER_BATCH,
       "batches": [[run_ref(c, b[3]) for c in kr.batch_cases(b, kr.REGIME_KAT_PER_BATCH)] for b in kr.batches()],
       "special": [run_ref(c, variant) for _, variant, c in kr.special_cases()]}
with gzip.GzipFile(os.path.join(HERE, "ksw_regime_kat.json.gz"), "wb", mtime=0) as f:
    f.write(json.dumps(reg, separators=(",", ":")).encode())
print("wrote", sum(len(b) for b in reg["batches"]) + len(reg["special"]), "regime cases")
