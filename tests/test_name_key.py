"""pansvr_amd/csrc/name_key.h on its own, without a GPU: tests/tools/name_key_check.cpp (plain and under AddressSanitizer + UBSan, a stand-alone
program both times) runs the device's recipe on the host -- a stable pass for the tie key, then one per 8-byte chunk from the last to the
first -- and holds it to name_order() of sorted_bam.h; here its order is held to a restatement, Python's sorted() on (name, flag & 0xc0,
index).  The cases are tests/name_cases.py's: the lengths around the chunk edges, prefixes, names that differ at a chunk's last or next
first byte, whole constant chunks, bytes above 0x7f, an early NUL with other bytes behind it, equal names with every arrival order of the
flags, duplicates, and a record that ends with its name."""
import os
import struct
import subprocess
import tempfile

import pytest

import name_cases as nc

HERE = os.path.dirname(os.path.abspath(__file__))
CHECK_SRC = os.path.join(HERE, "tools", "name_key_check.cpp")


@pytest.fixture(scope="module", params=[False, True], ids=["plain", "sanitized"])
def checker(request):
    tmp = tempfile.mkdtemp(prefix="psvr_nk_")
    exe = os.path.join(tmp, "name_key_check_asan" if request.param else "name_key_check")
    flags = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"] if request.param else ["-O2"]
    subprocess.check_call(["g++"] + flags + ["-std=c++17", "-Wall", "-Wno-unused-function", "-o", exe, CHECK_SRC, "-lz", "-lpthread"])
    return exe


def _run(exe, bufs):
    tmp = tempfile.mkdtemp(prefix="psvr_nk_")
    with open(os.path.join(tmp, "in"), "wb") as f:
        f.write(struct.pack("<I", len(bufs)) + b"".join(struct.pack("<I", len(b)) + b for b in bufs))
    r = subprocess.run([exe, os.path.join(tmp, "in"), os.path.join(tmp, "out")], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600)
    assert r.returncode == 0 and not r.stderr, "name_key_check: exit status %d\n%s" % (r.returncode, r.stderr.decode()[-4000:])
    return [[int(x) for x in l.split()] for l in open(os.path.join(tmp, "out")).read().split("\n") if l]


def test_the_passes_are_name_order_and_the_restatement(checker):
    g = nc.groups()
    names = sorted(g)
    cases = [nc.records(g[k], seed=3 + i) for i, k in enumerate(names)]
    # the same names in another arrival order, and without the bare last record
    cases += [list(reversed(nc.records(g[k], seed=40 + i, bare_last=False))) for i, k in enumerate(names)]
    got = _run(checker, [b"".join(c) for c in cases])
    assert len(got) == len(cases)
    for ci, (recs, line) in enumerate(zip(cases, got)):
        what = names[ci % len(names)]
        longest = max([len(nc.name_of(r)) for r in recs], default=0)
        assert line[0] == ci and line[1] == (longest + 7) // 8, what
        assert line[2:] == nc.restated_order(recs), what
    # the cases are what they claim: a record that ends with its name, 254 bytes, whole constant chunks, an order that is not the arrival's
    every = cases[names.index("everything")]
    assert every[-1][12] == len(every[-1]) - 36 and max(len(nc.name_of(r)) for r in every) == 254
    assert {len(nc.name_of(r)) for r in every} >= set(nc.LENGTHS)
    for k, n in (("shared prefix of 16", 16), ("shared prefix of 24", 24)):
        assert len({nc.name_of(r)[:n] for r in cases[names.index(k)]}) == 1 and len({nc.name_of(r) for r in cases[names.index(k)]}) > 3
    assert nc.restated_order(every) != list(range(len(every)))


def test_the_restatement_is_strcmp_on_unsigned_bytes():
    recs = nc.records(nc.groups()["unsigned bytes"] + nc.groups()["early NUL"])
    order = [nc.name_of(recs[i]) for i in nc.restated_order(recs)]
    assert order.index(b"a\x7f") < order.index(b"a\x80") < order.index(b"a\xff") and order.index(b"ab") < order.index(b"abc")
    assert order[0] == b"" and order.count(b"ab") == 4
