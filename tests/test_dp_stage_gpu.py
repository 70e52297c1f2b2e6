"""-m gpu: the engine's DP stage -- planned and placed on the device behind the walk, launched from one plan record -- on a round
large enough for the team kernel (the generator gives about 0.65 DP problems per pair: 64 000 pairs pass the 32 768 problems below
which a round goes to the wavefront-per-alignment kernels).  Exact parity with the oracle on a prefix, and every record of the team
route against the same pairs run through the other kernels, one stream against overlapped launches, buffer growth and arena overflow
behind the queued placement, and the rounds with nothing to plan."""
import json
import os
import shutil
import subprocess
import sys
import tempfile

import numpy as np
import pytest

import aln_common as ac
import bench_data
from test_fullsize_gpu import canon

pytestmark = pytest.mark.gpu
N_PAIRS = 64000
N_ORACLE = 8000
STAT = (150, 200, 400, 600)
TEAM, TINY, FETCH = "extd2_team_kernel", "extd2_tiny_kernel", "k_dp_fetch"


@pytest.fixture(scope="module")
def setup():
    from pansvr_amd import aln
    anc = bench_data.make_anchors(1000, seed=11)
    ix = bench_data.build_index(anc, dense=True)
    index = aln.Index(ix, ["chr1", "chr2"], device=0)
    bases, base_off, ori, isize = bench_data.make_reads(anc, N_PAIRS, seed=13)
    s = dict(aln=aln, anc=anc, ix=ix, index=index, bases=bases, base_off=base_off, ori=ori, isize=isize, params=aln.default_params(STAT))
    # the reference result of the module: the whole set as one batch on a fresh engine, every kernel timed on the one stream
    eng = aln.Engine(index, s["params"])
    eng.upload(bases, base_off, ori)
    eng.run(timing=True)
    s["kernels"] = eng.stats()["kernels"]
    s["timed"] = eng.download()
    s["eng"] = eng
    yield s
    eng.close()
    index.close()


def same(a, b):
    return canon(a[0], a[2]) == canon(b[0], b[2]) and a[1].tobytes() == b[1].tobytes()


def oracle_records(s, bases, base_off, ori, isize, n):
    tmp = tempfile.mkdtemp(prefix="psvr_dpstage_")
    try:
        small = {k: v for k, v in s["ix"].items() if k != "hash"}
        bench_data.write_index_dir(small, os.path.join(tmp, "idx"))
        bench_data.write_fastq(os.path.join(tmp, "sample.fq"), bases, base_off, ori, isize, stat=STAT, n_pairs=n)
        with open(os.path.join(tmp, "header.sam"), "w") as f:
            f.write("@SQ\tSN:chr1\tLN:250000000\n@SQ\tSN:chr2\tLN:250000000\n")
        out = subprocess.run([ac.ORACLE_EXE, os.path.join(tmp, "idx"), os.path.join(tmp, "sample.fq"), os.path.join(tmp, "header.sam")],
                             stdout=subprocess.PIPE, check=True).stdout.decode()
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
    want = [json.loads(l) for l in out.split("\n") if l.lstrip().startswith("{")][:n]
    assert len(want) == n
    return want


def assert_oracle(s, got, bases, base_off, ori, isize, n):
    want = oracle_records(s, bases, base_off, ori, isize, n)
    reads, pairs, cig = got
    rec = ac.engine_records(reads, pairs, cig, ori, np.diff(base_off), 0, n)
    bad = [i for i in range(n) if want[i] != rec[i]]
    assert not bad, "%d/%d pairs differ, first %d:\noracle %s\nengine %s" % (len(bad), n, bad[0], json.dumps(want[bad[0]]), json.dumps(rec[bad[0]]))


def test_prefix_parity(setup):
    """The first 8 000 pairs of the team-route round equal the oracle's records, every pair compared."""
    s = setup
    for k in (TEAM, TINY, FETCH):
        assert k in s["kernels"] and s["kernels"][k]["launches"] > 0, "%s did not run: %s" % (k, sorted(s["kernels"]))
    assert_oracle(s, s["timed"], s["bases"], s["base_off"], s["ori"], s["isize"], N_ORACLE)


def test_route_independence(setup):
    """The same pairs as four consecutive batches of 16 000 stay below the team threshold: the wavefront kernels and the tiny kernel give
    the records the team route gave."""
    s = setup
    reads, pairs, cig = s["timed"]
    eng = s["aln"].Engine(s["index"], s["params"])
    q = N_PAIRS // 4
    bo = s["base_off"]
    for lo in range(0, N_PAIRS, q):
        hi = lo + q
        eng.upload(s["bases"][bo[2 * lo]:bo[2 * hi]], bo[2 * lo:2 * hi + 1] - bo[2 * lo], s["ori"][2 * lo:2 * hi])
        eng.run(timing=True)
        k = eng.stats()["kernels"]
        assert not any(n.startswith("extd2_team") for n in k), sorted(k)
        assert TINY in k and FETCH in k
        r2, p2, c2 = eng.download()
        assert p2.tobytes() == pairs[lo:hi].tobytes()
        a, b = reads[2 * lo:2 * hi].copy(), r2.copy()
        for x in (a, b):
            for fld in ("seed_hash", "chain_hash", "n_seed"):      # (they carry the batch's position in the draw streams)
                x[fld] = 0
        assert canon(a, cig) == canon(b, c2)
    eng.close()


def test_one_stream_vs_overlapped(setup):
    """Every kernel on the one stream, the overlapped launches of a plain run, and a second plain run of the resident batch: identical records."""
    s = setup
    eng = s["eng"]
    eng.run()
    first = eng.download()
    assert same(s["timed"], first)
    eng.run()
    assert same(first, eng.download())


CHILD = r"""
import os, sys
import numpy as np
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, os.path.dirname(sys.argv[1]))
import bench_data
from test_fullsize_gpu import canon
from pansvr_amd import aln
anc = bench_data.make_anchors(1000, seed=11)
index = aln.Index(bench_data.build_index(anc, dense=True), ["chr1", "chr2"], device=0)
bases, base_off, ori, isize = bench_data.make_reads(anc, 64000, seed=13)
params = aln.default_params((150, 200, 400, 600))
def run(shrink, small_first):
    if shrink: os.environ["PSVR_ARENA_SHRINK"] = shrink
    else: os.environ.pop("PSVR_ARENA_SHRINK", None)
    eng = aln.Engine(index, params)
    if small_first:
        eng.upload(bases[:base_off[4000]], base_off[:4001], ori[:4000])
        eng.run()
        eng.download()
    eng.upload(bases, base_off, ori)
    if small_first:
        eng.set_stream_pos([2, 0, 0])      # where a fresh engine starts: the handlers' seeds are draws 0 and 1 (an upload continues the streams)
    eng.run()
    r, p, c = eng.download()
    eng.close()
    return canon(r, c), p.tobytes()
want = run(None, False)
assert run(None, True) == want, "growth behind a small batch changed the records"
assert run("64", False) == want, "arena overflow changed the records"
print("ok")
"""


def test_growth_and_overflow():
    """In a process of its own: a 2 000-pair batch first, then the 64 000 on the same engine (DP buffers, slab and scratch all grow under the
    queued placement); the 64 000 with 1/64 of the arenas (the DP and candidate arenas overflow behind queued plan passes).  Both give
    a fresh default engine's records."""
    r = subprocess.run([sys.executable, "-c", CHILD, ac.HERE], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600)
    assert r.returncode == 0 and r.stdout.decode().strip().endswith("ok"), r.stderr.decode()[-3000:]


def exact_reads(anc, n_pairs, seed, L=150):
    """Pairs whose two ends are exact copies of an anchor's sequence: they align end to end, nothing is left for the DP kernels."""
    rng = np.random.RandomState(seed)
    codes, starts, lens = anc["codes"], anc["starts"], anc["lens"]
    a = rng.randint(1, len(lens), size=n_pairs)
    flen = rng.randint(300, 501, size=n_pairs)
    off = (rng.random_sample(n_pairs) * np.maximum(lens[a] - flen - 2, 1)).astype(np.int64)
    g0 = starts[a] + off
    ar = np.arange(L)
    end1 = codes[g0[:, None] + ar[None, :]]
    end2 = 3 - codes[(g0 + flen - 1)[:, None] - ar[None, :]]
    asc = np.frombuffer(b"ACGT", dtype=np.uint8)[np.stack([end1, end2], axis=1).reshape(2 * n_pairs, L)]
    ori = np.zeros(2 * n_pairs, dtype=bench_data.ORI_DTYPE)
    pos1 = anc["st_pos"][a] + off
    fwd = np.arange(2 * n_pairs) % 2 == 0
    ori["ref_bg"] = np.where(fwd, np.repeat(pos1, 2), np.repeat(pos1 + flen - L, 2))
    ori["read_bg"], ori["align_score"], ori["mapq"] = 40, 140, 20
    ori["direction"] = fwd.astype(np.uint8)
    return asc.reshape(-1), np.arange(2 * n_pairs + 1, dtype=np.int64) * L, ori, flen


@pytest.mark.parametrize("case", ["no_dp_problem", "hundred_pairs"])
def test_degenerate_rounds(setup, case):
    """A batch without a single DP problem, and one of 100 pairs (far below the team route): the oracle's records."""
    s = setup
    if case == "no_dp_problem":
        bases, base_off, ori, isize = exact_reads(s["anc"], 200, seed=5)
    else:
        bases, base_off, ori, isize = s["bases"][:s["base_off"][200]], s["base_off"][:201], s["ori"][:200], s["isize"][:100]
    eng = s["aln"].Engine(s["index"], s["params"])
    eng.upload(bases, base_off, ori)
    eng.run(timing=True)
    st = eng.stats()
    got = eng.download()
    eng.close()
    assert not any(n.startswith("extd2_team") for n in st["kernels"])
    if case == "no_dp_problem":
        assert st["dp_problems"] == 0 and TINY not in st["kernels"]
    else:
        assert st["dp_problems"] > 0
    assert_oracle(s, got, bases, base_off, ori, isize, len(isize))
