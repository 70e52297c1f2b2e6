"""The device coordinate sort: psvr_sort_order_u64 against numpy's stable argsort, and `panSVR aln --sort` against `panSVR aln` followed
by `panSVR sort` (the sorted .bam and its .bai byte for byte, the ori file unchanged) on every input route."""
import os
import subprocess
import tempfile

import numpy as np
import pytest

import aln_common as ac
import bench_data
import test_sort_cli
from pansvr_amd.sort import sort_order

pytestmark = pytest.mark.gpu
CLI = os.path.join(ac.ROOT, "pansvr_amd", "bin", "panSVR")
TILE = 2048                                          # keys per tile of the scatter (sort.hip kSortTile)


def coord_keys(rng, n, n_tid=25, max_pos=1 << 28, unplaced=0.02):
    """samtools' key of n records: (uint64)tid << 32 | (uint32)(pos + 1) << 1 | reverse, a share of them unplaced (tid -1, pos -1)"""
    tid = rng.randint(0, n_tid, n).astype(np.uint64)
    pos = rng.randint(-1, max_pos, n).astype(np.uint64) + np.uint64(1)
    keys = tid << np.uint64(32) | pos << np.uint64(1) | rng.randint(0, 2, n).astype(np.uint64)
    un = rng.random_sample(n) < unplaced
    keys[un] = np.uint64(0xFFFFFFFF) << np.uint64(32) | rng.randint(0, 2, int(un.sum())).astype(np.uint64)
    return keys


def check(keys):
    got = sort_order(keys)
    want = np.argsort(keys, kind="stable")
    assert got.dtype == np.uint32 and len(got) == len(keys)
    bad = np.nonzero(got.astype(np.int64) != want)[0]
    assert len(bad) == 0, "%d of %d positions differ, first at %d" % (len(bad), len(keys), bad[0])


@pytest.mark.parametrize("n", [0, 1, 2, 3, TILE - 1, TILE, TILE + 1, 4 * TILE + 7])
def test_order_small_sizes(n):
    rng = np.random.RandomState(n + 1)
    check(rng.randint(0, 1 << 62, n, dtype=np.int64).astype(np.uint64) * np.uint64(3))
    check(coord_keys(rng, n))


def test_order_heavy_ties():
    rng = np.random.RandomState(2)
    vals = rng.randint(0, 1 << 63, 1000, dtype=np.int64).astype(np.uint64) * np.uint64(2)
    check(vals[rng.randint(0, 1000, 1000000)])


@pytest.mark.parametrize("shape", ["equal", "sorted", "reverse", "full_range", "unplaced"])
def test_order_shapes(shape):
    rng = np.random.RandomState(3)
    n = 300001
    if shape == "equal":
        keys = np.full(n, 0x0123456789ABCDEF, dtype=np.uint64)
    elif shape == "sorted":
        keys = np.sort(coord_keys(rng, n))
    elif shape == "reverse":
        keys = np.sort(coord_keys(rng, n))[::-1].copy()
    elif shape == "full_range":
        keys = rng.randint(0, 1 << 32, n, dtype=np.int64).astype(np.uint64) << np.uint64(32) | rng.randint(0, 1 << 32, n, dtype=np.int64).astype(np.uint64)
    else:
        keys = coord_keys(rng, n, unplaced=0.5)
    check(keys)


def test_order_fifty_million_keys():
    """the record count of the largest configuration (25 M pairs, two main-file records each)"""
    check(coord_keys(np.random.RandomState(4), 50000000))


def test_order_rejects_what_it_cannot_order():
    from pansvr_amd._lib import lib
    import ctypes as C
    k = np.zeros(1, np.uint64)
    o = np.zeros(1, np.uint32)
    assert lib().psvr_sort_order_u64(0, C.c_int64(-1), k.ctypes.data_as(C.c_void_p), o.ctypes.data_as(C.c_void_p)) == 1      # PSVR_ERR_ARG
    assert lib().psvr_sort_order_u64(0, C.c_int64(1 << 32), k.ctypes.data_as(C.c_void_p), o.ctypes.data_as(C.c_void_p)) == 2  # PSVR_ERR_UNSUPPORTED


def files(path):
    return open(path, "rb").read(), open(path + ".bai", "rb").read()


def two_routes(pos_args, flags=(), stdin_path=None):
    """`aln` + `sort` and `aln --sort` on the same input: returns the three files of each route"""
    tmp = tempfile.mkdtemp(prefix="psvr_alnsort_")
    out = {}
    for route in ("two_step", "sort"):
        o, p = os.path.join(tmp, route + ".bam"), os.path.join(tmp, route + ".ori.bam")
        extra = ["--sort"] if route == "sort" else []
        stdin = open(stdin_path, "rb") if stdin_path else None
        r = subprocess.run([CLI, "aln"] + list(flags) + extra + ["-o", o, "-p", p] + list(pos_args), stdin=stdin, stdout=subprocess.PIPE,
                           stderr=subprocess.PIPE, timeout=900)
        assert r.returncode == 0, r.stderr.decode()[-2000:]
        if route == "two_step":
            s = os.path.join(tmp, "two_step.sorted.bam")
            r2 = subprocess.run([CLI, "sort", "-o", s, o], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=900)
            assert r2.returncode == 0, r2.stderr.decode()[-2000:]
            assert "ordered on the device" in r2.stderr.decode()
            out[route] = files(s) + (open(p, "rb").read(),)
        else:
            assert '"sort_s":' in r.stderr.decode()
            out[route] = files(o) + (open(p, "rb").read(),)
    return out


def assert_same(out):
    a, b = out["two_step"], out["sort"]
    assert a[0] == b[0], "sorted .bam differs (%d vs %d bytes)" % (len(a[0]), len(b[0]))
    assert a[1] == b[1], ".bai differs"
    assert a[2] == b[2], "the ori file differs from the run without --sort"


@pytest.mark.parametrize("name,rname,flags", [("fx1", "reads150", []), ("fx2", "reads250", []), ("fx3", "ragged", []), ("fx5", "hicopy", []),
                                              ("fx1", "reads150", ["--batch", "97", "--sub-batch", "31"]),
                                              ("fx2", "reads150", ["-R", "700", "--devices", "0,0"])])
def test_aln_sort_equals_aln_then_sort(name, rname, flags):
    w = ac.workdir(name)
    assert_same(two_routes([ac.index_dir(name), os.path.join(w, rname + ".fq"), os.path.join(w, "header.sam")], flags))


def test_aln_sort_from_stdin():
    w = ac.workdir("fx3")
    assert_same(two_routes([ac.index_dir("fx3"), "-", os.path.join(w, "header.sam")], stdin_path=os.path.join(w, "ragged.fq")))


def test_aln_sort_fused_bam_input():
    """the fused signal route: a BAM as the reads argument (tests/golden/fused inputs)"""
    import test_fused_signal as tf
    tmp = tempfile.mkdtemp(prefix="psvr_alnsort_fused_")
    bam = os.path.join(tmp, "in.bam")
    tf.bam_of("fx1", "reads150", 2000, bam)
    assert_same(two_routes([ac.index_dir("fx1"), bam, os.path.join(tmp, "h.sam")], ["-N", "-D"]))


def test_aln_sort_bench_set_200k():
    tmp = tempfile.mkdtemp(prefix="psvr_alnsort_bench_")
    anc = bench_data.make_anchors(1500, seed=23)
    bench_data.write_index_dir(bench_data.build_index_cli(anc, dense=False), os.path.join(tmp, "idx"))
    bases, base_off, ori, isize = bench_data.make_reads(anc, 200000, seed=29)
    fq = os.path.join(tmp, "reads.fq")
    bench_data.write_fastq(fq, bases, base_off, ori, isize, procs=min(16, os.cpu_count() or 1))
    with open(os.path.join(tmp, "header.sam"), "w") as f:
        f.write("@SQ\tSN:chr1\tLN:250000000\n@SQ\tSN:chr2\tLN:250000000\n")
    assert_same(two_routes([os.path.join(tmp, "idx"), fq, os.path.join(tmp, "header.sam")], ["-t", "8"]))


def test_sort_on_the_device_matches_a_python_stable_sort(tmp_path):
    err = test_sort_cli.check_sort_against_python(tmp_path, 20000, 97)
    assert "ordered on the device" in err
