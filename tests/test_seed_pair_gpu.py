"""-m gpu: the seeding kernel's lane-pair filter look-up (aln_device.h seed_pair_answers) and the canonical filter it reads.

The filter the device builds must be, word for word, the one the build rule gives on the host (tests/tools/seed_filter_check.cpp),
and the engine's records with --trace -- candidates, CIGARs, pairing, and per strand n_seed, seed_hash, chain_hash -- must be the
oracle's on batches that take the lane-pair path (read lengths whose stride-5 offsets mirror between the strands: 100, 150, 250, 25,
30), the per-probe path (24, 101-104, 151), and both inside one wavefront.

The shortest reads here have 24 bases, not 20: for a read of 20 to 23 bases the reference's STR screen (read_realignment.cpp:549-598,
`kmers.size() < kmer_number - 15` in unsigned arithmetic, then seed_list[read_l - 20 - o] for o < 5) indexes in front of its array --
oracle/aln_oracle, which restates it, ends with a segmentation fault on such a batch, and the engine's restatement would write in
front of its staging array.  There is no reference result to compare with; the 20-base case of the lane-pair scheme itself is
checked on the host (tests/test_seed_filter.py)."""
import ctypes as C
import os
import subprocess
import tempfile

import numpy as np
import pytest

import aln_common as ac
import datasets
import synth
from test_emu_aln import normalise
from test_seed_filter import build_tool

pytestmark = pytest.mark.gpu
CLI = os.path.join(ac.ROOT, "pansvr_amd", "bin", "panSVR")
SET = "fx2"

# name -> (pairs, make_reads arguments, environment).  Short reads cannot carry an STR insert (synth puts >= 30 bases in).
LONG = dict(frag=(500, 700), stat=(250, 300, 600, 900))
BATCHES = {
    "len100": (320, dict(L=100), None),
    "len150": (320, dict(L=150), None),
    "len250": (300, dict(L=250, **LONG), None),
    "len101_104": (320, dict(lengths=[101, 102, 103, 104]), None),
    "len151": (320, dict(L=151), None),
    "len24_25": (400, dict(lengths=[24, 25], str_frac=0.0), None),
    "mixed": (600, dict(lengths=[24, 25, 30, 100, 101, 102, 103, 104, 150, 151, 250], str_frac=0.0, **LONG), None),
    "n_bases": (320, dict(L=150, n_frac=0.2), None),
    "str_even_odd": (400, dict(lengths=[100, 101, 150, 151], str_frac=0.4), None),
    "unmapped": (320, dict(L=150, unmapped_frac=0.3), None),
    "partial_wavefront": (333, dict(L=150), None),
    "lane_per_pair_prep": (400, dict(lengths=[100, 150, 151]), {"PSVR_PREP_PAIR_MIN": "1"}),
}


@pytest.fixture(scope="module")
def anchors():
    return datasets.anchors_of(SET)[1:]


@pytest.mark.parametrize("name", list(BATCHES))
def test_engine_records_equal_the_oracle(name, anchors):
    pairs, kw, env = BATCHES[name]
    w = ac.workdir(SET)
    rname = "seed_pair_" + name
    synth.write_fastq(os.path.join(w, rname + ".fq"), synth.make_reads(anchors, pairs, seed=101 + len(name), **kw))
    tmp = tempfile.mkdtemp(prefix="psvr_seedpair_")
    rec = os.path.join(tmp, "records.jsonl")
    cmd = [CLI, "aln", "-S", "-o", os.path.join(tmp, "out.sam"), "-p", os.path.join(tmp, "ori.sam"), "--records", rec, "--trace",
           ac.index_dir(SET), os.path.join(w, rname + ".fq"), os.path.join(w, "header.sam")]
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=dict(os.environ, **(env or {})))
    assert r.returncode == 0, r.stderr.decode()[-2000:]
    got = [normalise(l) for l in open(rec).read().split("\n") if l.strip()]
    want = [normalise(l) for l in ac.run_oracle(SET, rname, trace=True)]
    assert len(got) == len(want) == pairs
    bad = [i for i, (a, b) in enumerate(zip(want, got)) if a != b]
    assert not bad, "%d/%d pairs differ; first %d:\nref: %s\ngpu: %s" % (len(bad), len(want), bad[0], want[bad[0]], got[bad[0]])
    # the comparison covered seeds: reads with results carry their strands' n_seed / seed_hash / chain_hash
    # (reads of 24 to 30 bases end without a result, and the trace of such a read is not a result: see normalise)
    traced = [rd["tr"] for d in want for rd in d["reads"] if "tr" in rd]
    assert len(traced) > pairs // 4 or min(kw.get("lengths", [kw.get("L", 150)])) < 100


def test_device_built_filter_equals_the_host_built_one():
    from pansvr_amd._lib import check, lib
    L = lib()
    tmp = tempfile.mkdtemp(prefix="psvr_bloom_")
    host_file = os.path.join(tmp, "host.bloom")
    subprocess.check_call([build_tool(), "index", ac.index_dir("fx1"), host_file], stdout=subprocess.DEVNULL)
    host = np.fromfile(host_file, dtype=np.uint64)
    h = C.c_void_p()
    check(L.psvr_index_load(ac.index_dir("fx1").encode(), os.path.join(ac.workdir("fx1"), "header.sam").encode(), 0, C.byref(h)))
    try:
        n, shift = C.c_int64(0), C.c_uint32(0)
        check(L.psvr_index_bloom_read(h, None, C.c_int64(0), C.byref(n), C.byref(shift)))
        assert n.value == len(host) and shift.value == 64 - int(np.log2(len(host)))
        dev = np.zeros(n.value, dtype=np.uint64)
        check(L.psvr_index_bloom_read(h, dev.ctypes.data_as(C.c_void_p), n, None, None))
    finally:
        L.psvr_index_destroy(h)
    assert np.count_nonzero(host) > 10000
    assert np.array_equal(dev, host), "%d words differ" % int(np.count_nonzero(dev != host))
