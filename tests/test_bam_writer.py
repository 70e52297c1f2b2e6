"""Host-side BAM/BGZF encoder of the CLI (pansvr_amd/csrc/bam_writer.h) against the independent reader in
tests/bam_reader.py: header, reference list, every fixed field, CIGAR, 4-bit sequence, qualities, bin, integer tag
widths, string/char tags, multi-block BGZF with per-block sizes and the EOF marker."""
import os
import subprocess
import tempfile

import aln_common as ac
import bam_reader

DRIVER = r'''
#include "bam_writer.h"
int main(int argc, char **argv)
{
	psvr::BamWriter w;
	std::vector<psvr::BamRef> refs = {{"chr1", 1000000}, {"chr2", 2000000}};
	const int level = argc > 2 ? atoi(argv[2]) : Z_DEFAULT_COMPRESSION;        // -2: the built-in encoder (--bgzf-fast)
	if (!w.open(argv[1], "@HD\tVN:1.6\n@SQ\tSN:chr1\tLN:1000000\n@SQ\tSN:chr2\tLN:2000000\n", refs, 3, level)) return 2;
	for (int i = 0; i < 3000; ++i) {
		psvr::SamFields f;
		f.qname = "r" + std::to_string(i), f.flag = i % 2 ? 0x50 : 0x83, f.tid = i % 2, f.pos1 = 100 + i * 337, f.mapq = i % 61;
		f.cigar = i % 3 ? "40S100M5I5M2D" : "150M";
		f.mtid = i % 5 ? f.tid : (i % 7 ? 1 - f.tid : -1), f.mpos1 = 500 + i, f.isize = (i % 2 ? 1 : -1) * (300 + i);
		f.seq = std::string(150 - i % 2, "ACGTN"[i % 5]), f.qual = std::string(150 - i % 2, (char)(33 + i % 40));
		f.tags = "\tAS:i:" + std::to_string(i * 97 - 1000) + "\tOS:i:300\tOA:Z:0,1,2,3,M;\tRC:Z:comment_" + std::to_string(i) + "\tXX:A:Q\tNM:i:70000\tYY:i:-40000\tZZ:i:-7";
		if (!w.write(f)) return 3;
	}
	return w.close() ? 0 : 4;
}
'''


import pytest


@pytest.mark.parametrize("level", [-1, 1, -2])
def test_bam_writer_round_trip(level):
    d = tempfile.mkdtemp(prefix="psvr_bamw_")
    open(os.path.join(d, "t.cpp"), "w").write(DRIVER)
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-I" + os.path.join(ac.ROOT, "pansvr_amd", "csrc"), "-o", os.path.join(d, "t"), os.path.join(d, "t.cpp"), "-lz", "-lpthread"])
    subprocess.check_call([os.path.join(d, "t"), os.path.join(d, "x.bam"), str(level)])
    assert bam_reader.check_bgzf(os.path.join(d, "x.bam")) > 2          # several 0xff00-byte blocks + EOF
    text, refs, recs = bam_reader.read_bam(os.path.join(d, "x.bam"))
    assert text.startswith("@HD") and refs == [("chr1", 1000000), ("chr2", 2000000)] and len(recs) == 3000
    for i, r in enumerate(recs):
        tid = i % 2
        mtid = tid if i % 5 else ((1 - tid) if i % 7 else -1)
        want = ["r%d" % i, str(0x50 if i % 2 else 0x83), "chr%d" % (tid + 1), str(100 + i * 337), str(i % 61), "40S100M5I5M2D" if i % 3 else "150M",
                "*" if mtid < 0 else ("=" if mtid == tid else "chr%d" % (mtid + 1)), str(500 + i), str((1 if i % 2 else -1) * (300 + i)),
                "ACGTN"[i % 5] * (150 - i % 2), chr(33 + i % 40) * (150 - i % 2),
                "AS:i:%d" % (i * 97 - 1000), "OS:i:300", "OA:Z:0,1,2,3,M;", "RC:Z:comment_%d" % i, "XX:A:Q", "NM:i:70000", "YY:i:-40000", "ZZ:i:-7"]
        assert r == want, (i, r, want)


# BgzfWriter's device route (compiled with PSVR_BGZF_ON_DEVICE, as the CLI is) against a stand-in for the engine library: the first
# psvr_bgzf_compress call makes the members on the host (zlib), every later call fails.  The writer must carry on on the host with the
# bytes of the failed call, the rest of that write() and what later write() calls bring, in order.
FALLBACK = r'''
#include "bam_writer.h"
static int calls = 0;
extern "C" {
const char *psvr_last_error(void) { return "stand-in failure"; }
void *psvr_host_alloc(size_t n) { return malloc(n); }
void psvr_host_free(void *p) { free(p); }
int64_t psvr_bgzf_bound(int64_t n) { return (n / 0xff00 + 1) * (0x10000 + 64); }
int psvr_bgzf_compress(int, const void *in, int64_t n, void *out, int64_t cap, int64_t *got)
{
	if (calls++ > 0) return 3;
	uint8_t *o = (uint8_t *)out;
	int64_t at = 0;
	for (int64_t p = 0; p < n; p += 0xff00) {
		if (at + 0x10000 + 64 > cap) return 1;
		const size_t m = n - p < 0xff00 ? (size_t)(n - p) : 0xff00;
		const size_t k = psvr::BgzfWriter::compress_block_public((const uint8_t *)in + p, m, o + at);
		if (!k) return 1;
		at += (int64_t)k;
	}
	*got = at;
	return 0;
}
}
int main(int argc, char **argv)
{
	psvr::BgzfWriter w(4);                                   // four blocks gathered per device call
	if (!w.open(argv[1], 1)) return 2;                       // (one thread: the host flushes every eight blocks)
	w.set_device(0);
	FILE *f = fopen(argv[2], "rb");
	std::vector<uint8_t> in(atoi(argv[3]));
	if (!f || fread(in.data(), 1, in.size(), f) != in.size()) return 3;
	for (size_t at = 0, k = 0; at < in.size(); ++k) {           // writes of uneven sizes: the failing call leaves a residue behind
		const size_t m = std::min(in.size() - at, (size_t)(1000 + k * 7919 % 60000));
		w.write(in.data() + at, m), at += m;
	}
	return w.close() && calls >= 2 ? 0 : 4;
}
'''


def test_bgzf_writer_device_failure_continues_in_order_on_the_host():
    import gzip
    import numpy as np
    d = tempfile.mkdtemp(prefix="psvr_bgzff_")
    open(os.path.join(d, "t.cpp"), "w").write(FALLBACK)
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-DPSVR_BGZF_ON_DEVICE", "-I" + os.path.join(ac.ROOT, "pansvr_amd", "csrc"), "-o", os.path.join(d, "t"),
                           os.path.join(d, "t.cpp"), "-lz", "-lpthread"])
    rng = np.random.RandomState(5)
    n = 0xff00 * 30 + 12345                                  # seven gather buffers and more: host batches flush before close()
    data = (rng.randint(0, 4, size=n).astype(np.uint8) * 17 + rng.randint(0, 3, size=n).astype(np.uint8)).tobytes()
    open(os.path.join(d, "in.bin"), "wb").write(data)
    r = subprocess.run([os.path.join(d, "t"), os.path.join(d, "x.bgzf"), os.path.join(d, "in.bin"), str(n)], env=dict(os.environ, PSVR_BGZF_DEVICE_MIN_BLOCKS="1"),
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    assert r.returncode == 0, r.stderr.decode()
    assert "BGZF on the device failed" in r.stderr.decode()
    assert bam_reader.check_bgzf(os.path.join(d, "x.bgzf")) > 20
    got = gzip.open(os.path.join(d, "x.bgzf"), "rb").read()
    assert len(got) == n
    assert got == data, "decoded stream differs from the input first at byte %d" % next(i for i in range(n) if got[i] != data[i])
