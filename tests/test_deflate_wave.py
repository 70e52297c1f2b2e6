"""The wavefront-per-member BGZF encoder (pansvr_amd/csrc/deflate_wave_device.h) in its host build with one lane, whose bytes are the
device's bytes (tests/test_deflate_wave_gpu.py compares them): zlib inflates every member to its input, the plain and the sanitizer
build agree, a member depends on its own input bytes only, and the total on BAM records is no larger than what the lane-per-block
encoder of deflate_device.h makes at the device route's setting.  Then the two writers' device-members route against stand-in
compressors that succeed once and fail afterwards, and the commands' option rules."""
import gzip
import os
import subprocess
import tempfile
import zlib

import numpy as np
import pytest

import aln_common as ac
import bam_reader
import deflate_wave_cases as dc
import inflate_cases as ic
import test_signal as ts

CLI = ts.CLI
CSRC = os.path.join(ac.ROOT, "pansvr_amd", "csrc")


@pytest.fixture(scope="module")
def checkers():
    tmp = tempfile.mkdtemp(prefix="psvr_dfw_")
    return dc.build_checker(tmp, False), dc.build_checker(tmp, True)


@pytest.fixture(scope="module")
def records():
    return dc.fx2_records()


@pytest.mark.parametrize("member_bytes", dc.MEMBER_SIZES)
def test_every_member_inflates_to_its_input(checkers, records, member_bytes):
    plain, asan = checkers
    sizes = {}
    for name, data in dc.cases(member_bytes, records):
        raw = dc.host_members(plain, data, member_bytes)
        ms = dc.check_members(raw, data, member_bytes)
        assert dc.host_members(asan, data, member_bytes) == raw, name          # the sanitizer build: clean, and the same bytes
        if name == "random":                                                   # incompressible: stored, and within BGZF's 64 KB
            for i, m in enumerate(ms):
                n = min(member_bytes, len(data) - i * member_bytes)
                assert len(m) == n + 31 and m[18] == 1 and len(m) <= 65536, (name, i)
        sizes[name] = len(raw)
        if name in ("zeros", "period 2") and member_bytes == 0xff00:
            assert len(raw) < 400, (name, len(raw))
    if member_bytes == 0xff00:                                                 # the 300 bytes that return at distance 32768 (four bits each as literals) are found
        assert sizes["a match at distance 32768"] < sizes["no match at distance 32768"] - 100, sizes


def test_a_member_depends_on_its_own_bytes_only(checkers, records):
    plain, _ = checkers
    for mb in (4096, 0xff00):
        piece = records[:mb]
        alone = dc.host_members(plain, piece, mb)
        assert dc.host_members(plain, piece, mb) == alone                      # twice
        longer = ic.bam_like(2 * mb, 4) + piece + ic.bam_like(mb // 2, 6)      # as the third member of a longer buffer
        ms = ic.split_members(dc.host_members(plain, longer, mb))
        assert len(ms) == 4 and ms[2] == alone
        assert ic.split_members(dc.host_members(plain, b"\x00" * mb + piece, mb))[1] == alone


def test_no_larger_than_the_lane_per_block_encoder(checkers, records):
    """The guard of the ratio: fx2's BAM records at 0xff00 bytes per member against deflate_block of deflate_device.h at the device route's
    own setting (16 KB blocks, hbits = 9), 26 wrapper bytes per member on both sides."""
    plain, _ = checkers
    new = len(dc.host_members(plain, records, 0xff00))
    tmp = tempfile.mkdtemp(prefix="psvr_dfw_")
    open(os.path.join(tmp, "in"), "wb").write(records)
    old = int(subprocess.check_output([plain, "--old", "16384", "9", os.path.join(tmp, "in")]).decode())
    z = {lv: sum(len(ic.wrap(ic.deflate(records[i:i + 0xff00], lv), records[i:i + 0xff00])) for i in range(0, len(records), 0xff00)) for lv in (1, 6)}
    print("fx2 records %d bytes: wavefront encoder %d, lane-per-block encoder %d, zlib level 1 %d, zlib default %d" % (len(records), new, old, z[1], z[6]))
    assert new <= old, (new, old)


# ---- the writers' route through a compressor handed in as a pointer ------------------------------------------------------------------------
STANDIN = r'''
static int calls = 0;
// zlib-made members with their offsets the first time, a failure every time after it
static int standin_members(int, const void *in, int64_t n, int32_t mb, void *out, int64_t cap, int64_t *got, int64_t *off, int64_t off_cap, int64_t *nm)
{
	if (calls++ > 0) return 3;
	uint8_t *o = (uint8_t *)out;
	std::vector<uint8_t> tmp(0x10000 + 64);
	int64_t at = 0, k = 0;
	for (int64_t p = 0; p < n; p += mb, ++k) {
		const size_t m = n - p < mb ? (size_t)(n - p) : (size_t)mb;
		const size_t c = psvr::BgzfWriter::compress_block_public((const uint8_t *)in + p, m, tmp.data());
		if (!c || at + (int64_t)c > cap || (off && k >= off_cap)) return 1;
		if (off) off[k] = at;
		memcpy(o + at, tmp.data(), c), at += (int64_t)c;
	}
	if (off) off[k] = at;
	if (nm) *nm = k;
	*got = at;
	return 0;
}
'''

WRITER = r'''
#include "bam_writer.h"
extern "C" {
const char *psvr_last_error(void) { return "stand-in failure"; }
void *psvr_host_alloc(size_t n) { return malloc(n); }
void psvr_host_free(void *p) { free(p); }
int64_t psvr_bgzf_bound(int64_t n) { return n; }
int psvr_bgzf_compress(int, const void *, int64_t, void *, int64_t, int64_t *) { abort(); }   // (the other device route: not this test's)
}
''' + STANDIN + r'''
int main(int argc, char **argv)
{
	psvr::BgzfWriter w;
	if (!w.open(argv[1], 1)) return 2;                       // (one thread: the host flushes every eight blocks)
	w.set_device_members(0, &standin_members, 4);            // four members gathered per call
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


def test_bgzf_writer_members_failure_continues_in_order_on_the_host():
    d = tempfile.mkdtemp(prefix="psvr_dfwf_")
    open(os.path.join(d, "t.cpp"), "w").write(WRITER)
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-DPSVR_BGZF_ON_DEVICE", "-I" + CSRC, "-o", os.path.join(d, "t"), os.path.join(d, "t.cpp"), "-lz", "-lpthread"])
    rng = np.random.RandomState(5)
    n = 0xff00 * 30 + 12345
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


SORTED = r'''
#include "sorted_bam.h"
extern "C" {
const char *psvr_last_error(void) { return "stand-in failure"; }
int psvr_device_count(void) { return 0; }
int psvr_sort_order_u64(int, int64_t, const uint64_t *, uint32_t *) { abort(); }
void *psvr_host_alloc(size_t n) { return malloc(n); }
void psvr_host_free(void *p) { free(p); }
int64_t psvr_bgzf_bound(int64_t n) { return n; }
int psvr_bgzf_compress(int, const void *, int64_t, void *, int64_t, int64_t *) { abort(); }   // (the other device route: not this test's)
}
''' + STANDIN + r'''
int main(int argc, char **argv)
{
	using namespace psvr;
	SortRecords R;
	uint32_t x = 12345;
	auto rnd = [&]() { x = x * 1664525u + 1013904223u; return x >> 8; };
	for (int i = 0; i < 7000; ++i) {
		uint8_t f[32] = {0};
		auto p32 = [&](int o, uint32_t v) { for (int k = 0; k < 4; ++k) f[o + k] = (uint8_t)(v >> (8 * k)); };
		const bool unplaced = rnd() % 50 == 0;
		char name[32];
		const int ln = snprintf(name, sizeof name, "read%06d", i) + 1;
		p32(0, unplaced ? 0xffffffffu : rnd() % 3), p32(4, unplaced ? 0xffffffffu : rnd() % 3000000);
		f[8] = (uint8_t)ln, f[9] = 60, f[12] = unplaced ? 0 : 1, f[14] = (uint8_t)(unplaced ? 4 : (rnd() & 16)), p32(16, 100), p32(20, 0xffffffffu), p32(24, 0xffffffffu);
		std::vector<uint8_t> d(name, name + ln);
		if (!unplaced) { const uint32_t c = 100u << 4; for (int k = 0; k < 4; ++k) d.push_back((uint8_t)(c >> (8 * k))); }
		for (int k = 0; k < 50; ++k) d.push_back((uint8_t)(0x11 << (rnd() & 3)));
		for (int k = 0; k < 100; ++k) d.push_back((uint8_t)(20 + rnd() % 20));
		R.add(f, d.data(), d.size());
	}
	std::vector<uint32_t> ord;
	bool on_device = true;
	std::string err;
	if (!coordinate_order(R, 0, ord, &on_device, &err) || on_device) return 2;
	const std::vector<std::pair<std::string, int32_t>> refs = {{"chr1", 4000000}, {"chr2", 4000000}, {"chr3", 4000000}};
	if (!write_sorted_bam(argv[1], "@HD\tVN:1.6\n", refs, R, ord, false, 3, &err)) return 3;
	if (!write_sorted_bam(argv[2], "@HD\tVN:1.6\n", refs, R, ord, false, 3, &err, &standin_members, 0, 4)) return 4;
	return calls >= 2 ? 0 : 5;
}
'''


def test_write_sorted_bam_members_failure_equals_the_host_route():
    d = tempfile.mkdtemp(prefix="psvr_dfws_")
    open(os.path.join(d, "t.cpp"), "w").write(SORTED)
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-DPSVR_BGZF_ON_DEVICE", "-I" + CSRC, "-o", os.path.join(d, "t"), os.path.join(d, "t.cpp"), "-lz", "-lpthread"])
    host, dev = os.path.join(d, "host.bam"), os.path.join(d, "dev.bam")
    r = subprocess.run([os.path.join(d, "t"), host, dev], stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    assert r.returncode == 0, r.stderr.decode()
    assert r.stderr.decode().count("BGZF on the device failed") == 1
    assert bam_reader.check_bgzf(dev) > 16                                      # several windows of four blocks: one from the stand-in, the rest from the host
    assert gzip.open(dev, "rb").read() == gzip.open(host, "rb").read()
    assert open(dev, "rb").read() == open(host, "rb").read()                    # (the stand-in uses zlib: the very same bytes)
    assert open(dev + ".bai", "rb").read() == open(host + ".bai", "rb").read()
    assert len(bam_reader.read_bam(dev)[2]) == 7000


# ---- the commands --------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("flags,name", [(["-S"], "-S"), (["--compress-level", "1"], "--compress-level"), (["--bgzf-fast"], "--bgzf-fast"),
                                        (["--bgzf-device"], "--bgzf-device")])
def test_deflate_device_refuses_conflicting_options(tmp_path, flags, name):
    missing = [str(tmp_path / "no_idx"), str(tmp_path / "no_reads.fq"), str(tmp_path / "no_header.sam")]
    for first in (["--deflate-device"] + flags, flags + ["--deflate-device"]):
        r = subprocess.run([CLI, "aln"] + first + ["-o", str(tmp_path / "o.bam"), "-p", str(tmp_path / "p.bam")] + missing, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=60)
        err = r.stderr.decode()
        assert r.returncode == 1, err
        assert "--deflate-device cannot be combined with %s" % name in err, err
        assert "loading index" not in err and not os.path.exists(str(tmp_path / "o.bam")) and not os.path.exists(str(tmp_path / "p.bam"))
    # with --sort the older rule speaks first, as before
    r = subprocess.run([CLI, "aln", "--sort", "--deflate-device"] + flags + missing, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=60)
    assert r.returncode == 1 and "--sort cannot be combined with %s" % name in r.stderr.decode()


def test_usage_lists_deflate_device():
    r = subprocess.run([CLI, "aln"], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=60)
    assert r.returncode == 1 and "--deflate-device" in r.stderr.decode()
    r = subprocess.run([CLI, "sort"], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=60)
    assert r.returncode == 1 and "--deflate-device" in r.stderr.decode()
