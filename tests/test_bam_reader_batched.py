"""The batched BGZF reader of pansvr_amd/csrc/bam_reader.h (--inflate-threads / --inflate-device: a reader thread takes the file in
chunks, cuts each at its last whole member and has the members inflated side by side) against the serial default: `panSVR sort` and
`panSVR signal [-N]` must write byte-identical files from a file and from stdin at chunk sizes that put the boundaries inside members and
inside records; when a device call fails the host pool takes over without a gap or a repeat; truncated and corrupted files end as today."""
import os
import struct
import subprocess
import tempfile
import zlib

import pytest

import aln_common as ac
import inflate_cases as ic
import test_signal as ts
from test_fused_signal import bam_of

CLI = ts.CLI
BATCHES = ["1000", "70000", None]


def env_of(batch):
    e = dict(os.environ)
    e.pop("PSVR_INFLATE_BATCH", None)
    if batch:
        e["PSVR_INFLATE_BATCH"] = batch
    return e


def run_sort(tmp, tag, bam, extra, batch=None, stdin=False):
    out = os.path.join(tmp, tag + ".bam")
    r = subprocess.run([CLI, "sort", "-o", out] + extra + ["-" if stdin else bam], stdin=open(bam, "rb") if stdin else None, env=env_of(batch), stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    return r, out


def run_signal(tmp, tag, bam, flags, extra, batch=None, stdin=False):
    """-> the process, and everything the run leaves behind: exit status, FASTQ, header file, status file, the command's own last message"""
    h, s = os.path.join(tmp, tag + ".h.sam"), os.path.join(tmp, tag + ".s.txt")
    for fn in (h, s):
        if os.path.exists(fn):
            os.remove(fn)
    r = subprocess.run([CLI, "signal"] + flags + extra + ["-H", h, "-S", s, "-" if stdin else bam], stdin=open(bam, "rb") if stdin else None, env=env_of(batch),
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    msg = [l for l in r.stderr.decode(errors="replace").split("\n") if "[panSVR-amd] signal:" in l]
    return r, (r.returncode, r.stdout, open(h, "rb").read() if os.path.exists(h) else None, open(s, "rb").read() if os.path.exists(s) else None, msg[-1:] )


@pytest.fixture(scope="module")
def bams():
    """name -> path: the golden fused BAMs, a name-sorted and a position-sorted generated BAM, the input of a golden fused run, and a BAM
    of one-byte members"""
    tmp = tempfile.mkdtemp(prefix="psvr_batched_")
    out = {}
    for fn in sorted(os.listdir(os.path.join(ac.HERE, "golden", "fused"))):
        if fn.endswith(".bam"):
            out["golden-" + fn] = os.path.join(ac.HERE, "golden", "fused", fn)
    recs, refs = ts.make_pairs(4242, 3000)
    out["by-name"] = os.path.join(tmp, "name.bam")
    ts.write_bam(out["by-name"], recs, refs)

    def key(i):
        tid, pos = struct.unpack_from("<ii", recs[i], 4)
        return (tid if tid >= 0 else 1 << 31, pos, i)
    out["by-pos"] = os.path.join(tmp, "pos.bam")
    ts.write_bam(out["by-pos"], [recs[i] for i in sorted(range(len(recs)), key=key)], refs)
    out["fused-input"] = os.path.join(tmp, "fused.bam")
    bam_of("fx1", "reads150", 1000, out["fused-input"])
    small, refs2 = ts.make_pairs(5, 12)
    ts.write_bam(os.path.join(tmp, "small.bam"), small, refs2)
    raw = b"".join(ic.oracle(m) for m in ic.split_members(open(os.path.join(tmp, "small.bam"), "rb").read()))
    out["one-byte-members"] = os.path.join(tmp, "bytes.bam")
    with open(out["one-byte-members"], "wb") as f:
        for k in range(len(raw)):
            f.write(ic.wrap(ic.deflate(raw[k:k + 1], 6), raw[k:k + 1]))
        f.write(ic.wrap(ic.deflate(b""), b""))
    return out


def test_sort_writes_the_same_files(bams):
    tmp = tempfile.mkdtemp(prefix="psvr_batched_")
    for name, bam in bams.items():
        if name == "by-pos":
            continue
        r, want = run_sort(tmp, "default", bam, [])
        assert r.returncode == 0, (name, r.stderr.decode()[-800:])
        for batch in BATCHES:
            for stdin in (False, True):
                r, got = run_sort(tmp, "batched", bam, ["--inflate-threads", "4"], batch, stdin)
                assert r.returncode == 0, (name, batch, stdin, r.stderr.decode()[-800:])
                assert open(got, "rb").read() == open(want, "rb").read(), (name, batch, stdin)
                assert open(got + ".bai", "rb").read() == open(want + ".bai", "rb").read(), (name, batch, stdin)


GOLDEN_FUSED = ["golden-fx1_reads150.bam", "golden-fx1_reads150.ori.bam", "golden-fx2_reads150.bam", "golden-fx2_reads150.ori.bam"]


@pytest.mark.parametrize("flags,names", [(["-N", "-D"], ["by-name", "fused-input", "one-byte-members"] + GOLDEN_FUSED), (["-N"], ["by-name"] + GOLDEN_FUSED), (["-D"], ["by-pos"]),
                                         ([], ["by-pos"])])
def test_signal_writes_the_same_files(bams, flags, names):
    """From a file and from stdin.  Two things the default route does stay what they are, and the batched route must do the same, to the exit
    status and the command's last message: the two golden main files (the aln step's output: a supplementary record's mate is not
    "second in template") end `signal -N` in its abort, after the same FASTQ bytes; and `signal` cannot read from a pipe at all -- its
    statistics pass reads the input first and the main pass then finds it used up ("not a BAM file")."""
    tmp = tempfile.mkdtemp(prefix="psvr_batched_")
    worked = 0
    for name in names:
        for stdin in (False, True):
            r, want = run_signal(tmp, "default", bams[name], flags, [], None, stdin)
            if stdin:
                assert want[0] == 1 and want[1] == b"" and "not a BAM file" in want[4][0], (name, want[0], want[4])
            elif name in ("golden-fx1_reads150.bam", "golden-fx2_reads150.bam"):
                assert want[0] == -6 and want[4], (name, want[0], want[4])
            else:
                assert want[0] == 0 and len(want[1]) > 1000, (name, r.stderr.decode()[-800:])
                worked += 1
            for batch in BATCHES:
                r, got = run_signal(tmp, "batched", bams[name], flags, ["--inflate-threads", "4"], batch, stdin)
                assert got == want, (name, batch, stdin, got[0], got[4], want[0], want[4])
    assert worked >= 1


def test_inflate_device_without_a_gpu_reads_on_the_host(bams):
    from pansvr_amd import lib
    if lib().psvr_device_count() > 0:
        pytest.skip("a HIP device is visible: the message of the route without one cannot be provoked here")
    tmp = tempfile.mkdtemp(prefix="psvr_batched_")
    r, want = run_sort(tmp, "default", bams["by-name"], [])
    r, got = run_sort(tmp, "device", bams["by-name"], ["--inflate-device"], "70000")
    assert r.returncode == 0 and "no HIP device visible" in r.stderr.decode(), r.stderr.decode()
    assert open(got, "rb").read() == open(want, "rb").read()


@pytest.mark.parametrize("damage", ["truncated-in-a-member", "truncated-in-a-header", "corrupted", "bad-crc", "bad-magic"])
def test_damaged_files_end_as_today(bams, damage):
    tmp = tempfile.mkdtemp(prefix="psvr_batched_")
    raw = bytearray(open(bams["by-name"], "rb").read())
    members = ic.split_members(bytes(raw))
    assert len(members) > 8
    at = sum(len(m) for m in members[:5])
    if damage == "truncated-in-a-member":
        raw = raw[:at + 300]
    elif damage == "truncated-in-a-header":
        raw = raw[:at + 7]
    elif damage == "corrupted":
        raw[at + 18 + 40] ^= 0xff
        assert ic.oracle(bytes(raw[at:])) is None
    elif damage == "bad-crc":
        raw[at + len(members[5]) - 6] ^= 1
    else:
        raw[at + 1] = 0
    bad = os.path.join(tmp, "bad.bam")
    open(bad, "wb").write(bytes(raw))
    for cmd in ("sort", "signal"):
        outs = []
        for extra, batch in (([], None), (["--inflate-threads", "3"], "1000"), (["--inflate-threads", "3"], "70000"), (["--inflate-threads", "3"], None)):
            if cmd == "sort":
                r, _ = run_sort(tmp, "x", bad, extra, batch)
            else:
                r, _ = run_signal(tmp, "x", bad, ["-N", "-D"], extra, batch)
            msg = [l for l in r.stderr.decode(errors="replace").split("\n") if l.startswith("[panSVR-amd] " + cmd + ":")]
            outs.append((r.returncode, msg, r.stdout if cmd == "signal" else b""))
        if damage == "bad-crc":
            # the serial reader does not look at the CRC (it stays as it is); every batched back-end does, as htslib does
            assert outs[0][0] == 0 and all(o[0] != 0 and o[1:] == outs[1][1:] for o in outs[1:]), (cmd, outs)
            continue
        assert outs[0][0] != 0 and outs[0][1], (cmd, outs[0])
        for o in outs[1:]:
            assert o == outs[0], (cmd, damage, o[:2], outs[0][:2])


# BgzfReader's device route (compiled with PSVR_BGZF_ON_DEVICE, as the CLI is) against a stand-in for the engine library: the first
# psvr_bgzf_decompress call inflates on the host (zlib), every later call fails.  The reader must go on with the host pool from the first
# member of the slot whose call failed: the bytes it hands out are the file's, no gap, nothing twice.
FALLBACK = r'''
#include "bam_reader.h"
static int calls = 0;
extern "C" {
const char *psvr_last_error(void) { return "stand-in failure"; }
int psvr_device_count(void) { return 1; }
void *psvr_host_alloc(size_t n) { return malloc(n); }
void psvr_host_free(void *p) { free(p); }
int psvr_bgzf_decompress(int, const void *in_, int64_t n, int64_t *used, void *out_, int64_t cap, int64_t *got, int64_t *, int64_t, int64_t *nm, int64_t *bad)
{
	if (calls++ > 0) return PSVR_ERR_DEVICE;
	const uint8_t *in = (const uint8_t *)in_;
	uint8_t *out = (uint8_t *)out_;
	int64_t at = 0, o = 0, k = 0;
	while (at < n) {
		uint32_t bsize, xlen;
		if (psvr::bgzf_member_header(in + at, (uint64_t)(n - at), &bsize, &xlen) || bsize > n - at) break;
		uint32_t isize;
		memcpy(&isize, in + at + bsize - 4, 4);
		if (o + isize > cap) return PSVR_ERR_OVERFLOW;
		z_stream zs;
		memset(&zs, 0, sizeof zs);
		inflateInit2(&zs, -15);
		zs.next_in = (Bytef *)(in + at + 12 + xlen), zs.avail_in = bsize - 12 - xlen - 8, zs.next_out = out + o, zs.avail_out = isize;
		const int rc = inflate(&zs, Z_FINISH);
		inflateEnd(&zs);
		if (rc != Z_STREAM_END) { *bad = k; return PSVR_ERR_IO; }
		at += bsize, o += isize, ++k;
	}
	*used = at, *got = o, *nm = k;
	return PSVR_OK;
}
}
int main(int argc, char **argv)
{
	psvr::BgzfReader z;
	z.set_batched(0, 3);
	if (!z.open(argv[1])) return 2;
	FILE *o = fopen(argv[2], "wb");
	std::vector<uint8_t> buf(12345);
	for (size_t k = 0;; ++k) {                               // reads of uneven sizes, across slots; then byte by byte to the end
		const size_t n = k < 400 ? 1 + k * 7919 % buf.size() : 1;
		if (!z.read(buf.data(), n)) break;
		fwrite(buf.data(), 1, n, o);
	}
	fclose(o);
	if (!z.error().empty() && z.error() != "truncated BAM stream") { fprintf(stderr, "%s\n", z.error().c_str()); return 3; }
	return calls >= 2 ? 0 : 4;
}
'''


def test_device_failure_continues_on_the_host_without_gap_or_repeat():
    d = tempfile.mkdtemp(prefix="psvr_batchedf_")
    open(os.path.join(d, "t.cpp"), "w").write(FALLBACK)
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-DPSVR_BGZF_ON_DEVICE", "-I" + os.path.join(ac.ROOT, "pansvr_amd", "csrc"), "-o", os.path.join(d, "t"),
                           os.path.join(d, "t.cpp"), "-lz", "-lpthread"])
    data = ic.bam_like_big(3 << 20, 9)
    members = ic.members_of(data, block=30000)
    open(os.path.join(d, "in.bgzf"), "wb").write(b"".join(members) + ic.wrap(ic.deflate(b""), b""))
    r = subprocess.run([os.path.join(d, "t"), os.path.join(d, "in.bgzf"), os.path.join(d, "out.bin")], env=env_of("200000"), stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    assert r.returncode == 0, (r.returncode, r.stderr.decode())
    assert r.stderr.decode().count("BGZF inflate on the device failed") == 1, r.stderr.decode()
    got = open(os.path.join(d, "out.bin"), "rb").read()
    # (a read() that meets the end of the stream hands out nothing: the bytes behind the last whole request are not written)
    assert len(got) > len(data) - 12345 and got == data[:len(got)], "first difference at byte %d" % next((i for i in range(min(len(got), len(data))) if got[i] != data[i]), -1)


# A slot's inflated bytes are bounded (kSlotOutMax, 256 MB): members that inflate a thousandfold fill several slots from one chunk of the
# file, what a cut slot leaves behind goes first into the next, and the stream is the same.
CAPPED = r'''
#include "bam_reader.h"
int main(int argc, char **argv)
{
	psvr::BgzfReader z;
	z.set_batched(-1, 4);
	if (!z.open(argv[1])) return 2;
	std::vector<uint8_t> buf(1 << 20);
	unsigned long long n = 0;
	uint32_t crc = (uint32_t)crc32(0L, Z_NULL, 0);
	while (z.read(buf.data(), buf.size())) n += buf.size(), crc = (uint32_t)crc32(crc, buf.data(), (uInt)buf.size());
	printf("%llu %u [%s]", n, crc, z.error().c_str());
	return 0;
}
'''


def test_a_slot_is_cut_where_its_inflated_bytes_pass_the_bound():
    d = tempfile.mkdtemp(prefix="psvr_batchedc_")
    open(os.path.join(d, "t.cpp"), "w").write(CAPPED)
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-I" + os.path.join(ac.ROOT, "pansvr_amd", "csrc"), "-o", os.path.join(d, "t"), os.path.join(d, "t.cpp"), "-lz", "-lpthread"])
    blocks = [bytes([k]) * 65280 for k in range(7)]
    members = [ic.wrap(ic.deflate(b), b) for b in blocks]
    n = 12288                                                 # 802 MB inflated, a whole number of the driver's 1 MiB requests
    crc = 0
    with open(os.path.join(d, "in.bgzf"), "wb") as f:
        for k in range(n):
            f.write(members[k % 7])
            crc = zlib.crc32(blocks[k % 7], crc)
        f.write(ic.wrap(ic.deflate(b""), b""))
    total = n * 65280
    assert total % (1 << 20) == 0 and os.path.getsize(os.path.join(d, "in.bgzf")) < 2 << 20 and total > 2 * (256 << 20)     # one chunk of the file, three slots
    r = subprocess.run([os.path.join(d, "t"), os.path.join(d, "in.bgzf")], env=env_of(None), stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    assert r.returncode == 0, r.stderr.decode()
    assert r.stdout.decode().split() == [str(total), str(crc), "[]"], r.stdout.decode()


def test_options_that_cannot_apply_are_not_silent(bams):
    r = subprocess.run([CLI, "sort", "--inflate-threads", "0", "-o", os.path.join(tempfile.mkdtemp(prefix="psvr_batched_"), "x.bam"), bams["by-name"]], stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    assert r.returncode == 1 and "--inflate-threads wants a positive number" in r.stderr.decode()
    r = subprocess.run([CLI, "signal", "--inflate-threads", "0", bams["by-name"]], stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    assert r.returncode == 1 and "--inflate-threads wants a positive number" in r.stderr.decode()
