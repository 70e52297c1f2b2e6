// bam_reader.h -- sequential BAM reader for the `signal` step (SAM/BAM specification v1, sections 4.1-4.2): BGZF members
// inflated with zlib, the header, then one alignment record after the other.  Host C++ only; it replaces the reference's use of
// htslib (sam_read1 / bam_aux_get / bam_aux2i) for the fields that step looks at.
// Two ways through the BGZF layer behind the same read(): the serial one (a member at a time on the calling thread, the default), and a
// batched one (set_batched: --inflate-device / --inflate-threads) in which a reader thread takes the file in chunks, cuts each at its last
// whole member and has the members inflated side by side -- on the device (psvr_bgzf_decompress, one wavefront per member) or with zlib on
// a pool of host threads -- while the caller walks the bytes of the chunk before.
#pragma once
#include <zlib.h>
#include <atomic>
#include <condition_variable>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <string>
#include <thread>
#include <vector>
#include "inflate_device.h"
#include "worker_pool.h"
#include "bam_record.h"
#ifdef PSVR_BGZF_ON_DEVICE                            /* (the CLI, which links the engine library: psvr_bgzf_decompress, page-locked slots) */
#include "../../include/psvr_engine.h"
#endif

namespace psvr {

// a host buffer that owns its memory: page-locked (psvr_host_alloc) when the device reads or writes it, plain otherwise
struct InflateBuf {
	uint8_t *p = nullptr;
	size_t cap = 0;
	bool pinned = false;
	InflateBuf() = default;
	InflateBuf(const InflateBuf &) = delete;
	InflateBuf &operator=(const InflateBuf &) = delete;
	~InflateBuf() { release(); }
	void release()
	{
#ifdef PSVR_BGZF_ON_DEVICE
		if (p && pinned) psvr_host_free(p), p = nullptr;
#endif
		free(p), p = nullptr, cap = 0;
	}
	bool ensure(size_t n, size_t keep, bool want_pinned)   // room for n bytes; the first `keep` survive
	{
		if (n <= cap) return true;
		n += n / 4 + 64;
		uint8_t *q = nullptr;
		bool q_pinned = false;
#ifdef PSVR_BGZF_ON_DEVICE
		if (want_pinned && (q = (uint8_t *)psvr_host_alloc(n))) q_pinned = true;
#endif
		(void)want_pinned;
		if (!q && !(q = (uint8_t *)malloc(n))) return false;
		if (keep) memcpy(q, p, keep);
		release();
		p = q, cap = n, pinned = q_pinned;
		return true;
	}
};

class BgzfReader {
	FILE *f = nullptr;
	std::vector<uint8_t> in, out;
	const uint8_t *cur_p = nullptr;       // the inflated bytes being handed out: `out` (serial) or a slot's (batched)
	size_t cur_n = 0;
	size_t pos = 0;                       // read position in them
	size_t taken = 0;                     // inflated bytes handed out so far
	bool eof = false;
	std::string err;

	// ---- the batched mode ------------------------------------------------------------------------------------------------------------
	struct Member { size_t in_off, out_off; uint32_t bsize, hdr, isize; };
	struct Slot {
		InflateBuf in, out;
		std::vector<Member> mem;
		size_t len = 0;                   // inflated bytes that are valid
		std::string err;                  // what ends the stream behind them
		bool last = false, ready = false;
	};
	bool batched = false;
	int device = -1, threads = 0;
	size_t chunk = 0;
	Slot slot[2];
	int cur = -1;
	bool finished = false, stop = false;
	std::string pending_err;              // the last slot's error, due when its bytes are used up
	std::mutex mu;
	std::condition_variable cv;
	std::thread producer;

	static const size_t kSlotOutMax = (size_t)256 << 20;   // inflated bytes per slot (16 MiB of BAM members inflate to 40 - 80 MB)
	static size_t batch_bytes()            // PSVR_INFLATE_BATCH=<bytes>: compressed bytes per chunk
	{
		static const size_t v = [] { const char *e = getenv("PSVR_INFLATE_BATCH"); const long long x = e ? atoll(e) : 0; return (size_t)(x >= 1 ? x : (16ll << 20)); }();
		return v;
	}
	// the members M of S.in inflated into S.out: -1, or the first member that is corrupt
	long long inflate_host(Slot &S)
	{
		const int nt = threads < 1 ? 1 : threads > 64 ? 64 : threads;
		std::atomic<size_t> next(0);
		std::atomic<long long> bad(-1);
		thread_pool().run(nt, [&](int) {
			z_stream zs;
			memset(&zs, 0, sizeof zs);
			if (inflateInit2(&zs, -15) != Z_OK) { bad = 0; return; }
			for (;;) {
				const size_t i = next++;
				if (i >= S.mem.size()) break;
				const Member &m = S.mem[i];
				const uint8_t *p = S.in.p + m.in_off;
				inflateReset(&zs);
				zs.next_in = (Bytef *)(p + m.hdr), zs.avail_in = m.bsize - m.hdr - 8, zs.next_out = S.out.p + m.out_off, zs.avail_out = m.isize;
				const int rc = inflate(&zs, Z_FINISH);
				const uint32_t want = p[m.bsize - 8] | (uint32_t)p[m.bsize - 7] << 8 | (uint32_t)p[m.bsize - 6] << 16 | (uint32_t)p[m.bsize - 5] << 24;
				if (rc != Z_STREAM_END || zs.total_out != m.isize || (uint32_t)crc32(crc32(0L, Z_NULL, 0), S.out.p + m.out_off, m.isize) != want) {
					long long seen = bad.load();
					while ((seen < 0 || (long long)i < seen) && !bad.compare_exchange_weak(seen, (long long)i)) {}
				}
			}
			inflateEnd(&zs);
		});
		return bad.load();
	}
	long long inflate_slot(Slot &S, size_t used, size_t total)
	{
#ifdef PSVR_BGZF_ON_DEVICE
		if (device >= 0) {
			int64_t in_used = 0, out_bytes = 0, nm = 0, bad = -1;
			const int rc = psvr_bgzf_decompress(device, S.in.p, (int64_t)used, &in_used, S.out.p, (int64_t)total, &out_bytes, nullptr, 0, &nm, &bad);
			if (rc == PSVR_OK && (size_t)in_used == used && (size_t)out_bytes == total) return -1;
			if (rc == PSVR_ERR_IO && bad >= 0 && bad < (int64_t)S.mem.size()) return bad;
			// the device route is given up: this slot, from its first member, and everything behind it go through the host pool
			fprintf(stderr, "[panSVR-amd] BGZF inflate on the device failed (%s): reading on %d host threads from here on\n", rc == PSVR_OK ? "sizes differ" : psvr_last_error(), threads);
			device = -1;
		}
#endif
		(void)used, (void)total;
		return inflate_host(S);
	}
	void produce()
	{
		std::vector<uint8_t> carry;                           // what lay behind the last whole member of the chunk before
		bool file_end = false;
		for (int s = 0;; s ^= 1) {
			Slot &S = slot[s];
			{
				std::unique_lock<std::mutex> lk(mu);
				cv.wait(lk, [&] { return stop || !S.ready; });
				if (stop) return;
			}
			const bool pin = device >= 0;
			S.len = 0, S.err.clear(), S.last = false, S.mem.clear();
			size_t have = carry.size(), used = 0, total = 0;
			bool ok = S.in.ensure(have + (file_end ? 0 : chunk), 0, pin), capped = false;
			if (ok && have) memcpy(S.in.p, carry.data(), have);
			carry.clear();
			for (bool first = true; ok; first = false) {      // chunks until one whole member is there (a chunk may be smaller than a member)
				if (!file_end && (!first || have < chunk)) {  // (what a capped slot left behind is used up before more is read)
					if (!(ok = S.in.ensure(have + chunk, have, pin))) break;
					const size_t k = fread(S.in.p + have, 1, chunk, f);
					have += k;
					if (k < chunk) file_end = true;
				}
				while (used < have) {
					const uint8_t *p = S.in.p + used;
					uint32_t bsize = 0, xlen = 0;
					const int h = bgzf_member_header(p, have - used, &bsize, &xlen);
					if (h == 1 || (h == 0 && bsize > have - used)) break;
					if (h == 2) { S.err = (p[0] != 0x1f || p[1] != 0x8b || p[2] != 8 || !(p[3] & 4)) ? "not a BGZF block" : "BGZF block without a BC field"; break; }
					const uint32_t isize = p[bsize - 4] | (uint32_t)p[bsize - 3] << 8 | (uint32_t)p[bsize - 2] << 16 | (uint32_t)p[bsize - 1] << 24;
					if (!inf_isize_possible(isize, bsize - 12 - xlen - 8)) { S.err = "corrupt BGZF block"; break; }
					// (ISIZE is the file's word: a slot is cut where its inflated bytes pass a bound, so that a hostile file meets the
					// decoder's "corrupt BGZF block" a member or a few at a time, as in the serial reader, not an allocation of its choosing)
					if (!S.mem.empty() && total + isize > kSlotOutMax) { capped = true; break; }
					S.mem.push_back({used, total, bsize, 12 + xlen, isize});
					used += bsize, total += isize;
				}
				if (!S.err.empty() || !S.mem.empty() || file_end) break;                        // (capped implies a member)
			}
			if (!ok) S.err = "out of memory for a BGZF batch";
			else if (S.err.empty() && !capped && file_end && used < have) S.err = have - used < 18 ? "not a BGZF block" : "truncated BGZF block";
			else if (S.err.empty()) carry.assign(S.in.p + used, S.in.p + have);
			if (ok && !S.mem.empty()) {
				if (!S.out.ensure(total + 1, 0, pin)) S.err = "out of memory for a BGZF batch";
				else {
					const long long bad = inflate_slot(S, used, total);
					if (bad >= 0) S.len = S.mem[(size_t)bad].out_off, S.err = "corrupt BGZF block";
					else S.len = total;
				}
			}
			S.last = !S.err.empty() || (file_end && carry.empty());
			const bool last = S.last;
			{
				std::lock_guard<std::mutex> lk(mu);
				S.ready = true;
			}
			cv.notify_all();
			if (last) return;
		}
	}
	bool next_slot()
	{
		if (cur >= 0) {
			{
				std::lock_guard<std::mutex> lk(mu);
				slot[cur].ready = false;
			}
			cv.notify_all();
		}
		cur_p = nullptr, cur_n = 0, pos = 0;
		if (finished) { err = pending_err; eof = true; return false; }
		cur = cur < 0 ? 0 : cur ^ 1;
		Slot &S = slot[cur];
		{
			std::unique_lock<std::mutex> lk(mu);
			cv.wait(lk, [&] { return S.ready; });
		}
		cur_p = S.out.p, cur_n = S.len;
		if (S.last) {
			finished = true;
			if (cur_n == 0) { err = S.err; eof = true; cur = -1; return false; }
			pending_err = S.err;
			cur = -1;                                         // (the producer is through: nothing to hand back)
		}
		return true;
	}

	bool next_block()
	{
		uint8_t h[18];
		size_t got = fread(h, 1, 18, f);
		if (got == 0) { eof = true; return false; }
		if (got != 18 || h[0] != 0x1f || h[1] != 0x8b || h[2] != 8 || !(h[3] & 4)) { err = "not a BGZF block"; eof = true; return false; }
		const unsigned xlen = h[10] | (unsigned)h[11] << 8;
		// the BC subfield is the first one in every BGZF writer's output; walk the extra field to be safe
		std::vector<uint8_t> extra(xlen);
		memcpy(extra.data(), h + 12, xlen < 6 ? xlen : 6);
		if (xlen > 6 && fread(extra.data() + 6, 1, xlen - 6, f) != xlen - 6) { err = "truncated BGZF block"; eof = true; return false; }
		unsigned bsize = 0;
		for (unsigned o = 0; o + 4 <= xlen;) {
			const unsigned slen = extra[o + 2] | (unsigned)extra[o + 3] << 8;
			if (extra[o] == 'B' && extra[o + 1] == 'C' && slen == 2 && o + 6 <= xlen) bsize = (extra[o + 4] | (unsigned)extra[o + 5] << 8) + 1;
			o += 4 + slen;
		}
		if (bsize < 12 + xlen + 8) { err = "BGZF block without a BC field"; eof = true; return false; }
		const size_t clen = bsize - 12 - xlen - 8;
		in.resize(clen + 8);
		if (fread(in.data(), 1, clen + 8, f) != clen + 8) { err = "truncated BGZF block"; eof = true; return false; }
		const uint32_t isize = in[clen + 4] | (uint32_t)in[clen + 5] << 8 | (uint32_t)in[clen + 6] << 16 | (uint32_t)in[clen + 7] << 24;
		out.resize(isize);
		pos = 0, cur_p = out.data(), cur_n = isize;
		if (isize == 0) return true;      // the end-of-file marker block (or an empty one)
		z_stream zs;
		memset(&zs, 0, sizeof zs);
		if (inflateInit2(&zs, -15) != Z_OK) { err = "zlib"; eof = true; return false; }
		zs.next_in = in.data(), zs.avail_in = (uInt)clen, zs.next_out = out.data(), zs.avail_out = isize;
		const int rc = inflate(&zs, Z_FINISH);
		inflateEnd(&zs);
		if (rc != Z_STREAM_END || zs.total_out != isize) { err = "corrupt BGZF block"; eof = true; return false; }
		return true;
	}

public:
	// Before open(): members are inflated a chunk at a time, on HIP device `dev` (>= 0) or by `nthreads` host threads (which also take over
	// when a device call fails).  Without a visible device, or in a build without the engine library, the host threads do the work.
	void set_batched(int dev, int nthreads)
	{
		batched = true, device = dev, threads = nthreads >= 1 ? nthreads : 4, chunk = batch_bytes();
		if (dev < 0) return;
#ifdef PSVR_BGZF_ON_DEVICE
		if (psvr_device_count() > 0) return;
		fprintf(stderr, "[panSVR-amd] --inflate-device: no HIP device visible, reading on %d host threads\n", threads);
#else
		fprintf(stderr, "[panSVR-amd] --inflate-device: this build has no device route, reading on %d host threads\n", threads);
#endif
		device = -1;
	}
	bool open(const char *path)
	{
		f = !strcmp(path, "-") ? stdin : fopen(path, "rb");
		if (f && batched) producer = std::thread([this] { produce(); });
		return f != nullptr;
	}
	void close()
	{
		if (producer.joinable()) {
			{
				std::lock_guard<std::mutex> lk(mu);
				stop = true, slot[0].ready = slot[1].ready = false;
			}
			cv.notify_all();
			producer.join();
		}
		if (f && f != stdin) fclose(f);
		f = nullptr;
	}
	~BgzfReader() { close(); }
	const std::string &error() const { return err; }
	size_t bytes_read() const { return taken; }
	// exactly n bytes, or false at the end of the file (err is set when the end comes inside a request)
	bool read(void *dst, size_t n)
	{
		uint8_t *d = (uint8_t *)dst;
		size_t done = 0;
		while (done < n) {
			if (pos == cur_n) {
				if (eof || !(batched ? next_slot() : next_block())) { if (done) err = "truncated BAM stream"; return false; }
				continue;
			}
			const size_t k = cur_n - pos < n - done ? cur_n - pos : n - done;
			memcpy(d + done, cur_p + pos, k);
			pos += k, done += k, taken += k;
		}
		return true;
	}
};

struct BamRecord {                     // one alignment, fields as in bam1_core_t
	int32_t tid = -1, pos = -1, mtid = -1, mpos = -1, isize = 0, l_qseq = 0;
	uint16_t flag = 0, n_cigar = 0;
	uint8_t mapq = 0, l_qname = 0;
	std::vector<uint8_t> data;         // qname | cigar | seq (4-bit) | qual | aux
	const char *qname() const { return (const char *)data.data(); }
	uint32_t cig(unsigned k) const { uint32_t v; memcpy(&v, data.data() + l_qname + 4 * (size_t)k, 4); return v; }   // the CIGAR words are not aligned (the name's length decides)
	const uint8_t *seq() const { return data.data() + l_qname + 4 * (size_t)n_cigar; }
	const uint8_t *qual() const { return seq() + (l_qseq + 1) / 2; }
	const uint8_t *aux() const { return qual() + l_qseq; }
	const uint8_t *aux_end() const { return data.data() + data.size(); }
	// bam_aux_get: pointer to the type byte of the tag, or null.  A tag is only returned when its whole value lies inside the
	// record (Z/H: including the terminating NUL), so num_tag()/string_tag() and their callers never read past the end of a
	// malformed record.
	const uint8_t *aux_get(const char tag[2]) const { return bam_aux_find(aux(), aux_end(), tag[0], tag[1]); }   // (bam_record.h: the device walks the same function)
	// bam_get_string_tag (clib/bam_file.c:427-438): only 'Z'
	const char *string_tag(const char tag[2]) const
	{
		const uint8_t *p = aux_get(tag);
		return p && p[0] == 'Z' ? (const char *)(p + 1) : nullptr;
	}
	// bam_get_num_tag (clib/bam_file.c:456-468): integer codes only
	bool num_tag(const char tag[2], int32_t *num) const { return bam_aux_int(aux_get(tag), num); }
};

// the fixed part of a record (h: its first 36 bytes, block_size first) into r's fields
inline void bam_record_head(const uint8_t *h, BamRecord &r)
{
	r.tid = bam_i32(h + 4), r.pos = bam_i32(h + 8);
	r.l_qname = h[12], r.mapq = h[13];
	r.n_cigar = bam_u16(h + 16), r.flag = bam_u16(h + 18);
	r.l_qseq = bam_i32(h + 20), r.mtid = bam_i32(h + 24), r.mpos = bam_i32(h + 28), r.isize = bam_i32(h + 32);
}
// what BamReader::next asks of a record whose head and data are there: null, or what is wrong with it
inline const char *bam_record_check(const uint8_t *h, const BamRecord &r)
{
	if (!bam_rec_fields_inside(h)) return "bad BAM record";
	if (r.l_qname == 0 || r.data[(size_t)r.l_qname - 1] != 0) return "bad BAM record (read name not NUL-terminated)";   // qname() is used as a C string
	return nullptr;
}
// a BamRecord from a record's bytes (block_size first, `avail` bytes are there), by the reader's rules: null, or what is wrong with it
inline const char *bam_record_from_bytes(const uint8_t *rec, size_t avail, BamRecord &r)
{
	if (avail < 4 || bam_i32(rec) < (int32_t)kBamRecMinBlock) return "bad BAM record";
	if (avail - 4 < (size_t)bam_u32(rec)) return "truncated BAM record";
	bam_record_head(rec, r);
	r.data.assign(rec + kBamRecHead, rec + 4 + (size_t)bam_u32(rec));
	return bam_record_check(rec, r);
}

class BamReader {
	BgzfReader z;
	std::string err;

public:
	std::string header_text;
	std::vector<std::pair<std::string, int32_t>> refs;
	size_t header_bytes = 0;              // inflated bytes in front of the first record (set by open)
	const std::string &error() const { return err.empty() ? z.error() : err; }
	void set_batched(int device, int threads) { z.set_batched(device, threads); }   // before open(): see BgzfReader
	bool open(const char *path)
	{
		if (!z.open(path)) { err = std::string("cannot open ") + path; return false; }
		char magic[4];
		int32_t l_text = 0, n_ref = 0;
		if (!z.read(magic, 4) || memcmp(magic, "BAM\1", 4)) { err = "not a BAM file"; return false; }
		if (!z.read(&l_text, 4) || l_text < 0) { err = "bad BAM header"; return false; }
		header_text.resize((size_t)l_text);
		if (l_text && !z.read(&header_text[0], (size_t)l_text)) { err = "bad BAM header"; return false; }
		while (!header_text.empty() && header_text.back() == '\0') header_text.pop_back();
		if (!z.read(&n_ref, 4) || n_ref < 0) { err = "bad BAM header"; return false; }
		for (int i = 0; i < n_ref; ++i) {
			int32_t l_name = 0, l_ref = 0;
			if (!z.read(&l_name, 4) || l_name <= 0) { err = "bad BAM header"; return false; }
			std::string name((size_t)l_name, '\0');
			if (!z.read(&name[0], (size_t)l_name) || !z.read(&l_ref, 4)) { err = "bad BAM header"; return false; }
			name.resize(strlen(name.c_str()));
			refs.push_back({name, l_ref});
		}
		header_bytes = z.bytes_read();
		return true;
	}
	// sam_read1: false at the end of the file (error() is empty then) or on a malformed record
	bool next(BamRecord &r)
	{
		uint8_t h[kBamRecHead];                                      // the record's head as bam_record.h takes it: block_size first
		if (!z.read(h, 4)) return false;
		const int32_t block = bam_i32(h);
		if (block < (int32_t)kBamRecMinBlock) { err = "bad BAM record"; return false; }
		if (!z.read(h + 4, 32)) { err = "truncated BAM record"; return false; }
		bam_record_head(h, r);
		r.data.resize((size_t)block - 32);
		if (block > 32 && !z.read(r.data.data(), (size_t)block - 32)) { err = "truncated BAM record"; return false; }
		if (const char *bad = bam_record_check(h, r)) { err = bad; return false; }
		return true;
	}
};

} // namespace psvr
