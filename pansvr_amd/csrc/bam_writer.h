// bam_writer.h -- BGZF + BAM record encoder for the CLI's two output files.
//
// Replaces the reference's text -> sam_parse1 -> sam_write1 route when the output is BAM (`output_BAM`,
// `output_ori_bam` rr.cpp:479-536,656-719 write through htslib; `init_run` opens the files "wb" unless -S).
// The vendored htslib cannot be built in this image, so this encoder follows the published
// format (SAM/BAM specification v1, sections 4.1 BGZF and 4.2 BAM) and the typing rules of htslib's sam_parse1:
//   * integer tags take the smallest type that holds the value (c/C/s/S/i/I),
//   * bin = reg2bin(pos, pos + reference length of the CIGAR), or reg2bin(pos, pos + 1) without a CIGAR or with FLAG 0x4
//     (sam_parse1 takes a span of 1 for an unmapped record whatever its CIGAR, htslib sam.c:1270-1278; bam_reg2bin and the length a CIGAR
//     word covers are bam_record.h's, the 0x4 / no-CIGAR decision is this encoder's),
//   * sequence as 4-bit codes of "=ACMGRSVTWYHKDBN", qualities as phred (text - 33), '*' -> 0xff.
// BgzfWriter is the one BGZF block writer: the stream cut every 0xff00 bytes, each block one member (bgzf_format.h has the framing), made
// by zlib or the built-in encoder on the worker pool or, a batch gathered in page-locked memory at a time, by a device compressor of the
// shape of BgzfMembersFn; a failed device call hands its batch and everything after it to the host, in order.  It can log where every
// block starts in the file, which is what the sorted writer's .bai is built from (sorted_bam.h).
// Byte-identity with htslib's BGZF blocks is not claimed (block boundaries and deflate output depend on the
// zlib build); the decompressed stream is pinned byte for byte against the reference's own htslib output
// (tests/golden/<set>/<reads>.bam, written by bam_hdr_write / bam_write1: tests/test_bam_golden.py, tests/test_aln_gpu.py).
#pragma once
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <zlib.h>
#include <atomic>
#include <memory>
#include <string>
#include <vector>
#include "worker_pool.h"
#include "deflate_device.h"
#include "bam_record.h"
#ifdef PSVR_BGZF_ON_DEVICE                            /* (the CLI, which links the engine library: psvr_bgzf_compress) */
#include "../../include/psvr_engine.h"
#endif

namespace psvr {

// A byte buffer whose resize() does not zero what it adds: the record formatters reserve a bound, write through a raw pointer and
// shrink to what they wrote (value-initialising the slack was a second pass over every output byte).
// The shape of psvr_bgzf_compress_members (include/psvr_engine.h): `in` cut into members of member_bytes, written side by side into `out`,
// their offsets into member_off[0..n] when that is not NULL.  The writers take the compressor as a pointer of this type and do not name
// the engine's symbol themselves (cli_main.cpp hands &psvr_bgzf_compress_members in; the tests hand in stand-ins).
typedef int (*BgzfMembersFn)(int device, const void *in, int64_t n_bytes, int32_t member_bytes, void *out, int64_t out_cap, int64_t *out_bytes,
                             int64_t *member_off, int64_t member_cap, int64_t *n_members);

template <class T> struct NoInitAlloc : std::allocator<T> {
	template <class U> struct rebind { typedef NoInitAlloc<U> other; };
	NoInitAlloc() = default;
	template <class U> NoInitAlloc(const NoInitAlloc<U> &) {}
	template <class U> void construct(U *p) { ::new ((void *)p) U; }
	template <class U, class A0, class... A> void construct(U *p, A0 &&a0, A &&...a) { ::new ((void *)p) U(std::forward<A0>(a0), std::forward<A>(a)...); }
};
typedef std::vector<uint8_t, NoInitAlloc<uint8_t>> Bytes;

class BgzfWriter {
	FILE *f_ = nullptr;
	std::vector<uint8_t> buf_;
	std::vector<uint8_t> out_;                    // compressed blocks of a flush
	static const size_t kBlock = kBgzfBlock;      // every block but the last holds this much of the stream, on every route
	static const size_t kOut = 0x10000 + 64;
	bool ok_ = true, compress_failed_ = false;
	int threads_ = 1;
	int level_ = Z_DEFAULT_COMPRESSION;           // htslib's "wb" is zlib's default level too
	int device_ = -1;                             // >= 0: a flush of dev_min_ blocks or more goes to members_ on that device
	BgzfMembersFn members_ = nullptr;
	bool members_are_blocks_ = false;             // the compressor makes one member of every kBlock bytes (set_device_members; not set_device)
	size_t dev_min_;
	uint8_t *pin_in_ = nullptr, *pin_out_ = nullptr;   // page-locked: the records of a batch, its members
	size_t pin_n_ = 0, pin_out_cap_ = 0;
	size_t gather_blocks_;                        // blocks of records gathered in page-locked memory per device call
	bool log_ = false;
	std::vector<uint64_t> starts_;                // log_block_starts()
	std::vector<int64_t> dev_off_;
	uint64_t fpos_ = 0;                           // bytes handed to fwrite
	void put(const uint8_t *p, size_t n) { if (fwrite(p, 1, n, f_) != n) ok_ = false; fpos_ += n; }
	static uint32_t crc_of(const uint8_t *p, size_t n) { return (uint32_t)crc32(crc32(0L, Z_NULL, 0), p, (uInt)n); }
	// one member: raw deflate inside bgzf_wrap (bgzf_format.h); returns the member size
	static size_t compress_block(const uint8_t *p, size_t n, uint8_t *out, int level = Z_DEFAULT_COMPRESSION)
	{
		z_stream zs;
		memset(&zs, 0, sizeof zs);
		if (deflateInit2(&zs, level, Z_DEFLATED, -15, 8, Z_DEFAULT_STRATEGY) != Z_OK) return 0;
		zs.next_in = (Bytef *)p, zs.avail_in = (uInt)n;
		zs.next_out = out + 18, zs.avail_out = (uInt)(kOut - 18 - 8);
		int rc = deflate(&zs, Z_FINISH);
		deflateEnd(&zs);
		if (rc != Z_STREAM_END) return 0;
		return bgzf_wrap(out, (uint32_t)zs.total_out, crc_of(p, n), (uint32_t)n);
	}
	// the same member from this repository's own encoder (deflate_device.h, the one the device route runs a lane per member, here a host
	// thread per member): greedy LZ77 + one dynamic-Huffman block.  1.6 x zlib level 1's speed per thread for members 8 - 10 % larger.
	static size_t compress_block_fast(const uint8_t *p, size_t n, uint8_t *out)
	{
		static const int hbits = 13;
		static thread_local std::vector<uint8_t> fast;
		static thread_local std::vector<uint32_t> tok;
		if (fast.empty()) fast.resize(df_fast_bytes(hbits) + 16), tok.resize(kDfMaxIn + 16);
		if (n > kDfMaxIn) return 0;
		uint32_t *tk = (uint32_t *)(((uintptr_t)tok.data() + 15) & ~(uintptr_t)15);
		const size_t clen = deflate_block(p, (uint32_t)n, out + 18, (uint32_t)(0x10000 - 26), fast.data(), hbits, tk);
		if (!clen) return 0;
		return bgzf_wrap(out, (uint32_t)clen, crc_of(p, n), (uint32_t)n);
	}
#ifdef PSVR_BGZF_ON_DEVICE
	// psvr_bgzf_compress (a lane per block of its own size) in the shape of BgzfMembersFn: the members decode like any other, but they are
	// not members of member_bytes, so it has no offsets to give
	static int lane_per_block(int device, const void *in, int64_t n, int32_t, void *out, int64_t cap, int64_t *got, int64_t *, int64_t, int64_t *) { return psvr_bgzf_compress(device, in, n, out, cap, got); }
#endif
public:
	static const int kLevelFast = -2;             // `level`: zlib's levels, Z_DEFAULT_COMPRESSION (-1), or this: compress_block_fast
	static size_t compress_block_public(const uint8_t *p, size_t n, uint8_t *out) { return compress_block(p, n, out); }   // out: 0x10000 + 64 bytes
private:
	// blocks are independent: from the device in one call, or compressed on `threads_` threads; written in order
	void flush_blocks(const uint8_t *p, size_t n)
	{
		const size_t nb = (n + kBlock - 1) / kBlock;
#ifdef PSVR_BGZF_ON_DEVICE
		if (device_ >= 0 && nb >= dev_min_) {
			const size_t need = members_are_blocks_ ? (size_t)bgzf_members_max((int64_t)n, kBlock) : (size_t)psvr_bgzf_bound((int64_t)n);
			if (need > pin_out_cap_) { if (pin_out_) psvr_host_free(pin_out_); pin_out_ = (uint8_t *)psvr_host_alloc(need), pin_out_cap_ = pin_out_ ? need : 0; }
			int64_t got = 0, nm = 0;
			if (log_) dev_off_.assign(nb + 1, 0);
			if (pin_out_ && members_(device_, p, (int64_t)n, (int32_t)kBlock, pin_out_, (int64_t)pin_out_cap_, &got, log_ ? dev_off_.data() : nullptr, log_ ? (int64_t)nb : 0, log_ ? &nm : nullptr) == 0 &&
			    (!log_ || (size_t)nm == nb)) {
				if (log_) for (size_t b = 0; b < nb; ++b) starts_.push_back(fpos_ + (uint64_t)dev_off_[b]);
				put(pin_out_, (size_t)got);
				return;
			}
			fprintf(stderr, "[panSVR-amd] BGZF on the device failed (%s): compressing on the host\n", psvr_last_error());
			device_ = -1;
		}
#endif
		if (out_.size() < nb * kOut) out_.resize(nb * kOut);      // (kept across calls: a fresh vector was 0.8 GB of zeroing per 1 M pairs)
		std::vector<uint8_t> &out = out_;
		std::vector<size_t> len(nb, 0);
		std::atomic<size_t> next(0);
		auto work = [&]() {
			for (size_t b = next++; b < nb; b = next++) {
				const size_t o = b * kBlock, m = n - o < kBlock ? n - o : kBlock;
				len[b] = level_ == kLevelFast ? compress_block_fast(p + o, m, out.data() + b * kOut) : compress_block(p + o, m, out.data() + b * kOut, level_);
			}
		};
		const int nt = threads_ < 1 ? 1 : (size_t)threads_ > nb ? (int)nb : threads_;
		thread_pool().run(nt, [&](int) { work(); });
		for (size_t b = 0; b < nb; ++b) {
			if (!len[b]) { ok_ = false, compress_failed_ = true; continue; }
			if (log_) starts_.push_back(fpos_);
			put(out.data() + b * kOut, len[b]);
		}
	}
public:
	// dev_min: PSVR_BGZF_DEVICE_MIN_BLOCKS (tests: small files through the device too)
	explicit BgzfWriter(size_t gather_blocks = 3072) : dev_min_(getenv("PSVR_BGZF_DEVICE_MIN_BLOCKS") ? (size_t)atoll(getenv("PSVR_BGZF_DEVICE_MIN_BLOCKS")) : 64), gather_blocks_(gather_blocks < 1 ? 1 : gather_blocks) {}
	bool open(const char *fn, int threads = 1, int level = Z_DEFAULT_COMPRESSION) { f_ = fopen(fn, "wb"); threads_ = threads; level_ = level; return f_ != nullptr; }
	// continues a file that is open already, at a member boundary: whoever wrote it so far has written whole members only (bgzf_stream_sink.h)
	void adopt(FILE *f, int threads = 1, int level = Z_DEFAULT_COMPRESSION) { f_ = f, threads_ = threads, level_ = level; }
	bool ok() const { return ok_; }                             // nothing has failed so far; when something has: in compressing, or in writing
	bool compress_failed() const { return compress_failed_; }
#ifdef PSVR_BGZF_ON_DEVICE
	// compress on HIP device `d` (psvr_bgzf_compress: a lane per block; the members decode like any other, their bytes are not zlib's);
	// refused (false) when the block starts are logged
	bool set_device(int d) { if (log_) return false; device_ = d, members_ = &lane_per_block, members_are_blocks_ = false; return true; }
	// compress on HIP device `d` through `fn` (psvr_bgzf_compress_members: a wavefront per member of 0xff00 bytes), gather_blocks members per
	// call (0: as constructed); before the first write() after open()'s header.  A failed call is handled as on the other device route.
	void set_device_members(int d, BgzfMembersFn fn, size_t gather_blocks = 0) { device_ = d, members_ = fn, members_are_blocks_ = true; if (gather_blocks && !pin_in_) gather_blocks_ = gather_blocks; }
	// a flush of fewer blocks than this (the stream's tail, as a rule) goes to the host though a device is set
	void set_device_min_blocks(size_t n) { dev_min_ = n; }
#endif
	// Keeps the file offset at which every block starts, the EOF block's last: what virtual file offsets (the .bai) are made of.  Block b
	// holds bytes [b * 0xff00, (b + 1) * 0xff00) of the stream on the host route and the members route; set_device's route cuts its own
	// blocks, and the two refuse each other (false).  Before the first write().
	bool log_block_starts() { if (device_ >= 0 && !members_are_blocks_) return false; log_ = true; return true; }
	const std::vector<uint64_t> &block_starts() const { return starts_; }
	void write(const void *p, size_t n)
	{
		const uint8_t *b = (const uint8_t *)p;
#ifdef PSVR_BGZF_ON_DEVICE
		if (device_ >= 0) {
			// the records gather in page-locked memory (the transfer starts from where they lie: out of pageable memory the runtime copies
			// them once more), whole batches go to the device, what is left at close() to the device or, below dev_min_ blocks, the host's zlib
			const size_t cap = kBlock * gather_blocks_;
			if (!pin_in_ && !(pin_in_ = (uint8_t *)psvr_host_alloc(cap))) { device_ = -1; }
			else {
				if (!buf_.empty()) { std::vector<uint8_t> first; first.swap(buf_); write(first.data(), first.size()); }   // (what was written before set_device: the BAM header)
				while (n && device_ >= 0) {                   // (a failed device call turns device_ off: the rest of this call goes the host's way)
					const size_t m = cap - pin_n_ < n ? cap - pin_n_ : n;
					memcpy(pin_in_ + pin_n_, b, m), pin_n_ += m, b += m, n -= m;
					if (pin_n_ == cap) flush_blocks(pin_in_, pin_n_), pin_n_ = 0;
				}
				if (!n) return;
			}
		}
		// records gathered for the device and not yet sent come before anything written from here on
		if (pin_n_) buf_.insert(buf_.end(), pin_in_, pin_in_ + pin_n_), pin_n_ = 0;
#endif
		buf_.insert(buf_.end(), b, b + n);
		// enough whole blocks to keep every thread busy; on the device a call lasts as long as ONE block takes a lane (tens of ms) however
		// many blocks it holds, so the batches are large
		const size_t batch = device_ >= 0 ? kBlock * gather_blocks_ : kBlock * (size_t)(threads_ < 1 ? 1 : threads_) * 8;
		if (buf_.size() < batch) return;
		const size_t whole = buf_.size() / kBlock * kBlock;
		flush_blocks(buf_.data(), whole);
		buf_.erase(buf_.begin(), buf_.begin() + whole);
	}
	bool close()
	{
		if (!f_) return false;
#ifdef PSVR_BGZF_ON_DEVICE
		if (pin_n_) flush_blocks(pin_in_, pin_n_), pin_n_ = 0;
		if (pin_in_) psvr_host_free(pin_in_), pin_in_ = nullptr;
		if (pin_out_) psvr_host_free(pin_out_), pin_out_ = nullptr, pin_out_cap_ = 0;
#endif
		if (!buf_.empty()) flush_blocks(buf_.data(), buf_.size());
		if (log_) starts_.push_back(fpos_);
		put(kBgzfEof, sizeof kBgzfEof);
		if (fclose(f_) != 0) ok_ = false;
		f_ = nullptr;
		return ok_;
	}
};

// htslib's seq_nt16_table (hts.c:62-80): the 4-bit code a SEQ character is stored as -- IUPAC letters in either case, '=' and
// the digits 0-3 (A, C, G, T); everything else is N.  A record that went through BAM comes back as "=ACMGRSVTWYHKDBN"[code].
inline int nt16_code(char ch)
{
	static const char *nt16 = "=ACMGRSVTWYHKDBN";
	if (ch >= '0' && ch <= '3') return 1 << (ch - '0');
	if (ch >= 'a' && ch <= 'z') ch = (char)(ch - 32);
	const char *q = ch ? strchr(nt16, ch) : nullptr;
	return q ? (int)(q - nt16) : 15;
}
inline char nt16_char(char ch) { return "=ACMGRSVTWYHKDBN"[nt16_code(ch)]; }
struct Nt16Table { uint8_t code[256]; Nt16Table() { for (int c = 0; c < 256; ++c) code[c] = (uint8_t)nt16_code((char)c); } };
inline const uint8_t *nt16_table() { static const Nt16Table t; return t.code; }        // (nt16_code per base is a strchr per base)

struct BamRef { std::string name; uint32_t len; };

// what a BAM stream starts with (SAMv1 4.2): magic, header text, reference names and lengths
inline std::vector<uint8_t> bam_header_block(const std::string &text, const std::vector<BamRef> &refs)
{
	std::vector<uint8_t> h = {'B', 'A', 'M', 1};
	auto put32 = [&](uint32_t x) { for (int i = 0; i < 4; ++i) h.push_back((uint8_t)(x >> (8 * i))); };
	put32((uint32_t)text.size());
	h.insert(h.end(), text.begin(), text.end());
	put32((uint32_t)refs.size());
	for (const BamRef &r : refs) { put32((uint32_t)r.name.size() + 1); h.insert(h.end(), r.name.begin(), r.name.end()); h.push_back(0); put32(r.len); }
	return h;
}

// one alignment record in SAM terms (what the CLI's emit_record prints)
struct SamFields {
	std::string qname, cigar, seq, qual, tags;   // tags: "\tXX:t:value..." as in the SAM line; cigar/seq/qual may be "*"
	int flag = 0, tid = -1, mapq = 0, mtid = -1, isize = 0;
	int64_t pos1 = 0, mpos1 = 0;                 // 1-based; 0 = unset
};

class BamWriter {
	BgzfWriter z_;
public:
	explicit BamWriter(size_t gather_blocks = 3072) : z_(gather_blocks) {}      // gather_blocks: BgzfWriter's, per device call
private:
	template <class V> static void put32(V &v, uint32_t x) { for (int i = 0; i < 4; ++i) v.push_back((uint8_t)(x >> (8 * i))); }
	template <class V> static void put16(V &v, uint16_t x) { v.push_back((uint8_t)x), v.push_back((uint8_t)(x >> 8)); }
	template <class V> static void put_int_tag(V &v, long long x)   // smallest type, as sam_parse1 chooses
	{
		if (x < 0) {
			if (x >= -128) v.push_back('c'), v.push_back((uint8_t)(int8_t)x);
			else if (x >= -32768) v.push_back('s'), put16(v, (uint16_t)(int16_t)x);
			else v.push_back('i'), put32(v, (uint32_t)(int32_t)x);
		} else {
			if (x <= 255) v.push_back('C'), v.push_back((uint8_t)x);
			else if (x <= 65535) v.push_back('S'), put16(v, (uint16_t)x);
			else v.push_back('I'), put32(v, (uint32_t)x);
		}
	}
	template <class V> static bool put_tags(V &v, const std::string &tags)
	{
		size_t i = 0;
		while (i < tags.size()) {
			if (tags[i] == '\t') { ++i; continue; }
			size_t e = tags.find('\t', i);
			if (e == std::string::npos) e = tags.size();
			if (e - i < 5 || tags[i + 2] != ':' || tags[i + 4] != ':') return false;
			v.push_back((uint8_t)tags[i]), v.push_back((uint8_t)tags[i + 1]);
			const char ty = tags[i + 3];
			const std::string val = tags.substr(i + 5, e - (i + 5));
			if (ty == 'i') put_int_tag(v, strtoll(val.c_str(), nullptr, 10));
			else if (ty == 'A') { v.push_back('A'); v.push_back(val.empty() ? ' ' : (uint8_t)val[0]); }
			else if (ty == 'f') { v.push_back('f'); float fl = strtof(val.c_str(), nullptr); uint32_t u; memcpy(&u, &fl, 4); put32(v, u); }
			else if (ty == 'Z' || ty == 'H') { v.push_back((uint8_t)ty); v.insert(v.end(), val.begin(), val.end()); v.push_back(0); }
			else if (ty == 'B') {
				if (val.empty()) return false;
				const char st = val[0];
				std::vector<std::string> items;
				size_t p = 1;
				while (p < val.size()) { size_t q = val.find(',', p + 1); if (q == std::string::npos) q = val.size(); items.push_back(val.substr(p + 1, q - p - 1)); p = q; }
				v.push_back('B'), v.push_back((uint8_t)st), put32(v, (uint32_t)items.size());
				for (const std::string &it : items) {
					if (st == 'f') { float fl = strtof(it.c_str(), nullptr); uint32_t u; memcpy(&u, &fl, 4); put32(v, u); }
					else {
						long long x = strtoll(it.c_str(), nullptr, 10);
						if (st == 'c' || st == 'C') v.push_back((uint8_t)x);
						else if (st == 's' || st == 'S') put16(v, (uint16_t)x);
						else put32(v, (uint32_t)x);
					}
				}
			} else return false;
			i = e;
		}
		return true;
	}
public:
	bool open(const char *fn, const std::string &header_text, const std::vector<BamRef> &refs, int threads = 1, int level = Z_DEFAULT_COMPRESSION)
	{
		if (!z_.open(fn, threads, level)) return false;
		const std::vector<uint8_t> h = bam_header_block(header_text, refs);
		z_.write(h.data(), h.size());
		return true;
	}
	// appends one encoded record (block_size + body) to `out`; thread-safe (touches no writer state)
	template <class V> static bool encode(const SamFields &s, V &rec_)
	{
		const size_t base = rec_.size();
		if (s.qname.empty() || s.qname.size() > 254) return false;   // l_read_name is one byte (htslib: "query name too long")
		std::vector<uint32_t> cig;
		int64_t rlen = 0;
		if (!s.cigar.empty() && s.cigar != "*") {
			long long n = 0;
			bool neg = false;
			for (char ch : s.cigar) {
				if (ch == '-') { neg = true; continue; }
				if (ch >= '0' && ch <= '9') { n = n * 10 + (ch - '0'); continue; }
				const char *ops = "MIDNSHP=XB", *q = strchr(ops, ch);       // BAM_CIGAR_STR
				if (!q) return false;
				if (neg) n = -n;
				const int op = (int)(q - ops);
				cig.push_back((uint32_t)n << 4 | (uint32_t)op);
				rlen += bam_cigar_ref_len(cig.back());
				n = 0, neg = false;
			}
		}
		const bool no_seq = s.seq.empty() || s.seq == "*";
		const uint32_t l_seq = no_seq ? 0 : (uint32_t)s.seq.size();
		const int64_t pos0 = s.pos1 - 1;
		put32(rec_, 0);                                             // block_size, patched below
		put32(rec_, (uint32_t)s.tid), put32(rec_, (uint32_t)(int32_t)pos0);
		rec_.push_back((uint8_t)(s.qname.size() + 1)), rec_.push_back((uint8_t)s.mapq);
		const bool has_cigar = !s.cigar.empty() && s.cigar != "*";
		put16(rec_, (uint16_t)bam_reg2bin(pos0 < 0 ? 0 : pos0, (pos0 < 0 ? 0 : pos0) + (has_cigar && !(s.flag & 0x4) ? rlen : 1)));
		if (cig.size() > 0xffff) { rec_.resize(base); return false; }     // n_cigar_op is 16 bits (no CG:B long-CIGAR tag is written)
		put16(rec_, (uint16_t)cig.size()), put16(rec_, (uint16_t)s.flag);
		put32(rec_, l_seq);
		put32(rec_, (uint32_t)s.mtid), put32(rec_, (uint32_t)(int32_t)(s.mpos1 - 1)), put32(rec_, (uint32_t)s.isize);
		rec_.insert(rec_.end(), s.qname.begin(), s.qname.end());
		rec_.push_back(0);
		for (uint32_t c : cig) put32(rec_, c);
		if (l_seq) {
			const uint8_t *T = nt16_table();
			const size_t at = rec_.size(), nb = (l_seq + 1) / 2;
			rec_.resize(at + nb + l_seq);
			uint8_t *q = &rec_[at];
			const uint8_t *sq = (const uint8_t *)s.seq.data();
			for (uint32_t i = 0; i + 1 < l_seq; i += 2) *q++ = (uint8_t)(T[sq[i]] << 4 | T[sq[i + 1]]);
			if (l_seq & 1) *q++ = (uint8_t)(T[sq[l_seq - 1]] << 4);
			if (s.qual.empty() || s.qual == "*" || s.qual.size() != l_seq) memset(q, 0xff, l_seq);
			else for (uint32_t i = 0; i < l_seq; ++i) q[i] = (uint8_t)(s.qual[i] - 33);
		}
		if (!put_tags(rec_, s.tags)) { rec_.resize(base); return false; }
		const uint32_t bs = (uint32_t)(rec_.size() - base) - 4;
		for (int i = 0; i < 4; ++i) rec_[base + i] = (uint8_t)(bs >> (8 * i));
		return true;
	}
	bool write(const SamFields &s)
	{
		std::vector<uint8_t> rec;
		if (!encode(s, rec)) return false;
		z_.write(rec.data(), rec.size());
		return true;
	}
	void write_raw(const void *p, size_t n) { z_.write(p, n); }
	BgzfWriter &bgzf() { return z_; }                          // (set_device, set_device_members)
	bool close() { return z_.close(); }
};

} // namespace psvr
