// sorted_bam.h -- the sorted BAM writer shared by `panSVR sort` (bam_sort.h) and `panSVR aln --sort` (cli_main.cpp): what
// `samtools sort` + `samtools index` produce between the `aln` and `fc_sv` steps of panSVR_run.sh (lines 53-54).  Host C++ above the C ABI.
//   SortRecords          the encoded records (block_size + body, the fixed part re-encoded with the bin taken from the CIGAR's span)
//                        and samtools' coordinate key of each; what a record is, its span, bin and key are bam_record.h's
//   coordinate_order     samtools' order (bam_sort.c bam1_lt): reference id as unsigned (unplaced records last), position, forward strand
//                        before reverse, ties in input order.  On the device (psvr_sort_order_u64) when one is visible and every
//                        position lies in SAMv1's range; otherwise std::stable_sort on the host.
//   write_sorted_bam     the header with SO rewritten and the records in the given order through BgzfWriter (bam_writer.h: blocks of
//                        0xff00 bytes from `threads` pool threads or, with a device compressor, a window of blocks per call, the stream's
//                        tail included; a failed call hands that window and all later ones to the host), and (coordinate order) the .bai
//                        of SAMv1 section 5.2 from the writer's log of block starts: bins with their chunk lists (virtual file offsets),
//                        the 16 kbp linear index, the per-reference metadata pseudo-bin 37450 and n_no_coor.
//   write_sorted_store   the same file and index from a device-resident record store (psvr_bam_store_*): ordered, gathered and compressed
//                        there, so that only the compressed members and the table the .bai is built from come to the host; and
//                        finish_sorted_store, what `panSVR sort --sort-device` and `--nsort-device` end with
// The sorted stream never exists in memory as a whole, only the records do.
#pragma once
#include <stdint.h>
#include <stdio.h>
#include <string.h>
#include <time.h>
#include <algorithm>
#include <map>
#include <string>
#include <utility>
#include <vector>
#include "../../include/psvr_engine.h"
#include "bam_writer.h"
#include "member_take.h"

namespace psvr {

// what the sorter and the .bai need of one record (bam_rec_derived, bam_record.h): end = max(pos, 0) + the CIGAR's reference span (1 base without
// one), len = 4 + block_size
struct BaiRecord { int32_t tid, pos; int64_t end; uint32_t bin, flag, len; };

struct SortRecords {
	// every record (block_size + body) in chunks of kChunk bytes that are allocated once and never grow: the records take their own
	// size in memory, not the up to 3x of one vector that doubles as it fills
	static const size_t kChunk = (size_t)64 << 20;
	std::vector<std::vector<uint8_t>> chunk;
	std::vector<uint64_t> off;              // record i: chunk index << 32 | offset in the chunk
	std::vector<uint64_t> key;              // bam_sort_key (bam_record.h)
	bool key_exact = true;                  // bam_key_exact for every record: the key orders exactly as the comparator
	uint64_t bytes = 0;                     // the records' total size
	size_t size() const { return off.size(); }
	const uint8_t *rec(size_t i) const { return chunk[(size_t)(off[i] >> 32)].data() + (off[i] & 0xffffffffu); }
	static uint32_t u32(const uint8_t *p) { return bam_u32(p); }                   // (the names the sink's stand-in store reads a record by)
	static int64_t ref_span(const uint8_t *r) { return bam_rec_ref_span(r); }
	// one record: `fixed` = the 32 bytes after block_size (bam1_core_t as in the file), `data` = qname | cigar | seq | qual | aux.
	// The bin is recomputed from pos and the CIGAR's span (1 base without one); every other byte is kept.
	void add(const uint8_t fixed[32], const uint8_t *data, size_t n_data)
	{
		const size_t len = 36 + n_data;
		if (chunk.empty() || chunk.back().capacity() - chunk.back().size() < len) {
			chunk.emplace_back();
			chunk.back().reserve(len > kChunk ? len : kChunk);
		}
		std::vector<uint8_t> &c = chunk.back();
		const uint64_t o = c.size();
		c.resize(o + len);                       // (within the capacity: the records already in the chunk stay where they are)
		uint8_t *r = c.data() + o;
		const uint32_t bs = (uint32_t)(32 + n_data);
		for (int k = 0; k < 4; ++k) r[k] = (uint8_t)(bs >> (8 * k));
		memcpy(r + 4, fixed, 32);
		if (n_data) memcpy(r + 36, data, n_data);
		BaiRecord m;
		bam_rec_derived(r, &m);
		r[14] = (uint8_t)m.bin, r[15] = (uint8_t)(m.bin >> 8);
		if (!bam_key_exact(m.pos)) key_exact = false;
		off.push_back((uint64_t)(chunk.size() - 1) << 32 | o);
		bytes += len;
		key.push_back(bam_sort_key(m.tid, m.pos, m.flag));
	}
	// records back to back as in a BAM stream (what the formatter produces for the main file); false on a malformed one
	bool add_stream(const uint8_t *p, size_t n)
	{
		for (size_t i = 0; i < n; i += 4 + (size_t)bam_u32(p + i)) {
			if (!bam_rec_frame(p + i, n - i) || !bam_rec_cigar_inside(p + i)) return false;
			add(p + i + 4, p + i + 36, bam_u32(p + i) - 32);
		}
		return true;
	}
};

// members of 0xff00 bytes per call of the device compressor (--deflate-device: BgzfWriter's gather buffer and write_sorted_bam's window)
static const size_t kDeflateDeviceBlocks = 1024;

// the order in which write_sorted_bam takes the records.  Returns false (and the reason) only when the device sort fails.
inline bool coordinate_order(const SortRecords &R, int device, std::vector<uint32_t> &ord, bool *on_device, std::string *err)
{
	const size_t n = R.size();
	ord.resize(n);
	*on_device = false;
	if (n > 0 && R.key_exact && n < ((size_t)1 << 32) && psvr_device_count() > 0) {
		if (psvr_sort_order_u64(device, (int64_t)n, R.key.data(), ord.data())) { *err = psvr_last_error(); return false; }
		*on_device = true;
		return true;
	}
	for (size_t i = 0; i < n; ++i) ord[i] = (uint32_t)i;
	std::stable_sort(ord.begin(), ord.end(), [&](uint32_t a, uint32_t b) {
		const uint8_t *x = R.rec(a), *y = R.rec(b);
		const uint32_t xt = bam_u32(x + 4), yt = bam_u32(y + 4);
		if (xt != yt) return xt < yt;
		const int32_t xp = bam_i32(x + 8), yp = bam_i32(y + 8);
		if (xp != yp) return xp < yp;
		return (x[18] & 0x10) < (y[18] & 0x10);
	});
	return true;
}

// name order (`panSVR sort -n`): the names with strcmp, first read before second, ties in input order
inline void name_order(const SortRecords &R, std::vector<uint32_t> &ord)
{
	ord.resize(R.size());
	for (size_t i = 0; i < ord.size(); ++i) ord[i] = (uint32_t)i;
	std::stable_sort(ord.begin(), ord.end(), [&](uint32_t a, uint32_t b) {
		const uint8_t *x = R.rec(a), *y = R.rec(b);
		const int c = strcmp((const char *)x + 36, (const char *)y + 36);
		if (c) return c < 0;
		return (x[18] & 0xc0) < (y[18] & 0xc0);
	});
}

// the header text with the sort order stated, as samtools rewrites it
inline std::string sorted_header_text(const std::string &header_text, bool by_name)
{
	std::string text = header_text;
	while (!text.empty() && text.back() == '\0') text.pop_back();
	const std::string so = by_name ? "queryname" : "coordinate";
	if (text.compare(0, 3, "@HD") == 0) {
		const size_t eol = text.find('\n');
		std::string hd = text.substr(0, eol);
		const size_t p = hd.find("\tSO:");
		if (p != std::string::npos) { size_t e = hd.find('\t', p + 1); hd.erase(p, (e == std::string::npos ? hd.size() : e) - p); }
		hd += "\tSO:" + so;
		text = hd + text.substr(eol == std::string::npos ? text.size() : eol);
	} else text = "@HD\tVN:1.6\tSO:" + so + "\n" + text;
	return text;
}

// The .bai of SAMv1 section 5.2 for a sorted stream of n records behind header_bytes of BAM header, cut into blocks of 0xff00 bytes: cstart =
// the file offset at which every block starts, the EOF block's last (BgzfWriter::block_starts); view(i) = record i in sorted order.  The one
// builder: write_sorted_bam calls it over SortRecords, sort_store_sink.h over psvr_bam_store_meta's table.
template <class View> inline std::vector<uint8_t> build_bai(size_t n_refs, size_t n, uint64_t header_bytes, const std::vector<uint64_t> &cstart, View view)
{
	const size_t nb = cstart.size() - 1, kBlock = kBgzfBlock;
	auto voff = [&](uint64_t u) { const size_t b = (size_t)(u / kBlock); return b < nb ? (cstart[b] << 16) | (u % kBlock) : (cstart[nb] << 16); };   // (the end of the data = the EOF block)
	struct RefIdx { std::map<uint32_t, std::vector<std::pair<uint64_t, uint64_t>>> bins; std::vector<uint64_t> lin; uint64_t beg = ~0ull, end = 0, n_mapped = 0, n_unmapped = 0; };
	std::vector<RefIdx> ri(n_refs);
	uint64_t n_no_coor = 0, u = header_bytes;
	for (size_t i = 0; i < n; ++i) {
		const BaiRecord h = view(i);
		const uint64_t us = u;
		u += h.len;
		const uint32_t tid = (uint32_t)h.tid;
		if (h.tid < 0 || tid >= ri.size()) { ++n_no_coor; continue; }
		const uint64_t vb = voff(us), ve = voff(u);
		RefIdx &X = ri[tid];
		auto &ch = X.bins[h.bin];
		if (!ch.empty() && ch.back().second == vb) ch.back().second = ve;       // adjacent records of a bin share a chunk
		else ch.push_back({vb, ve});
		// reference span from the CIGAR (1 base without one), for the linear index
		const int64_t beg = h.pos < 0 ? 0 : h.pos, end = h.end;
		for (int64_t w = beg >> 14; w <= (end - 1) >> 14; ++w) {
			if ((size_t)w >= X.lin.size()) X.lin.resize((size_t)w + 1, 0);
			if (X.lin[(size_t)w] == 0) X.lin[(size_t)w] = vb;
		}
		if (vb < X.beg) X.beg = vb;
		if (ve > X.end) X.end = ve;
		if (h.flag & 0x4) ++X.n_unmapped; else ++X.n_mapped;
	}
	std::vector<uint8_t> bai = {'B', 'A', 'I', 1};
	auto b32 = [&](uint32_t v) { for (int k = 0; k < 4; ++k) bai.push_back((uint8_t)(v >> (8 * k))); };
	auto b64 = [&](uint64_t v) { for (int k = 0; k < 8; ++k) bai.push_back((uint8_t)(v >> (8 * k))); };
	b32((uint32_t)ri.size());
	for (RefIdx &X : ri) {
		const bool any = !X.bins.empty();
		b32((uint32_t)X.bins.size() + (any ? 1 : 0));
		for (auto &kv : X.bins) { b32(kv.first); b32((uint32_t)kv.second.size()); for (auto &c : kv.second) b64(c.first), b64(c.second); }
		if (any) { b32(37450), b32(2), b64(X.beg), b64(X.end), b64(X.n_mapped), b64(X.n_unmapped); }
		for (size_t w = 1; w < X.lin.size(); ++w) if (X.lin[w] == 0) X.lin[w] = X.lin[w - 1];          // empty windows point at the previous one, as samtools fills them
		b32((uint32_t)X.lin.size());
		for (uint64_t v : X.lin) b64(v);
	}
	b64(n_no_coor);
	return bai;
}
inline bool write_bai(const std::string &out_fn, const std::vector<uint8_t> &bai, std::string *err)
{
	FILE *fi = fopen((out_fn + ".bai").c_str(), "wb");
	if (!fi || fwrite(bai.data(), 1, bai.size(), fi) != bai.size() || fclose(fi) != 0) { *err = "fail to write file '" + out_fn + ".bai'"; return false; }
	return true;
}
// record i of SortRecords as the .bai builder sees it
inline BaiRecord bai_record(const uint8_t *h)
{
	BaiRecord m;
	bam_rec_derived(h, &m);                          // (its bin is the record's own: SortRecords::add has written it)
	return m;
}

// writes out_fn (and out_fn + ".bai" unless by_name); false with the reason in *err
inline bool write_sorted_bam(const std::string &out_fn, const std::string &header_text, const std::vector<std::pair<std::string, int32_t>> &refs,
                             const SortRecords &R, const std::vector<uint32_t> &ord, bool by_name, int threads, std::string *err,
                             BgzfMembersFn dev_fn = nullptr, int device = 0, size_t dev_window_blocks = kDeflateDeviceBlocks)
{
	const std::string text = sorted_header_text(header_text, by_name);
	std::vector<BamRef> brefs;
	for (auto &rf : refs) brefs.push_back({rf.first, (uint32_t)rf.second});
	const std::vector<uint8_t> head = bam_header_block(text, brefs);
	const uint64_t header_bytes = head.size();
	BgzfWriter w(dev_window_blocks);
	if (!w.open(out_fn.c_str(), threads)) { *err = "fail to open file '" + out_fn + "'"; return false; }
	w.log_block_starts();
	if (dev_fn) w.set_device_members(device, dev_fn), w.set_device_min_blocks(1);       // (the tail of the stream goes to the device too)
	w.write(head.data(), head.size());
	for (size_t i = 0; i < ord.size() && w.ok(); ++i) {
		const uint8_t *r = R.rec(ord[i]);
		w.write(r, 4 + bam_u32(r));
	}
	if (!w.close()) { *err = w.compress_failed() ? "compression failed" : "fail to write file '" + out_fn + "'"; return false; }
	if (by_name) return true;
	// ---- .bai: from the stream's blocks of 0xff00 bytes, the header included (their file offsets give the virtual offsets)
	return write_bai(out_fn, build_bai(refs.size(), ord.size(), header_bytes, w.block_starts(), [&](size_t i) { return bai_record(R.rec(ord[i])); }), err);
}

// The sorted file from a device-resident record store, over a backend (cli_main.cpp has the product's, tests/tools/sink_host.h one in host
// memory; every int is 0 or a status whose text last_error() gives):
//   int store_order() / int store_order_names()                coordinate order / name order (by_name)
//   int store_info(int64_t *n_records, int64_t *n_bytes)       waits for the queued appends
//   int store_meta(int64_t first_rank, int64_t n, psvr_bam_rec_meta_t *)
//   int store_stream(int64_t first_rank, int64_t n)            those ranks' records behind the stream's pending bytes
//   int stream_create() / void stream_destroy() / int stream_append(const void *, int64_t), and what MemberTake asks (member_take.h)
// The BAM header with the order stated goes into a fresh BGZF stream; then windows of sorted ranks -- as many as fill take_members members --
// are gathered into the stream, taken (the last window with finish, so the tail becomes the last, shorter member) and written, their starts
// logged; then the EOF block, and unless by_name the .bai from the meta table and the member starts.
struct StoreWritten {
	int status = 0;                                      // 0: written; -1: the backend call `failed` failed (the file, if begun, is closed and partial); 2: the file cannot be written (said on stderr)
	const char *failed = nullptr;
	bool begun = false;                                  // the file was opened
	long long records = 0, members = 0, header_bytes = 0;
	double t_order = 0;                                  // the order's own time
};
template <class Backend> StoreWritten write_sorted_store(Backend &be, const std::string &fn, const std::string &header_text, const std::vector<BamRef> &refs, bool by_name, size_t take_members)
{
	auto now = [] { struct timespec ts; clock_gettime(CLOCK_MONOTONIC, &ts); return ts.tv_sec + 1e-9 * ts.tv_nsec; };
	StoreWritten w;
	auto failed = [&](const char *call) { w.status = -1, w.failed = call; return w; };
	auto cannot = [&](const std::string &why) { fprintf(stderr, "%s\n", why.c_str()); w.status = 2; return w; };
	const double t0 = now();
	if (by_name ? be.store_order_names() : be.store_order()) return failed("order");
	w.t_order = now() - t0;
	int64_t n = 0, nb = 0;
	if (be.store_info(&n, &nb)) return failed("info");
	std::vector<psvr_bam_rec_meta_t> meta((size_t)n);
	if (n && be.store_meta(0, n, meta.data())) return failed("meta");
	FILE *f = fopen(fn.c_str(), "wb");
	if (!f) return cannot("fail to open file '" + fn + "'");
	w.begun = true;
	const std::vector<uint8_t> head = bam_header_block(sorted_header_text(header_text, by_name), refs);
	std::vector<uint64_t> starts;
	MemberTake<Backend> take(be);
	const char *bad = nullptr;
	if (be.stream_create()) bad = "stream create";
	else {
		int64_t pending = 0, used = 0;
		if (be.stream_append(head.data(), (int64_t)head.size())) bad = "stream append";
		else pending = (int64_t)head.size();
		const int64_t want = (int64_t)take_members * (int64_t)kBgzfBlock;
		for (int64_t a = 0; !bad && a < n;) {
			int64_t b = a, bytes = 0;
			while (b < n && pending + bytes < want) bytes += meta[(size_t)b++].len;
			if (be.store_stream(a, b - a)) { bad = "stream from the store"; break; }
			pending += bytes;
			if (!take(f, b == n, pending, &used, &starts)) bad = b == n ? "the last take" : "take";
			pending -= used, a = b;
		}
		if (!bad && n == 0 && !take(f, 1, pending, &used, &starts)) bad = "the last take";
		be.stream_destroy();
	}
	if (bad) { fclose(f); return failed(bad); }
	starts.push_back(take.fpos);
	if (fwrite(kBgzfEof, 1, sizeof kBgzfEof, f) != sizeof kBgzfEof) take.wrote = false;
	if (fclose(f) != 0 || !take.wrote) return cannot("fail to write file '" + fn + "'");
	if (!by_name) {                                      // (a name-sorted file has no index)
		std::string err;
		const std::vector<uint8_t> bai = build_bai(refs.size(), (size_t)n, head.size(), starts, [&](size_t i) {
			const psvr_bam_rec_meta_t &m = meta[i];
			return BaiRecord{m.tid, m.pos, m.end, m.bin, m.flag, m.len};
		});
		if (!write_bai(fn, bai, &err)) return cannot(err);
	}
	w.records = n, w.members = take.members, w.header_bytes = (long long)head.size();
	return w;
}

// A store that the caller has created through the backend and filled itself (`panSVR sort --sort-device`, bam_sort.h, from the file's own members)
// into its sorted file, and the store destroyed.  w->status is the answer; the caller of -1 has its input still, and the one line here says
// that it starts over from it
template <class Backend> int finish_sorted_store(Backend &be, const std::string &fn, const std::string &header_text, const std::vector<BamRef> &refs, bool by_name, size_t take_members, StoreWritten *w)
{
	*w = write_sorted_store(be, fn, header_text, refs, by_name, take_members < 1 ? 1 : take_members);
	if (w->status < 0) fprintf(stderr, "[panSVR-amd] record store on the device failed (%s: %s): the input is read again and sorted by the host's route\n", w->failed, be.last_error());
	be.store_destroy();
	return w->status;
}

} // namespace psvr
