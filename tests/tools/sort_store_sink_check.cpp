// sort_store_sink_check.cpp -- the writer of `panSVR aln --sort-device`'s main file (pansvr_amd/csrc/sort_store_sink.h) over a stand-in backend,
// without a GPU: the record store is kept in host memory by the store's rules (the records validated as SortRecords::add_stream validates them,
// the bin recomputed, samtools' key, a stable order), the BGZF stream is a byte vector whose members are made by the encoder's host build
// (dfw_member<1>, as bgzf_stream_sink_check.cpp makes them), the "emitters" are byte arrays with pair offsets, and any one backend call can
// be made to fail.  The yardstick is write_sorted_bam on the same records, its members from the same host build.
// usage: sort_store_sink_check <scenario> <out.bam> <ref.bam> <fail_at> <fail_download>
//   scenario       device | host | alternating | empty: which chunks of the pieces come from an emitter and which from the host
//   out.bam        the file the sink writes (and out.bam.bai)
//   ref.bam        what write_sorted_bam writes for the same records (and ref.bam.bai)
//   fail_at        the k-th backend call (counted from 1) fails; 0: none does
//   fail_download  1: the store's download fails as well
// prints "calls <n> left <0|1> sorter <s> records <n> members <n> device_bytes <n> host_bytes <n> device_chunks <n> host_chunks <n>"; exit status
// 0 when the files were written, otherwise the sink's status (2: it gave up, the message is on stderr), 9 on a mistake of the check's own.
#define PSVR_BGZF_ON_DEVICE 1
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <algorithm>
#include <string>
#include <vector>
#include "../../pansvr_amd/csrc/deflate_wave_device.h"
#include "../../pansvr_amd/csrc/sort_store_sink.h"
using namespace psvr;

// the engine library's symbols that the included headers name (no device here)
extern "C" {
const char *psvr_last_error(void) { return "stand-in"; }
int psvr_device_count(void) { return 0; }
int psvr_sort_order_u64(int, int64_t, const uint64_t *, uint32_t *) { abort(); }
void *psvr_host_alloc(size_t n) { return malloc(n); }
void psvr_host_free(void *p) { free(p); }
int64_t psvr_bgzf_bound(int64_t n) { return n; }
int psvr_bgzf_compress(int, const void *, int64_t, void *, int64_t, int64_t *) { abort(); }
}

// members of 0xff00 bytes from the encoder's host build, in the shape of psvr_bgzf_compress_members
static int host_members(int, const void *in, int64_t n, int32_t member_bytes, void *out, int64_t cap, int64_t *got, int64_t *off, int64_t off_cap, int64_t *nm)
{
	static DfwLds *lds = new DfwLds;
	const size_t mb = (size_t)member_bytes;
	int64_t at = 0, k = 0;
	for (size_t o = 0; o < (size_t)n; o += mb, ++k) {
		const uint32_t m = (uint32_t)((size_t)n - o < mb ? (size_t)n - o : mb);
		std::vector<uint8_t> src((const uint8_t *)in + o, (const uint8_t *)in + o + m);   // the member's input, slot and tokens in blocks of exactly their sizes
		std::vector<uint32_t> slot(dfw_slot_bytes(m) / 4), tok(m + 1);
		memset(lds, 0xa5, sizeof *lds);
		const uint32_t size = dfw_member<1>(src.data(), m, (uint8_t *)slot.data(), tok.data(), lds, 0);
		if (size > dfw_member_max(m) || at + size > cap || (off && k >= off_cap)) { fprintf(stderr, "sort_store_sink_check: a member of %u bytes from %u\n", size, m); exit(9); }
		if (off) off[k] = at;
		memcpy((uint8_t *)out + at, slot.data(), size), at += size;
	}
	if (off) off[k] = at;
	if (nm) *nm = k;
	*got = at;
	return 0;
}

static const int kSlots = 5;
struct FakeEmitter { std::vector<uint8_t> bytes; std::vector<int64_t> off; std::vector<uint8_t> state; };

struct StandIn {
	SortRecords R;                                                     // the store
	std::vector<uint32_t> ord;
	bool created = false, ordered = false, stream_on = false;
	std::vector<uint8_t> pend;                                         // the stream
	FakeEmitter em[kSlots];
	long long calls = 0, fail_at = 0;
	bool fail_download = false;
	std::string err;
	bool failing(const char *what)
	{
		if (++calls != fail_at) return false;
		err = std::string("stand-in failure in ") + what;
		return true;
	}
	const char *last_error() { return err.c_str(); }
	int store_create() { created = true; return 0; }
	void store_destroy() { created = false; }
	int store_append(const void *p, int64_t n)
	{
		if (failing("append")) return 3;
		if (ordered) { err = "ordered"; return 1; }
		// (nothing is appended from a malformed stream: the rules are add_stream's, asked before anything is kept)
		SortRecords probe;
		if (!probe.add_stream((const uint8_t *)p, (size_t)n)) { err = "malformed"; return 1; }
		R.add_stream((const uint8_t *)p, (size_t)n);
		return 0;
	}
	int store_append_emit(int slot, int64_t first, int64_t n)
	{
		if (failing("append_emit")) return 3;
		const FakeEmitter &e = em[slot];
		if (ordered || first < 0 || n < 0 || first + n + 1 > (int64_t)e.off.size()) { err = "pair range outside the run"; return 1; }
		for (int64_t p = first; p < first + n; ++p)
			if (e.state[(size_t)p] == 1 && !R.add_stream(e.bytes.data() + e.off[(size_t)p], (size_t)(e.off[(size_t)p + 1] - e.off[(size_t)p]))) { err = "chain"; return 3; }
		return 0;
	}
	int store_info(int64_t *nr, int64_t *nb)
	{
		if (failing("info")) return 3;
		*nr = (int64_t)R.size(), *nb = (int64_t)R.bytes;
		return 0;
	}
	int store_order()
	{
		if (failing("order")) return 3;
		if (!R.key_exact) { err = "inexact"; return 7; }
		ord.resize(R.size());
		for (size_t i = 0; i < ord.size(); ++i) ord[i] = (uint32_t)i;
		std::stable_sort(ord.begin(), ord.end(), [&](uint32_t a, uint32_t b) { return R.key[a] < R.key[b]; });
		ordered = true;
		return 0;
	}
	int store_meta(int64_t first, int64_t n, psvr_bam_rec_meta_t *m)
	{
		if (failing("meta")) return 3;
		if (!ordered || first < 0 || n < 0 || first + n > (int64_t)R.size()) { err = "ranks"; return 1; }
		for (int64_t r = 0; r < n; ++r) {
			const uint8_t *h = R.rec(ord[(size_t)(first + r)]);
			const int32_t pos = (int32_t)SortRecords::u32(h + 8);
			const int64_t span = SortRecords::ref_span(h);
			psvr_bam_rec_meta_t &x = m[r];
			x.tid = (int32_t)SortRecords::u32(h + 4), x.pos = pos, x.end = (pos < 0 ? 0 : pos) + (span > 0 ? span : 1), x.len = 4 + SortRecords::u32(h), x.index = ord[(size_t)(first + r)];
			x.bin = (uint16_t)(h[14] | h[15] << 8), x.flag = (uint16_t)(h[18] | h[19] << 8), x.pad = 0;
		}
		return 0;
	}
	int store_stream(int64_t first, int64_t n)
	{
		if (failing("stream")) return 3;
		if (!ordered || !stream_on || first < 0 || n < 0 || first + n > (int64_t)R.size()) { err = "ranks"; return 1; }
		for (int64_t r = first; r < first + n; ++r) {
			const uint8_t *h = R.rec(ord[(size_t)r]);
			pend.insert(pend.end(), h, h + 4 + SortRecords::u32(h));
		}
		return 0;
	}
	int store_download(void *bytes, int64_t cap, int64_t *n)
	{
		if (fail_download) { err = "stand-in failure in download"; return 3; }
		*n = (int64_t)R.bytes;
		if (cap < *n) { err = "no room"; return 6; }
		uint8_t *o = (uint8_t *)bytes;
		for (size_t i = 0; i < R.size(); ++i) { const uint8_t *h = R.rec(i); const size_t len = 4 + SortRecords::u32(h); memcpy(o, h, len), o += len; }
		return 0;
	}
	int stream_create()
	{
		if (failing("stream create")) return 3;
		stream_on = true, pend.clear();
		return 0;
	}
	void stream_destroy() { stream_on = false; }
	int stream_append(const void *p, int64_t n)
	{
		if (failing("stream append")) return 3;
		pend.insert(pend.end(), (const uint8_t *)p, (const uint8_t *)p + n);
		return 0;
	}
	int64_t bound(int64_t n) { return n > 0 ? bgzf_members_max(n, kBgzfBlock) : 0; }
	int take(int finish, void *out, int64_t cap, int64_t *got, int64_t *off, int64_t off_cap, int64_t *nm, int64_t *used)
	{
		if (failing(finish ? "the last take" : "take")) return 3;
		*got = *nm = *used = 0;
		if (cap < bound((int64_t)pend.size())) { err = "no room"; return 6; }
		const size_t mb = kBgzfBlock, whole = finish ? pend.size() : pend.size() / mb * mb;
		if (whole) host_members(0, pend.data(), (int64_t)whole, (int32_t)mb, out, cap, got, off, off_cap, nm);
		pend.erase(pend.begin(), pend.begin() + (long)whole);
		*used = (int64_t)whole;
		return 0;
	}
	int emit_view(int slot, int64_t P, const int64_t **off, const uint8_t **state)
	{
		if ((int64_t)em[slot].off.size() != P + 1) { err = "another piece"; return 1; }
		*off = em[slot].off.data(), *state = em[slot].state.data();
		return 0;
	}
	int emit_fetch(int slot, int64_t p0, int64_t p1, std::vector<uint8_t> *out)
	{
		const FakeEmitter &e = em[slot];
		out->assign(e.bytes.begin() + e.off[(size_t)p0], e.bytes.begin() + e.off[(size_t)p1]);
		return 0;
	}
	void *host_alloc(size_t n) { return malloc(n); }
	void host_free(void *p) { free(p); }
};

// one BAM record (block_size first): a name, 0-3 CIGAR operations, l_seq bases and qualities, different for every seed; the bin field is left 0
static void record(std::vector<uint8_t> &v, uint32_t seed)
{
	uint32_t x = seed * 2654435761u + 12345u;
	auto rnd = [&]() { x = x * 1664525u + 1013904223u; return x >> 8; };
	const bool unplaced = rnd() % 23 == 0;
	const uint32_t n_cig = unplaced ? 0 : rnd() % 4, l_seq = 900 + rnd() % 700;
	char name[32];
	const int ln = snprintf(name, sizeof name, "r%07u", seed) + 1;
	std::vector<uint8_t> r(36, 0);
	auto p32 = [&](size_t o, uint32_t val) { for (int k = 0; k < 4; ++k) r[o + k] = (uint8_t)(val >> (8 * k)); };
	p32(4, unplaced ? 0xffffffffu : rnd() % 3), p32(8, unplaced ? 0xffffffffu : rnd() % 8 == 0 ? 777u : rnd() % 3000000);      // (ties on 777)
	r[12] = (uint8_t)ln, r[13] = 60, r[16] = (uint8_t)n_cig, r[18] = (uint8_t)((unplaced ? 4 : 0) | (rnd() & 16)), p32(20, l_seq), p32(24, 0xffffffffu), p32(28, 0xffffffffu);
	r.insert(r.end(), name, name + ln);
	static const uint32_t ops[4] = {0, 1, 2, 4};                                    // M I D S
	for (uint32_t k = 0; k < n_cig; ++k) { const uint32_t c = (1 + rnd() % (k == 0 ? 300000 : 90)) << 4 | ops[k == 0 ? 0 : rnd() % 4]; for (int b = 0; b < 4; ++b) r.push_back((uint8_t)(c >> (8 * b))); }
	for (uint32_t k = 0; k < (l_seq + 1) / 2; ++k) r.push_back((uint8_t)(0x11 << (rnd() & 3)));
	for (uint32_t k = 0; k < l_seq; ++k) r.push_back((uint8_t)(20 + rnd() % 20));
	p32(0, (uint32_t)r.size() - 4);
	v.insert(v.end(), r.begin(), r.end());
}

// `sort_store_sink_check bai <n>`: the .bai builder over a meta-shaped view (the fields restated from the record's bytes, without SortRecords'
// helpers) against the one over SortRecords (bai_record), n generated records in key order, blocks at made-up file offsets
static int bai_mode(size_t n)
{
	SortRecords R;
	std::vector<uint8_t> rec;
	for (size_t i = 0; i < n; ++i) { rec.clear(); record(rec, (uint32_t)i + 1); if (!R.add_stream(rec.data(), rec.size())) return 9; }
	std::vector<uint32_t> ord(n);
	for (size_t i = 0; i < n; ++i) ord[i] = (uint32_t)i;
	std::stable_sort(ord.begin(), ord.end(), [&](uint32_t a, uint32_t b) { return R.key[a] < R.key[b]; });
	std::vector<psvr_bam_rec_meta_t> meta(n);
	for (size_t r = 0; r < n; ++r) {
		const uint8_t *h = R.rec(ord[r]);
		auto u32 = [&](size_t o) { return (uint32_t)h[o] | (uint32_t)h[o + 1] << 8 | (uint32_t)h[o + 2] << 16 | (uint32_t)h[o + 3] << 24; };
		const int32_t pos = (int32_t)u32(8);
		int64_t span = 0;
		for (uint32_t k = 0; k < (uint32_t)(h[16] | h[17] << 8); ++k) { const uint32_t c = u32(36 + h[12] + 4 * k); if ((0x18d >> (c & 15)) & 1) span += c >> 4; }   // M D N = X
		if (span == 0) span = 1;
		const int64_t beg = pos < 0 ? 0 : pos;
		meta[r] = {beg + span, (int32_t)u32(4), pos, 4 + u32(0), ord[r], (uint16_t)bam_reg2bin(beg, beg + span), (uint16_t)(h[18] | h[19] << 8), 0};
	}
	const uint64_t header_bytes = 1234;
	std::vector<uint64_t> cstart;
	for (uint64_t b = 0; b <= (header_bytes + R.bytes + kBgzfBlock - 1) / kBgzfBlock; ++b) cstart.push_back(b * 20011);
	const std::vector<uint8_t> a = build_bai(3, n, header_bytes, cstart, [&](size_t i) { return bai_record(R.rec(ord[i])); });
	const std::vector<uint8_t> b = build_bai(3, n, header_bytes, cstart, [&](size_t i) { const psvr_bam_rec_meta_t &m = meta[i]; return BaiRecord{m.tid, m.pos, m.end, m.bin, m.flag, m.len}; });
	printf("bai %zu bytes from %zu records, %s\n", a.size(), n, a == b ? "equal" : "DIFFERENT");
	return a == b && a.size() > 1000 ? 0 : 1;
}

int main(int argc, char **argv)
{
	if (argc == 3 && !strcmp(argv[1], "bai")) return bai_mode((size_t)atoll(argv[2]));
	if (argc != 6) { fprintf(stderr, "usage: sort_store_sink_check <scenario> <out.bam> <ref.bam> <fail_at> <fail_download>\n"); return 9; }
	const std::string scenario = argv[1];
	if (scenario != "device" && scenario != "host" && scenario != "alternating" && scenario != "empty") { fprintf(stderr, "sort_store_sink_check: unknown scenario %s\n", argv[1]); return 9; }
	const std::string text = "@HD\tVN:1.6\tSO:unsorted\n@SQ\tSN:chr1\tLN:4000000\n@SQ\tSN:chr2\tLN:4000000\n@SQ\tSN:chr3\tLN:4000000\n";
	const std::vector<BamRef> refs = {{"chr1", 4000000}, {"chr2", 4000000}, {"chr3", 4000000}};
	const std::vector<std::pair<std::string, int32_t>> prefs = {{"chr1", 4000000}, {"chr2", 4000000}, {"chr3", 4000000}};
	// the host's sorted writer of the command: the order on the host (no device here), the members from the host build, windows of two
	auto sorted_writer = [&](const std::string &fn, const SortRecords &R) {
		std::vector<uint32_t> ord;
		bool on_device = false;
		std::string err;
		if (!coordinate_order(R, 0, ord, &on_device, &err) || !write_sorted_bam(fn, text, prefs, R, ord, false, 2, &err, &host_members, 0, 2)) { fprintf(stderr, "%s\n", err.c_str()); return 2; }
		return 0;
	};
	StandIn be;
	be.fail_at = atoll(argv[4]), be.fail_download = atoi(argv[5]) != 0;
	SortStoreSink<StandIn> sink(be, [&](const SortRecords &R) { return sorted_writer(argv[2], R); }, 2);   // a take once two members are pending
	sink.open(argv[2], text, refs);
	SortRecords all;                                                   // every record in input order: the yardstick's input
	bool fine = true;

	// five pieces of four chunks of eight pairs; what a chunk is depends on the scenario
	const int n_pieces = 5, n_chunks = 4, chunk_pairs = 8;
	uint32_t seed = 1;
	for (int pi = 0; pi < n_pieces && fine; ++pi) {
		const int slot = pi % kSlots;
		FakeEmitter &e = be.em[slot];
		const int P = pi == 3 ? n_chunks * chunk_pairs - 3 : n_chunks * chunk_pairs;      // (a piece whose last chunk is short)
		std::vector<int> dev((size_t)n_chunks);
		std::vector<std::vector<uint8_t>> host((size_t)n_chunks);
		e.bytes.clear(), e.off.assign(1, 0), e.state.assign((size_t)P, 1);
		for (int ci = 0; ci < n_chunks; ++ci) {
			const int p0 = ci * chunk_pairs, p1 = p0 + chunk_pairs < P ? p0 + chunk_pairs : P;
			const uint32_t id = (uint32_t)(pi * n_chunks + ci);
			const bool empty = scenario == "empty" && (id % 3 != 1 || pi == 2);           // (piece 2: nothing at all)
			dev[(size_t)ci] = scenario == "device" ? 1 : scenario == "host" ? 0 : scenario == "alternating" ? (int)((id ^ (id >> 2)) & 1) : (int)(id % 2);
			for (int p = p0; p < p1; ++p) {
				std::vector<uint8_t> rec;
				const int n_rec = empty ? 0 : (int)((id + (uint32_t)p) % 3);              // 0, 1 or 2 records of a pair
				for (int k = 0; k < n_rec; ++k) record(rec, seed++);
				if (!all.add_stream(rec.data(), rec.size())) return 9;
				if (dev[(size_t)ci]) e.bytes.insert(e.bytes.end(), rec.begin(), rec.end()), e.state[(size_t)p] = rec.empty() ? 0 : 1;
				else host[(size_t)ci].insert(host[(size_t)ci].end(), rec.begin(), rec.end()), e.state[(size_t)p] = 2;
				e.off.push_back((int64_t)e.bytes.size());
			}
		}
		// what the pipeline's writer does with a piece: the view first (the formatter's question), then adjacent device chunks joined into one range
		const int64_t *off = nullptr;
		const uint8_t *state = nullptr;
		if (sink.emit_view(slot, P, &off, &state) || off != e.off.data()) { fprintf(stderr, "sort_store_sink_check: emit_view\n"); return 9; }
		int run0 = -1;
		auto flush = [&](int p1) {
			if (run0 >= 0 && fine) fine = sink.device_chunks(slot, run0, p1, off[p1] - off[run0]);
			run0 = -1;
		};
		for (int ci = 0; ci < n_chunks && fine; ++ci) {
			const int p0 = ci * chunk_pairs;
			if (p0 >= P) break;
			if (dev[(size_t)ci]) { if (run0 < 0) run0 = p0; continue; }
			flush(p0);
			if (fine) fine = sink.host_chunk(host[(size_t)ci].data(), host[(size_t)ci].size());
		}
		flush(P);
		if (fine) fine = sink.piece_done();
	}
	const int rc = fine ? sink.finish() : 2;
	if (sorted_writer(argv[3], all)) return 9;
	const SortSinkStats &st = sink.st;
	printf("calls %lld left %d sorter %s records %lld members %lld device_bytes %lld host_bytes %lld device_chunks %lld host_chunks %lld\n", be.calls, st.left ? 1 : 0, sink.sorter(), st.records,
	       st.members, st.device_bytes, st.host_bytes, st.device_chunks, st.host_chunks);
	return rc;
}
