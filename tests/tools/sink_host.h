// sink_host.h -- the main file's device sinks without a GPU: what bgzf_stream_sink_check.cpp, sort_store_sink_check.cpp and nsort_sink_check.cpp
// share.  The BGZF stream is a byte vector whose members are made by the encoder's host build (dfw_member<1>, as deflate_wave_check.cpp makes
// them); the record store is a SortRecords in host memory by the store's rules (the records validated as SortRecords::add_stream validates
// them, the bin recomputed, samtools' key and a stable order, or name_order); the "emitters" are byte arrays with pair offsets; and one
// backend call can be made to fail: the k-th counted call, or the first call of a named kind.
//   StreamHost   bgzf_stream_sink.h's backend
//   StoreHost    sort_store_sink.h's and sorted_bam.h's store writer's
#pragma once
#define PSVR_BGZF_ON_DEVICE 1
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <algorithm>
#include <string>
#include <vector>
#include "../../pansvr_amd/csrc/deflate_wave_device.h"
#include "../../pansvr_amd/csrc/bgzf_stream_sink.h"
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
inline int host_members(int, const void *in, int64_t n, int32_t member_bytes, void *out, int64_t cap, int64_t *got, int64_t *off, int64_t off_cap, int64_t *nm)
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
		if (size > dfw_member_max(m) || at + size > cap || (off && k >= off_cap)) { fprintf(stderr, "sink_host: a member of %u bytes from %u\n", size, m); exit(9); }
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

// what both backends are made of: the fault injector, the stream's pending bytes and its take, the emitters
struct SinkHost {
	long long calls = 0, fail_at = 0;                                  // the fail_at-th counted call fails (0: none does) ...
	std::string fail_kind, err;                                        // ... or the first call of this kind
	std::vector<uint8_t> pend;                                         // the stream
	FakeEmitter em[kSlots];
	bool failing(const char *what)
	{
		if (++calls != fail_at && fail_kind != what) return false;
		fail_kind = "spent", err = std::string("stand-in failure in ") + what;
		return true;
	}
	const char *last_error() { return err.c_str(); }
	int add(const void *p, int64_t n) { pend.insert(pend.end(), (const uint8_t *)p, (const uint8_t *)p + n); return 0; }
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

// counted: append, append from the emitter, pending, take
struct StreamHost : SinkHost {
	bool fail_recover = false, created = false;
	int stream_create() { created = true; return 0; }
	void stream_destroy() { created = false; }
	int stream_append(const void *p, int64_t n) { return failing("append") ? 3 : add(p, n); }
	int stream_append_emit(int slot, int64_t first, int64_t n)
	{
		if (failing("append_emit")) return 3;
		const FakeEmitter &e = em[slot];
		if (first < 0 || n < 0 || first + n + 1 > (int64_t)e.off.size()) { err = "pair range outside the run"; return 1; }
		return add(e.bytes.data() + e.off[(size_t)first], e.off[(size_t)(first + n)] - e.off[(size_t)first]);
	}
	int64_t stream_pending() { return failing("pending") ? -3 : (int64_t)pend.size(); }
	int stream_recover(void *bytes, int64_t cap, int64_t *n)
	{
		if (fail_recover) { err = "stand-in failure in recover"; return 3; }
		*n = (int64_t)pend.size();
		if (cap < *n) { err = "no room"; return 6; }
		if (*n) memcpy(bytes, pend.data(), pend.size());
		pend.clear();
		return 0;
	}
	void host_route(BgzfWriter &) {}                                     // (zlib on the sink's threads)
};

// counted: append, append from the emitter, info, order, meta, stream from the store, stream create, stream append, take
struct StoreHost : SinkHost {
	SortRecords R;                                                     // the store
	std::vector<uint32_t> ord;
	int ordered = 0;                                                   // 1: by coordinate, 2: by name
	bool created = false, destroyed = false, stream_on = false, fail_download = false;
	int store_create() { created = true; return 0; }
	void store_destroy() { created = false, destroyed = true; }
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
		ordered = 1;
		return 0;
	}
	int store_order_names()
	{
		if (failing("order")) return 3;
		name_order(R, ord);
		ordered = 2;
		return 0;
	}
	bool ranks(int64_t first, int64_t n)
	{
		if (ordered && first >= 0 && n >= 0 && first + n <= (int64_t)R.size()) return true;
		err = "ranks";
		return false;
	}
	int store_meta(int64_t first, int64_t n, psvr_bam_rec_meta_t *m)
	{
		if (failing("meta")) return 3;
		if (!ranks(first, n)) return 1;
		for (int64_t r = 0; r < n; ++r) {
			bam_rec_derived(R.rec(ord[(size_t)(first + r)]), &m[r]);
			m[r].index = ord[(size_t)(first + r)], m[r].pad = 0;
		}
		return 0;
	}
	int store_stream(int64_t first, int64_t n)
	{
		if (failing("stream")) return 3;
		if (!stream_on || !ranks(first, n)) { err = "ranks"; return 1; }
		for (int64_t r = first; r < first + n; ++r) {
			const uint8_t *h = R.rec(ord[(size_t)r]);
			add(h, 4 + (int64_t)bam_u32(h));
		}
		return 0;
	}
	int store_download(void *bytes, int64_t cap, int64_t *n)
	{
		if (fail_download) { err = "stand-in failure in download"; return 3; }
		*n = (int64_t)R.bytes;
		if (cap < *n) { err = "no room"; return 6; }
		uint8_t *o = (uint8_t *)bytes;
		for (size_t i = 0; i < R.size(); ++i) { const uint8_t *h = R.rec(i); const size_t len = 4 + bam_u32(h); memcpy(o, h, len), o += len; }
		return 0;
	}
	int stream_create()
	{
		if (failing("stream create")) return 3;
		stream_on = true, pend.clear();
		return 0;
	}
	void stream_destroy() { stream_on = false; }
	int stream_append(const void *p, int64_t n) { return failing("stream append") ? 3 : add(p, n); }
};

// what the pipeline's writer does with a piece of P pairs in chunks of chunk_pairs (dev[c]: chunk c lies in the slot's emitter; host[c]: its bytes
// otherwise): the view first (the formatter's question), then adjacent device chunks joined into one range.  false: the sink gave up
template <class Sink> bool write_piece(Sink &sink, const FakeEmitter &e, int slot, int P, int chunk_pairs, const std::vector<int> &dev, const std::vector<std::vector<uint8_t>> &host)
{
	const int64_t *off = nullptr;
	const uint8_t *state = nullptr;
	if (sink.emit_view(slot, P, &off, &state) || off != e.off.data()) { fprintf(stderr, "sink_host: emit_view\n"); exit(9); }
	bool fine = true;
	int run0 = -1;
	auto flush = [&](int p1) {
		if (run0 >= 0 && fine) fine = sink.device_chunks(slot, run0, p1, off[p1] - off[run0]);
		run0 = -1;
	};
	for (size_t ci = 0; ci < dev.size() && fine; ++ci) {
		const int p0 = (int)ci * chunk_pairs;
		if (p0 >= P) break;
		if (dev[ci]) { if (run0 < 0) run0 = p0; continue; }
		flush(p0);
		if (fine) fine = sink.host_chunk(host[ci].data(), host[ci].size());
	}
	flush(P);
	return fine && sink.piece_done();
}
