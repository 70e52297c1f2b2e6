// bgzf_stream_sink_check.cpp -- the writer of `panSVR aln --stream-device`'s main file (pansvr_amd/csrc/bgzf_stream_sink.h) over a stand-in
// backend, without a GPU: the stream is kept in host memory, its members are made by the encoder's host build (dfw_member<1>, as
// deflate_wave_check.cpp makes them), the "emitters" are byte arrays with pair offsets, and any one backend call can be made to fail.
// usage: bgzf_stream_sink_check <scenario> <out.bam> <payload> <fail_at> <fail_recover>
//   scenario      device | host | alternating | empty | boundary: which chunks of the pieces come from an emitter and which from the host
//   out.bam       the file the sink writes
//   payload       what the file must inflate to: the BAM header and every chunk, in order
//   fail_at       the k-th backend call (append, append from the emitter, pending, take; counted from 1) fails; 0: none does
//   fail_recover  1: recover fails as well
// prints "calls <n> left <0|1> members <n> device_bytes <n> host_bytes <n> device_chunks <n> host_chunks <n>"; exit status 0 when the sink
// wrote the file, 3 when it gave up (the message is on stderr), 2 on a mistake of the check's own.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <string>
#include <vector>
#include "../../pansvr_amd/csrc/deflate_wave_device.h"
#include "../../pansvr_amd/csrc/bgzf_stream_sink.h"
using namespace psvr;

static const int kSlots = 5;
struct FakeEmitter { std::vector<uint8_t> bytes; std::vector<int64_t> off; std::vector<uint8_t> state; };

struct StandIn {
	std::vector<uint8_t> pend;
	FakeEmitter em[kSlots];
	long long calls = 0, fail_at = 0;
	bool fail_recover = false, created = false;
	std::string err;
	DfwLds *lds = new DfwLds;
	~StandIn() { delete lds; }
	bool failing(const char *what)
	{
		if (++calls != fail_at) return false;
		err = std::string("stand-in failure in ") + what;
		return true;
	}
	const char *last_error() { return err.c_str(); }
	int create() { created = true; return 0; }
	void destroy() { created = false; }
	int append(const void *p, int64_t n)
	{
		if (failing("append")) return 3;
		pend.insert(pend.end(), (const uint8_t *)p, (const uint8_t *)p + n);
		return 0;
	}
	int append_emit(int slot, int64_t first, int64_t n)
	{
		if (failing("append_emit")) return 3;
		const FakeEmitter &e = em[slot];
		if (first < 0 || n < 0 || first + n + 1 > (int64_t)e.off.size()) { err = "pair range outside the run"; return 1; }
		pend.insert(pend.end(), e.bytes.begin() + e.off[(size_t)first], e.bytes.begin() + e.off[(size_t)(first + n)]);
		return 0;
	}
	int64_t pending() { return failing("pending") ? -3 : (int64_t)pend.size(); }
	int64_t bound(int64_t n) { return n > 0 ? bgzf_members_max(n, kBgzfBlock) : 0; }
	int take(int finish, void *out, int64_t cap, int64_t *got, int64_t *nm, int64_t *used)
	{
		if (failing(finish ? "the last take" : "take")) return 3;
		*got = *nm = *used = 0;
		if (cap < bound((int64_t)pend.size())) { err = "no room"; return 6; }
		const size_t mb = kBgzfBlock, whole = finish ? pend.size() : pend.size() / mb * mb;
		for (size_t at = 0; at < whole; at += mb) {
			const uint32_t n = (uint32_t)(whole - at < mb ? whole - at : mb);
			uint8_t *src = new uint8_t[n];                               // the member's input, slot and tokens in blocks of exactly their sizes
			memcpy(src, pend.data() + at, n);
			uint32_t *slot = new uint32_t[dfw_slot_bytes(n) / 4];
			uint32_t *tok = new uint32_t[n + 1];
			memset(lds, 0xa5, sizeof *lds);
			const uint32_t size = dfw_member<1>(src, n, (uint8_t *)slot, tok, lds, 0);
			if (size > dfw_member_max(n) || *got + size > cap) { fprintf(stderr, "bgzf_stream_sink_check: a member of %u bytes from %u\n", size, n); exit(2); }
			memcpy((uint8_t *)out + *got, slot, size), *got += size, ++*nm;
			delete[] tok;
			delete[] slot;
			delete[] src;
		}
		pend.erase(pend.begin(), pend.begin() + (long)whole);
		*used = (int64_t)whole;
		return 0;
	}
	int recover(void *bytes, int64_t cap, int64_t *n)
	{
		if (fail_recover) { err = "stand-in failure in recover"; return 3; }
		*n = (int64_t)pend.size();
		if (cap < *n) { err = "no room"; return 6; }
		if (*n) memcpy(bytes, pend.data(), pend.size());
		pend.clear();
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
	void host_route(BgzfWriter &) {}                                     // (zlib on the sink's threads)
};

// record-like bytes: a few symbols, runs and repeats, different for every seed
static void fill(std::vector<uint8_t> &v, size_t n, uint32_t seed)
{
	uint32_t x = seed * 2654435761u + 12345u;
	auto rnd = [&]() { x = x * 1664525u + 1013904223u; return x >> 8; };
	v.clear();
	while (v.size() < n) {
		if (v.size() > 64 && rnd() % 3 == 0) { const size_t back = 1 + rnd() % 64, len = 4 + rnd() % 40; for (size_t k = 0; k < len; ++k) v.push_back(v[v.size() - back]); }
		else v.push_back((uint8_t)("ACGTN#I\0"[rnd() % 8] + (rnd() % 16 == 0 ? rnd() % 7 : 0)));
	}
	v.resize(n);
}

int main(int argc, char **argv)
{
	if (argc != 6) { fprintf(stderr, "usage: bgzf_stream_sink_check <scenario> <out.bam> <payload> <fail_at> <fail_recover>\n"); return 2; }
	const std::string scenario = argv[1];
	if (scenario != "device" && scenario != "host" && scenario != "alternating" && scenario != "empty" && scenario != "boundary") { fprintf(stderr, "bgzf_stream_sink_check: unknown scenario %s\n", argv[1]); return 2; }
	StandIn be;
	be.fail_at = atoll(argv[4]), be.fail_recover = atoi(argv[5]) != 0;
	BgzfStreamSink<StandIn> sink(be, 2);                                 // a take once two members are pending
	const std::string text = "@HD\tVN:1.6\tSO:unsorted\n@SQ\tSN:chr1\tLN:4000000\n";
	const std::vector<BamRef> refs = {{"chr1", 4000000}};
	std::vector<uint8_t> payload = bam_header_block(text, refs);
	bool fine = sink.open(argv[2], text, refs, 2);
	if (!fine && sink.ok()) { fprintf(stderr, "bgzf_stream_sink_check: cannot open %s\n", argv[2]); return 2; }

	// five pieces of four chunks of eight pairs; what a chunk is depends on the scenario
	const int n_pieces = 5, n_chunks = 4, chunk_pairs = 8;
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
			bool empty = scenario == "empty" && (id % 3 != 1 || pi == 2);               // (piece 2: nothing at all)
			dev[(size_t)ci] = scenario == "device" || scenario == "boundary" ? 1 : scenario == "host" ? 0 : scenario == "alternating" ? (int)((id ^ (id >> 2)) & 1) : (int)(id % 2);
			size_t bytes = empty ? 0 : 9000 + id * 3001 % 30000;
			if (scenario == "boundary" && pi == n_pieces - 1 && ci == n_chunks - 1) {    // the stream ends on a member boundary
				const size_t so_far = payload.size();
				bytes = (kBgzfBlock - so_far % kBgzfBlock) % kBgzfBlock + kBgzfBlock;
			}
			std::vector<uint8_t> rec;
			fill(rec, bytes, id + 1);
			// a device chunk's bytes over its pairs: its second pair carries the first third, its last pair the rest, the others none (state 0); a
			// host chunk's pairs are declined ones (state 2) without bytes in the emitter
			const size_t third = rec.size() / 3;
			const int mid = p1 - p0 > 1 ? p0 + 1 : p0;
			for (int p = p0; p < p1; ++p) {
				const size_t len = dev[(size_t)ci] ? (p == mid ? third : 0) + (p == p1 - 1 ? rec.size() - third : 0) : 0;
				e.off.push_back(e.off.back() + (int64_t)len);
				e.state[(size_t)p] = dev[(size_t)ci] ? (len ? 1 : 0) : 2;
			}
			if (dev[(size_t)ci]) e.bytes.insert(e.bytes.end(), rec.begin(), rec.end());
			else host[(size_t)ci] = rec;
			payload.insert(payload.end(), rec.begin(), rec.end());
		}
		if ((int)e.off.size() != P + 1 || e.off.back() != (int64_t)e.bytes.size()) { fprintf(stderr, "bgzf_stream_sink_check: offsets\n"); return 2; }
		// what the pipeline's writer does with a piece: the view first (the formatter's question), then adjacent device chunks joined into one range
		const int64_t *off = nullptr;
		const uint8_t *state = nullptr;
		if (sink.emit_view(slot, P, &off, &state) || off != e.off.data()) { fprintf(stderr, "bgzf_stream_sink_check: emit_view\n"); return 2; }
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
	const bool closed = sink.close();
	FILE *pf = fopen(argv[3], "wb");
	if (!pf || fwrite(payload.data(), 1, payload.size(), pf) != payload.size() || fclose(pf) != 0) return 2;
	const StreamSinkStats &st = sink.st;
	printf("calls %lld left %d members %lld device_bytes %lld host_bytes %lld device_chunks %lld host_chunks %lld\n", be.calls, st.left ? 1 : 0, st.members, st.device_bytes, st.host_bytes,
	       st.device_chunks, st.host_chunks);
	if (!fine || !closed) return 3;
	return 0;
}
