// bgzf_stream_sink_check.cpp -- the writer of `panSVR aln --stream-device`'s main file (pansvr_amd/csrc/bgzf_stream_sink.h) over a stand-in
// backend, without a GPU (sink_host.h's StreamHost: the stream is kept in host memory, its members are made by the encoder's host build, the
// "emitters" are byte arrays with pair offsets, and any one backend call can be made to fail).
// usage: bgzf_stream_sink_check <scenario> <out.bam> <payload> <fail_at> <fail_recover>
//   scenario      device | host | alternating | empty | boundary: which chunks of the pieces come from an emitter and which from the host
//   out.bam       the file the sink writes
//   payload       what the file must inflate to: the BAM header and every chunk, in order
//   fail_at       the k-th backend call (append, append from the emitter, pending, take; counted from 1) fails; 0: none does
//   fail_recover  1: recover fails as well
// prints "calls <n> left <0|1> members <n> device_bytes <n> host_bytes <n> device_chunks <n> host_chunks <n>"; exit status 0 when the sink
// wrote the file, 3 when it gave up (the message is on stderr), 2 on a mistake of the check's own (9: of the stand-in's).
#include "sink_host.h"

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
	StreamHost be;
	be.fail_at = atoll(argv[4]), be.fail_recover = atoi(argv[5]) != 0;
	BgzfStreamSink<StreamHost> sink(be, 2);                                 // a take once two members are pending
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
		fine = write_piece(sink, e, slot, P, chunk_pairs, dev, host);
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
