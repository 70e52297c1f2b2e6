// sort_store_sink_check.cpp -- the writer of `panSVR aln --sort-device`'s main file (pansvr_amd/csrc/sort_store_sink.h) over a stand-in backend,
// without a GPU (sink_host.h's StoreHost: the record store and the BGZF stream are kept in host memory by the device's rules, the "emitters" are
// byte arrays with pair offsets, and any one backend call can be made to fail).  The yardstick is write_sorted_bam on the same records, its
// members from the same host build.
// usage: sort_store_sink_check <scenario> <out.bam> <ref.bam> <fail_at> <fail_download>
//   scenario       device | host | alternating | empty: which chunks of the pieces come from an emitter and which from the host
//   out.bam        the file the sink writes (and out.bam.bai)
//   ref.bam        what write_sorted_bam writes for the same records (and ref.bam.bai)
//   fail_at        the k-th backend call (counted from 1) fails; 0: none does
//   fail_download  1: the store's download fails as well
// prints "calls <n> left <0|1> sorter <s> records <n> members <n> device_bytes <n> host_bytes <n> device_chunks <n> host_chunks <n>"; exit status
// 0 when the files were written, otherwise the sink's status (2: it gave up, the message is on stderr), 9 on a mistake of the check's own.
#include "sink_host.h"

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
	StoreHost be;
	be.fail_at = atoll(argv[4]), be.fail_download = atoi(argv[5]) != 0;
	SortStoreSink<StoreHost> sink(be, [&](const SortRecords &R) { return sorted_writer(argv[2], R); }, 2);   // a take once two members are pending
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
		fine = write_piece(sink, e, slot, P, chunk_pairs, dev, host);
	}
	const int rc = fine ? sink.finish() : 2;
	if (sorted_writer(argv[3], all)) return 9;
	const SortSinkStats &st = sink.st;
	printf("calls %lld left %d sorter %s records %lld members %lld device_bytes %lld host_bytes %lld device_chunks %lld host_chunks %lld\n", be.calls, st.left ? 1 : 0, sink.sorter(), st.records,
	       st.members, st.device_bytes, st.host_bytes, st.device_chunks, st.host_chunks);
	return rc;
}
