// bam_emit_device_check.cpp -- TEST TOOL.  The host build of pansvr_amd/csrc/bam_emit_device.h (the rules the kernels of bam_emit.hip run,
// compiled with one "lane") against SamEmitter::main_pair's direct BAM branch (sam_emit.h), per pair: state and bytes.
//   bam_emit_device_check run <in.fq> <class> <seed> <flags> <n_header> <anchors.txt | -> <out>
// The FASTQ text is parsed by the host parser (fastq_batch.h).  Results for its pairs are generated from <seed> by the rules of <class>
// (below; each is "plain": no pair may be declined, or "declining": every pair must be).  The anchors' strings come from <anchors.txt>
// (a line per anchor: print string, a tab, vcf id) or, with "-", are made up here: the last anchor's two strings then hold a tab.
// Expected states come from a plain restatement of the rules (expect_state); main_pair is called for every pair that is not expected to
// be declined (a declined pair may hold indices main_pair would follow out of its arrays) and must give the device rules' bytes.
// <out>: int64 {P, n_cands, n_cigar, n_bytes, n_records, n_written, n_declined, n_anchor}, hdr[2 P], pairs[P], cands[], cigar[], state[P],
// pair_off[P + 1], bytes[] -- what tests/test_bam_emit_gpu.py feeds through psvr_bam_emit_results and expects back.
// stdout: "class <name> <plain|declining> pairs <P> state0 <a> state1 <b> state2 <c> records <r> bytes <n>".  Exit status 0 = all agree.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <string>
#include <vector>
#define PSVR_NO_ENGINE_LIB 1
#include "../../pansvr_amd/csrc/sam_emit.h"
#include "../../pansvr_amd/csrc/bam_emit_device.h"

using namespace psvr;

static unsigned long long rng_state = 88172645463325252ull;
static unsigned long long rnd() { rng_state ^= rng_state << 13, rng_state ^= rng_state >> 7, rng_state ^= rng_state << 17; return rng_state; }
static int pick(int n) { return (int)(rnd() % (unsigned)n); }

struct FakeNames : SvNames {
	std::vector<std::string> ps, id;
	const char *print_string(int sv) const override { return sv >= 0 && sv < (int)ps.size() ? ps[(size_t)sv].c_str() : nullptr; }
	const char *vcf_id(int sv) const override { return sv >= 0 && sv < (int)id.size() ? id[(size_t)sv].c_str() : nullptr; }
};

static const long long kInts[] = {-32769, -32768, -129, -128, -1, 0, 255, 256, 65535, 65536};

struct Gen {
	std::vector<psvr_read_hdr_t> hdr;
	std::vector<psvr_pair_result_t> pairs;
	std::vector<psvr_cand_t> cands;
	std::vector<uint32_t> cig;
	int n_header = 0, n_anchor = 0, n_clean = 0;             // anchors [0, n_clean) hold no tab

	void cigar(psvr_cand_t &c, uint32_t n, uint32_t max_op, bool wide)
	{
		c.n_cigar = n, c.cigar_off = (int64_t)cig.size();
		for (uint32_t j = 0; j < n; ++j) {
			const uint32_t len = wide && pick(4) == 0 ? 0x8000u + (uint32_t)pick(0x8000) : 1u + (uint32_t)pick(200);
			cig.push_back(len << 4 | (uint32_t)pick((int)max_op + 1));
		}
	}
	int clean_sv() { return pick(3) == 0 || n_clean == 0 ? -1 : pick(n_clean); }
	psvr_cand_t good_cand()
	{
		psvr_cand_t c;
		memset(&c, 0, sizeof c);
		c.align_score = (uint32_t)pick(600), c.chain_score = (uint32_t)pick(600), c.ref_bg = 1u + (uint32_t)pick(200000000), c.read_bg = (uint32_t)pick(150);
		c.chr_id = pick(n_header), c.sv_id = clean_sv(), c.max_index = (uint32_t)pick(100), c.direction = (uint8_t)pick(2), c.mapq = (uint8_t)pick(61);
		cigar(c, 1u + (uint32_t)pick(9), 8, false);
		return c;
	}
	// a read that is written: primary = one of its candidates
	void good_read(psvr_read_hdr_t &h)
	{
		memset(&h, 0, sizeof h);
		h.n_result = 1 + pick(3), h.cand_off = (int64_t)cands.size();
		for (int i = 0; i < h.n_result; ++i) cands.push_back(good_cand());
		h.primary = pick(h.n_result), h.secondary = pick(2) ? -1 : pick(h.n_result);
		h.unmapped = (uint8_t)pick(2), h.has_mate = pick(2), h.mate_chr_id = pick(n_header), h.mate_ref_bg = 1u + (uint32_t)pick(200000000);
		h.prim_sv_id = clean_sv(), h.mate_sv_id = clean_sv();
	}
	psvr_cand_t &prim(psvr_read_hdr_t &h) { return cands[(size_t)(h.cand_off + h.primary)]; }

	// false: unknown class.  *declining says what the class promises
	bool make(const std::string &cls, long long P, bool *declining)
	{
		hdr.resize((size_t)(2 * P)), pairs.resize((size_t)P);
		static const char *plain[] = {"written", "mixed", "ints", "cigar_ok", "sv_ok", "index_edge"};
		static const char *decl[] = {"cigar_bad", "sv_bad", "index_bad"};
		bool known = false;
		for (const char *c : plain) if (cls == c) known = true, *declining = false;
		for (const char *c : decl) if (cls == c) known = true, *declining = true;
		if (!known) return false;
		for (long long p = 0; p < P; ++p) {
			psvr_pair_result_t &pr = pairs[(size_t)p];
			memset(&pr, 0, sizeof pr);
			pr.gain = 1, pr.cur_isize = pick(2000) - 1000, pr.max_score = pick(700), pr.proper = pick(2), pr.max1 = -1, pr.max2 = -1;
			for (int k = 0; k < 2; ++k) good_read(hdr[(size_t)(2 * p + k)]);
			const int k = pick(2);                               // the read a class works on
			psvr_read_hdr_t &h = hdr[(size_t)(2 * p + k)];
			if (cls == "mixed") {
				if (pick(8) == 0) pr.gain = 0;
				for (int q = 0; q < 2; ++q) {
					psvr_read_hdr_t &g = hdr[(size_t)(2 * p + q)];
					switch (pick(12)) {
					case 0: g.primary = -1; break;
					case 1: case 2: g.primary = -2; break;
					case 3: g.mate_chr_id = pick(3) == 0 ? -1 : pick(2) ? n_header : 1 << 30, g.has_mate = 1; break;
					case 4: g.mate_ref_bg = 0, g.has_mate = 1; break;
					case 5: prim(g).ref_bg = 0; break;
					case 6: prim(g).chr_id = pick(3) == 0 ? -1 : pick(2) ? n_header : (int32_t)0xffffffffu; break;
					case 7: g.has_mate = 7; break;                 // any non-zero value is a mate
					default: break;
					}
				}
			} else if (cls == "ints") {
				for (int q = 0; q < 2; ++q) {
					psvr_read_hdr_t &g = hdr[(size_t)(2 * p + q)];
					g.secondary = pick(g.n_result);
					prim(g).align_score = (uint32_t)kInts[pick(10)], prim(g).chain_score = (uint32_t)kInts[pick(10)];
					psvr_cand_t &sc = cands[(size_t)(g.cand_off + g.secondary)];
					if (&sc != &prim(g)) sc.align_score = (uint32_t)kInts[pick(10)], sc.read_bg = (uint32_t)kInts[pick(10)], sc.chr_id = (int32_t)kInts[pick(10)], sc.ref_bg = (uint32_t)kInts[pick(10)];
					pr.cur_isize = (int32_t)kInts[pick(10)];
				}
			} else if (cls == "cigar_ok") {
				static const uint32_t ns[] = {1, 9, 2, 17};          // (and a few of 65535: each is 256 KB of words)
				cigar(prim(h), p % 97 == 0 ? 65535u : ns[pick(4)], 8, true);
			} else if (cls == "cigar_bad") {
				switch (pick(3)) {
				case 0: prim(h).n_cigar = 0; break;
				case 1: if (p % 61 == 0) { cigar(prim(h), 65536, 8, false); break; }   // (a few: each is 256 KB of words)
				        /* fall through */
				default: cigar(prim(h), 1u + (uint32_t)pick(20), 8, false), cig[(size_t)prim(h).cigar_off + (size_t)pick((int)prim(h).n_cigar)] |= 9u + (uint32_t)pick(7); break;
				}
			} else if (cls == "sv_ok") {
				h.prim_sv_id = pick(2) ? -1 : n_clean - 1, h.mate_sv_id = pick(n_clean), h.has_mate = 1, h.secondary = h.primary, prim(h).sv_id = pick(2) ? -1 : pick(n_clean);
			} else if (cls == "sv_bad") {
				const int32_t bad = pick(3) == 0 ? n_anchor : pick(2) ? -2 - pick(5) : n_clean < n_anchor ? n_clean : n_anchor + 7;
				switch (pick(3)) {
				case 0: h.prim_sv_id = bad; break;
				case 1: h.mate_sv_id = bad, h.has_mate = 1; break;
				default: h.secondary = h.primary, prim(h).sv_id = bad; break;
				}
			} else if (cls == "index_bad") {
				switch (pick(6)) {
				case 0: h.primary = (int32_t)(1 << 28) + pick(100); break;
				case 1: h.cand_off = -1 - pick(5); break;
				case 2: h.secondary = (int32_t)(1 << 28); break;
				case 3: prim(h).cigar_off = -1 - pick(5); break;
				case 4: prim(h).cigar_off = ((int64_t)1 << 40) + pick(9); break;
				default: h.cand_off = ((int64_t)1 << 40); break;
				}
			}
		}
		if (cls == "index_bad" && P > 0) {                       // the very ends of both arrays, left by one
			psvr_read_hdr_t &h = hdr[(size_t)(2 * P - 1)];
			psvr_read_hdr_t *g = P > 1 ? &hdr[(size_t)(2 * P - 3)] : nullptr;
			if (g) good_read(*g), pairs[(size_t)P - 2].gain = 1, hdr[(size_t)(2 * P - 4)].primary = -1;
			good_read(h), pairs[(size_t)P - 1].gain = 1;
			hdr[(size_t)(2 * P - 2)].primary = -1;
			h.primary = h.n_result;                              // cand_off + primary == n_cands
			if (g) cigar(prim(*g), 5, 8, false), prim(*g).n_cigar = 6;   // cigar_off + n_cigar == n_cigar_words + 1
		}
		if (cls == "index_edge" && P > 0) {                      // the last candidate and the last CIGAR word of the arrays: still inside
			psvr_read_hdr_t &h = hdr[(size_t)(2 * P - 1)];
			good_read(h), pairs[(size_t)P - 1].gain = 1;
			h.primary = h.n_result - 1, h.secondary = h.n_result - 1;
			cigar(prim(h), 5, 8, false);
		}
		return true;
	}
};

// ---- the rules restated read by read, in the issue's order, with nothing shared with bam_emit_device.h
struct Expect {
	const FastqBatch &B; const Gen &G; const FakeNames &N; bool not_ori;
	bool tab_ps(int id) const { return N.ps[(size_t)id].find('\t') != std::string::npos; }
	bool tab_id(int id) const { return N.id[(size_t)id].find('\t') != std::string::npos; }
	int read_state(long long p, int k) const
	{
		const psvr_read_hdr_t &h = G.hdr[(size_t)(2 * p + k)];
		const psvr_ori_t &ori = B.ori[2 * p + k];
		const long long nc = (long long)G.cands.size(), nw = (long long)G.cig.size();
		if (h.primary == -1) return 0;
		if (h.primary == -2 && not_ori) return 0;
		const psvr_cand_t *cd = nullptr;
		int chr;
		uint32_t ref_bg;
		if (h.primary == -2) chr = ori.chr_id, ref_bg = ori.ref_bg >= 0x7fffffffu ? 1u : ori.ref_bg;
		else {
			if (h.cand_off < 0 || h.cand_off > nc || h.cand_off + h.primary < 0 || h.cand_off + h.primary >= nc) return 2;
			cd = &G.cands[(size_t)(h.cand_off + h.primary)];
			chr = cd->chr_id, ref_bg = cd->ref_bg;
		}
		if ((uint32_t)chr == 0xffffffffu || chr < 0 || chr >= G.n_header) return 0;
		if ((long long)(int)ref_bg - 1 < 0) return 0;
		const char *t; int nn, cn, sn, qn;
		B.name(2 * p + k, t, nn);
		if (nn <= 0 || nn > 254) return 2;
		B.seq(2 * p + k, t, sn), B.qual(2 * p + k, t, qn);
		if (sn != qn) return 2;
		B.comment(2 * p + k, t, cn);
		for (int i = 0; i < cn; ++i) if (t[i] == '\t' || t[i] == 0) return 2;
		auto id_bad = [&](int id) { return id < -1 || id >= G.n_anchor; };
		if (id_bad(h.prim_sv_id) || (h.prim_sv_id >= 0 && tab_ps(h.prim_sv_id))) return 2;
		if (h.has_mate && (id_bad(h.mate_sv_id) || (h.mate_sv_id >= 0 && tab_ps(h.mate_sv_id)))) return 2;
		if (h.secondary >= 0) {
			if (h.cand_off < 0 || h.cand_off > nc || h.cand_off + h.secondary >= nc) return 2;
			const int id = G.cands[(size_t)(h.cand_off + h.secondary)].sv_id;
			if (id_bad(id) || (id >= 0 && tab_id(id))) return 2;
		}
		if (cd) {
			if (cd->n_cigar == 0 || cd->n_cigar > 0xffff) return 2;
			if (cd->cigar_off < 0 || cd->cigar_off > nw || cd->cigar_off + (long long)cd->n_cigar > nw) return 2;
			for (uint32_t j = 0; j < cd->n_cigar; ++j) if ((G.cig[(size_t)cd->cigar_off + j] & 0xf) > 8) return 2;
		}
		return 1;
	}
	int pair_state(long long p, int *records) const
	{
		*records = 0;
		if (!G.pairs[(size_t)p].gain) return 0;
		const int a = read_state(p, 0), b = read_state(p, 1);
		if (a == 2 || b == 2) return 2;
		*records = (a == 1) + (b == 1);
		return a == 1 || b == 1 ? 1 : 0;
	}
};

template <class T> static void put_raw(FILE *f, const T *p, size_t n) { if (n && fwrite(p, sizeof(T), n, f) != n) { fprintf(stderr, "write failed\n"); exit(2); } }

int main(int argc, char **argv)
{
	if (argc != 9 || strcmp(argv[1], "run")) { fprintf(stderr, "usage: bam_emit_device_check run <in.fq> <class> <seed> <flags> <n_header> <anchors.txt | -> <out>\n"); return 2; }
	const std::string cls = argv[3];
	rng_state ^= strtoull(argv[4], nullptr, 10) * 0x9E3779B97F4A7C15ull;
	for (int i = 0; i < 8; ++i) rnd();
	const int flags = atoi(argv[5]);
	Gen G;
	G.n_header = atoi(argv[6]);
	FakeNames N;
	if (!strcmp(argv[7], "-")) {
		for (int i = 0; i < 37; ++i) {
			N.ps.push_back(std::to_string(i) + "_" + std::to_string(i % 5) + "_" + std::to_string(1000 * i) + "_300_" + (i % 2 ? "INS" : "DEL") + "_sv" + std::to_string(i)), N.id.push_back("sv" + std::to_string(i));
			if (i == 7) N.ps.back() = "", N.id.back() = "";     // (empty strings are strings)
		}
		N.ps.push_back("tab\there"), N.id.push_back("id\ttab");
		G.n_clean = 37;
	} else {
		FILE *f = fopen(argv[7], "r");
		if (!f) { fprintf(stderr, "cannot open %s\n", argv[7]); return 2; }
		char *buf = nullptr;
		size_t cap = 0;
		ssize_t n;
		while ((n = getline(&buf, &cap, f)) > 0) {
			while (n > 0 && buf[n - 1] == '\n') buf[--n] = 0;
			char *t = strchr(buf, '\t');
			if (!t) { fprintf(stderr, "anchors: a line without a tab\n"); return 2; }
			N.ps.emplace_back(buf, t - buf), N.id.emplace_back(t + 1);
		}
		free(buf), fclose(f);
		G.n_clean = (int)N.ps.size();
	}
	G.n_anchor = (int)N.ps.size();

	FastqReader rd;
	FastqBatch B;
	if (!rd.open(argv[2])) { fprintf(stderr, "%s\n", rd.error().c_str()); return 2; }
	const bool any = rd.read(B, 1 << 24, 1ll << 40, 1);
	const long long P = any ? B.n_pairs() : 0;
	bool declining = false;
	if (!G.make(cls, P, &declining)) { fprintf(stderr, "unknown class %s\n", cls.c_str()); return 2; }

	BeTableHost tab;
	tab.build(G.n_anchor, [&](int i) { return N.ps[(size_t)i].c_str(); }, [&](int i) { return N.id[(size_t)i].c_str(); });
	const uint64_t ls0 = 0;
	BeInput in;
	memset(&in, 0, sizeof in);
	in.text = B.text, in.line_start = P ? B.ls.data() : &ls0, in.name_end = B.name_end.data(), in.ori = B.ori, in.first_pair = 0;
	in.hdr = G.hdr.data(), in.pairs = G.pairs.data(), in.cands = G.cands.data(), in.n_cands = (int64_t)G.cands.size(), in.cig = G.cig.data(), in.n_cig = (int64_t)G.cig.size();
	in.not_ori = flags & 1, in.T = tab.view(G.n_header);
	BeHostResult dev;
	be_emit_host(in, P, &dev);

	HeaderInfo H;
	for (int i = 0; i < G.n_header; ++i) H.names.push_back("c" + std::to_string(i)), H.lens.push_back(250000000u);
	EmitStats stats;
	SamEmitter em;
	em.H = &H, em.sv = &N, em.as_bam = true, em.bam_via_text = false, em.not_ori = (flags & 1) != 0, em.stats = &stats;
	ResultView V;
	V.hdr = G.hdr.data(), V.pairs = G.pairs.data(), V.cands = G.cands.data(), V.cig = G.cig.data(), V.pair0 = 0;
	const Expect X{B, G, N, (flags & 1) != 0};
	long long bad = 0, cnt[3] = {0, 0, 0}, records = 0;
	Bytes host;
	for (long long p = 0; p < P; ++p) {
		int nr;
		const int want = X.pair_state(p, &nr), got = dev.state[(size_t)p];
		++cnt[got < 3 ? got : 2];
		const uint8_t *db = dev.bytes.data() + dev.pair_off[(size_t)p];
		const size_t dn = (size_t)(dev.pair_off[(size_t)p + 1] - dev.pair_off[(size_t)p]);
		if (got != want) { if (bad++ < 10) fprintf(stderr, "pair %lld: state %d, expected %d\n", p, got, want); continue; }
		if (want == 1) records += nr;
		if (want == 2) { if (dn) { if (bad++ < 10) fprintf(stderr, "pair %lld: declined with %zu bytes\n", p, dn); } continue; }
		host.clear();
		const long long dropped = stats.dropped;
		em.main_pair(B, V, p, host);
		if (stats.dropped != dropped) { if (bad++ < 10) fprintf(stderr, "pair %lld: the host dropped a record of a pair in state %d\n", p, want); }
		if (host.size() != dn || (dn && memcmp(host.data(), db, dn))) {
			size_t at = 0;
			while (at < dn && at < host.size() && host[at] == db[at]) ++at;
			if (bad++ < 10) fprintf(stderr, "pair %lld (state %d): %zu bytes, the host's %zu, first difference at byte %zu\n", p, want, dn, host.size(), at);
		}
		if ((want == 1) != (dn > 0)) { if (bad++ < 10) fprintf(stderr, "pair %lld: state %d with %zu bytes\n", p, want, dn); }
	}
	if (records != dev.n_records || cnt[1] != dev.n_written || cnt[2] != dev.n_declined) { ++bad; fprintf(stderr, "counts differ: records %lld / %lld\n", records, (long long)dev.n_records); }
	if (declining && (cnt[0] || cnt[1])) { ++bad; fprintf(stderr, "class %s is declining: %lld + %lld pairs were not declined\n", cls.c_str(), cnt[0], cnt[1]); }
	if (!declining && cls != "written" && cnt[2]) { ++bad; fprintf(stderr, "class %s is plain: %lld pairs were declined\n", cls.c_str(), cnt[2]); }

	FILE *f = fopen(argv[8], "wb");
	if (!f) { fprintf(stderr, "cannot write %s\n", argv[8]); return 2; }
	const int64_t head[8] = {P, (int64_t)G.cands.size(), (int64_t)G.cig.size(), dev.pair_off[(size_t)P], dev.n_records, dev.n_written, dev.n_declined, G.n_anchor};
	put_raw(f, head, 8), put_raw(f, G.hdr.data(), G.hdr.size()), put_raw(f, G.pairs.data(), G.pairs.size()), put_raw(f, G.cands.data(), G.cands.size()), put_raw(f, G.cig.data(), G.cig.size());
	put_raw(f, dev.state.data(), dev.state.size()), put_raw(f, dev.pair_off.data(), dev.pair_off.size()), put_raw(f, dev.bytes.data(), dev.bytes.size());
	if (fclose(f)) { fprintf(stderr, "write failed\n"); return 2; }
	printf("class %s %s pairs %lld state0 %lld state1 %lld state2 %lld records %lld bytes %lld\n", cls.c_str(), declining ? "declining" : "plain", P, cnt[0], cnt[1], cnt[2], (long long)dev.n_records,
	       (long long)dev.pair_off[(size_t)P]);
	return bad ? 1 : 0;
}
