// bam_ori_device_check.cpp -- TEST TOOL.  The host build of pansvr_amd/csrc/bam_ori_device.h (the rules the ori kernels of bam_emit.hip run,
// compiled with one "lane") against the BAM branch of SamEmitter::ori_pair (sam_emit.h), per pair: state and bytes.
//   bam_ori_device_check run <in.fq> <class> <seed> <min_filter_score> <n_header> <out>
// The FASTQ text is parsed by the host parser (fastq_batch.h).  Results for its pairs are generated from <seed> by the rules of <class>
// (below).  ori_pair is called for every pair the rules do not decline (a declined pair may hold indices ori_pair would follow out of its
// arrays): a pair in state 0 must make it write nothing and report nothing, a pair in state 1 must make it write the rules' bytes and
// report nothing.  A class that is "declining" must have every pair declined, one that is "plain" none -- unless the text declines, which
// the caller knows (tests/bam_ori_cases.py labels each case and says which write every pair and which none).
// <out>: int64 {P, n_cands, n_cigar, n_bytes, n_records, n_written, n_declined, min_filter_score}, hdr[2 P], pairs[P], cands[], cigar[],
// state[P], pair_off[P + 1], bytes[] -- what tests/test_bam_ori_gpu.py feeds through psvr_bam_emit_ori_results and expects back.
// stdout: "class <name> <plain|declining> pairs <P> state0 <a> state1 <b> state2 <c> records <r> bytes <n>".  Exit status 0 = all agree.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <string>
#include <vector>
#define PSVR_NO_ENGINE_LIB 1
#include "../../pansvr_amd/csrc/sam_emit.h"
#include "../../pansvr_amd/csrc/bam_ori_device.h"

using namespace psvr;

static unsigned long long rng_state = 88172645463325252ull;
static unsigned long long rnd() { rng_state ^= rng_state << 13, rng_state ^= rng_state >> 7, rng_state ^= rng_state << 17; return rng_state; }
static int pick(int n) { return (int)(rnd() % (unsigned)n); }

struct Gen {
	std::vector<psvr_read_hdr_t> hdr;
	std::vector<psvr_pair_result_t> pairs;
	std::vector<psvr_cand_t> cands;
	std::vector<uint32_t> cig;
	int n_header = 0, mfs = 0;

	// a CIGAR whose 'I' lengths add up to ins (>= 0) in one or two operators, between other operators
	void cigar(psvr_cand_t &c, int ins)
	{
		c.cigar_off = (int64_t)cig.size();
		cig.push_back((uint32_t)(1 + pick(100)) << 4 | 0u);
		if (ins > 0) {
			const int a = pick(2) ? ins : pick(ins + 1);
			if (a) cig.push_back((uint32_t)a << 4 | 1u);
			cig.push_back((uint32_t)(1 + pick(50)) << 4 | (uint32_t)(pick(2) ? 0 : 2));
			if (ins - a) cig.push_back((uint32_t)(ins - a) << 4 | 1u);
		}
		if (pick(2)) cig.push_back((uint32_t)(1 + pick(30)) << 4 | 4u);
		c.n_cigar = (uint32_t)(cig.size() - (size_t)c.cigar_off);
	}
	void read(psvr_read_hdr_t &h, int ins)
	{
		memset(&h, 0, sizeof h);
		h.n_result = 1 + pick(3), h.cand_off = (int64_t)cands.size();
		for (int i = 0; i < h.n_result; ++i) {
			psvr_cand_t c;
			memset(&c, 0, sizeof c);
			c.align_score = (uint32_t)pick(600), c.ref_bg = 1u + (uint32_t)pick(200000000), c.chr_id = pick(n_header), c.sv_id = -1, c.direction = (uint8_t)pick(2), c.mapq = (uint8_t)pick(61);
			cigar(c, ins < 0 ? pick(40) : ins);
			cands.push_back(c);
		}
		h.primary = pick(h.n_result), h.secondary = -1, h.prim_sv_id = h.mate_sv_id = -1;
	}
	psvr_cand_t &at(long long p, int k, int mx) { return cands[(size_t)(hdr[(size_t)(2 * p + k)].cand_off + mx)]; }

	// false: unknown class.  *declining: every pair must be declined; *want: the state every pair has whatever the text holds, -1: the text
	// decides (on a text whose pairs all pass the gate and parse, i24 writes nothing and m1 / i25 / ncig0 / index_edge write every pair)
	bool make(const std::string &cls, long long P, bool *declining, int *want)
	{
		hdr.resize((size_t)(2 * P)), pairs.resize((size_t)P);
		static const char *names[] = {"kept", "mixed", "gate", "m1", "m2", "i24", "i25", "ncig0", "index_edge", "index_bad"};
		static const int wants[] = {-1, -1, 0, -1, -1, -1, -1, -1, -1, -1};
		int id = -1;
		for (int i = 0; i < 10; ++i) if (cls == names[i]) id = i;
		if (id < 0) return false;
		*declining = cls == "index_bad", *want = wants[id];
		const int ins = cls == "i24" || cls == "i25" || cls == "index_edge" ? 24 : cls == "m1" || cls == "ncig0" || cls == "index_bad" ? 3 : -1;
		for (long long p = 0; p < P; ++p) {
			psvr_pair_result_t &pr = pairs[(size_t)p];
			memset(&pr, 0, sizeof pr);
			static const int scores[] = {-32769, -32768, -129, -128, -1, 0, 255, 256, 65535, 65536};
			pr.gain = pick(2), pr.cur_isize = pick(2000) - 1000, pr.proper = 0, pr.max1 = -1, pr.max2 = -1;
			pr.max_score = pick(4) ? pick(mfs + 1) : scores[pick(10)];
			if (pr.max_score > mfs) pr.max_score = mfs;
			for (int k = 0; k < 2; ++k) read(hdr[(size_t)(2 * p + k)], ins);
			const int n1 = hdr[(size_t)(2 * p)].n_result, n2 = hdr[(size_t)(2 * p + 1)].n_result;
			if (cls == "kept") continue;
			if (cls == "gate") { pr.max_score = mfs + 1 + pick(1000), pr.proper = pick(2); continue; }
			pr.proper = 1, pr.max1 = pick(n1), pr.max2 = pick(n2);   // (with ins < 25: both reads leave the pair proper)
			const int k = pick(2);                               // the read a class works on
			psvr_read_hdr_t &h = hdr[(size_t)(2 * p + k)];
			int32_t &mx = k ? pr.max2 : pr.max1;
			if (cls == "mixed") {
				if (pick(4) == 0) pr.max_score = mfs + 1 + pick(100);
				pr.proper = pick(3) ? pick(2) : 7;                   // any non-zero value is proper
				const int a = pick(4), b = pick(4);
				if (a < 2) pr.max1 = -1 - a;
				if (b < 2) pr.max2 = -1 - b;
			} else if (cls == "m1") mx = -1;
			else if (cls == "m2") pr.max1 = pr.max2 = -2;
			else if (cls == "i25") cigar(at(p, k, mx), 25 + pick(3));
			else if (cls == "ncig0") at(p, k, mx).n_cigar = 0;
			else if (cls == "index_bad") {
				switch (pick(6)) {
				case 0: mx = (int32_t)(1 << 28) + pick(100); break;
				case 1: h.cand_off = -1 - pick(5); break;
				case 2: mx = -3 - pick(1000), h.cand_off = 0; break;   // cand_off + max < 0
				case 3: at(p, k, mx).cigar_off = -1 - pick(5); break;
				case 4: at(p, k, mx).cigar_off = ((int64_t)1 << 40) + pick(9); break;
				default: h.cand_off = ((int64_t)1 << 40); break;
				}
			}
		}
		if (cls == "index_bad" && P > 1) {                       // the very ends of both arrays, left by one
			for (int r = 4; r >= 1; --r) read(hdr[(size_t)(2 * P - r)], 3);
			psvr_pair_result_t &a = pairs[(size_t)P - 1], &b = pairs[(size_t)P - 2];
			a.max1 = b.max1 = b.max2 = 0;
			a.max2 = hdr[(size_t)(2 * P - 1)].n_result;          // cand_off + max2 == n_cands
			cigar(at(P - 2, 1, 0), 3), at(P - 2, 1, 0).n_cigar += 1;   // cigar_off + n_cigar == n_cigar_words + 1
		}
		if (cls == "index_edge" && P > 0) {                      // the last candidate and the last CIGAR words of the arrays: still inside
			read(hdr[(size_t)(2 * P - 1)], 24);
			psvr_pair_result_t &a = pairs[(size_t)P - 1];
			a.max2 = hdr[(size_t)(2 * P - 1)].n_result - 1;
			cigar(at(P - 1, 1, a.max2), 25);
		}
		return true;
	}
};

template <class T> static void put_raw(FILE *f, const T *p, size_t n) { if (n && fwrite(p, sizeof(T), n, f) != n) { fprintf(stderr, "write failed\n"); exit(2); } }

int main(int argc, char **argv)
{
	if (argc != 8 || strcmp(argv[1], "run")) { fprintf(stderr, "usage: bam_ori_device_check run <in.fq> <class> <seed> <min_filter_score> <n_header> <out>\n"); return 2; }
	const std::string cls = argv[3];
	rng_state ^= strtoull(argv[4], nullptr, 10) * 0x9E3779B97F4A7C15ull;
	for (int i = 0; i < 8; ++i) rnd();
	Gen G;
	G.mfs = atoi(argv[5]), G.n_header = atoi(argv[6]);

	FastqReader rd;
	FastqBatch B;
	if (!rd.open(argv[2])) { fprintf(stderr, "%s\n", rd.error().c_str()); return 2; }
	const bool any = rd.read(B, 1 << 24, 1ll << 40, 1);
	const long long P = any ? B.n_pairs() : 0;
	bool declining = false;
	int want_all = -1;
	if (!G.make(cls, P, &declining, &want_all)) { fprintf(stderr, "unknown class %s\n", cls.c_str()); return 2; }

	const uint64_t ls0 = 0;
	BoInput in;
	memset(&in, 0, sizeof in);
	in.text = B.text, in.line_start = P ? B.ls.data() : &ls0, in.name_end = B.name_end.data(), in.ori = B.ori, in.first_pair = 0;
	in.hdr = G.hdr.data(), in.pairs = G.pairs.data(), in.cands = G.cands.data(), in.n_cands = (int64_t)G.cands.size(), in.cig = G.cig.data(), in.n_cig = (int64_t)G.cig.size();
	in.min_filter_score = G.mfs, in.n_header = G.n_header;
	BeHostResult dev;
	bo_emit_host(in, P, &dev);

	HeaderInfo H;
	for (int i = 0; i < G.n_header; ++i) H.names.push_back("c" + std::to_string(i)), H.lens.push_back(250000000u);
	EmitStats stats;
	SamEmitter em;
	em.H = &H, em.as_bam = true, em.min_filter_score = G.mfs, em.stats = &stats;
	ResultView V;
	V.hdr = G.hdr.data(), V.pairs = G.pairs.data(), V.cands = G.cands.data(), V.cig = G.cig.data(), V.pair0 = 0;
	long long bad = 0, cnt[3] = {0, 0, 0}, records = 0;
	Bytes host;
	for (long long p = 0; p < P; ++p) {
		const int got = dev.state[(size_t)p];
		++cnt[got < 3 ? got : 2];
		const uint8_t *db = dev.bytes.data() + dev.pair_off[(size_t)p];
		const size_t dn = (size_t)(dev.pair_off[(size_t)p + 1] - dev.pair_off[(size_t)p]);
		if (want_all >= 0 && got != want_all) { if (bad++ < 10) fprintf(stderr, "pair %lld: state %d, class %s expects %d\n", p, got, cls.c_str(), want_all); continue; }
		if (got == 2) { if (dn) { if (bad++ < 10) fprintf(stderr, "pair %lld: declined with %zu bytes\n", p, dn); } continue; }
		if (got > 2 || (got == 1) != (dn > 0)) { if (bad++ < 10) fprintf(stderr, "pair %lld: state %d with %zu bytes\n", p, got, dn); continue; }
		host.clear();
		const long long dropped = stats.dropped;
		em.ori_pair(B, V, p, host);
		if (stats.dropped != dropped) { if (bad++ < 10) fprintf(stderr, "pair %lld: the host reported a record of a pair in state %d\n", p, got); }
		if (host.size() != dn || (dn && memcmp(host.data(), db, dn))) {
			size_t at = 0;
			while (at < dn && at < host.size() && host[at] == db[at]) ++at;
			if (bad++ < 10) fprintf(stderr, "pair %lld (state %d): %zu bytes, the host's %zu, first difference at byte %zu\n", p, got, dn, host.size(), at);
		}
		for (size_t at = 0; at + 4 <= dn; ++records) at += 4 + ((size_t)db[at] | (size_t)db[at + 1] << 8 | (size_t)db[at + 2] << 16 | (size_t)db[at + 3] << 24);
	}
	if (records != dev.n_records || cnt[1] != dev.n_written || cnt[2] != dev.n_declined) { ++bad; fprintf(stderr, "counts differ: records %lld / %lld\n", records, (long long)dev.n_records); }
	if (declining && (cnt[0] || cnt[1])) { ++bad; fprintf(stderr, "class %s is declining: %lld + %lld pairs were not declined\n", cls.c_str(), cnt[0], cnt[1]); }

	FILE *f = fopen(argv[7], "wb");
	if (!f) { fprintf(stderr, "cannot write %s\n", argv[7]); return 2; }
	const int64_t head[8] = {P, (int64_t)G.cands.size(), (int64_t)G.cig.size(), dev.pair_off[(size_t)P], dev.n_records, dev.n_written, dev.n_declined, G.mfs};
	put_raw(f, head, 8), put_raw(f, G.hdr.data(), G.hdr.size()), put_raw(f, G.pairs.data(), G.pairs.size()), put_raw(f, G.cands.data(), G.cands.size()), put_raw(f, G.cig.data(), G.cig.size());
	put_raw(f, dev.state.data(), dev.state.size()), put_raw(f, dev.pair_off.data(), dev.pair_off.size()), put_raw(f, dev.bytes.data(), dev.bytes.size());
	if (fclose(f)) { fprintf(stderr, "write failed\n"); return 2; }
	printf("class %s %s pairs %lld state0 %lld state1 %lld state2 %lld records %lld bytes %lld\n", cls.c_str(), declining ? "declining" : "plain", P, cnt[0], cnt[1], cnt[2], (long long)dev.n_records,
	       (long long)dev.pair_off[(size_t)P]);
	return bad ? 1 : 0;
}
