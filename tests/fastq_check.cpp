// fastq_check.cpp -- TEST-ONLY: the host build of pansvr_amd/csrc/fastq_device.h (the rules the device's FASTQ parser runs, one "lane")
// held to the host parser of fastq_batch.h (FastqReader::read) on the same bytes and limits, every output byte compared.
//   fastq_check parse <text file> <at_end> <max_pairs> <max_bases> <out file>
//       at_end = 0 has no counterpart in FastqReader (a reader always sees its input's end eventually); by the contract an unterminated
//       tail is then no line, so the yardstick is FastqReader on the text cut behind its last '\n'.
//       The out file (what tests/test_fastq_gpu.py compares the device with): int64 n_pairs, used_bytes, total_bases, n_lines, stop, then
//       line_start[8P + 1] u64, name_end[2P] u16, base_off[2P + 1] i64, ori[2P] (20 bytes each), bases[total_bases + 1]
//   fastq_check cut <text file>
//       every byte offset c: [0, c) parsed with at_end = 0, the rest from used_bytes on with at_end = 1; the two concatenated == the whole
//   fastq_check constants        prints the newline pass's tile and the extract pass's group
// Exit status 0 and nothing on stderr: equal.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <string>
#include <vector>
#define PSVR_NO_ENGINE_LIB 1
#include "../pansvr_amd/csrc/fastq_batch.h"
#include "../pansvr_amd/csrc/fastq_device.h"

using namespace psvr;

static std::vector<char> slurp(const char *fn)
{
	std::vector<char> v;
	FILE *f = fopen(fn, "rb");
	if (!f) { fprintf(stderr, "cannot open %s\n", fn); exit(2); }
	char buf[1 << 16];
	size_t k;
	while ((k = fread(buf, 1, sizeof buf, f)) > 0) v.insert(v.end(), buf, buf + k);
	fclose(f);
	return v;
}

static int fail(const char *what, long long i, long long a, long long b)
{
	fprintf(stderr, "MISMATCH %s[%lld]: device rules %lld, fastq_batch.h %lld\n", what, i, a, b);
	return 1;
}

static int parse_main(int argc, char **argv)
{
	if (argc != 7) return 2;
	std::vector<char> text = slurp(argv[2]);
	const int at_end = atoi(argv[3]);
	const long long max_pairs = atoll(argv[4]), max_bases = atoll(argv[5]);
	// a heap copy of exactly n bytes: the sanitizer sees every read behind the window's end
	char *win = (char *)malloc(text.size() ? text.size() : 1);
	if (!text.empty()) memcpy(win, text.data(), text.size());
	FqHostResult D;
	fq_parse_host(win, text.size(), at_end, max_pairs, max_bases, &D);
	free(win);

	// the yardstick
	size_t n_ref = text.size();
	if (!at_end) while (n_ref > 0 && text[n_ref - 1] != '\n') --n_ref;
	std::string tmp = std::string(argv[6]) + ".ref_in";
	FILE *f = fopen(tmp.c_str(), "wb");
	if (!f || (n_ref && fwrite(text.data(), 1, n_ref, f) != n_ref)) { fprintf(stderr, "cannot write %s\n", tmp.c_str()); return 2; }
	fclose(f);
	FastqReader rd;
	if (!rd.open(tmp.c_str())) { fprintf(stderr, "%s\n", rd.error().c_str()); return 2; }
	FastqBatch B;
	const bool got = max_pairs > 0 && rd.read(B, max_pairs, max_bases, 3);
	remove(tmp.c_str());
	const long long P = got ? B.n_pairs() : 0, R = 2 * P;
	if (D.info.n_pairs != P) return fail("n_pairs", 0, D.info.n_pairs, P);
	std::vector<uint64_t> ls = got ? B.ls : std::vector<uint64_t>(1, 0);
	if ((long long)ls.size() != 8 * P + 1) return fail("line index size", 0, 8 * P + 1, (long long)ls.size());
	for (long long i = 0; i <= 8 * P; ++i) if (D.line_start[(size_t)i] != ls[(size_t)i]) return fail("line_start", i, (long long)D.line_start[(size_t)i], (long long)ls[(size_t)i]);
	if (D.info.used_bytes != (long long)ls[(size_t)(8 * P)]) return fail("used_bytes", 0, D.info.used_bytes, (long long)ls[(size_t)(8 * P)]);
	for (long long r = 0; r < R; ++r) if (D.name_end[(size_t)r] != B.name_end[(size_t)r]) return fail("name_end", r, D.name_end[(size_t)r], B.name_end[(size_t)r]);
	for (long long r = 0; r <= R; ++r) { const long long want = got ? B.base_off[r] : 0; if (D.base_off[(size_t)r] != want) return fail("base_off", r, D.base_off[(size_t)r], want); }
	const long long total = got ? B.base_off[R] : 0;
	if (D.info.total_bases != total) return fail("total_bases", 0, D.info.total_bases, total);
	for (long long r = 0; r < R; ++r)
		if (memcmp(&D.ori[(size_t)r], &B.ori[r], sizeof(psvr_ori_t))) {
			const unsigned char *a = (const unsigned char *)&D.ori[(size_t)r], *b = (const unsigned char *)&B.ori[r];
			for (size_t k = 0; k < sizeof(psvr_ori_t); ++k) if (a[k] != b[k]) return fail("ori byte", r * (long long)sizeof(psvr_ori_t) + (long long)k, a[k], b[k]);
		}
	for (long long i = 0; i <= total; ++i) { const char want = got ? B.bases[i] : 0; if (D.bases[(size_t)i] != want) return fail("bases", i, D.bases[(size_t)i], want); }
	// the two fields FastqReader does not report, from their definitions
	long long lines = 0;
	for (size_t i = 0; i < text.size(); ++i) lines += text[i] == '\n';
	if (at_end && !text.empty() && text.back() != '\n') ++lines;
	const long long n_lines = lines / 8 < max_pairs ? lines : 8 * max_pairs;
	if (D.info.n_lines != n_lines) return fail("n_lines", 0, D.info.n_lines, n_lines);
	const int stop = P < n_lines / 8 ? 1 : P == max_pairs ? 0 : total >= max_bases ? 1 : 2;
	if (D.info.stop != stop) return fail("stop", 0, D.info.stop, stop);
	if (D.info.reserved != 0) return fail("reserved", 0, D.info.reserved, 0);

	f = fopen(argv[6], "wb");
	if (!f) { fprintf(stderr, "cannot write %s\n", argv[6]); return 2; }
	const int64_t head[5] = {D.info.n_pairs, D.info.used_bytes, D.info.total_bases, D.info.n_lines, D.info.stop};
	fwrite(head, 8, 5, f);
	fwrite(D.line_start.data(), 8, D.line_start.size(), f);
	if (!D.name_end.empty()) fwrite(D.name_end.data(), 2, D.name_end.size(), f);
	fwrite(D.base_off.data(), 8, D.base_off.size(), f);
	if (!D.ori.empty()) fwrite(D.ori.data(), sizeof(psvr_ori_t), D.ori.size(), f);
	fwrite(D.bases.data(), 1, D.bases.size(), f);
	return fclose(f) == 0 ? 0 : 2;
}

static int cut_main(int argc, char **argv)
{
	if (argc != 3) return 2;
	std::vector<char> text = slurp(argv[2]);
	const size_t n = text.size();
	const long long big = 1 << 20, bases = 1ll << 40;
	FqHostResult W;
	fq_parse_host(text.data(), n, 1, big, bases, &W);
	for (size_t c = 0; c <= n; ++c) {
		char *a = (char *)malloc(c ? c : 1);
		if (c) memcpy(a, text.data(), c);
		FqHostResult A, B;
		fq_parse_host(a, c, 0, big, bases, &A);
		free(a);
		const size_t u = (size_t)A.info.used_bytes, m = n - u;
		char *b = (char *)malloc(m ? m : 1);
		if (m) memcpy(b, text.data() + u, m);
		fq_parse_host(b, m, 1, big, bases, &B);
		free(b);
		const long long P = A.info.n_pairs + B.info.n_pairs;
		if (P != W.info.n_pairs) { fprintf(stderr, "cut at %zu: ", c); return fail("n_pairs", 0, P, W.info.n_pairs); }
		if (u + (size_t)B.info.used_bytes != (size_t)W.info.used_bytes) { fprintf(stderr, "cut at %zu: ", c); return fail("used_bytes", 0, (long long)u + B.info.used_bytes, W.info.used_bytes); }
		std::vector<uint64_t> ls(A.line_start);
		for (size_t i = 1; i < B.line_start.size(); ++i) ls.push_back(B.line_start[i] + u);
		std::vector<int64_t> off(A.base_off);
		for (size_t i = 1; i < B.base_off.size(); ++i) off.push_back(B.base_off[i] + A.info.total_bases);
		std::vector<uint16_t> ne(A.name_end);
		ne.insert(ne.end(), B.name_end.begin(), B.name_end.end());
		std::vector<psvr_ori_t> ori(A.ori);
		ori.insert(ori.end(), B.ori.begin(), B.ori.end());
		std::vector<char> bs(A.bases.begin(), A.bases.end() - 1);
		bs.insert(bs.end(), B.bases.begin(), B.bases.end());
		const bool same = ls == W.line_start && off == W.base_off && ne == W.name_end && bs == W.bases && ori.size() == W.ori.size() &&
		                  (ori.empty() || !memcmp(ori.data(), W.ori.data(), ori.size() * sizeof(psvr_ori_t)));
		if (!same) { fprintf(stderr, "MISMATCH: cut at %zu: the two parts concatenated differ from the whole\n", c); return 1; }
	}
	printf("cuts %zu pairs %lld\n", n + 1, (long long)W.info.n_pairs);
	return 0;
}

int main(int argc, char **argv)
{
	if (argc >= 2 && !strcmp(argv[1], "constants")) { printf("tile_bytes %d piece %d group %d\n", kFqTileBytes, kFqPiece, kFqGroup); return 0; }
	if (argc >= 2 && !strcmp(argv[1], "parse")) return parse_main(argc, argv);
	if (argc >= 2 && !strcmp(argv[1], "cut")) return cut_main(argc, argv);
	fprintf(stderr, "usage: fastq_check parse <text> <at_end> <max_pairs> <max_bases> <out> | cut <text> | constants\n");
	return 2;
}
