// name_key_check.cpp -- pansvr_amd/csrc/name_key.h on the host, a stand-alone program (tests/test_name_key.py builds it plain and with
// -fsanitize=address,undefined): the name order as the device computes it -- the tie key, then the 8-byte chunks from the last to the first, a
// stable sort each over the order of the pass before -- against name_order() of sorted_bam.h over the same records, and name_chunk_words (the
// chunk from two aligned words, as k_name_chunk loads them) against name_chunk for every address residue.
// usage: name_key_check <in> <out>
//   in    u32 cases; per case u32 bytes, then BAM records back to back (block_size first)
//   out   per case one line: the case's number, the number of chunks, then the order
// Every record is looked at in a heap block of exactly its own size, so a read behind a record's last byte is the sanitizer's to report.
// Exit status 0; 1 with a line on stderr when the two orders or the two chunk functions disagree; 9 on a mistake of the input.
#define PSVR_BGZF_ON_DEVICE 1
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <algorithm>
#include <vector>
#include "../../pansvr_amd/csrc/name_key.h"
#include "../../pansvr_amd/csrc/sorted_bam.h"
using namespace psvr;

// the engine library's symbols that sorted_bam.h names (no device here)
extern "C" {
const char *psvr_last_error(void) { return "stand-in"; }
int psvr_device_count(void) { return 0; }
int psvr_sort_order_u64(int, int64_t, const uint64_t *, uint32_t *) { abort(); }
void *psvr_host_alloc(size_t n) { return malloc(n); }
void psvr_host_free(void *p) { free(p); }
int64_t psvr_bgzf_bound(int64_t n) { return n; }
int psvr_bgzf_compress(int, const void *, int64_t, void *, int64_t, int64_t *) { abort(); }
}

// the two aligned words around name bytes [at, at + nbytes) of a record of rec_len bytes, as if the name began at an address of residue r0:
// bytes of the record where the words cover it (the CIGAR behind the name among them), 0xee where they leave it
static uint64_t chunk_by_words(const uint8_t *rec, size_t rec_len, uint32_t len, uint32_t c, uint32_t r0)
{
	const uint32_t at = 8 * c;
	if (at >= len) return 0;
	const uint32_t nbytes = len - at < 8 ? len - at : 8, r = (r0 + at) & 7;
	const long first = 36 + (long)at - (long)r;                  // the record offset of w0's first byte
	uint64_t w[2] = {0, 0};
	for (int k = 0; k < 16; ++k) {
		const long o = first + k;
		const uint8_t b = o >= 0 && (size_t)o < rec_len ? rec[o] : 0xee;
		w[k / 8] |= (uint64_t)b << (8 * (k % 8));
	}
	return name_chunk_words(w[0], r + nbytes > 8 ? w[1] : 0xeeeeeeeeeeeeeeeeull, r, nbytes);
}

int main(int argc, char **argv)
{
	if (argc != 3) { fprintf(stderr, "usage: name_key_check <in> <out>\n"); return 9; }
	FILE *f = fopen(argv[1], "rb"), *out = fopen(argv[2], "w");
	if (!f || !out) return 9;
	uint32_t n_cases = 0;
	if (fread(&n_cases, 4, 1, f) != 1) return 9;
	for (uint32_t ci = 0; ci < n_cases; ++ci) {
		uint32_t n_bytes = 0;
		if (fread(&n_bytes, 4, 1, f) != 1) return 9;
		std::vector<uint8_t> buf(n_bytes);
		if (n_bytes && fread(buf.data(), 1, n_bytes, f) != n_bytes) return 9;
		SortRecords R;
		if (!R.add_stream(buf.data(), buf.size())) { fprintf(stderr, "name_key_check: case %u is no record stream\n", ci); return 9; }
		const size_t n = R.size();
		std::vector<uint8_t *> rec(n);
		std::vector<size_t> rlen(n);
		std::vector<uint32_t> len(n);
		uint32_t longest = 0;
		for (size_t i = 0, at = 0; i < n; ++i) {
			rlen[i] = 4 + (size_t)bam_u32(buf.data() + at);
			rec[i] = (uint8_t *)malloc(rlen[i]);
			memcpy(rec[i], buf.data() + at, rlen[i]), at += rlen[i];
			len[i] = name_len_rec(rec[i]);
			if (len[i] > longest) longest = len[i];
		}
		const uint32_t C = (longest + 7) / 8;
		if (C > kNameMaxChunks) { fprintf(stderr, "name_key_check: case %u: %u chunks\n", ci, C); return 1; }
		// the chunk from aligned words is the chunk from bytes, wherever the name begins; behind the name's end it is 0
		for (size_t i = 0; i < n; ++i)
			for (uint32_t c = 0; c <= C; ++c) {
				const uint64_t want = name_chunk(rec[i] + 36, len[i], c);
				if (8 * c >= len[i] && want != 0) { fprintf(stderr, "name_key_check: case %u record %zu chunk %u: %016llx behind the name\n", ci, i, c, (unsigned long long)want); return 1; }
				for (uint32_t r0 = 0; r0 < 8; ++r0) {
					const uint64_t got = chunk_by_words(rec[i], rlen[i], len[i], c, r0);
					if (got != want) { fprintf(stderr, "name_key_check: case %u record %zu chunk %u residue %u: words %016llx, bytes %016llx\n", ci, i, c, r0, (unsigned long long)got, (unsigned long long)want); return 1; }
				}
			}
		// the passes: the tie key, then chunk C - 1 down to chunk 0
		std::vector<uint32_t> ord(n);
		for (size_t i = 0; i < n; ++i) ord[i] = (uint32_t)i;
		std::vector<uint64_t> key(n);
		for (int c = -1, pass = 0; pass <= (int)C; ++pass, c = pass == 1 ? (int)C - 1 : c - 1) {
			for (size_t i = 0; i < n; ++i) key[i] = c < 0 ? name_tie_key(bam_u16(rec[i] + 18)) : name_chunk(rec[i] + 36, len[i], (uint32_t)c);
			std::stable_sort(ord.begin(), ord.end(), [&](uint32_t a, uint32_t b) { return key[a] < key[b]; });
		}
		std::vector<uint32_t> want;
		name_order(R, want);
		if (ord != want) {
			size_t k = 0;
			while (ord[k] == want[k]) ++k;
			fprintf(stderr, "name_key_check: case %u rank %zu: the passes put record %u, name_order record %u\n", ci, k, ord[k], want[k]);
			return 1;
		}
		fprintf(out, "%u %u", ci, C);
		for (uint32_t v : ord) fprintf(out, " %u", v);
		fprintf(out, "\n");
		for (uint8_t *p : rec) free(p);
	}
	fclose(f);
	return fclose(out) == 0 ? 0 : 9;
}
