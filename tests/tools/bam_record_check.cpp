// bam_record_check -- pansvr_amd/csrc/bam_record.h on its own, on the host: what every rule layer says about the records of a buffer, and what
// the derived fields are.  tests/test_bam_record.py builds it plain and under AddressSanitizer + UBSan and holds it to a Python restatement.
//   bam_record_check records <cases> <results>     cases: uint32 count, then per case uint32 length and the bytes.  Every case is copied into
//       an allocation of exactly its length and walked from byte 0: per record one line
//           <case> <at> <frame> <cigar_inside> <fields_inside> <reader_fits> <name_ends> <span> <beg> <end> <bin> <key> <key_exact> <tid> <pos> <len> <flag>
//       (a layer whose preconditions the layers before it have not vouched for is not asked: -1, as are the fields of a record whose CIGAR
//       leaves it), on to the next record while the frame holds, then "<case> end <at>"
//   bam_record_check words <words> <results>       uint32 CIGAR words in, int64 bam_cigar_ref_len of each out
#include <stdint.h>
#include <stdio.h>
#include <vector>
#include "../../pansvr_amd/csrc/bam_record.h"

using namespace psvr;

struct Derived { int32_t tid, pos; int64_t end; uint32_t len, bin, flag; };

static bool read_all(FILE *f, void *p, size_t n) { return n == 0 || fread(p, 1, n, f) == n; }

int main(int argc, char **argv)
{
	if (argc != 4) { fprintf(stderr, "usage: bam_record_check records|words <in> <out>\n"); return 2; }
	const bool words = argv[1][0] == 'w';
	FILE *f = fopen(argv[2], "rb"), *o = fopen(argv[3], "wb");
	if (!f || !o) { fprintf(stderr, "bam_record_check: cannot open the files\n"); return 2; }
	if (words) {
		uint32_t w;
		while (fread(&w, 4, 1, f) == 1) { const int64_t v = bam_cigar_ref_len(w); fwrite(&v, 8, 1, o); }
		return fclose(o) == 0 ? 0 : 2;
	}
	uint32_t n_cases = 0;
	if (!read_all(f, &n_cases, 4)) { fprintf(stderr, "bam_record_check: short file\n"); return 2; }
	for (uint32_t c = 0; c < n_cases; ++c) {
		uint32_t n = 0;
		if (!read_all(f, &n, 4)) { fprintf(stderr, "bam_record_check: short file\n"); return 2; }
		std::vector<uint8_t> buf(n);
		if (!read_all(f, buf.data(), n)) { fprintf(stderr, "bam_record_check: short file\n"); return 2; }
		size_t at = 0;
		while (at < n) {
			const uint8_t *rec = buf.data() + at;
			const int frame = bam_rec_frame(rec, n - at);
			int cigar = -1, fields = -1, reader = -1, nul = -1;
			if (frame) cigar = bam_rec_cigar_inside(rec), fields = bam_rec_fields_inside(rec), reader = bam_rec_reader_fits(rec);
			if (reader == 1) nul = bam_rec_name_ends(rec);
			fprintf(o, "%u %zu %d %d %d %d %d", c, at, frame, cigar, fields, reader, nul);
			if (cigar == 1) {
				Derived d;
				bam_rec_derived(rec, &d);
				fprintf(o, " %lld %lld %lld %u %llu %d %d %d %u %u\n", (long long)bam_rec_ref_span(rec), (long long)(d.pos < 0 ? 0 : d.pos), (long long)d.end, d.bin,
				        (unsigned long long)bam_sort_key(d.tid, d.pos, d.flag), (int)bam_key_exact(d.pos), d.tid, d.pos, d.len, d.flag);
			} else fprintf(o, " -1 -1 -1 -1 -1 -1 -1 -1 -1 -1\n");
			if (!frame) break;
			at += 4 + (size_t)bam_u32(rec);
		}
		fprintf(o, "%u end %zu\n", c, at);
	}
	return fclose(o) == 0 ? 0 : 2;
}
