// bam_chain_check -- the host build of pansvr_amd/csrc/bam_chain_device.h (one "lane"): the record-chain finder of psvr_bam_store_append_bgzf
// run over inflated BAM streams without a GPU (tests/test_bam_chain.py; also built with -fsanitize=address,undefined).
//   bam_chain_check <cases> <results>
// cases:   uint32 count, then per case  int64 start, int32 n_ref, int64 seg_bytes, uint32 n, the n bytes of the stream
// results: per case one line  "total tail segments no_guess wrong_guess rewalked first_malformed | entry[0] ... entry[segments]"
//          (first_malformed: how many whole records the chain holds in front of its first malformed one, or -1)
// Every stream is copied into an allocation of exactly its size, so a load behind it is the sanitizer's to report.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <vector>
#include "../../pansvr_amd/csrc/bam_chain_device.h"

using namespace psvr;

int main(int argc, char **argv)
{
	if (argc != 3) { fprintf(stderr, "usage: bam_chain_check <cases> <results>\n"); return 2; }
	FILE *f = fopen(argv[1], "rb"), *o = fopen(argv[2], "w");
	if (!f || !o) { fprintf(stderr, "bam_chain_check: cannot open the files\n"); return 2; }
	uint32_t n_cases = 0;
	if (fread(&n_cases, 4, 1, f) != 1) return 2;
	for (uint32_t c = 0; c < n_cases; ++c) {
		int64_t start = 0, seg = 0;
		int32_t n_ref = 0;
		uint32_t n = 0;
		if (fread(&start, 8, 1, f) != 1 || fread(&n_ref, 4, 1, f) != 1 || fread(&seg, 8, 1, f) != 1 || fread(&n, 4, 1, f) != 1) return 2;
		uint8_t *bytes = (uint8_t *)malloc(n ? n : 1);
		if (n && fread(bytes, 1, n, f) != n) return 2;
		if (seg < kChainMinSeg || start < 0 || start > (int64_t)n) { fprintf(stderr, "bam_chain_check: case %u: bad start or segment size\n", c); return 2; }
		const long long n_seg = chain_segments(n, seg);
		std::vector<ChainSeg> sg((size_t)n_seg);
		std::vector<long long> entry((size_t)n_seg + 1);
		std::vector<int32_t> cnt((size_t)n_seg + 1);
		for (long long s = 0; s < n_seg; ++s) chain_guess<1>(bytes, n, seg, start, n_ref, s, sg.data(), 0);
		const ChainResult R = chain_settle<1>(bytes, n, seg, start, n_seg, sg.data(), entry.data(), cnt.data(), 0);
		long long first_bad = -1;
		if (R.bad_seg >= 0) {
			first_bad = 0;
			for (long long s = 0; s <= R.bad_seg; ++s) first_bad += cnt[(size_t)s];
		}
		fprintf(o, "%lld %lld %lld %lld %lld %lld %lld |", R.total, R.tail, n_seg, R.no_guess, R.wrong_guess, R.rewalked, first_bad);
		for (long long s = 0; s <= n_seg; ++s) fprintf(o, " %lld", entry[(size_t)s]);
		fprintf(o, "\n");
		free(bytes);
	}
	fclose(f);
	return fclose(o) == 0 ? 0 : 2;
}
