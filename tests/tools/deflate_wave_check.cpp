// deflate_wave_check.cpp -- the one-wavefront-per-member BGZF encoder of pansvr_amd/csrc/deflate_wave_device.h, compiled for the host (one
// lane): the input is cut into members of <member_bytes>, each member's input, slot and token scratch lie in heap blocks of exactly the
// sizes the encoder is promised, so that the sanitizer build (-fsanitize=address,undefined) reports any access outside them.
// usage: deflate_wave_check <member_bytes> <in> <out>          members side by side, as psvr_bgzf_compress_members writes them
//        deflate_wave_check --old <block_bytes> <hbits> <in>   prints the total of deflate_device.h's deflate_block + 26 bytes per block
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <vector>
#include "../../pansvr_amd/csrc/deflate_wave_device.h"
using namespace psvr;

static std::vector<uint8_t> slurp(const char *fn)
{
	std::vector<uint8_t> v;
	FILE *f = fopen(fn, "rb");
	if (!f) { fprintf(stderr, "deflate_wave_check: cannot open %s\n", fn); exit(2); }
	uint8_t buf[65536];
	for (size_t k; (k = fread(buf, 1, sizeof buf, f)) > 0;) v.insert(v.end(), buf, buf + k);
	fclose(f);
	return v;
}

int main(int argc, char **argv)
{
	if (argc == 5 && !strcmp(argv[1], "--old")) {
		const uint32_t blk = (uint32_t)atol(argv[2]);
		const int hbits = atoi(argv[3]);
		const std::vector<uint8_t> in = slurp(argv[4]);
		std::vector<uint8_t> fast(df_fast_bytes(hbits)), out(blk + 64);
		std::vector<uint32_t> tok(blk + 4);
		unsigned long long total = 0;
		for (size_t at = 0; at < in.size(); at += blk) {
			const uint32_t n = (uint32_t)(in.size() - at < blk ? in.size() - at : blk);
			total += deflate_block(in.data() + at, n, out.data(), blk + 64 - 26, fast.data(), hbits, tok.data()) + 26;
		}
		printf("%llu\n", total);
		return 0;
	}
	if (argc != 4) { fprintf(stderr, "usage: deflate_wave_check <member_bytes> <in> <out>\n"); return 2; }
	const uint32_t mb = (uint32_t)atol(argv[1]);
	if (mb < 256 || mb > kDfMaxIn) { fprintf(stderr, "deflate_wave_check: member_bytes outside 256..0xff00\n"); return 2; }
	const std::vector<uint8_t> in = slurp(argv[2]);
	FILE *o = fopen(argv[3], "wb");
	if (!o) return 2;
	DfwLds *lds = new DfwLds;
	for (size_t at = 0; at < in.size(); at += mb) {
		const uint32_t n = (uint32_t)(in.size() - at < mb ? in.size() - at : mb);
		uint8_t *src = new uint8_t[n];                                 // the member's input alone
		memcpy(src, in.data() + at, n);
		uint32_t *slot = new uint32_t[dfw_slot_bytes(n) / 4];
		uint32_t *tok = new uint32_t[n + 1];
		memset(lds, 0xa5, sizeof *lds);                                // (nothing may depend on what the tables held before)
		memset(slot, 0x5a, dfw_slot_bytes(n));
		const uint32_t size = dfw_member<1>(src, n, (uint8_t *)slot, tok, lds, 0);
		if (size > dfw_member_max(n)) { fprintf(stderr, "deflate_wave_check: a member of %u bytes from %u\n", size, n); return 3; }
		fwrite(slot, 1, size, o);
		delete[] tok;
		delete[] slot;
		delete[] src;
	}
	delete lds;
	return fclose(o) == 0 ? 0 : 2;
}
