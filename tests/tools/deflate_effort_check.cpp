// deflate_effort_check.cpp -- dfw_member_effort of pansvr_amd/csrc/deflate_wave_device.h (the wavefront-per-member BGZF encoder with hash
// chains and lazy matching, efforts 0..3), compiled for the host (one lane).  As in deflate_wave_check.cpp the input is cut into members of
// <member_bytes>, and each member's input, slot, token scratch and link scratch lie in heap blocks of exactly the sizes the encoder is
// promised, so that the sanitizer build (-fsanitize=address,undefined) reports any access outside them.  Effort 0 gets no link scratch at all.
// usage: deflate_effort_check [--dirty] [--tokens <file>] <effort> <member_bytes> <in> <out>
//        --dirty    tok and link are filled with 0xff before every member (otherwise with 0): the bytes may not depend on it
//        --tokens   every member's tokens as little-endian words, the end of block included: a literal is its byte, a match is
//                   0x80000000 | (length - 3) << 16 | (distance - 1), the end of block is 0x40000100
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
	if (!f) { fprintf(stderr, "deflate_effort_check: cannot open %s\n", fn); exit(2); }
	uint8_t buf[65536];
	for (size_t k; (k = fread(buf, 1, sizeof buf, f)) > 0;) v.insert(v.end(), buf, buf + k);
	fclose(f);
	return v;
}

static uint32_t member(int effort, const uint8_t *in, uint32_t n, uint8_t *slot, uint32_t *tok, uint16_t *link, DfwLds *t)
{
	switch (effort) {
	case 0: return dfw_member_effort<1, 0>(in, n, slot, tok, link, t, 0);
	case 1: return dfw_member_effort<1, 1>(in, n, slot, tok, link, t, 0);
	case 2: return dfw_member_effort<1, 2>(in, n, slot, tok, link, t, 0);
	default: return dfw_member_effort<1, 3>(in, n, slot, tok, link, t, 0);
	}
}

int main(int argc, char **argv)
{
	bool dirty = false;
	const char *tokens_fn = nullptr;
	int a = 1;
	for (; a < argc; ++a) {
		if (!strcmp(argv[a], "--dirty")) dirty = true;
		else if (!strcmp(argv[a], "--tokens") && a + 1 < argc) tokens_fn = argv[++a];
		else break;
	}
	if (argc - a != 4) { fprintf(stderr, "usage: deflate_effort_check [--dirty] [--tokens <file>] <effort> <member_bytes> <in> <out>\n"); return 2; }
	const int effort = atoi(argv[a]);
	const uint32_t mb = (uint32_t)atol(argv[a + 1]);
	if (effort < 0 || effort > kDfwMaxEffort) { fprintf(stderr, "deflate_effort_check: effort outside 0..3\n"); return 2; }
	if (mb < 256 || mb > kDfMaxIn) { fprintf(stderr, "deflate_effort_check: member_bytes outside 256..0xff00\n"); return 2; }
	const std::vector<uint8_t> in = slurp(argv[a + 2]);
	FILE *o = fopen(argv[a + 3], "wb");
	FILE *tf = tokens_fn ? fopen(tokens_fn, "wb") : nullptr;
	if (!o || (tokens_fn && !tf)) return 2;
	DfwLds *lds = new DfwLds;
	for (size_t at = 0; at < in.size(); at += mb) {
		const uint32_t n = (uint32_t)(in.size() - at < mb ? in.size() - at : mb);
		uint8_t *src = new uint8_t[n];                                 // the member's input alone
		memcpy(src, in.data() + at, n);
		uint32_t *slot = new uint32_t[dfw_slot_bytes(n) / 4];
		uint32_t *tok = new uint32_t[n + 1];
		uint16_t *link = effort ? new uint16_t[n] : nullptr;
		memset(lds, 0xa5, sizeof *lds);                                // (nothing may depend on what the tables held before)
		memset(slot, 0x5a, dfw_slot_bytes(n));
		memset(tok, dirty ? 0xff : 0, 4 * (size_t)(n + 1));
		if (link) memset(link, dirty ? 0xff : 0, 2 * (size_t)n);
		const uint32_t size = member(effort, src, n, (uint8_t *)slot, tok, link, lds);
		if (size > dfw_member_max(n)) { fprintf(stderr, "deflate_effort_check: a member of %u bytes from %u\n", size, n); return 3; }
		fwrite(slot, 1, size, o);
		if (tf) {
			uint32_t nt = 0;
			while (nt <= n && tok[nt] != 0x40000100u) ++nt;
			if (nt > n) { fprintf(stderr, "deflate_effort_check: no end of block among %u tokens\n", n + 1); return 3; }
			fwrite(tok, 4, nt + 1, tf);
		}
		delete[] link;
		delete[] tok;
		delete[] slot;
		delete[] src;
	}
	delete lds;
	if (tf && fclose(tf) != 0) return 2;
	return fclose(o) == 0 ? 0 : 2;
}
