// inflate_check.cpp -- the one-wavefront-per-member BGZF decoder of pansvr_amd/csrc/inflate_device.h, compiled for the host (one lane):
// every case of a case file goes through bgzf_member_header + inf_member, the member and its output slice each in a heap block of exactly
// their size, so that the sanitizer build (-fsanitize=address,undefined) reports any access outside them.
// usage: inflate_check <cases> <results>
//   cases:   u32 n, then n x { u32 len, len bytes }           (a buffer that starts with one member)
//   results: n x { u32 status, u32 isize, isize bytes if status == 0 }
//   status: inflate_device.h's, or 100 + bgzf_member_header's answer, or 110 when BSIZE reaches beyond the buffer
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <vector>
#include "../../pansvr_amd/csrc/inflate_device.h"
using namespace psvr;

static bool get32(FILE *f, uint32_t *v) { return fread(v, 4, 1, f) == 1; }

int main(int argc, char **argv)
{
	if (argc != 3) { fprintf(stderr, "usage: inflate_check <cases> <results>\n"); return 2; }
	FILE *f = fopen(argv[1], "rb"), *o = fopen(argv[2], "wb");
	if (!f || !o) { fprintf(stderr, "inflate_check: cannot open the files\n"); return 2; }
	uint32_t n = 0;
	if (!get32(f, &n)) return 2;
	InfLds *lds = new InfLds;
	for (uint32_t c = 0; c < n; ++c) {
		uint32_t len = 0;
		if (!get32(f, &len)) return 2;
		uint8_t *buf = new uint8_t[len];
		if (len && fread(buf, 1, len, f) != len) return 2;
		uint32_t bsize = 0, xlen = 0, status, isize = 0;
		uint8_t *out = nullptr;
		const int h = bgzf_member_header(buf, len, &bsize, &xlen);
		if (h) status = 100u + (uint32_t)h;
		else if (bsize > len) status = 110;
		else {
			uint8_t *m = new uint8_t[bsize];                       // the member alone
			memcpy(m, buf, bsize);
			isize = m[bsize - 4] | (uint32_t)m[bsize - 3] << 8 | (uint32_t)m[bsize - 2] << 16 | (uint32_t)m[bsize - 1] << 24;
			if (!inf_isize_possible(isize, bsize - 12 - xlen - 8)) status = kInfTooShort;
			else {
				out = new uint8_t[isize];
				memset(lds, 0xa5, sizeof *lds);                    // (nothing may depend on what the tables held before)
				status = (uint32_t)inf_member<1>(m, bsize, 12 + xlen, out, isize, lds, 0);
			}
			delete[] m;
		}
		fwrite(&status, 4, 1, o), fwrite(&isize, 4, 1, o);
		if (status == 0 && isize) fwrite(out, 1, isize, o);
		delete[] out;
		delete[] buf;
	}
	delete lds;
	fclose(f);
	return fclose(o) == 0 ? 0 : 2;
}
