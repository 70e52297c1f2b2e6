// inflate_check.cpp -- the one-wavefront-per-member BGZF decoder of pansvr_amd/csrc/inflate_device.h, compiled for the host (one lane):
// every case of a case file goes through bgzf_member_header + inf_member, the member and its output slice each in a heap block of exactly
// their size, so that the sanitizer build (-fsanitize=address,undefined) reports any access outside them.
// usage: inflate_check <cases> <results>
//        inflate_check direct <cases> <results>               (a case: u32 hdr, u32 isize, the member; inf_member alone, with what the case says)
//        inflate_check constants                             (the statuses' names and numbers, a pair a line)
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
	if (argc == 2 && !strcmp(argv[1], "constants")) {
#define K(x) printf(#x " %d\n", (int)x)
		K(kInfOk), K(kInfHeader), K(kInfBlockType), K(kInfStored), K(kInfTruncated), K(kInfCounts), K(kInfCodeLengths), K(kInfNoEob), K(kInfLitTable), K(kInfDistTable);
		K(kInfLitCode), K(kInfDistCode), K(kInfFarBack), K(kInfTooLong), K(kInfTooShort), K(kInfCrc);
#undef K
		return 0;
	}
	const bool direct = argc == 4 && !strcmp(argv[1], "direct");
	if (argc != 3 && !direct) { fprintf(stderr, "usage: inflate_check [direct] <cases> <results> | inflate_check constants\n"); return 2; }
	FILE *f = fopen(argv[argc - 2], "rb"), *o = fopen(argv[argc - 1], "wb");
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
		if (direct) {                                              // buf = u32 hdr, u32 isize, then the member: inf_member as a caller with its own layout calls it
			if (len < 8) return 2;
			uint32_t hdr;
			memcpy(&hdr, buf, 4), memcpy(&isize, buf + 4, 4);
			uint8_t *m = new uint8_t[len - 8];
			memcpy(m, buf + 8, len - 8);
			out = new uint8_t[isize];
			memset(lds, 0xa5, sizeof *lds);
			status = (uint32_t)inf_member<1>(m, len - 8, hdr, out, isize, lds, 0);
			delete[] m;
			fwrite(&status, 4, 1, o), fwrite(&isize, 4, 1, o);
			if (status == 0 && isize) fwrite(out, 1, isize, o);
			delete[] out;
			delete[] buf;
			continue;
		}
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
