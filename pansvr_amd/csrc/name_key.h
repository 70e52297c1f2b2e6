// name_key.h -- the name order of `panSVR sort -n` as radix keys, once, for the host and the device (name_sort.hip's kernels, the checker
// tests/tools/name_key_check.cpp).  Compiled for both sides, as bam_record.h is; no STL, no allocation.
// The order is name_order's (sorted_bam.h): the names as strcmp compares them (unsigned bytes up to the first NUL), equal names by
// flag & 0xc0 (first read before second), then input order.  As keys:
//   name_len(p, bound)        the first NUL inside p[0, bound), or bound without one: what lies behind a NUL inside the name field is no name
//   name_chunk(p, len, c)     name bytes [8c, 8c + 8) as a big-endian uint64; every byte at or behind len is 0
//   name_tie_key(flag)        flag & 0xc0
// Comparing the chunk sequences lexicographically, then the tie key, then the index gives that order: NUL is the smallest byte and ends
// a name, so the shorter of two names pads with the smallest value, and equal names pad alike.  A stable sort by the tie key, then by the
// chunks from the last to the first (LSD), is the same order.
//   name_chunk_words(w0, w1, r, nbytes)   name_chunk from the two aligned 8-byte words that cover the chunk (little-endian loads; r = the
//                             chunk's address mod 8, nbytes = 1..8 bytes of it that belong to the name; w1 counts only when r + nbytes > 8)
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define PSVR_NK __host__ __device__ inline
#else
#define PSVR_NK inline
#endif

namespace psvr {

static const uint32_t kNameMaxLen = 254;                     // l_read_name is one byte and counts the NUL
static const uint32_t kNameMaxChunks = 32;                   // ceil(255 / 8): a name field without a NUL included

PSVR_NK uint32_t name_len(const uint8_t *p, uint32_t bound)
{
	uint32_t k = 0;
	while (k < bound && p[k]) ++k;
	return k;
}
// ... of a record (rec points at block_size; bam_rec_cigar_inside holds, so the name field lies inside the record).  name_order()'s strcmp has
// no such bound: the two agree for every record whose name field holds a NUL (the reader's rule, bam_rec_name_ends); without one the name is
// the l_read_name bytes here, never what follows them
PSVR_NK uint32_t name_len_rec(const uint8_t *rec) { return name_len(rec + 36, rec[12]); }

PSVR_NK uint64_t name_chunk(const uint8_t *p, uint32_t len, uint32_t c)
{
	uint64_t k = 0;
	for (uint32_t b = 0; b < 8; ++b) {
		const uint32_t i = 8 * c + b;
		k = k << 8 | (i < len ? p[i] : 0u);
	}
	return k;
}

PSVR_NK uint32_t name_tie_key(uint32_t flag) { return flag & 0xc0u; }

// bytes s .. s + 3 of the eight bytes hi:lo (s = 0..3)
PSVR_NK uint32_t name_align_bytes(uint32_t hi, uint32_t lo, uint32_t s)
{
#if defined(__HIP_DEVICE_COMPILE__)
	return __builtin_amdgcn_alignbyte(hi, lo, s);            // v_alignbyte_b32
#else
	return (uint32_t)(((uint64_t)hi << 32 | lo) >> (8 * s));
#endif
}
PSVR_NK uint64_t name_chunk_words(uint64_t w0, uint64_t w1, uint32_t r, uint32_t nbytes)
{
	uint32_t a0 = (uint32_t)w0, a1 = (uint32_t)(w0 >> 32), a2 = (uint32_t)w1;
	const uint32_t a3 = (uint32_t)(w1 >> 32);
	if (r & 4u) a0 = a1, a1 = a2, a2 = a3;
	const uint32_t lo = name_align_bytes(a1, a0, r & 3u), hi = name_align_bytes(a2, a1, r & 3u);   // name bytes 0..3 and 4..7, the first one lowest
	const uint64_t be = (uint64_t)__builtin_bswap32(lo) << 32 | __builtin_bswap32(hi);             // (v_perm_b32 on the device)
	return nbytes >= 8 ? be : be & ~(~0ull >> (8 * nbytes));
}

} // namespace psvr
