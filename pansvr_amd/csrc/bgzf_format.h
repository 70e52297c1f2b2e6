// bgzf_format.h -- what SAMv1 section 4.1 fixes about a BGZF file, once, for the host and the device: the block size every writer here
// cuts the stream at, the wrapper around a member's deflate payload, the bound on a member's size and the EOF block.  dfw_member
// (deflate_wave_device.h) writes the same header a byte per lane, and bgzf_member_header (inflate_device.h) checks it.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define PSVR_BGZF_HD __host__ __device__ inline
#else
#define PSVR_BGZF_HD inline
#endif

namespace psvr {

static const uint32_t kBgzfBlock = 0xff00;          // uncompressed bytes per BGZF block (htslib's BGZF_BLOCK_SIZE)
// the empty member that ends every BGZF file
static const uint8_t kBgzfEof[28] = {0x1f, 0x8b, 8, 4, 0, 0, 0, 0, 0, 0xff, 6, 0, 'B', 'C', 2, 0, 0x1b, 0, 3, 0, 0, 0, 0, 0, 0, 0, 0, 0};

// a member is at most its input in one stored block, 18 + 5 + 8 bytes around it; and n bytes cut into members of member_bytes each
PSVR_BGZF_HD int64_t bgzf_member_max(int64_t n) { return n + 31; }
PSVR_BGZF_HD int64_t bgzf_members_max(int64_t n, int64_t member_bytes) { return n + (n + member_bytes - 1) / member_bytes * bgzf_member_max(0); }

// The member around a deflate payload of clen bytes already in place at out + 18, in its two halves (k_bgzf_deflate computes the CRC
// between them): the gzip header with the BC extra field (BSIZE = member size - 1) ...
PSVR_BGZF_HD void bgzf_wrap_head(uint8_t *out, uint32_t clen)
{
	const uint32_t bsize = clen + 18 + 8 - 1;
	const uint8_t hdr[16] = {0x1f, 0x8b, 8, 4, 0, 0, 0, 0, 0, 0xff, 6, 0, 'B', 'C', 2, 0};
	for (int i = 0; i < 16; ++i) out[i] = hdr[i];
	out[16] = (uint8_t)bsize, out[17] = (uint8_t)(bsize >> 8);
}
// ... and CRC32 and ISIZE of the uncompressed bytes
PSVR_BGZF_HD void bgzf_wrap_tail(uint8_t *out, uint32_t clen, uint32_t crc, uint32_t isize)
{
	uint8_t *t = out + 18 + clen;
	for (int i = 0; i < 4; ++i) t[i] = (uint8_t)(crc >> (8 * i)), t[4 + i] = (uint8_t)(isize >> (8 * i));
}
// both; returns the member's size
PSVR_BGZF_HD uint32_t bgzf_wrap(uint8_t *out, uint32_t clen, uint32_t crc, uint32_t isize) { return bgzf_wrap_head(out, clen), bgzf_wrap_tail(out, clen, crc, isize), clen + 26; }

} // namespace psvr
