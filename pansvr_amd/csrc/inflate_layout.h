// inflate_layout.h -- a batch of BGZF members laid out from their BSIZE / ISIZE fields alone: what the host does before a wavefront per
// member inflates them (inflate.hip: psvr_bgzf_decompress; bam_store.hip: psvr_bam_store_append_bgzf).  Host C++ only.
#pragma once
#include <vector>
#include "inflate_device.h"

namespace psvr {

struct InfMember {                       // where a member lies in the batch and where its bytes go
	long long in_off, out_off;
	uint32_t bsize, hdr, isize, pad;
};

// The BSIZE chain of in[0, n_bytes): whole members only, *used their bytes and *total their inflated bytes.  -1, or the index of the member
// that ends the chain: a header that is no BGZF header, or an ISIZE its payload cannot reach.  A member that is cut off is the caller's to complete.
inline long long inf_layout(const uint8_t *in, long long n_bytes, std::vector<InfMember> &mem, long long *used, long long *total)
{
	long long at = 0, out = 0, bad = -1;
	while (at < n_bytes) {
		uint32_t bsize = 0, xlen = 0;
		const int h = bgzf_member_header(in + at, (uint64_t)(n_bytes - at), &bsize, &xlen);
		if (h == 1 || (h == 0 && (long long)bsize > n_bytes - at)) break;
		if (h == 2) { bad = (long long)mem.size(); break; }
		const uint8_t *t = in + at + bsize - 4;
		const uint32_t isize = t[0] | (uint32_t)t[1] << 8 | (uint32_t)t[2] << 16 | (uint32_t)t[3] << 24;
		if (!inf_isize_possible(isize, bsize - 12 - xlen - 8)) { bad = (long long)mem.size(); break; }
		mem.push_back({at, out, bsize, 12 + xlen, isize, 0});
		at += bsize, out += isize;
	}
	*used = at, *total = out;
	return bad;
}

} // namespace psvr
