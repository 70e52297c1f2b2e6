// copy_aligned_device.h -- bytes from an unaligned source to a destination in 16-byte stores that are aligned on the destination (source
// and destination differ modulo 16: the loads are not aligned).  The one body of k_bs_append (bgzf_stream.hip) and k_store_copy
// (bam_store.hip); k_store_gather (bam_store.hip) cuts every record the same way with copy_lead and keeps its own loop.
//   [0, lead)                 byte stores, up to the destination's next 16-byte boundary
//   [lead, lead + 16 nv)      uint4 stores
//   [lead + 16 nv, len)       byte stores, fewer than 16
// The callers check their bounds before they come here: nothing outside s[0, len) is read, nothing outside d[0, len) written.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace psvr {

// bytes in front of d's next 16-byte boundary, len at the most
__device__ inline uint32_t copy_lead(const uint8_t *d, uint64_t len)
{
	const uint32_t lead = (16u - (uint32_t)((uintptr_t)d & 15u)) & 15u;
	return lead > len ? (uint32_t)len : lead;
}

// s[0, len) -> d[0, len) by the whole launch (workgroups of 256 lanes, any number of them): a vector per lane and step, head and tail
// bytes by the first workgroup
__device__ inline void copy_aligned_grid(const uint8_t *__restrict__ s, uint8_t *__restrict__ d, long long len)
{
	const long long lead = copy_lead(d, (uint64_t)len), nv = (len - lead) / 16, done = lead + 16 * nv;
	for (long long v = (long long)blockIdx.x * 256 + threadIdx.x; v < nv; v += (long long)gridDim.x * 256) {
		uint4 x;
		__builtin_memcpy(&x, s + lead + 16 * v, 16);
		*(uint4 *)(d + lead + 16 * v) = x;
	}
	if (blockIdx.x == 0) {
		if ((long long)threadIdx.x < lead) d[threadIdx.x] = s[threadIdx.x];
		if ((long long)threadIdx.x < len - done) d[done + threadIdx.x] = s[done + threadIdx.x];
	}
}

} // namespace psvr
