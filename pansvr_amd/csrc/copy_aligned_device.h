// copy_aligned_device.h -- bytes from an unaligned source to a destination in 16-byte stores that are aligned on the destination (source
// and destination differ modulo 16: the loads are not aligned).  The one body of k_bs_append (bgzf_stream.hip), k_store_copy
// (bam_store.hip) and the tiles of k_sg_window (signal_window_device.h); k_store_gather (bam_store.hip) cuts every record the same way
// with copy_lead and keeps its own loop.
//   [0, lead)                 byte stores, up to the destination's next 16-byte boundary
//   [lead, lead + 16 nv)      uint4 stores
//   [lead + 16 nv, len)       byte stores, fewer than 16
// The callers check their bounds before they come here: nothing outside s[0, len) is read, nothing outside d[0, len) written.
// copy_lead and copy_aligned_lanes also compile for the host (one lane: the checkers' build); the grid form is the device's alone.
#pragma once
#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define PSVR_COPY __host__ __device__ inline
#else
#define PSVR_COPY inline
#endif
#include <stdint.h>

namespace psvr {

// bytes in front of d's next 16-byte boundary, len at the most
PSVR_COPY uint32_t copy_lead(const uint8_t *d, uint64_t len)
{
	const uint32_t lead = (16u - (uint32_t)((uintptr_t)d & 15u)) & 15u;
	return lead > len ? (uint32_t)len : lead;
}

// s[0, len) -> d[0, len) by lanes [0, n_lanes) that all come here, each with its own `lane`: a vector per lane and step, head and tail
// bytes by the first lanes
PSVR_COPY void copy_aligned_lanes(const uint8_t *__restrict__ s, uint8_t *__restrict__ d, long long len, long long lane, long long n_lanes)
{
	const long long lead = copy_lead(d, (uint64_t)len), nv = (len - lead) / 16, done = lead + 16 * nv;
	for (long long v = lane; v < nv; v += n_lanes) {
#if defined(__HIP_DEVICE_COMPILE__)
		uint4 x;
		__builtin_memcpy(&x, s + lead + 16 * v, 16);
		*(uint4 *)(d + lead + 16 * v) = x;
#else
		__builtin_memcpy(d + lead + 16 * v, s + lead + 16 * v, 16);
#endif
	}
	for (long long i = lane; i < lead; i += n_lanes) d[i] = s[i];
	for (long long i = done + lane; i < len; i += n_lanes) d[i] = s[i];
}

#if defined(__HIPCC__)
// s[0, len) -> d[0, len) by the whole launch (workgroups of 256 lanes, any number of them)
__device__ inline void copy_aligned_grid(const uint8_t *__restrict__ s, uint8_t *__restrict__ d, long long len)
{
	copy_aligned_lanes(s, d, len, (long long)blockIdx.x * 256 + threadIdx.x, (long long)gridDim.x * 256);
}
#endif

} // namespace psvr
