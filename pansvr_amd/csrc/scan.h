// scan.h -- exclusive scan of int32 counts into int64 offsets on the device, shared by engine.hip (the DP planning) and sort.hip (the
// radix sort's (digit, tile) offsets).  The kernels are static: every translation unit that includes this has its own copy.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace psvr {

// exclusive scan of int32 counts into int64 offsets, three small launches: per-tile sums, scan of the tile sums
// (one workgroup), per-tile exclusive scan + tile base.  Up to three arrays of one length go through the same three launches
// (blockIdx.y picks the array): the DP planning scans three, and a launch is ~5 us whatever it does.
static const int kScanTile = 2048;      // elements per 256-thread workgroup
struct ScanSet {
	const int32_t *cnt[3];
	long long *out[3];
	int stride[3], off[3];
	long long base[3];
};
static __global__ __launch_bounds__(256) void k_scan_sums(ScanSet S, long long n, long long *tile_sum)
{
	__shared__ long long red[256];
	const int y = blockIdx.y;
	const int32_t *cnt = S.cnt[y];
	const int stride = S.stride[y], off = S.off[y];
	const long long base = blockIdx.x * (long long)kScanTile;
	long long s = 0;
	for (int k = 0; k < kScanTile / 256; ++k) {
		long long i = base + k * 256 + threadIdx.x;
		if (i < n) s += cnt[off + i * stride];
	}
	red[threadIdx.x] = s;
	__syncthreads();
	for (int d = 128; d > 0; d >>= 1) { if ((int)threadIdx.x < d) red[threadIdx.x] += red[threadIdx.x + d]; __syncthreads(); }
	if (threadIdx.x == 0) tile_sum[(long long)y * gridDim.x + blockIdx.x] = red[0];
}
static __global__ __launch_bounds__(1024) void k_scan_tiles(long long *tile_sum_all, long long ntile, ScanSet S)
{
	__shared__ long long part[1024];
	__shared__ long long carry;
	const int tid = threadIdx.x;
	long long *tile_sum = tile_sum_all + (long long)blockIdx.x * ntile;
	if (tid == 0) carry = S.base[blockIdx.x];
	__syncthreads();
	for (long long t0 = 0; t0 < ntile; t0 += 1024) {
		long long i = t0 + tid;
		long long v = i < ntile ? tile_sum[i] : 0;
		part[tid] = v;
		__syncthreads();
		for (int d = 1; d < 1024; d <<= 1) {
			long long t = tid >= d ? part[tid - d] : 0;
			__syncthreads();
			part[tid] += t;
			__syncthreads();
		}
		if (i < ntile) tile_sum[i] = carry + part[tid] - v;
		__syncthreads();
		if (tid == 1023) carry += part[1023];
		__syncthreads();
	}
}
static __global__ __launch_bounds__(256) void k_scan_apply(ScanSet S, long long n, const long long *tile_base)
{
	__shared__ long long part[256];
	const int y = blockIdx.y;
	const int32_t *cnt = S.cnt[y];
	long long *out = S.out[y];
	const int stride = S.stride[y], off = S.off[y];
	const long long base = blockIdx.x * (long long)kScanTile;
	const int per = kScanTile / 256;
	long long v[per], s = 0;
	for (int k = 0; k < per; ++k) {
		long long i = base + (long long)threadIdx.x * per + k;
		v[k] = i < n ? cnt[off + i * stride] : 0;
		s += v[k];
	}
	part[threadIdx.x] = s;
	__syncthreads();
	for (int d = 1; d < 256; d <<= 1) {
		long long t = (int)threadIdx.x >= d ? part[threadIdx.x - d] : 0;
		__syncthreads();
		part[threadIdx.x] += t;
		__syncthreads();
	}
	long long run = tile_base[(long long)y * gridDim.x + blockIdx.x] + part[threadIdx.x] - s;
	for (int k = 0; k < per; ++k) {
		long long i = base + (long long)threadIdx.x * per + k;
		if (i < n) out[off + i * stride] = run;
		run += v[k];
	}
}

// bytes of the tile-sum scratch scan_launch needs
static inline size_t scan_tmp_bytes(int n_sets, long long n) { return (size_t)((long long)n_sets * ((n + kScanTile - 1) / kScanTile) + 1) * 8; }
// the three launches on `stream`; tile_tmp: scan_tmp_bytes(n_sets, n) bytes of device memory
static inline void scan_launch(const ScanSet &S, int n_sets, long long n, long long *tile_tmp, hipStream_t stream)
{
	if (n <= 0 || n_sets <= 0) return;
	const long long ntile = (n + kScanTile - 1) / kScanTile;
	hipLaunchKernelGGL(k_scan_sums, dim3((unsigned)ntile, (unsigned)n_sets), dim3(256), 0, stream, S, n, tile_tmp);
	hipLaunchKernelGGL(k_scan_tiles, dim3((unsigned)n_sets), dim3(1024), 0, stream, tile_tmp, ntile, S);
	hipLaunchKernelGGL(k_scan_apply, dim3((unsigned)ntile, (unsigned)n_sets), dim3(256), 0, stream, S, n, (const long long *)tile_tmp);
}

} // namespace psvr
