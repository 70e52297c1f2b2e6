// sort.hip -- psvr_sort_order_u64 (include/psvr_engine.h): the stable order of n 64-bit keys, as an LSD radix sort with 8-bit digits.
// `panSVR aln --sort` and `panSVR sort` order their records by samtools' coordinate key with it (sorted_bam.h).
//   histogram: one read of the keys builds all eight digit histograms (a slab per workgroup, summed by a second launch); the host
//              reads them back and skips every pass whose digit is the same for every key
//   per pass:  k_sort_count (digit counts per tile of kSortTile keys, stored in (digit, tile) order) -> the exclusive scan of scan.h
//              -> k_sort_scatter (a stable rank inside the tile from per-wavefront ballots, the wavefronts' offsets through LDS)
// Every phase hands over to the next at a kernel boundary: no workgroup waits for another inside a launch.
#include <hip/hip_runtime.h>
#include <vector>
#include "../../include/psvr_engine.h"
#include "common.h"
#include "scan.h"
#include "sort_device.h"

namespace psvr {

static const int kSortThreads = 256, kSortItems = 8, kSortTile = kSortThreads * kSortItems;   // 2048 keys per tile, 512 per wavefront
static const int kSortWaves = kSortThreads / 64;
static const int kHistBlocks = 1024;

// the eight digit histograms of this workgroup's share of the keys (grid-stride), counted in LDS, stored as its slab of 8 x 256
__global__ __launch_bounds__(256) void k_sort_hist(const uint64_t *keys, long long n, uint32_t *slab)
{
	__shared__ uint32_t h[8 * 256];
	for (int i = threadIdx.x; i < 8 * 256; i += 256) h[i] = 0;
	__syncthreads();
	for (long long i = blockIdx.x * 256ll + threadIdx.x; i < n; i += (long long)gridDim.x * 256) {
		const uint64_t k = keys[i];
#pragma unroll
		for (int d = 0; d < 8; ++d) atomicAdd(&h[d * 256 + (int)((k >> (8 * d)) & 255)], 1u);
	}
	__syncthreads();
	for (int i = threadIdx.x; i < 8 * 256; i += 256) slab[(size_t)blockIdx.x * 2048 + i] = h[i];
}
// the slabs summed: hist[d * 256 + v] = keys whose digit d is v
__global__ __launch_bounds__(256) void k_sort_hist_sum(const uint32_t *slab, int n_slab, uint32_t *hist)
{
	const int j = blockIdx.x * 256 + threadIdx.x;
	uint32_t s = 0;
	for (int b = 0; b < n_slab; ++b) s += slab[(size_t)b * 2048 + j];
	hist[j] = s;
}
// digit counts of tile t, stored at cnt[digit * ntile + t]: the scan over that order gives every (digit, tile) its first output slot
__global__ __launch_bounds__(kSortThreads) void k_sort_count(const uint64_t *keys, long long n, int shift, long long ntile, int32_t *cnt)
{
	__shared__ int32_t h[256];
	h[threadIdx.x] = 0;
	__syncthreads();
	const long long t = blockIdx.x, base = t * kSortTile;
#pragma unroll
	for (int r = 0; r < kSortItems; ++r) {
		const long long i = base + r * kSortThreads + threadIdx.x;
		if (i < n) atomicAdd(&h[(int)((keys[i] >> shift) & 255)], 1);
	}
	__syncthreads();
	cnt[threadIdx.x * ntile + t] = h[threadIdx.x];
}
// the stable scatter of tile t.  Wavefront w holds keys [base + 512 w, base + 512 (w + 1)) in 8 rounds of 64 (lane order = input order).
// A round's lanes with equal digits find each other by 8 ballots; a key's rank is the number of earlier keys of its digit in the
// wavefront: the wavefront's running count (LDS) plus the matching lanes below it (mbcnt).  The group's lowest lane moves the count on.
// Then per digit the wavefronts' counts become offsets in wavefront order, on top of the scanned (digit, tile) offset.
// iin == nullptr: the first pass, the index is the position.
__global__ __launch_bounds__(kSortThreads) void k_sort_scatter(const uint64_t *kin, const uint32_t *iin, long long n, int shift, long long ntile, const long long *off,
                                                               uint64_t *kout, uint32_t *iout)
{
	__shared__ uint32_t wcnt[kSortWaves][256];
	for (int i = threadIdx.x; i < kSortWaves * 256; i += kSortThreads) (&wcnt[0][0])[i] = 0;
	__syncthreads();
	const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
	const long long t = blockIdx.x, base = t * kSortTile + (long long)w * 64 * kSortItems;
	uint64_t key[kSortItems];
	uint32_t idx[kSortItems], rank[kSortItems];
	int dig[kSortItems];
#pragma unroll
	for (int r = 0; r < kSortItems; ++r) {
		const long long i = base + r * 64 + lane;
		const bool ok = i < n;
		key[r] = ok ? kin[i] : 0;
		idx[r] = ok ? (iin ? iin[i] : (uint32_t)i) : 0;
	}
	const unsigned long long below = (1ull << lane) - 1;
#pragma unroll
	for (int r = 0; r < kSortItems; ++r) {
		const bool ok = base + r * 64 + lane < n;
		const int d = (int)((key[r] >> shift) & 255);
		unsigned long long m = __ballot(ok);
#pragma unroll
		for (int b = 0; b < 8; ++b) {
			const unsigned long long v = __ballot((d >> b) & 1);
			m &= ((d >> b) & 1) ? v : ~v;
		}
		const uint32_t before = wcnt[w][d];
		rank[r] = before + (uint32_t)__popcll(m & below);
		dig[r] = d;
		__builtin_amdgcn_wave_barrier();                           // every lane has read the count before the group's lowest lane moves it
		if (ok && (m & below) == 0) wcnt[w][d] = before + (uint32_t)__popcll(m);
		__builtin_amdgcn_wave_barrier();
	}
	__syncthreads();
	{
		const int d = threadIdx.x;                                 // kSortThreads == 256 digits
		uint32_t s = (uint32_t)off[(long long)d * ntile + t];      // < n < 2^32
		for (int q = 0; q < kSortWaves; ++q) { const uint32_t c = wcnt[q][d]; wcnt[q][d] = s; s += c; }
	}
	__syncthreads();
#pragma unroll
	for (int r = 0; r < kSortItems; ++r) {
		if (base + r * 64 + lane >= n) continue;
		const uint32_t p = wcnt[w][dig[r]] + rank[r];
		if (p < n) kout[p] = key[r], iout[p] = idx[r];             // (always: the counts and the ranks see the same keys)
	}
}

struct SortCtx : DeviceService {
	std::vector<uint32_t> h_hist;            // what an asynchronous copy writes on the host lives as long as the stream
};
static SortCtx &sort_ctx() { static SortCtx c; return c; }

} // namespace psvr

using namespace psvr;


// the body of the sort over device pointers (sort_device.h): psvr_sort_order_u64 below and psvr_bam_store_order (bam_store.hip) both run it
// the scratch of a sort of n keys (sort_device.h): nothing is launched, nothing but S is touched
int psvr::sort_scratch_reserve(long long n, SortScratch &S, const char *who)
{
	if (n <= 0) return PSVR_OK;
	const long long ntile = (n + kSortTile - 1) / kSortTile, ncnt = 256 * ntile;
	const int nhb = (int)(ntile < kHistBlocks ? ntile : kHistBlocks);
	// a second key array and two index arrays (ping-pong with the caller's keys), the (digit, tile) counts and offsets, the scan's and the histogram's scratch
	const size_t need = (size_t)n * 16 + (size_t)ncnt * 12 + scan_tmp_bytes(1, ncnt) + (size_t)(nhb + 1) * 8192;
	// (a buffer that is large enough stays: a run that continues an order finds it in S.i0 or S.i1, where the run before left it)
	auto room = [](DevBuf &b, size_t bytes) { return b.p && b.bytes >= bytes ? hipSuccess : b.alloc(bytes); };
	if (room(S.k1, (size_t)n * 8) || room(S.i0, (size_t)n * 4) || room(S.i1, (size_t)n * 4) || room(S.cnt, (size_t)ncnt * 4) ||
	    room(S.off, (size_t)ncnt * 8) || room(S.tmp, scan_tmp_bytes(1, ncnt)) || room(S.slab, (size_t)nhb * 8192) || room(S.hist, 8192)) {
		(void)hipGetLastError();
		return set_error(PSVR_ERR_NOMEM, "%s: %zu bytes of device memory needed for %lld keys", who, need + (size_t)n * 8, n);
	}
	return PSVR_OK;
}

int psvr::sort_order_device(hipStream_t st, long long n, uint64_t *d_keys, SortScratch &S, std::vector<uint32_t> &h, const uint32_t **d_order, const char *who,
                            const uint32_t *d_order_in)
{
	*d_order = d_order_in;
	if (n <= 0) return PSVR_OK;
	if (int rc = sort_scratch_reserve(n, S, who)) return rc;       // (no allocation when a run before, or the caller, has made the room)
	const long long ntile = (n + kSortTile - 1) / kSortTile, ncnt = 256 * ntile;
	const int nhb = (int)(ntile < kHistBlocks ? ntile : kHistBlocks);
	h.assign(2048, 0);
	StreamDrain drain{st};                                         // (after the buffers: nothing is in flight when they are freed)
	hipLaunchKernelGGL(k_sort_hist, dim3((unsigned)nhb), dim3(256), 0, st, (const uint64_t *)d_keys, n, S.slab.as<uint32_t>());
	hipLaunchKernelGGL(k_sort_hist_sum, dim3(8), dim3(256), 0, st, (const uint32_t *)S.slab.p, nhb, S.hist.as<uint32_t>());
	PSVR_HIP(hipGetLastError());
	PSVR_HIP(hipMemcpyAsync(h.data(), S.hist.p, 8192, hipMemcpyDeviceToHost, st));
	PSVR_HIP(hipStreamSynchronize(st));
	uint64_t *kin = d_keys, *kout = S.k1.as<uint64_t>();
	// the incoming order is read by the first pass that runs: that pass writes the other index array
	const uint32_t *iin = d_order_in;
	uint32_t *iout = d_order_in == S.i0.as<uint32_t>() ? S.i1.as<uint32_t>() : S.i0.as<uint32_t>();
	for (int d = 0; d < 8; ++d) {
		bool constant = false;
		for (int v = 0; v < 256; ++v) if (h[(size_t)d * 256 + v] == (uint32_t)n) constant = true;
		if (constant) continue;                                    // this digit orders nothing
		hipLaunchKernelGGL(k_sort_count, dim3((unsigned)ntile), dim3(kSortThreads), 0, st, (const uint64_t *)kin, n, 8 * d, ntile, S.cnt.as<int32_t>());
		ScanSet X = {};
		X.cnt[0] = S.cnt.as<int32_t>(), X.out[0] = S.off.as<long long>(), X.stride[0] = 1;
		scan_launch(X, 1, ncnt, S.tmp.as<long long>(), st);
		hipLaunchKernelGGL(k_sort_scatter, dim3((unsigned)ntile), dim3(kSortThreads), 0, st, (const uint64_t *)kin, iin, n, 8 * d, ntile,
		                   (const long long *)S.off.p, kout, iout);
		PSVR_HIP(hipGetLastError());
		std::swap(kin, kout);
		iin = iout, iout = (iout == S.i0.as<uint32_t>()) ? S.i1.as<uint32_t>() : S.i0.as<uint32_t>();
	}
	drain.armed = false;                                           // (what is queued reads and writes the caller's keys and S only: the caller waits)
	*d_order = iin;
	return PSVR_OK;
}

extern "C" int psvr_sort_order_u64(int device, int64_t n, const uint64_t *keys, uint32_t *order)
{
	if (n < 0 || (n > 0 && (!keys || !order))) return set_error(PSVR_ERR_ARG, "psvr_sort_order_u64: bad argument");
	if (n >= ((int64_t)1 << 32)) return set_error(PSVR_ERR_UNSUPPORTED, "psvr_sort_order_u64: %lld keys, the order is 32-bit (at most 2^32 - 1 keys)", (long long)n);
	if (n == 0) return PSVR_OK;
	if (psvr_device_count() <= 0) return set_error(PSVR_ERR_DEVICE, "no HIP device visible: the engine has no CPU path");
	SortCtx &c = sort_ctx();
	std::lock_guard<std::mutex> lk(c.mu);
	if (int rc = c.bind(device, false, [] {})) return rc;                                  // (the buffers are the call's own)
	hipStream_t st = c.stream;
	const long long ntile = (n + kSortTile - 1) / kSortTile, ncnt = 256 * ntile;
	const int nhb = (int)(ntile < kHistBlocks ? ntile : kHistBlocks);
	// two key arrays and two index arrays (ping-pong), the (digit, tile) counts and offsets, the scan's and the histogram's scratch
	const size_t need = (size_t)n * 24 + (size_t)ncnt * 12 + scan_tmp_bytes(1, ncnt) + (size_t)(nhb + 1) * 8192;
	size_t free_b = 0, total_b = 0;
	PSVR_HIP(hipMemGetInfo(&free_b, &total_b));
	if (need > free_b) return set_error(PSVR_ERR_NOMEM, "psvr_sort_order_u64: %zu bytes of device memory needed for %lld keys, %zu free", need, (long long)n, free_b);
	DevBuf k0;
	SortScratch S;
	if (k0.alloc((size_t)n * 8)) {
		(void)hipGetLastError();
		return set_error(PSVR_ERR_NOMEM, "psvr_sort_order_u64: %zu bytes of device memory needed for %lld keys", need, (long long)n);
	}
	StreamDrain drain{st};                                         // (after the buffers: nothing is in flight when they are freed)
	PSVR_HIP(hipMemcpyAsync(k0.p, keys, (size_t)n * 8, hipMemcpyHostToDevice, st));
	const uint32_t *iin = nullptr;
	if (int rc = sort_order_device(st, (long long)n, k0.as<uint64_t>(), S, c.h_hist, &iin, "psvr_sort_order_u64")) return rc;
	if (iin) PSVR_HIP(hipMemcpyAsync(order, iin, (size_t)n * 4, hipMemcpyDeviceToHost, st));
	drain.armed = false;
	PSVR_HIP(hipStreamSynchronize(st));
	if (!iin) for (int64_t i = 0; i < n; ++i) order[i] = (uint32_t)i;   // every digit constant: all keys equal, the input order stands
	return PSVR_OK;
}

extern "C" int psvr_sort_order_names(int device, int64_t n, const void *names, int64_t n_bytes, const int64_t *name_off, const uint8_t *tie, uint32_t *order)
{
	if (psvr_device_count() <= 0) return set_error(PSVR_ERR_DEVICE, "no HIP device visible: the engine has no CPU path");
	if (n < 0 || n_bytes < 0 || (n > 0 && (!names || !name_off || !order))) return set_error(PSVR_ERR_ARG, "psvr_sort_order_names: bad argument");
	if (n >= ((int64_t)1 << 32)) return set_error(PSVR_ERR_UNSUPPORTED, "psvr_sort_order_names: %lld names, the order is 32-bit (at most 2^32 - 1 names)", (long long)n);
	if (n == 0) return PSVR_OK;
	for (int64_t i = 0; i < n; ++i)                                // (the kernel asks again; here nothing has been uploaded yet)
		if (name_off[i] < 0 || name_off[i] >= n_bytes) return set_error(PSVR_ERR_ARG, "psvr_sort_order_names: name %lld begins at byte %lld of %lld", (long long)i, (long long)name_off[i], (long long)n_bytes);
	SortCtx &c = sort_ctx();
	std::lock_guard<std::mutex> lk(c.mu);
	if (int rc = c.bind(device, false, [] {})) return rc;                                  // (the buffers are the call's own)
	hipStream_t st = c.stream;
	// the names (in whole 8-byte words: k_name_chunk loads the aligned words a name touches), their offsets and tie keys, the keys, the entries
	const size_t blob_bytes = ((size_t)n_bytes + 7) / 8 * 8;
	DevBuf blob, off, tk, k0;
	NameScratch N;
	SortScratch S;
	if (blob.alloc(blob_bytes) || off.alloc((size_t)n * 8) || (tie && tk.alloc((size_t)n)) || k0.alloc((size_t)n * 8)) {
		(void)hipGetLastError();
		return set_error(PSVR_ERR_NOMEM, "psvr_sort_order_names: %zu bytes of device memory needed for %lld names in %lld bytes", blob_bytes + (size_t)n * 41, (long long)n, (long long)n_bytes);
	}
	StreamDrain drain{st};                                         // (after the buffers: nothing is in flight when they are freed)
	PSVR_HIP(hipMemsetAsync((uint8_t *)blob.p + (blob_bytes - 8), 0, 8, st));
	PSVR_HIP(hipMemcpyAsync(blob.p, names, (size_t)n_bytes, hipMemcpyHostToDevice, st));
	PSVR_HIP(hipMemcpyAsync(off.p, name_off, (size_t)n * 8, hipMemcpyHostToDevice, st));
	if (tie) PSVR_HIP(hipMemcpyAsync(tk.p, tie, (size_t)n, hipMemcpyHostToDevice, st));
	const NameSrc src = {nullptr, blob.as<uint8_t>(), (long long)n_bytes, off.as<long long>(), tie ? tk.as<uint8_t>() : nullptr};
	const uint32_t *ord = nullptr;
	if (int rc = sort_order_names_device(st, (long long)n, src, k0.as<uint64_t>(), N, S, c.h_hist, &ord, "psvr_sort_order_names")) return rc;
	if (ord) PSVR_HIP(hipMemcpyAsync(order, ord, (size_t)n * 4, hipMemcpyDeviceToHost, st));
	drain.armed = false;
	PSVR_HIP(hipStreamSynchronize(st));
	if (!ord) for (int64_t i = 0; i < n; ++i) order[i] = (uint32_t)i;   // every key equal: the input order stands
	return PSVR_OK;
}
