// name_sort.hip -- name order on the device (sort_device.h: sort_order_names_device; the rules are name_key.h's): what name_order()
// (sorted_bam.h) computes with std::stable_sort and strcmp, as runs of sort.hip's stable radix sort over 8-byte chunks of the names.
//   k_name_len     a lane per name: where it lies, how long it is and its tie key, packed into one entry (address | length << 48 | tie << 56);
//                  the longest length and a refusal are reduced in the wavefront by shuffles, then in the workgroup through four LDS words,
//                  and reach ctl[] with one atomic max each per workgroup
//   k_name_chunk   a lane per rank i of the order so far: key[i] = chunk c of name order[i], or its tie key (c < 0).  A name begins at any
//                  byte: the lane loads the one or two aligned 8-byte words that hold the chunk's name bytes and shifts, swaps and masks them in
//                  registers (name_chunk_words).  A word is loaded only when it holds a byte of the name, so no load begins behind the name's
//                  last byte, and none lies in an 8-byte word that the name does not touch
//   the runs       the tie key first, then chunk C - 1 down to chunk 0 (C = ceil(longest / 8)): every run is stable and takes the order of the
//                  run before (sort_order_device's d_order_in), so together they are an LSD sort over (chunks, tie, index).  A chunk that is
//                  the same for every name costs its histogram and hands the order on: the shared prefix of read names is cheap
// psvr_sort_order_names (sort.hip) runs it over names from the host, psvr_bam_store_order_names (bam_store.hip) over a store's records.
#include <hip/hip_runtime.h>
#include <vector>
#include "../../include/psvr_engine.h"
#include "common.h"
#include "sort_device.h"
#include "name_key.h"

namespace psvr {

static const uint64_t kNameAddrMask = (1ull << 48) - 1;

__global__ __launch_bounds__(256) void k_name_len(NameSrc src, long long n, uint64_t *nent, uint32_t *ctl)
{
	__shared__ uint32_t wlen[4], wbad[4];
	const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
	uint32_t len = 0, bad = kNameFine;
	if (i < n) {
		const uint8_t *p = src.blob;
		uint32_t tie = 0;
		if (src.rec_addr) {
			const uint8_t *rec = (const uint8_t *)(uintptr_t)src.rec_addr[i];
			p = rec + 36, len = name_len_rec(rec), tie = src.first_read_tie ? (rec[18] & 0x40u ? 0u : 1u) : name_tie_key(rec[18]);   // (signal_mate_device.h: sm_left_tie)
		} else {
			const long long o = src.off[i];
			if (o < 0 || o >= src.n_bytes) bad = kNameNoEnd;
			else {
				const long long room = src.n_bytes - o;
				const uint32_t bound = room > (long long)kNameMaxLen + 1 ? kNameMaxLen + 1 : (uint32_t)room;
				p = src.blob + o, len = name_len(p, bound);
				if (len == bound) bad = bound == kNameMaxLen + 1 ? kNameTooLong : kNameNoEnd, len = 0;
			}
			tie = src.tie ? src.tie[i] : 0u;
		}
		const uint64_t a = (uint64_t)(uintptr_t)p;
		if (a & ~kNameAddrMask) bad = kNameAddress, len = 0;
		nent[i] = (a & kNameAddrMask) | (uint64_t)len << 48 | (uint64_t)(tie & 0xffu) << 56;
	}
#pragma unroll
	for (int o = 32; o; o >>= 1) {
		const uint32_t l2 = (uint32_t)__shfl_xor((int)len, o), b2 = (uint32_t)__shfl_xor((int)bad, o);
		len = l2 > len ? l2 : len, bad = b2 > bad ? b2 : bad;
	}
	if ((threadIdx.x & 63) == 0) wlen[threadIdx.x >> 6] = len, wbad[threadIdx.x >> 6] = bad;
	__syncthreads();
	if (threadIdx.x == 0) {
		for (int w = 1; w < 4; ++w) len = wlen[w] > len ? wlen[w] : len, bad = wbad[w] > bad ? wbad[w] : bad;
		if (len) atomicMax(&ctl[0], len);
		if (bad) atomicMax(&ctl[1], bad);
	}
}

__global__ __launch_bounds__(256) void k_name_chunk(const uint32_t *__restrict__ order, const uint64_t *__restrict__ nent, long long n, int c, uint64_t *__restrict__ key)
{
	const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
	if (i >= n) return;
	const long long j = order ? (long long)order[i] : i;
	uint64_t k = 0;
	if (j < n) {                                                 // (an order is a permutation: always)
		const uint64_t e = nent[j];
		const uint32_t len = (uint32_t)(e >> 48) & 0xffu, at = 8u * (uint32_t)c;
		if (c < 0) k = e >> 56;
		else if (at < len) {
			const uint32_t nbytes = len - at < 8u ? len - at : 8u;
			const uint64_t a = (e & kNameAddrMask) + at;
			const uint32_t r = (uint32_t)a & 7u;
			const uint64_t *w = (const uint64_t *)(uintptr_t)(a - r);
			const uint64_t w0 = w[0], w1 = r + nbytes > 8u ? w[1] : 0ull;   // (the second word only when a byte of the name lies in it)
			k = name_chunk_words(w0, w1, r, nbytes);
		}
	}
	key[i] = k;
}

} // namespace psvr

using namespace psvr;

int psvr::sort_order_names_device(hipStream_t st, long long n, const NameSrc &src, uint64_t *d_keys, NameScratch &N, SortScratch &S, std::vector<uint32_t> &h, const uint32_t **d_order,
                                  const char *who)
{
	*d_order = nullptr;
	N.keys_written = false;
	if (n <= 0) return PSVR_OK;
	// every allocation first -- the entries and the runs' whole scratch -- so that nothing that can fail for want of memory comes behind the
	// first write to d_keys (a store's coordinate keys: psvr_bam_store_order_names)
	if (N.nent.alloc((size_t)n * 8) || N.ctl.alloc(8)) {
		(void)hipGetLastError();
		return set_error(PSVR_ERR_NOMEM, "%s: %zu bytes of device memory needed for the entries of %lld names", who, (size_t)n * 8 + 8, n);
	}
	if (int rc = sort_scratch_reserve(n, S, who)) return rc;
	const unsigned grid = (unsigned)((n + 255) / 256);
	StreamDrain drain{st};                                       // (after the buffers: nothing is in flight when they are freed)
	PSVR_HIP(hipMemsetAsync(N.ctl.p, 0, 8, st));
	hipLaunchKernelGGL(k_name_len, dim3(grid), dim3(256), 0, st, src, n, N.nent.as<uint64_t>(), N.ctl.as<uint32_t>());
	PSVR_HIP(hipGetLastError());
	PSVR_HIP(hipMemcpyAsync(N.h_ctl, N.ctl.p, 8, hipMemcpyDeviceToHost, st));
	PSVR_HIP(hipStreamSynchronize(st));
	if (N.h_ctl[1] == kNameAddress) return set_error(PSVR_ERR_DEVICE, "%s: a name lies at an address of more than 48 bits", who);
	if (N.h_ctl[1] == kNameTooLong) return set_error(PSVR_ERR_UNSUPPORTED, "%s: a name of more than %u bytes", who, kNameMaxLen);
	if (N.h_ctl[1] != kNameFine) return set_error(PSVR_ERR_ARG, "%s: a name begins outside the %lld bytes given or has no NUL before their end", who, src.n_bytes);
	const int C = (int)((N.h_ctl[0] + 7) / 8);                   // at most kNameMaxChunks
	const bool has_tie = src.rec_addr || src.tie;
	const uint32_t *ord = nullptr;
	if (!has_tie && C == 0) { drain.armed = false; return PSVR_OK; }   // every name is empty: the input order stands
	for (int c = has_tie ? -1 : C - 1;;) {
		N.keys_written = true;
		hipLaunchKernelGGL(k_name_chunk, dim3(grid), dim3(256), 0, st, ord, (const uint64_t *)N.nent.p, n, c, d_keys);
		PSVR_HIP(hipGetLastError());
		if (int rc = sort_order_device(st, n, d_keys, S, h, &ord, who, ord)) return rc;
		c = c < 0 ? C - 1 : c - 1;                               // the tie key, then the last chunk down to the first
		if (c < 0) break;
	}
	drain.armed = false;
	*d_order = ord;
	return PSVR_OK;
}
