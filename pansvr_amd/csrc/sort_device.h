// sort_device.h -- the radix sort of sort.hip over device pointers, shared by its two callers: psvr_sort_order_u64 (keys from the host) and
// psvr_bam_store_order (bam_store.hip: the keys of a record store lie in HBM already).
#pragma once
#include <vector>
#include "common.h"

namespace psvr {

struct SortScratch {                                              // about 16 bytes per key; *d_order points into it
	DevBuf k1, i0, i1, cnt, off, tmp, slab, hist;
	void release() { k1.release(), i0.release(), i1.release(), cnt.release(), off.release(), tmp.release(), slab.release(), hist.release(); }
};

// Queues on `st` the stable order of d_keys[0, n) (0 < n < 2^32, memory of st's device); the keys are sorted where they lie (d_keys and
// S.k1 are the two sides of the ping-pong, so d_keys' content is unspecified afterwards).  One wait inside (the digit histograms come back
// to `h`, which must live as long as the stream); the caller waits for the rest.  *d_order: n indices in S, or nullptr when every key is
// equal and the input order stands.  `who` names the entry point in an error's text.
int sort_order_device(hipStream_t st, long long n, uint64_t *d_keys, SortScratch &S, std::vector<uint32_t> &h, const uint32_t **d_order, const char *who);

} // namespace psvr
