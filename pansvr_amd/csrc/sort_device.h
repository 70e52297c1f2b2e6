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
// d_order_in: the order the keys come in (d_keys[i] is the key of record d_order_in[i]): nullptr for the identity, or what an earlier run
// over the same S gave.  The run is stable, so it refines that order; when every key is equal *d_order is d_order_in itself.
int sort_order_device(hipStream_t st, long long n, uint64_t *d_keys, SortScratch &S, std::vector<uint32_t> &h, const uint32_t **d_order, const char *who,
                      const uint32_t *d_order_in = nullptr);
// The scratch a sort of n keys needs, allocated in S where S does not hold it yet (sort_order_device asks itself; a caller that must know that
// the memory is there before it writes its keys asks first).  Nothing is launched.  PSVR_ERR_NOMEM with the byte count.
int sort_scratch_reserve(long long n, SortScratch &S, const char *who);

// Name order (name_sort.hip; the rules are name_key.h's): the names compared as strcmp compares them, then the tie key, then the index.
// Where the names are: records of a store (rec_addr[i] = the record's address, the name at +36 inside l_read_name bytes, the tie key from
// its flag), or a blob (name i at blob + off[i], ending before blob + n_bytes; tie[i] or, with tie == nullptr, nothing).  The records' tie key is the
// caller's choice: name_tie_key for everyone but SignalStep's by-name pass over its left-overs, which has records with 0x40 first.
struct NameSrc {
	const uint64_t *rec_addr;
	const uint8_t *blob;
	long long n_bytes;
	const long long *off;
	const uint8_t *tie;
	int first_read_tie;                                           // records: the tie key is !(flag & 0x40) (SignalStep's by-name pass) instead of name_tie_key's flag & 0xc0
};
struct NameScratch {                                              // 8 bytes per name: address | length << 48 | tie key << 56
	DevBuf nent, ctl;
	uint32_t h_ctl[2] = {0, 0};                                   // the longest name, the refusal (what an asynchronous copy writes lives as long as the call)
	bool keys_written = false;                                    // a launch that writes d_keys has been queued: until then a failed call has left d_keys as they were
	void release() { nent.release(), ctl.release(); }
};
enum { kNameFine = 0, kNameNoEnd = 1, kNameTooLong = 2, kNameAddress = 3 };   // NameScratch::h_ctl[1]
// Queues on `st` the name order of n names (0 < n < 2^32): a run of sort_order_device for the tie key, then one per 8-byte chunk of the
// longest name, last chunk first; d_keys (n keys) and S are those runs'.  Waits once for the lengths and once per run.  PSVR_ERR_ARG: a
// blob name without a NUL before the blob's end or an offset outside it; PSVR_ERR_UNSUPPORTED: a blob name of more than 254 bytes; nothing
// has been sorted then.  Every allocation (the entries, the runs' whole scratch) and the lengths' check come before the first launch that
// writes d_keys: a call that fails with N.keys_written still false has not touched them.  *d_order as sort_order_device's.
int sort_order_names_device(hipStream_t st, long long n, const NameSrc &src, uint64_t *d_keys, NameScratch &N, SortScratch &S, std::vector<uint32_t> &h, const uint32_t **d_order,
                            const char *who);

} // namespace psvr
