// bam_store_run.h -- what a psvr_bam_store_t is (bam_store.hip owns and fills it; signal.hip's psvr_signal_run reads the records where they
// lie, through the address table, under the same mutex on the same stream).
#pragma once
#include <memory>
#include <vector>
#include "common.h"
#include "bgzf_members.h"
#include "inflate_layout.h"
#include "sort_device.h"
#include "bam_chain_device.h"

struct psvr_bam_store {
	int device = 0;
	size_t chunk_bytes = 0;                                  // what a fresh chunk holds (a longer append gets a chunk of its own size)
	std::vector<std::unique_ptr<psvr::DevBuf>> chunks;       // the records; the last one is being filled
	psvr::DevBuf addr, meta, key;                            // the table, in append order: uint64 address, psvr_bam_rec_meta_t, uint64 key
	long long cap_rec = 0;
	psvr::DevBuf ctl;                                        // long long: {records, bytes of the last chunk in use, bytes in all, refused, a position outside the key's range}
	long long *h_ctl = nullptr;                              // page-locked read-back of ctl
	long long n_rec = 0, fill = 0, n_bytes = 0;              // the host's copies, exact when `exact`
	long long rec_upper = 0, fill_upper = 0;                 // never below what the device holds
	bool exact = true, key_exact = true, bad = false, keys_spent = false;
	int ordered = 0;                                         // 1: by samtools' coordinate key, 2: by name
	psvr::DevBuf cnt, off, tmp, poff;                        // an append's scratch: records per pair, their scan, the scan's scratch, a host append's offsets
	psvr::SortScratch S;                                     // order
	std::vector<uint32_t> h_hist;
	psvr::DevBuf g_src, smeta, slen, rank_off;               // per sorted rank: address, meta, length, exclusive scan of the lengths (n + 1)
	std::vector<long long> h_rank_off;
	// append_bgzf: the tail lies in the last chunk at [fill, fill + tail); the rest is a call's scratch
	long long tail = 0, seg_bytes = 0;
	psvr_bam_chain_info_t chain = {0, 0, 0, 0, 0};
	psvr::DevBuf zin, zmem, zstatus, cseg, centry, ccnt, cres;
	std::vector<psvr::InfMember> h_mem;                      // (what asynchronous copies touch on the host lives as long as the store)
	std::vector<int32_t> h_status;
	psvr::ChainResult *h_res = nullptr;                      // page-locked, behind h_ctl's entries
	// drop: a released chunk of the standard size, kept for the next st_chunk; the table's other half, which the kept entries slide into
	std::unique_ptr<psvr::DevBuf> spare;
	psvr::DevBuf addr2, meta2, key2;
	long long generation = 0;                                // drops so far: who remembers record indices asks whether they still hold
};

namespace psvr {
// the counts as the device holds them, after a wait when `wait`; an unusable store says so (bam_store.hip).  The caller holds DfwCtx's mutex
int store_refresh(psvr_bam_store *st, DfwCtx &c, bool wait);
} // namespace psvr
