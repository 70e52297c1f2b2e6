// bam_emit_run.h -- what a psvr_bam_emit_t is: the device buffers of one emitted run of pairs (bam_emit.hip fills them, bgzf_stream.hip's
// psvr_bgzf_stream_append_emit reads bytes and pair_off device to device).
#pragma once
#include "common.h"
#include "bam_emit_device.h"

struct psvr_bam_emit {
	int device = 0;
	hipStream_t stream = nullptr;
	psvr::BeTables T = {nullptr, nullptr, nullptr, 0, 0};
	psvr::DevBuf hdr, pairs, cands, cig;                     // psvr_bam_emit_results: the caller's arrays
	psvr::DevBuf cnt, pair_off, state, bytes, tmp, counters;
	long long *h_back = nullptr;                             // page-locked: {bytes, records, written pairs, declined pairs} of a run
	int64_t n_pairs = 0, n_bytes = 0;
	bool valid = false;
};
