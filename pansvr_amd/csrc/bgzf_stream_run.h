// bgzf_stream_run.h -- what a psvr_bgzf_stream_t is (bgzf_stream.hip owns it) and the steps of an append, for the one other writer of its pending
// bytes: psvr_bam_store_stream (bam_store.hip) gathers records device to device behind them.  All of it runs under DfwCtx's mutex, on its
// stream, bound to the stream's device (bgzf_members.h).
#pragma once
#include "common.h"
#include "bgzf_members.h"

struct psvr_bgzf_stream {
	int device = 0;
	uint32_t mb = 0;
	int effort = 0;                                          // the encoder's effort of the next take (psvr_bgzf_stream_set_effort)
	psvr::DevBuf pend, ctl;                                  // the pending bytes [0, count); {count, count, bad append} as long long
	long long *h_ctl = nullptr;                              // page-locked: [0..2] read-back of ctl, [3] the count an upload sets
	int cur = 0;                                             // which slot of ctl holds the count
	long long n = 0, upper = 0;                              // the host's copy of the count; never below what the device holds
	bool exact = true;                                       // n is the device's count
	bool bad = false;                                        // an append from an emitter was refused on the device, or a call failed after it had begun to change
	                                                         // the pending bytes: what is pending cannot be trusted any more, and every later call says so
};

namespace psvr {

int bs_bad(const psvr_bgzf_stream *s);                           // PSVR_ERR_DEVICE and the text of an unusable stream
int bs_refresh(psvr_bgzf_stream *s, DfwCtx &c);                  // the count as the device holds it (a wait, when the host does not know it); an unusable stream says so
int bs_room(psvr_bgzf_stream *s, DfwCtx &c, long long need);     // pend holds `need` bytes; what is pending is kept
int bs_set_count(psvr_bgzf_stream *s, DfwCtx &c, long long n);   // queued; the caller waits

} // namespace psvr
