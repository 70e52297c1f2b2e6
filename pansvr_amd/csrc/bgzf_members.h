// bgzf_members.h -- the one device-call scaffold of the wavefront-per-member BGZF encoder, shared by its two entry points:
// psvr_bgzf_compress_members (deflate_wave.hip: the input comes from the host) and psvr_bgzf_stream_take (bgzf_stream.hip: the input lies in
// HBM already).  Both hold DfwCtx's mutex, bind it to their device, queue the same launch sequence on its stream and wait once.
#pragma once
#include <vector>
#include "common.h"

namespace psvr {

struct DfwCtx : DeviceService {
	DevBuf in, slots, tok, link, len, off, tmp, packed;     // (link: the hash chains of efforts 1..3, ensured only by a call that walks them)
	std::vector<long long> h_off;            // what an asynchronous copy writes on the host lives as long as the stream
};
DfwCtx &dfw_ctx();
bool dfw_member_bytes_ok(int32_t mb);
bool dfw_effort_ok(int32_t effort);        // 0..3: deflate_wave_device.h
// makes `device` current and the context its; the caller holds c.mu
int dfw_bind(DfwCtx &c, int device);

struct DfwCall { long long nm = 0, bound = 0; };
// Queues on c.stream, for d_in[0, n_bytes) in the memory of c's device (n_bytes > 0): member kernel at `effort` (0..3) -> scan of the sizes -> pack -> the
// downloads of the offsets and of whatever of the bound fits out[0, out_cap).  No wait: the caller may queue more behind it.
int dfw_members_queue(DfwCtx &c, const uint8_t *d_in, long long n_bytes, uint32_t mb, int effort, void *out, long long out_cap, DfwCall *call);
// The one wait of a call, and its results; `who` names the entry point in an error's text.
int dfw_members_wait(DfwCtx &c, const DfwCall &call, long long out_cap, int64_t *out_bytes, int64_t *member_off, int64_t *n_members, const char *who);

} // namespace psvr
