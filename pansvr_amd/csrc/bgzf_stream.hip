// bgzf_stream.hip -- psvr_bgzf_stream_* (include/psvr_engine.h): a BGZF byte stream that lives in HBM, the hand-over between the record
// encoder (bam_emit.hip) and the wavefront-per-member compressor (deflate_wave.hip).  Records encoded on the device are appended device to
// device (k_bs_append), host bytes (the BAM header, chunks the host formatted) are uploaded behind them, and a take compresses the whole
// members that are pending through the same scaffold psvr_bgzf_compress_members runs on (bgzf_members.h: DfwCtx's buffers, its stream of
// the lowest priority, its mutex) and moves the rest, less than a member, to the front: a member always starts at a multiple of
// member_bytes of the stream, so the members are the one-call form's, byte for byte.
//
// The pending count lives on the device in two slots, ctl[0] and ctl[1]; the host knows which one is current.  k_bs_append reads the
// current slot and writes count + length into the other one, which is current from then on: every thread of the launch reads the same
// count whenever its workgroup runs, no atomic is needed, and the call queues without the host having seen either the count or the
// length.  The host's copy of the count (n) is exact unless such an append has been queued since the last read-back.
// Bounds: k_bs_append checks 0 <= pair_off[first] <= pair_off[first + n] <= the run's bytes and count + length <= the capacity before it
// copies anything; a launch that fails the check copies nothing, keeps the count and raises ctl[2]; the next read-back sees it and marks the
// stream unusable (`bad`, kept on the host), as does a call that fails after it began to change the pending bytes: every later call answers
// PSVR_ERR_DEVICE, so no caller can take or recover a stream that lacks bytes it was given.
#include <hip/hip_runtime.h>
#include "../../include/psvr_engine.h"
#include "common.h"
#include "bam_emit_run.h"
#include "bgzf_format.h"
#include "bgzf_members.h"
#include "bgzf_stream_run.h"
#include "copy_aligned_device.h"

namespace psvr {

// bytes[pair_off[first], pair_off[first + n_pairs]) of an emitted run behind the pending bytes (the copy itself: copy_aligned_device.h)
__global__ __launch_bounds__(256) void k_bs_append(const uint8_t *__restrict__ src, long long src_bytes, const long long *__restrict__ pair_off, long long first, long long n_pairs,
                                                   uint8_t *__restrict__ dst, long long dst_cap, long long *ctl, int cur)
{
	const long long s0 = pair_off[first], s1 = pair_off[first + n_pairs], at = ctl[cur];
	const bool ok = s0 >= 0 && s0 <= s1 && s1 <= src_bytes && at >= 0 && at <= dst_cap && s1 - s0 <= dst_cap - at;
	const long long len = ok ? s1 - s0 : 0;
	if (blockIdx.x == 0 && threadIdx.x == 0) {
		ctl[cur ^ 1] = at + len;
		if (!ok) ctl[2] = 1;
	}
	if (len == 0) return;
	copy_aligned_grid(src + s0, dst + at, len);
}

// what follows runs under DfwCtx's mutex, on its stream, bound to the stream's device
int bs_bad(const psvr_bgzf_stream *s)
{
	return set_error(PSVR_ERR_DEVICE, "psvr_bgzf_stream: the stream is unusable: an append from an emitter was out of bounds and was not made, or an earlier call failed while it changed the pending bytes");
}
int bs_refresh(psvr_bgzf_stream *s, DfwCtx &c)      // the count as the device holds it (a wait, when the host does not know it); an unusable stream says so
{
	if (s->bad) return bs_bad(s);
	if (s->exact) return PSVR_OK;
	PSVR_HIP(hipMemcpyAsync(s->h_ctl, s->ctl.p, 3 * 8, hipMemcpyDeviceToHost, c.stream));
	PSVR_HIP(hipStreamSynchronize(c.stream));
	s->n = s->upper = s->h_ctl[s->cur], s->exact = true;
	if (s->h_ctl[2]) { s->bad = true; return bs_bad(s); }
	return PSVR_OK;
}
int bs_set_count(psvr_bgzf_stream *s, DfwCtx &c, long long n)   // queued; the caller waits
{
	s->h_ctl[3] = n;
	PSVR_HIP(hipMemcpyAsync(s->ctl.as<long long>() + s->cur, s->h_ctl + 3, 8, hipMemcpyHostToDevice, c.stream));
	return PSVR_OK;
}
int bs_room(psvr_bgzf_stream *s, DfwCtx &c, long long need)     // pend holds `need` bytes; what is pending is kept
{
	if ((size_t)need <= s->pend.bytes) return PSVR_OK;
	DevBuf bigger;
	if (bigger.alloc((size_t)need + (size_t)need / 2) != hipSuccess) {
		(void)hipGetLastError();
		return set_error(PSVR_ERR_NOMEM, "psvr_bgzf_stream: device allocation failed for %lld pending bytes", need);
	}
	if (s->upper) PSVR_HIP(hipMemcpyAsync(bigger.p, s->pend.p, (size_t)s->upper, hipMemcpyDeviceToDevice, c.stream));
	PSVR_HIP(hipStreamSynchronize(c.stream));
	s->pend.release();
	s->pend.p = bigger.p, s->pend.bytes = bigger.bytes, bigger.p = nullptr, bigger.bytes = 0;
	return PSVR_OK;
}
static int bs_no_device() { return set_error(PSVR_ERR_DEVICE, "no HIP device visible: the engine has no CPU path"); }

} // namespace psvr

using namespace psvr;

extern "C" int psvr_bgzf_stream_create(int device, int32_t member_bytes, psvr_bgzf_stream_t **out)
{
	if (!out || !dfw_member_bytes_ok(member_bytes)) return set_error(PSVR_ERR_ARG, "psvr_bgzf_stream_create: bad argument");
	if (psvr_device_count() <= 0) return bs_no_device();
	DfwCtx &c = dfw_ctx();
	std::lock_guard<std::mutex> lk(c.mu);
	if (int rc = dfw_bind(c, device)) return rc;
	psvr_bgzf_stream *s = new psvr_bgzf_stream;
	s->device = device, s->mb = member_bytes ? (uint32_t)member_bytes : kBgzfBlock;
	hipError_t e = s->ctl.alloc(3 * 8);
	if (e == hipSuccess) e = s->pend.alloc((size_t)s->mb * 4);
	if (e == hipSuccess) e = hipHostMalloc((void **)&s->h_ctl, 4 * sizeof(long long), hipHostMallocDefault);
	if (e == hipSuccess) e = hipMemsetAsync(s->ctl.p, 0, 3 * 8, c.stream);
	if (e == hipSuccess) e = hipStreamSynchronize(c.stream);
	if (e != hipSuccess) {
		if (s->h_ctl) (void)hipHostFree(s->h_ctl);
		delete s;
		return set_error(PSVR_ERR_DEVICE, "psvr_bgzf_stream_create: %s", hipGetErrorString(e));
	}
	*out = s;
	return PSVR_OK;
}

extern "C" void psvr_bgzf_stream_destroy(psvr_bgzf_stream_t *s)
{
	if (!s) return;
	DfwCtx &c = dfw_ctx();
	std::lock_guard<std::mutex> lk(c.mu);
	(void)hipSetDevice(s->device);
	if (c.stream) (void)hipStreamSynchronize(c.stream);      // (an append may still be queued)
	if (s->h_ctl) (void)hipHostFree(s->h_ctl);
	delete s;                                                // (its DevBufs free themselves)
}

extern "C" int psvr_bgzf_stream_set_effort(psvr_bgzf_stream_t *s, int32_t effort)
{
	if (!s || !dfw_effort_ok(effort)) return set_error(PSVR_ERR_ARG, "psvr_bgzf_stream_set_effort: %s", s ? "the effort is outside 0..3" : "null argument");
	DfwCtx &c = dfw_ctx();
	std::lock_guard<std::mutex> lk(c.mu);                    // (a take reads it under the same mutex)
	s->effort = (int)effort;
	return PSVR_OK;
}

extern "C" int psvr_bgzf_stream_append(psvr_bgzf_stream_t *s, const void *bytes, int64_t n_bytes)
{
	if (!s || n_bytes < 0 || (n_bytes > 0 && !bytes)) return set_error(PSVR_ERR_ARG, "psvr_bgzf_stream_append: bad argument");
	if (n_bytes == 0) return PSVR_OK;
	DfwCtx &c = dfw_ctx();
	std::lock_guard<std::mutex> lk(c.mu);
	if (int rc = dfw_bind(c, s->device)) return rc;
	if (int rc = bs_refresh(s, c)) return rc;                // (where the bytes go is the count)
	if (int rc = bs_room(s, c, s->n + n_bytes)) return rc;
	StreamDrain drain{c.stream};
	// (bytes behind the count are not part of the stream: a failure before the count is set leaves it as it was)
	PSVR_HIP(hipMemcpyAsync(s->pend.as<uint8_t>() + s->n, bytes, (size_t)n_bytes, hipMemcpyHostToDevice, c.stream));
	if (int rc = bs_set_count(s, c, s->n + n_bytes)) return rc;
	drain.armed = false;
	if (hipStreamSynchronize(c.stream) != hipSuccess) { s->bad = true; return bs_bad(s); }   // (the count may or may not have arrived); otherwise the caller's bytes are free again
	s->n += n_bytes, s->upper = s->n;
	return PSVR_OK;
}

extern "C" int psvr_bgzf_stream_append_emit(psvr_bgzf_stream_t *s, const psvr_bam_emit_t *em, int64_t first_pair, int64_t n_pairs)
{
	if (!s || !em) return set_error(PSVR_ERR_ARG, "psvr_bgzf_stream_append_emit: null argument");
	if (s->bad) return bs_bad(s);
	if (!em->valid) return set_error(PSVR_ERR_ARG, "psvr_bgzf_stream_append_emit: no emitted run of pairs");
	if (em->device != s->device) return set_error(PSVR_ERR_ARG, "psvr_bgzf_stream_append_emit: the records were encoded on device %d, the stream is on device %d", em->device, s->device);
	if (first_pair < 0 || n_pairs < 0 || first_pair > em->n_pairs || n_pairs > em->n_pairs - first_pair)
		return set_error(PSVR_ERR_ARG, "psvr_bgzf_stream_append_emit: pairs [%lld, %lld) are not in the emitted run (%lld pairs)", (long long)first_pair, (long long)(first_pair + n_pairs), (long long)em->n_pairs);
	if (n_pairs == 0 || em->n_bytes == 0) return PSVR_OK;
	DfwCtx &c = dfw_ctx();
	std::lock_guard<std::mutex> lk(c.mu);
	if (int rc = dfw_bind(c, s->device)) return rc;
	// the range's length is known on the device only: room for the whole run behind the most that can be pending.  Until the next read-back of
	// the count every append_emit adds the run's size to that bound, however short its range: a caller that appends many short ranges of one
	// large run asks `pending` in between (the command does after every piece) or lives with a buffer of ranges x run bytes
	if (int rc = bs_room(s, c, s->upper + em->n_bytes)) return rc;
	const long long nv = (long long)em->n_bytes / 16 + 1;
	const unsigned grid = (unsigned)(nv / 256 + 1 < 2048 ? nv / 256 + 1 : 2048);
	hipLaunchKernelGGL(k_bs_append, dim3(grid), dim3(256), 0, c.stream, em->bytes.as<uint8_t>(), (long long)em->n_bytes, (const long long *)em->pair_off.p, (long long)first_pair,
	                   (long long)n_pairs, s->pend.as<uint8_t>(), (long long)s->pend.bytes, s->ctl.as<long long>(), s->cur);
	PSVR_HIP(hipGetLastError());
	s->cur ^= 1, s->upper += em->n_bytes, s->exact = false;
	return PSVR_OK;
}

extern "C" int64_t psvr_bgzf_stream_pending(psvr_bgzf_stream_t *s)
{
	if (!s) return -(int64_t)set_error(PSVR_ERR_ARG, "psvr_bgzf_stream_pending: null argument");
	DfwCtx &c = dfw_ctx();
	std::lock_guard<std::mutex> lk(c.mu);
	if (int rc = dfw_bind(c, s->device)) return -(int64_t)rc;
	if (s->bad) return -(int64_t)bs_bad(s);
	if (s->exact) {                                          // (the promise to an emitter's owner -- what was appended from it has been read -- is a wait all the same)
		if (hipStreamSynchronize(c.stream) != hipSuccess) return -(int64_t)set_error(PSVR_ERR_DEVICE, "psvr_bgzf_stream_pending: the stream's work failed");
		return s->n;
	}
	if (int rc = bs_refresh(s, c)) return -(int64_t)rc;
	return s->n;
}

extern "C" int psvr_bgzf_stream_take(psvr_bgzf_stream_t *s, int finish, void *out, int64_t out_cap, int64_t *out_bytes, int64_t *member_off, int64_t member_cap, int64_t *n_members,
                                     int64_t *in_bytes)
{
	if (!s || !out_bytes || out_cap < 0 || (out_cap > 0 && !out) || (member_off && member_cap < 0)) return set_error(PSVR_ERR_ARG, "psvr_bgzf_stream_take: bad argument");
	*out_bytes = 0;
	if (n_members) *n_members = 0;
	if (in_bytes) *in_bytes = 0;
	if (member_off) member_off[0] = 0;
	DfwCtx &c = dfw_ctx();
	std::lock_guard<std::mutex> lk(c.mu);
	if (int rc = dfw_bind(c, s->device)) return rc;
	if (int rc = bs_refresh(s, c)) return rc;
	const long long mb = s->mb, whole = finish ? s->n : s->n / mb * mb, nm = (whole + mb - 1) / mb, rest = s->n - whole;
	const long long bound = s->n ? bgzf_members_max(s->n, mb) : 0;
	if (out_cap < bound) return set_error(PSVR_ERR_OVERFLOW, "psvr_bgzf_stream_take: %lld bytes are pending, their members may take %lld bytes, have %lld", s->n, bound, (long long)out_cap);
	if (member_off && nm > member_cap) return set_error(PSVR_ERR_OVERFLOW, "psvr_bgzf_stream_take: %lld members, room for %lld offsets", nm, (long long)member_cap);
	if (whole == 0) return PSVR_OK;
	StreamDrain drain{c.stream};
	DfwCall call;
	if (int rc = dfw_members_queue(c, s->pend.as<uint8_t>(), whole, (uint32_t)mb, s->effort, out, (long long)out_cap, &call)) return rc;
	// behind the members: what is left, less than a member, to the front (whole >= mb > rest: the two ranges do not overlap), and its count.
	// From the first of the two on the pending bytes change: a failure then leaves a stream whose bytes nobody may take for good ones
	hipError_t e = rest ? hipMemcpyAsync(s->pend.p, s->pend.as<uint8_t>() + whole, (size_t)rest, hipMemcpyDeviceToDevice, c.stream) : hipSuccess;
	int rc = e == hipSuccess ? bs_set_count(s, c, rest) : set_error(PSVR_ERR_DEVICE, "psvr_bgzf_stream_take: %s", hipGetErrorString(e));
	if (!rc) {
		drain.armed = false;
		rc = dfw_members_wait(c, call, (long long)out_cap, out_bytes, member_off, n_members, "psvr_bgzf_stream_take");
	}
	if (rc) { s->bad = true; return rc; }                  // (out_cap holds the bound: no overflow is left to report here)
	s->n = s->upper = rest;
	if (in_bytes) *in_bytes = whole;
	return PSVR_OK;
}

extern "C" int psvr_bgzf_stream_recover(psvr_bgzf_stream_t *s, void *bytes, int64_t cap, int64_t *n_bytes)
{
	if (!s || !n_bytes || cap < 0 || (cap > 0 && !bytes)) return set_error(PSVR_ERR_ARG, "psvr_bgzf_stream_recover: bad argument");
	*n_bytes = 0;
	DfwCtx &c = dfw_ctx();
	std::lock_guard<std::mutex> lk(c.mu);
	if (int rc = dfw_bind(c, s->device)) return rc;
	if (int rc = bs_refresh(s, c)) return rc;
	*n_bytes = s->n;
	if (cap < s->n) return set_error(PSVR_ERR_OVERFLOW, "psvr_bgzf_stream_recover: %lld bytes are pending, the buffer has %lld", s->n, (long long)cap);
	StreamDrain drain{c.stream};
	if (s->n) PSVR_HIP(hipMemcpyAsync(bytes, s->pend.p, (size_t)s->n, hipMemcpyDeviceToHost, c.stream));
	if (int rc = bs_set_count(s, c, 0)) return rc;
	drain.armed = false;
	if (hipStreamSynchronize(c.stream) != hipSuccess) { s->bad = true; return bs_bad(s); }
	s->n = s->upper = 0;
	return PSVR_OK;
}
