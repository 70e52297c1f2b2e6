// deflate_wave.hip -- BGZF members compressed on the device, ONE WAVEFRONT PER MEMBER: psvr_bgzf_compress_members (include/psvr_engine.h).
// The reference writes its BAM through htslib, whose bgzf_compress deflates 0xff00-byte blocks with zlib on a host thread (htslib bgzf.c:
// bgzf_write -> bgzf_flush -> bgzf_compress).  bgzf.hip's k_bgzf_deflate gives a block to one lane, and a call lasts as long as one lane
// needs; here a member's 64 KB are shared by the 64 lanes (deflate_wave_device.h), the member sizes become offsets on the device (scan.h)
// and a pack launch lays the members side by side, so that nothing returns to the host between compressing and packing.
#include <hip/hip_runtime.h>
#include <vector>
#include "../../include/psvr_engine.h"
#include "common.h"
#include "bgzf_members.h"
#include "deflate_wave_device.h"
#include "scan.h"

namespace psvr {

// link: tok_stride half-words per member at efforts 1..3 (the chains of deflate_wave_device.h), not touched at effort 0
template <int EFFORT>
__global__ __launch_bounds__(64) void k_bgzf_deflate_wave(const uint8_t *__restrict__ in, long long n_bytes, uint32_t mb, uint8_t *slots, uint32_t slot, uint32_t *tok,
                                                          uint32_t tok_stride, uint16_t *link, int32_t *len)
{
	__shared__ DfwLds lds;
	const long long b = blockIdx.x, at = b * (long long)mb;
	const uint32_t n = (uint32_t)(n_bytes - at < (long long)mb ? n_bytes - at : (long long)mb);
	uint16_t *lk = EFFORT ? link + b * (long long)tok_stride : nullptr;
	const uint32_t size = dfw_member_effort<64, EFFORT>(in + at, n, slots + b * (long long)slot, tok + b * (long long)tok_stride, lk, &lds, (int)threadIdx.x);
	if (threadIdx.x == 0) len[b] = (int32_t)size;
}
// the members side by side: a workgroup per member, whole dwords once the destination is aligned
__global__ __launch_bounds__(256) void k_bgzf_pack_members(const uint8_t *__restrict__ slots, uint32_t slot, const int32_t *__restrict__ len, const long long *__restrict__ off,
                                                           uint8_t *__restrict__ packed)
{
	const long long b = blockIdx.x;
	const uint8_t *s = slots + b * (long long)slot;
	uint8_t *d = packed + off[b];
	const uint32_t n = (uint32_t)len[b];
	uint32_t lead = (uint32_t)(-(intptr_t)d) & 3u;
	if (lead > n) lead = n;
	const uint32_t nw = (n - lead) / 4u, done = lead + 4u * nw;
	if (threadIdx.x < lead) d[threadIdx.x] = s[threadIdx.x];
	for (uint32_t w = threadIdx.x; w < nw; w += 256) {
		uint32_t v;
		__builtin_memcpy(&v, s + lead + 4u * w, 4);
		*(uint32_t *)(d + lead + 4u * w) = v;
	}
	if (threadIdx.x < n - done) d[done + threadIdx.x] = s[done + threadIdx.x];
}

DfwCtx &dfw_ctx() { static DfwCtx c; return c; }

bool dfw_member_bytes_ok(int32_t mb) { return mb == 0 || (mb >= 256 && mb <= (int32_t)kDfMaxIn); }
bool dfw_effort_ok(int32_t effort) { return effort >= 0 && effort <= kDfwMaxEffort; }

int dfw_bind(DfwCtx &c, int device)
{
	// (a device-resident stream may have work queued on the stream that a change of device is about to destroy: it is waited for first)
	return c.bind(device, true, [&] {
		if (c.stream) (void)hipStreamSynchronize(c.stream);
		c.in.release(), c.slots.release(), c.tok.release(), c.link.release(), c.len.release(), c.off.release(), c.tmp.release(), c.packed.release();
	});
}

int dfw_members_queue(DfwCtx &c, const uint8_t *d_in, long long n_bytes, uint32_t mb, int effort, void *out, long long out_cap, DfwCall *call)
{
	const long long nm = (n_bytes + mb - 1) / mb;
	const uint32_t slot = dfw_slot_bytes(mb), tok_stride = (mb + 1u + 63u) & ~63u;         // (words: a token per input byte at most, and the end of block)
	const long long bound = bgzf_members_max(n_bytes, mb);
	call->nm = nm, call->bound = bound;
	PSVR_HIP(c.slots.ensure((size_t)nm * slot));
	PSVR_HIP(c.tok.ensure((size_t)nm * tok_stride * 4));
	if (effort > 0) PSVR_HIP(c.link.ensure((size_t)nm * tok_stride * 2));                  // (the chains: only a call that walks them pays for them)
	PSVR_HIP(c.len.ensure((size_t)(nm + 1) * 4));
	PSVR_HIP(c.off.ensure((size_t)(nm + 1) * 8));
	PSVR_HIP(c.tmp.ensure(scan_tmp_bytes(1, nm + 1)));
	PSVR_HIP(c.packed.ensure((size_t)bound));
	c.h_off.assign((size_t)nm + 1, 0);
	PSVR_HIP(hipMemsetAsync(c.len.as<int32_t>() + nm, 0, 4, c.stream));                     // (the scan runs over nm + 1 sizes: its last offset is the total)
	auto launch = [&](auto kernel) {
		hipLaunchKernelGGL(kernel, dim3((unsigned)nm), dim3(64), 0, c.stream, d_in, n_bytes, mb, c.slots.as<uint8_t>(), slot, c.tok.as<uint32_t>(), tok_stride,
		                   effort > 0 ? c.link.as<uint16_t>() : (uint16_t *)nullptr, c.len.as<int32_t>());
	};
	switch (effort) {
	case 0: launch(k_bgzf_deflate_wave<0>); break;
	case 1: launch(k_bgzf_deflate_wave<1>); break;
	case 2: launch(k_bgzf_deflate_wave<2>); break;
	case 3: launch(k_bgzf_deflate_wave<3>); break;
	default: return set_error(PSVR_ERR_ARG, "BGZF members: effort %d is outside 0..%d", effort, kDfwMaxEffort);
	}
	PSVR_HIP(hipGetLastError());
	ScanSet S = {};
	S.cnt[0] = c.len.as<int32_t>(), S.out[0] = c.off.as<long long>(), S.stride[0] = 1, S.off[0] = 0, S.base[0] = 0;
	scan_launch(S, 1, nm + 1, c.tmp.as<long long>(), c.stream);
	PSVR_HIP(hipGetLastError());
	hipLaunchKernelGGL(k_bgzf_pack_members, dim3((unsigned)nm), dim3(256), 0, c.stream, c.slots.as<uint8_t>(), slot, c.len.as<int32_t>(), c.off.as<long long>(), c.packed.as<uint8_t>());
	PSVR_HIP(hipGetLastError());
	// One download, one wait: the total is known only on the device, so whatever of the bound fits `out` comes back with the offsets, and what
	// lies behind the total is not part of the result.  (The alternative, a wait for the offsets and a second one for exactly the bytes,
	// moves fewer bytes and costs a second wake-up; tools/deflate_bench.py measures the call as it is.)
	const long long take = bound < out_cap ? bound : out_cap;
	PSVR_HIP(hipMemcpyAsync(c.h_off.data(), c.off.p, (size_t)(nm + 1) * 8, hipMemcpyDeviceToHost, c.stream));
	if (take) PSVR_HIP(hipMemcpyAsync(out, c.packed.p, (size_t)take, hipMemcpyDeviceToHost, c.stream));
	return PSVR_OK;
}

int dfw_members_wait(DfwCtx &c, const DfwCall &call, long long out_cap, int64_t *out_bytes, int64_t *member_off, int64_t *n_members, const char *who)
{
	PSVR_HIP(hipStreamSynchronize(c.stream));
	const long long nm = call.nm, total = c.h_off[(size_t)nm];
	if (n_members) *n_members = nm;
	*out_bytes = total;
	if (member_off) for (long long i = 0; i <= nm; ++i) member_off[i] = c.h_off[(size_t)i];
	if (total > out_cap) return set_error(PSVR_ERR_OVERFLOW, "%s: need %lld bytes, have %lld", who, total, out_cap);
	return PSVR_OK;
}

} // namespace psvr

using namespace psvr;

extern "C" int64_t psvr_bgzf_members_bound(int64_t n_bytes, int32_t member_bytes)
{
	if (n_bytes <= 0 || !dfw_member_bytes_ok(member_bytes)) return 0;
	const int64_t mb = member_bytes ? member_bytes : (int64_t)kDfMaxIn;
	return bgzf_members_max(n_bytes, mb);
}

extern "C" int psvr_bgzf_compress_members(int device, const void *in, int64_t n_bytes, int32_t member_bytes, void *out, int64_t out_cap, int64_t *out_bytes,
                                          int64_t *member_off, int64_t member_cap, int64_t *n_members)
{
	return psvr_bgzf_compress_members_effort(device, in, n_bytes, member_bytes, out, out_cap, out_bytes, member_off, member_cap, n_members, 0);
}

extern "C" int psvr_bgzf_compress_members_effort(int device, const void *in, int64_t n_bytes, int32_t member_bytes, void *out, int64_t out_cap, int64_t *out_bytes,
                                                 int64_t *member_off, int64_t member_cap, int64_t *n_members, int32_t effort)
{
	if (!dfw_effort_ok(effort)) return set_error(PSVR_ERR_ARG, "psvr_bgzf_compress_members: effort %d is outside 0..%d", (int)effort, kDfwMaxEffort);
	if (n_bytes < 0 || (n_bytes > 0 && (!in || !out)) || !out_bytes || out_cap < 0 || !dfw_member_bytes_ok(member_bytes) || (member_off && member_cap < 0))
		return set_error(PSVR_ERR_ARG, "psvr_bgzf_compress_members: bad argument");
	*out_bytes = 0;
	if (n_members) *n_members = 0;
	if (member_off) member_off[0] = 0;
	if (n_bytes == 0) return PSVR_OK;
	const uint32_t mb = member_bytes ? (uint32_t)member_bytes : kDfMaxIn;
	const long long nm = (n_bytes + mb - 1) / mb;
	if (member_off && nm > member_cap) return set_error(PSVR_ERR_OVERFLOW, "psvr_bgzf_compress_members: %lld members, room for %lld offsets", nm, (long long)member_cap);
	if (psvr_device_count() <= 0) return set_error(PSVR_ERR_DEVICE, "no HIP device visible: the engine has no CPU path");
	DfwCtx &c = dfw_ctx();
	std::lock_guard<std::mutex> lk(c.mu);
	if (int rc = dfw_bind(c, device)) return rc;
	PSVR_HIP(c.in.ensure((size_t)n_bytes));
	StreamDrain drain{c.stream};
	PSVR_HIP(hipMemcpyAsync(c.in.p, in, (size_t)n_bytes, hipMemcpyHostToDevice, c.stream));   // the upload is this entry point's; the rest is the shared scaffold
	DfwCall call;
	if (int rc = dfw_members_queue(c, c.in.as<uint8_t>(), (long long)n_bytes, mb, (int)effort, out, (long long)out_cap, &call)) return rc;
	drain.armed = false;
	return dfw_members_wait(c, call, (long long)out_cap, out_bytes, member_off, n_members, "psvr_bgzf_compress_members");
}
