// inflate.hip -- BGZF members inflated on the device: psvr_bgzf_decompress (include/psvr_engine.h), the counterpart of bgzf.hip.  The
// reference reads its BAM through htslib, whose bgzf_read_block inflates one member at a time with zlib on the calling thread
// (htslib bgzf.c); members are independent and carry their compressed and inflated sizes in the clear, so the host lays a batch out from
// the BSIZE / ISIZE fields alone and ONE WAVEFRONT PER MEMBER decodes it (inflate_device.h), CRC32 and ISIZE checked on the device.
#include <hip/hip_runtime.h>
#include <vector>
#include "../../include/psvr_engine.h"
#include "common.h"
#include "inflate_device.h"
#include "inflate_layout.h"

namespace psvr {

__global__ __launch_bounds__(64) void k_bgzf_inflate(const uint8_t *__restrict__ in, const InfMember *__restrict__ mem, uint8_t *out, int32_t *status)
{
	__shared__ InfLds lds;
	const InfMember m = mem[blockIdx.x];
	const int rc = inf_member<64>(in + m.in_off, m.bsize, m.hdr, out + m.out_off, m.isize, &lds, (int)threadIdx.x);
	if (threadIdx.x == 0) status[blockIdx.x] = rc;
}

struct InflateCtx : DeviceService {
	DevBuf in, out, mem, status;
	std::vector<InfMember> h_mem;        // what asynchronous copies read and write on the host lives as long as the stream
	std::vector<int32_t> h_status;
};
static InflateCtx &inflate_ctx() { static InflateCtx c; return c; }

} // namespace psvr

using namespace psvr;

extern "C" int psvr_bgzf_decompress(int device, const void *in_, int64_t n_bytes, int64_t *in_used, void *out, int64_t out_cap, int64_t *out_bytes,
                                    int64_t *member_off, int64_t member_cap, int64_t *n_members, int64_t *bad_member)
{
	if (!in_ || n_bytes < 0 || !in_used || !out_bytes || (out && out_cap < 0) || (member_off && member_cap < 0)) return set_error(PSVR_ERR_ARG, "psvr_bgzf_decompress: bad argument");
	const uint8_t *in = (const uint8_t *)in_;
	*in_used = 0, *out_bytes = 0;
	if (n_members) *n_members = 0;
	if (bad_member) *bad_member = -1;
	// the BSIZE chain: whole members only; a header that is no BGZF header (or an ISIZE its payload cannot reach) ends it as the bad member
	std::vector<InfMember> mem;
	long long at = 0, total = 0;
	const long long bad = inf_layout(in, n_bytes, mem, &at, &total);
	const long long nm = (long long)mem.size();
	*in_used = at, *out_bytes = total;
	if (n_members) *n_members = nm;
	if (member_off) {
		if (nm > member_cap) return set_error(PSVR_ERR_OVERFLOW, "psvr_bgzf_decompress: %lld members, room for %lld offsets", nm, (long long)member_cap);
		for (long long i = 0; i < nm; ++i) member_off[i] = mem[(size_t)i].out_off;
		member_off[nm] = total;
	}
	auto io_error = [&](long long m, int status) {
		if (bad_member) *bad_member = m;
		return set_error(PSVR_ERR_IO, "psvr_bgzf_decompress: corrupt BGZF block: member %lld at byte %lld (status %d)", m, m < nm ? mem[(size_t)m].in_off : at, status);
	};
	if (!out) return bad >= 0 ? io_error(bad, kInfHeader) : PSVR_OK;
	if (total > out_cap) return set_error(PSVR_ERR_OVERFLOW, "psvr_bgzf_decompress: need %lld bytes, have %lld", total, (long long)out_cap);
	if (nm == 0) return bad >= 0 ? io_error(bad, kInfHeader) : PSVR_OK;
	if (psvr_device_count() <= 0) return set_error(PSVR_ERR_DEVICE, "no HIP device visible: the engine has no CPU path");
	InflateCtx &c = inflate_ctx();
	std::lock_guard<std::mutex> lk(c.mu);
	if (int rc = c.bind(device, false, [&] { c.in.release(), c.out.release(), c.mem.release(), c.status.release(); })) return rc;
	c.h_mem = mem, c.h_status.assign((size_t)nm, -1);
	PSVR_HIP(c.in.ensure((size_t)at));
	PSVR_HIP(c.out.ensure((size_t)total));
	PSVR_HIP(c.mem.ensure((size_t)nm * sizeof(InfMember)));
	PSVR_HIP(c.status.ensure((size_t)nm * 4));
	StreamDrain drain{c.stream};
	PSVR_HIP(hipMemcpyAsync(c.in.p, in, (size_t)at, hipMemcpyHostToDevice, c.stream));
	PSVR_HIP(hipMemcpyAsync(c.mem.p, c.h_mem.data(), (size_t)nm * sizeof(InfMember), hipMemcpyHostToDevice, c.stream));
	hipLaunchKernelGGL(k_bgzf_inflate, dim3((unsigned)nm), dim3(64), 0, c.stream, c.in.as<uint8_t>(), c.mem.as<InfMember>(), c.out.as<uint8_t>(), c.status.as<int32_t>());
	PSVR_HIP(hipGetLastError());
	std::vector<int32_t> &status = c.h_status;
	PSVR_HIP(hipMemcpyAsync(status.data(), c.status.p, (size_t)nm * 4, hipMemcpyDeviceToHost, c.stream));
	if (total) PSVR_HIP(hipMemcpyAsync(out, c.out.p, (size_t)total, hipMemcpyDeviceToHost, c.stream));
	drain.armed = false;
	PSVR_HIP(hipStreamSynchronize(c.stream));
	for (long long i = 0; i < nm; ++i) if (status[(size_t)i] != kInfOk) return io_error(i, status[(size_t)i]);
	return bad >= 0 ? io_error(bad, kInfHeader) : PSVR_OK;
}
