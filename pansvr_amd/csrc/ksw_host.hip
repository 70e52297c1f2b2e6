// ksw_host.hip -- host side of seam B2 (psvr_extd2_batch / psvr_dp_plan_*): parameter
// checks, uploads and kernel launches.  The parameter preparation and the planning itself are dp_plan.h's (plain host arithmetic).
#include <hip/hip_runtime.h>
#include <cstdlib>
#include <algorithm>
#include <string>
#include <vector>
#include "common.h"
#include "ksw_device.h"
#include "ksw_launch.h"

namespace psvr {

std::string &last_error_ref()
{
	static thread_local std::string s;
	return s;
}

// make_dp_params with its one failure as the last error (the engine's dp_init calls this too)
int dp_params(const psvr_ksw_params_t *par, int variant, DpParams *P)
{
	if (!make_dp_params(par, variant, P)) return set_error(PSVR_ERR_UNSUPPORTED, "alphabet size m=%d (supported: 0..5)", par->m);
	return PSVR_OK;
}

} // namespace psvr

using namespace psvr;

struct psvr_dp_plan {
	int device = 0, variant = 0;
	int64_t n = 0;
	DpParams P;
	std::vector<DpLaunch> launches;
	DevBuf d_idx, d_poff, d_qlen, d_tlen, d_wstop;
	int64_t pslab_bytes = 0, ws_bytes = 0;    // direction-byte slab, then (256-aligned) the strip kernel's scratch
	std::string desc;
};

extern "C" const char *psvr_last_error(void) { return last_error_ref().c_str(); }
extern "C" void *psvr_host_alloc(size_t bytes)
{
	void *p = nullptr;
	hipError_t e = hipHostMalloc(&p, bytes ? bytes : 16, hipHostMallocPortable);   // page-locked for every device of the process
	if (e != hipSuccess) { set_error(PSVR_ERR_NOMEM, "psvr_host_alloc(%zu): %s", bytes, hipGetErrorString(e)); return nullptr; }
	return p;
}
extern "C" void psvr_host_free(void *p) { if (p) (void)hipHostFree(p); }

extern "C" int psvr_device_count(void)
{
	int n = 0;
	if (hipGetDeviceCount(&n) != hipSuccess) { set_error(PSVR_ERR_DEVICE, "hipGetDeviceCount failed"); return -1; }
	return n;
}

extern "C" int psvr_dp_plan_create(int device, int64_t n, const int32_t *qlen, const int32_t *tlen,
                                   const psvr_ksw_params_t *par, int variant, psvr_dp_plan_t **out)
{
	if (!out || !par || n < 0 || (n > 0 && (!qlen || !tlen)) || (variant != 0 && variant != 1))
		return set_error(PSVR_ERR_ARG, "psvr_dp_plan_create: bad argument");
	*out = nullptr;
	psvr_dp_plan *pl = new psvr_dp_plan;
	pl->device = device, pl->variant = variant, pl->n = n;
	struct Guard { psvr_dp_plan *p; ~Guard() { delete p; } } guard{pl};
	int rc = dp_params(par, variant, &pl->P);
	if (rc) return rc;
	for (int64_t i = 0; i < n; ++i)
		if (qlen[i] >= kDpMaxSeqLen || tlen[i] >= kDpMaxSeqLen)
			return set_error(PSVR_ERR_UNSUPPORTED, "problem %lld: qlen=%d tlen=%d: sequences of 2^28 bases or more are not supported", (long long)i, qlen[i], tlen[i]);
	const DpHostPlan hp = dp_plan_host(n, qlen, tlen, pl->P, variant);
	pl->pslab_bytes = hp.slab_bytes, pl->ws_bytes = hp.ws_bytes;
	pl->launches = hp.launches;
	for (const DpLaunch &L : pl->launches) {     // (the order they go out in; the team kernel's classes as one launch, last)
		char buf[160];
		snprintf(buf, sizeof buf, "%s[lds=%d] x%lld; ", dp_kind_name(L.kind, variant), dp_lds_class_bytes(L.cls), (long long)L.count);
		pl->desc += buf;
	}
	{
		hipError_t he = hipSetDevice(device);
		if (he != hipSuccess) return set_error(PSVR_ERR_DEVICE, "hipSetDevice(%d) failed: %s", device, hipGetErrorString(he));
	}
	PSVR_HIP(pl->d_idx.alloc(n * 4));
	PSVR_HIP(pl->d_poff.alloc(n * 8));
	PSVR_HIP(pl->d_qlen.alloc(n * 4));
	PSVR_HIP(pl->d_tlen.alloc(n * 4));
	PSVR_HIP(pl->d_wstop.alloc(16));      // the error flag (4 B, at offset 8)
	if (n) {
		PSVR_HIP(hipMemcpy(pl->d_idx.p, hp.idx.data(), n * 4, hipMemcpyHostToDevice));
		PSVR_HIP(hipMemcpy(pl->d_poff.p, hp.poff.data(), n * 8, hipMemcpyHostToDevice));
		PSVR_HIP(hipMemcpy(pl->d_qlen.p, qlen, n * 4, hipMemcpyHostToDevice));
		PSVR_HIP(hipMemcpy(pl->d_tlen.p, tlen, n * 4, hipMemcpyHostToDevice));
	}
	PSVR_HIP(dp_allow_big_lds());
	guard.p = nullptr;
	*out = pl;
	return PSVR_OK;
}

extern "C" int64_t psvr_dp_plan_workspace_bytes(const psvr_dp_plan_t *pl) { return pl ? ((pl->pslab_bytes + 255) & ~(int64_t)255) + pl->ws_bytes + 256 : 0; }

extern "C" int psvr_dp_plan_describe(const psvr_dp_plan_t *pl, char *buf, size_t buflen)
{
	if (!pl || !buf || !buflen) return set_error(PSVR_ERR_ARG, "psvr_dp_plan_describe: bad argument");
	snprintf(buf, buflen, "%s", pl->desc.c_str());
	return PSVR_OK;
}

extern "C" void psvr_dp_plan_destroy(psvr_dp_plan_t *pl) { delete pl; }

extern "C" int psvr_dp_regime(const psvr_ksw_params_t *par, int variant, psvr_dp_regime_t *out)
{
	if (!par || !out || (variant != 0 && variant != 1)) return set_error(PSVR_ERR_ARG, "psvr_dp_regime: bad argument");
	DpParams P;
	int rc = dp_params(par, variant, &P);
	if (rc) return rc;
	out->skip = P.skip, out->nowrap_ok = P.nowrap_ok, out->long_thres = P.long_thres;
	out->swapped = variant == 0 && !P.skip && par->q2 + par->e2 < par->q + par->e;
	out->qe_shift = P.skip ? 0 : P.qe_pre - (P.q + P.e);
	out->zdrop_inert = variant == 0 && !P.skip && dp_zdrop_inert(P);
	return PSVR_OK;
}

extern "C" int psvr_dp_plan_launch(psvr_dp_plan_t *pl, const uint8_t *d_qseq, const int64_t *d_q_off,
                                   const uint8_t *d_tseq, const int64_t *d_t_off,
                                   psvr_extz_t *d_ez, uint32_t *d_cigar, void *d_work, void *stream_)
{
	if (!pl) return set_error(PSVR_ERR_ARG, "psvr_dp_plan_launch: null plan");
	if (pl->n == 0) return PSVR_OK;
	if (!d_qseq || !d_q_off || !d_tseq || !d_t_off || !d_ez || !d_cigar || ((pl->pslab_bytes || pl->ws_bytes) && !d_work))
		return set_error(PSVR_ERR_ARG, "psvr_dp_plan_launch: null device pointer");
	hipStream_t stream = (hipStream_t)stream_;
	DpBatch B;
	B.qseq = d_qseq, B.q_off = d_q_off, B.qlen = pl->d_qlen.as<int32_t>();
	B.tseq = d_tseq, B.t_off = d_t_off, B.tlen = pl->d_tlen.as<int32_t>();
	B.ez = d_ez, B.cigar = d_cigar;
	B.pslab = (uint8_t *)d_work, B.p_off = pl->d_poff.as<int64_t>(), B.p_unit_shift = 0;
	B.ws = (uint8_t *)d_work + ((pl->pslab_bytes + 255) & ~(int64_t)255), B.ws_cap = (unsigned long long)pl->ws_bytes;
	B.err = (int *)(pl->d_wstop.as<unsigned long long>() + 1);
	PSVR_HIP(hipMemsetAsync(pl->d_wstop.p, 0, 16, stream));
	TeamLaunch team;
	for (const DpLaunch &L : pl->launches) {
		if (L.kind == PSVR_DP_KIND_STRIP) { team.add(L.cls, L.first, L.count, L.qmax); continue; }
		B.idx = pl->d_idx.as<int32_t>() + L.first;
		PSVR_HIP(dp_launch_kind(L.kind, pl->variant, (unsigned)L.count, dp_lds_class_bytes(L.cls), stream, B, pl->P));
		PSVR_HIP(hipGetLastError());
	}
	B.idx = pl->d_idx.as<int32_t>();
	// (tests: PSVR_DP_FORCE_LEAN=1 sends a plan whose parameters make the z-drop rule inert through the variant the engine's own launches
	// use; ez.max / max_q / max_t of its problems are then not filled in)
	team.launch(stream, B, pl->P, getenv("PSVR_DP_FORCE_LEAN") != nullptr && dp_zdrop_inert(pl->P));
	PSVR_HIP(hipGetLastError());
	return PSVR_OK;
}

static int dp_batch_host(int variant, int device, int64_t n,
                         const uint8_t *qseq, const int64_t *q_off, const int32_t *qlen,
                         const uint8_t *tseq, const int64_t *t_off, const int32_t *tlen,
                         const psvr_ksw_params_t *par, psvr_extz_t *ez, uint32_t *cigar, int64_t cigar_cap)
{
	if (n < 0 || !par || (n > 0 && (!qseq || !q_off || !qlen || !tseq || !t_off || !tlen || !ez)))
		return set_error(PSVR_ERR_ARG, "psvr_ext*_batch: bad argument");
	if (n == 0) return PSVR_OK;
	int ndev = psvr_device_count();
	if (ndev <= 0) return set_error(PSVR_ERR_DEVICE, "no HIP device visible: the engine has no CPU path");
	if (device < 0 || device >= ndev) return set_error(PSVR_ERR_ARG, "device %d out of range (have %d)", device, ndev);
	int64_t qbytes = 0, tbytes = 0, cig = 0;
	for (int64_t i = 0; i < n; ++i) {
		qbytes = std::max<int64_t>(qbytes, q_off[i] + std::max(qlen[i], 0));
		tbytes = std::max<int64_t>(tbytes, t_off[i] + std::max(tlen[i], 0));
		ez[i].cigar_off = cig;
		cig += psvr_cigar_bound(std::max(qlen[i], 0), std::max(tlen[i], 0));
	}
	const bool want_cigar = !(par->flag & PSVR_EZ_SCORE_ONLY);
	if (want_cigar && (cig > cigar_cap || !cigar))
		return set_error(PSVR_ERR_OVERFLOW, "cigar arena too small: need %lld uint32, have %lld", (long long)cig, (long long)cigar_cap);
	{
		hipError_t he = hipSetDevice(device);
		if (he != hipSuccess) return set_error(PSVR_ERR_DEVICE, "hipSetDevice(%d) failed: %s", device, hipGetErrorString(he));
	}
	DevBuf dq, dt, dqo, dto, dez, dcig, dwork;
	PSVR_HIP(dq.alloc(qbytes + 16)); PSVR_HIP(dt.alloc(tbytes + 16));
	PSVR_HIP(dqo.alloc(n * 8)); PSVR_HIP(dto.alloc(n * 8));
	PSVR_HIP(dez.alloc(n * sizeof(psvr_extz_t)));
	PSVR_HIP(dcig.alloc((want_cigar ? cig : 1) * 4));
	PSVR_HIP(hipMemcpy(dq.p, qseq, qbytes, hipMemcpyHostToDevice));
	PSVR_HIP(hipMemcpy(dt.p, tseq, tbytes, hipMemcpyHostToDevice));
	PSVR_HIP(hipMemcpy(dqo.p, q_off, n * 8, hipMemcpyHostToDevice));
	PSVR_HIP(hipMemcpy(dto.p, t_off, n * 8, hipMemcpyHostToDevice));
	PSVR_HIP(hipMemcpy(dez.p, ez, n * sizeof(psvr_extz_t), hipMemcpyHostToDevice));
	// the plan runs in groups of consecutive problems whose slab slices (direction bytes, extd2_hbm_kernel's images) stay under
	// min(4 GiB, free / 2); a problem beyond that budget runs alone if its workspace fits in free device memory
	size_t free_b = 0, total_b = 0;
	PSVR_HIP(hipMemGetInfo(&free_b, &total_b));
	const int64_t budget = std::min<int64_t>(int64_t(4) << 30, (int64_t)(free_b / 2));
	DpParams P;
	int rc = dp_params(par, variant, &P);
	if (rc) return rc;
	const bool fast_ok = dp_fast_ok(P.flag, variant);
	for (int64_t g0 = 0; g0 < n;) {
		int64_t g1 = g0, acc = 0;
		while (g1 < n) {
			const int ql = std::max(qlen[g1], 0), tl = std::max(tlen[g1], 0);
			const int64_t b = (ql < kDpMaxSeqLen && tl < kDpMaxSeqLen) ? dp_route(ql, tl, P.w, fast_ok, variant, P.skip != 0, dp_tiny_ok(P, fast_ok), true, want_cigar).slab : 0;
			if (g1 > g0 && acc + b > budget) break;
			acc += b, ++g1;
		}
		psvr_dp_plan_t *pl = nullptr;
		rc = psvr_dp_plan_create(device, g1 - g0, qlen + g0, tlen + g0, par, variant, &pl);
		if (rc) return rc;
		struct Guard { psvr_dp_plan_t *p; ~Guard() { psvr_dp_plan_destroy(p); } } guard{pl};
		const int64_t ws = psvr_dp_plan_workspace_bytes(pl);
		if (ws > (int64_t)dwork.bytes) {
			dwork.release();
			PSVR_HIP(hipMemGetInfo(&free_b, &total_b));
			if (ws > (int64_t)free_b || dwork.alloc(ws) != hipSuccess) {
				(void)hipGetLastError();
				return set_error(PSVR_ERR_NOMEM, "problems %lld..%lld need %lld bytes of device workspace, %zu bytes free",
				                 (long long)g0, (long long)g1 - 1, (long long)ws, free_b);
			}
		}
		rc = psvr_dp_plan_launch(pl, dq.as<uint8_t>(), dqo.as<int64_t>() + g0, dt.as<uint8_t>(), dto.as<int64_t>() + g0,
		                         dez.as<psvr_extz_t>() + g0, dcig.as<uint32_t>(), dwork.p, nullptr);
		if (rc) return rc;
		PSVR_HIP(hipDeviceSynchronize());
		int kerr = 0;
		PSVR_HIP(hipMemcpy(&kerr, (char *)pl->d_wstop.p + 8, 4, hipMemcpyDeviceToHost));
		if (kerr) return set_error(PSVR_ERR_OVERFLOW, "DP kernel scratch exhausted (internal error %d)", kerr);
		g0 = g1;
	}
	PSVR_HIP(hipMemcpy(ez, dez.p, n * sizeof(psvr_extz_t), hipMemcpyDeviceToHost));
	if (want_cigar) PSVR_HIP(hipMemcpy(cigar, dcig.p, cig * 4, hipMemcpyDeviceToHost));
	return PSVR_OK;
}

extern "C" int psvr_extd2_batch(int device, int64_t n, const uint8_t *qseq, const int64_t *q_off, const int32_t *qlen,
                                const uint8_t *tseq, const int64_t *t_off, const int32_t *tlen,
                                const psvr_ksw_params_t *par, psvr_extz_t *ez, uint32_t *cigar, int64_t cigar_cap)
{
	return dp_batch_host(0, device, n, qseq, q_off, qlen, tseq, t_off, tlen, par, ez, cigar, cigar_cap);
}

extern "C" int psvr_extz2_batch(int device, int64_t n, const uint8_t *qseq, const int64_t *q_off, const int32_t *qlen,
                                const uint8_t *tseq, const int64_t *t_off, const int32_t *tlen,
                                const psvr_ksw_params_t *par, psvr_extz_t *ez, uint32_t *cigar, int64_t cigar_cap)
{
	return dp_batch_host(1, device, n, qseq, q_off, qlen, tseq, t_off, tlen, par, ez, cigar, cigar_cap);
}
