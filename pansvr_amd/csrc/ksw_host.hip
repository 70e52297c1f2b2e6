// ksw_host.hip -- host side of seam B2 (psvr_extd2_batch / psvr_dp_plan_*): parameter
// preparation (ksw2_extd2_sse.c:60-98), size-class planning and kernel launches.
#include <hip/hip_runtime.h>
#include <cstdlib>
#include <algorithm>
#include <cstring>
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

static const int kLongLen = 8000;         // problems with a longer sequence take the long routes (dp_route)
static const int kMaxSeqLen = 1 << 28;    // per-sequence limit: keeps rows, column offsets and extd2_hbm_kernel's ranks in 32 bits
static const int kMaxLds = 160 * 1024;    // gfx950: 160 KiB LDS per CU / workgroup
static const int kLdsClasses[] = {2048, 4096, 6144, 8192, 12288, 16384, 24576, 32768, 49152, 65536, 98304, 131072, kMaxLds};
static const int kNumLdsClasses = sizeof(kLdsClasses) / sizeof(int);

static int lds_class(long long need)
{
	int cls = 0;
	while (cls < kNumLdsClasses - 1 && kLdsClasses[cls] < need) ++cls;
	return cls;
}

struct DpRoute {
	int kind, need;     // need: dynamic LDS bytes per alignment (dp_classify)
	int64_t slab;       // bytes of the problem's slice of the slab (direction bytes, extd2_hbm_kernel's image)
};

// Problems with both sequences of at most kLongLen bases go where dp_classify puts them (the LDS of every kind holds them).  Longer ones:
// the fast-flag banded shapes the ring kernels take when the query + target image fits LDS -- four alignments per workgroup while it
// fits a quarter of it, one otherwise; everything else (wide or no band, the other flags, extz2, images beyond LDS) extd2_hbm_kernel.
// A long problem without a CIGAR has no direction bytes.
static DpRoute dp_route(int ql, int tl, const psvr_ksw_params_t *par, const DpParams &P, int variant, bool fast_ok)
{
	DpRoute R{0, 0, 0};
	const bool with_cigar = !(par->flag & PSVR_EZ_SCORE_ONLY);
	if (ql <= kLongLen && tl <= kLongLen) {
		R.kind = dp_classify(ql, tl, par->w, fast_ok, variant, P.skip != 0, &R.need, dp_tiny_ok(P, fast_ok), true);
		if (R.kind >= 0 && dp_kind_uses_slab(R.kind) && ql > 0 && tl > 0) R.slab = (dp_p_bytes(ql, tl, par->w) + 255) & ~(int64_t)255;
		return R;
	}
	if (P.skip) { R.kind = 1; return R; }      // answered without a sweep (extd2_reg_kernel)
	const int wf = par->w < 0 ? std::max(ql, tl) : par->w, sh = std::min(ql, tl);
	const int span = std::min(wf, sh - 1) + 33;
	const long long ring_need = ((ql + 16 + 15) & ~15LL) + ((tl + 15) & ~15LL) + 16;
	if (fast_ok && span <= 256 && ring_need <= kMaxLds) {
		R.need = (int)ring_need;
		const bool four = (long long)kLdsClasses[lds_class(ring_need)] * kDpWaves <= kMaxLds;
		R.kind = span <= 192 ? (four ? PSVR_DP_KIND_RING3 : PSVR_DP_KIND_RING1_3) : (four ? PSVR_DP_KIND_RING4 : PSVR_DP_KIND_RING1_4);
		if (with_cigar) R.slab = (dp_p_bytes(ql, tl, par->w) + 255) & ~(int64_t)255;
		return R;
	}
	R.kind = PSVR_DP_KIND_HBM;
	R.slab = dp_hbm_img_off(ql, tl, par->w, with_cigar) + ((dp_hbm_img_bytes(ql, tl, variant) + 255) & ~(int64_t)255);
	return R;
}

int make_dp_params(const psvr_ksw_params_t *par, int variant, DpParams *P)
{
	memset(P, 0, sizeof *P);
	int m = par->m, q = par->q, e = par->e, q2 = par->q2, e2 = par->e2;
	if (m > 5 || m < 0) return set_error(PSVR_ERR_UNSUPPORTED, "alphabet size m=%d (supported: 0..5)", m);
	P->m = m;
	P->qe_pre = q + e;
	memcpy(P->mat, par->mat, 25);
	P->w = par->w, P->zdrop = par->zdrop, P->end_bonus = par->end_bonus, P->flag = par->flag;
	if (variant == 0) {
		if (m <= 1) { P->skip = 1; return PSVR_OK; }
		if (q2 + e2 < q + e) { int t = q; q = q2, q2 = t, t = e, e = e2, e2 = t; }   // :70
	} else {
		if (m <= 0) { P->skip = 1; return PSVR_OK; }
		q2 = q, e2 = e;
	}
	P->q = q, P->e = e, P->q2 = q2, P->e2 = e2;
	P->sc_mch = par->mat[0], P->sc_mis = par->mat[1];
	P->sc_N = par->mat[m * m - 1] == 0 ? (int8_t)(-e2) : par->mat[m * m - 1];
	if (variant == 1) P->sc_N = par->mat[m * m - 1] == 0 ? (int8_t)(-e) : par->mat[m * m - 1];
	P->m1 = m - 1;
	int min_sc = par->mat[1];
	for (int t = 1; t < m * m; ++t) min_sc = std::min<int>(min_sc, par->mat[t]);
	if (-min_sc > 2 * (q + e)) { P->skip = 1; return PSVR_OK; }                 // :93
	{
		// in-band deltas of the difference recurrences stay within [-(q2+e2) - max_sc, max_sc + 2(q2+e2)] and the sums the
		// kernel forms within twice that: far inside int8 for the usual scoring (2/-12, 16+1, 32+0 -> |v| <= 100)
		int max_sc = par->mat[0];
		for (int t = 1; t < m * m; ++t) max_sc = std::max<int>(max_sc, par->mat[t]);
		int g = std::max(q + e, q2 + e2);
		// That bound is an argument about a DP whose first row and column are charged what the recurrences charge inside.  The reference
		// charges them q+e, then e per base up to long_thres and e2 per base after it (:151,155): the cheaper of the two pairs at every
		// length exactly when the second pair is the long-gap pair (e > e2) or the pairs are the same; z <= sc_mch holds in every cell
		// then and z = min(z, sc_mch) (:193) never binds.  Otherwise the boundary overcharges and the clamp binds beside it.  With
		// e < e2 what it cuts off accumulates in x / y along a row until the reference's int8 lanes wrap (17+0k | 16+1k at 200 x 201:
		// score -66, without the wrap -65), which only the wavefront kernels reproduce.  With e == e2 and q2 > q the excess is
		// bounded by q2 - q and no wrap was seen, but the bound above is not proven there either: not the team / tiny kernels' regime
		const bool boundary_is_the_recurrences = e > e2 || (e == e2 && q == q2);
		P->nowrap_ok = (max_sc + 3 * g + std::max(-min_sc, 0) <= 127) && q >= 0 && e >= 0 && q2 >= 0 && e2 >= 0 && boundary_is_the_recurrences;
	}
	if (variant == 0) {
		int lt = e != e2 ? (q2 - q) / (e - e2) - 1 : 0;                             // :95-98
		if (q2 + e2 + lt * e2 > q + e + lt * e) ++lt;
		P->long_thres = lt;
		P->long_diff = lt * (e - e2) - (q2 - q) - e2;
	}
	return PSVR_OK;
}

struct Launch {
	int kind;           // 1..5: extd2_reg_kernel<kind>; 0: extd2_lds_kernel
	int lds_bytes;
	int64_t first, count;   // slice of the index list
	int qmax;               // team kernel: the longest query of the class
};

} // namespace psvr

using namespace psvr;

struct psvr_dp_plan {
	int device = 0, variant = 0;
	int64_t n = 0;
	DpParams P;
	std::vector<Launch> launches;
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
	int rc = make_dp_params(par, variant, &pl->P);
	if (rc) { delete pl; return rc; }
	{
		hipError_t he = hipSetDevice(device);
		if (he != hipSuccess) { delete pl; return set_error(PSVR_ERR_DEVICE, "hipSetDevice(%d) failed: %s", device, hipGetErrorString(he)); }
	}
	const int fast_flags = PSVR_EZ_EXTZ_ONLY | PSVR_EZ_REV_CIGAR | PSVR_EZ_SCORE_ONLY;
	const bool fast_ok = variant == 0 && (par->flag & ~fast_flags) == 0;
	// bucket = kind * classes + lds class
	std::vector<std::vector<int32_t>> bucket(PSVR_DP_NUM_HOST_KINDS * kNumLdsClasses);
	std::vector<int64_t> poff(n, 0);
	int64_t pslab = 0;
	for (int64_t i = 0; i < n; ++i) {
		int ql = qlen[i], tl = tlen[i];
		if (ql >= kMaxSeqLen || tl >= kMaxSeqLen) {
			delete pl;
			return set_error(PSVR_ERR_UNSUPPORTED, "problem %lld: qlen=%d tlen=%d: sequences of 2^28 bases or more are not supported", (long long)i, ql, tl);
		}
		const DpRoute R = dp_route(ql, tl, par, pl->P, variant, fast_ok);
		if (R.kind < 0) { delete pl; return set_error(PSVR_ERR_UNSUPPORTED, "problem %lld needs %d B of LDS", (long long)i, R.need); }
		if (R.slab) {
			poff[i] = pslab;
			pslab += R.slab;
		}
		bucket[R.kind * kNumLdsClasses + lds_class(R.need)].push_back((int32_t)i);
	}
	std::vector<int32_t> idx;
	idx.reserve(n);
	// the long problems' kernels first, then the general kernel, then the HBM-direction-byte kernels, then the LDS ones; large LDS classes first
	const int kind_order[PSVR_DP_NUM_HOST_KINDS] = {17, 16, 15, 0, 14, 13, 10, 9, 8, 7, 6, 5, 4, 3, 2, 1, 12, 11};
	for (int ko = 0; ko < PSVR_DP_NUM_HOST_KINDS; ++ko)
		for (int cls = kNumLdsClasses - 1; cls >= 0; --cls) {
			auto &b = bucket[kind_order[ko] * kNumLdsClasses + cls];
			if (b.empty()) continue;
			// team kernel: alignments of similar query length share a wavefront (their strips take similar numbers of steps)
			if (kind_order[ko] == PSVR_DP_KIND_STRIP) std::stable_sort(b.begin(), b.end(), [&](int32_t x, int32_t y) { return qlen[x] > qlen[y]; });
			Launch L{kind_order[ko], kLdsClasses[cls], (int64_t)idx.size(), (int64_t)b.size(), 0};
			if (L.kind == PSVR_DP_KIND_STRIP) {      // a wavefront's scratch slice is sized by the class's longest query
				for (int32_t i : b) L.qmax = std::max(L.qmax, qlen[i]);
				const int lanes = dp_team_lanes(cls + 1);
				pl->ws_bytes += (int64_t)(((uint64_t)b.size() * lanes + 63) / 64 * dp_team_ws_bytes(L.qmax > 0 ? L.qmax : 1, cls + 1, lanes));
			}
			pl->launches.push_back(L);
			idx.insert(idx.end(), b.begin(), b.end());
			char buf[160];
			snprintf(buf, sizeof buf, "%s[lds=%d] x%lld; ", dp_kind_name(L.kind, variant), L.lds_bytes, (long long)L.count);
			pl->desc += buf;
		}
	pl->pslab_bytes = pslab;
	PSVR_HIP(pl->d_idx.alloc(idx.size() * 4));
	PSVR_HIP(pl->d_poff.alloc(n * 8));
	PSVR_HIP(pl->d_qlen.alloc(n * 4));
	PSVR_HIP(pl->d_tlen.alloc(n * 4));
	PSVR_HIP(pl->d_wstop.alloc(16));      // the error flag (4 B, at offset 8)
	if (n) {
		PSVR_HIP(hipMemcpy(pl->d_idx.p, idx.data(), idx.size() * 4, hipMemcpyHostToDevice));
		PSVR_HIP(hipMemcpy(pl->d_poff.p, poff.data(), n * 8, hipMemcpyHostToDevice));
		PSVR_HIP(hipMemcpy(pl->d_qlen.p, qlen, n * 4, hipMemcpyHostToDevice));
		PSVR_HIP(hipMemcpy(pl->d_tlen.p, tlen, n * 4, hipMemcpyHostToDevice));
	}
	PSVR_HIP(dp_allow_big_lds());
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
	int rc = make_dp_params(par, variant, &P);
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
	for (const Launch &L : pl->launches) {
		if (L.kind == PSVR_DP_KIND_STRIP) { team.add(dp_class_of(L.lds_bytes) + 1, L.first, L.count, L.qmax); continue; }
		B.idx = pl->d_idx.as<int32_t>() + L.first;
		PSVR_HIP(dp_launch_kind(L.kind, pl->variant, (unsigned)L.count, L.lds_bytes, stream, B, pl->P));
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
	int rc = make_dp_params(par, variant, &P);
	if (rc) return rc;
	const int fast_flags = PSVR_EZ_EXTZ_ONLY | PSVR_EZ_REV_CIGAR | PSVR_EZ_SCORE_ONLY;
	const bool fast_ok = variant == 0 && (par->flag & ~fast_flags) == 0;
	for (int64_t g0 = 0; g0 < n;) {
		int64_t g1 = g0, acc = 0;
		while (g1 < n) {
			const int ql = std::max(qlen[g1], 0), tl = std::max(tlen[g1], 0);
			const int64_t b = (ql < kMaxSeqLen && tl < kMaxSeqLen) ? dp_route(ql, tl, par, P, variant, fast_ok).slab : 0;
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
