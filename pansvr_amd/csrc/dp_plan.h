// dp_plan.h -- the one place that decides where a DP problem goes and how a round of problems becomes launches: size classes, kinds,
// size formulas, parameter rules, routing, the team kernel's scratch, the launch order and the launch list.  Plain C++ for hipcc and
// g++ alike (no HIP header): the host planner of seam B2 (ksw_host.hip), the engine's device planner (engine.hip) and the test tools
// (tests/tools/dp_plan_order_check.cpp, dp_host_plan_check.cpp) all read the rules here; tests/ksw_regimes.py restates them.
#pragma once
#include <stdint.h>
#include <string.h>
#include <algorithm>
#include <vector>
#include "../../include/psvr_engine.h"

#if defined(__HIPCC__)
#define PSVR_HD __host__ __device__ __forceinline__
#else
#define PSVR_HD inline
#endif

namespace psvr {

// ---- size classes: a launch serves one class; its dynamic LDS (team kernel: its number of 16-column strips, class + 1) is the class's
#define PSVR_DP_NUM_LDS_CLASSES 13
#define PSVR_DP_MAX_LDS (160 * 1024)   // gfx950: 160 KiB LDS per CU / workgroup
PSVR_HD int dp_lds_class_bytes(int cls)
{
	const int t[PSVR_DP_NUM_LDS_CLASSES] = {2048, 4096, 6144, 8192, 12288, 16384, 24576, 32768, 49152, 65536, 98304, 131072, PSVR_DP_MAX_LDS};
	return t[cls];
}
// the smallest class that holds `need` bytes
PSVR_HD int dp_lds_class(long long need)
{
	int cls = 0;
	while (cls < PSVR_DP_NUM_LDS_CLASSES - 1 && dp_lds_class_bytes(cls) < need) ++cls;
	return cls;
}

// ---- kinds: 1..5 = extd2_reg_kernel<kind,false> (direction bytes in LDS), 6..10 = extd2_reg_kernel<kind-5,true> (in HBM), 0 = general kernel
#define PSVR_DP_KIND_TINY 11           // extd2_tiny_kernel: one thread per alignment
#define PSVR_DP_KIND_STRIP 12          // extd2_team_kernel
#define PSVR_DP_KIND_RING3 13          // extd2_ring_kernel<3>: any tlen, band (+ its 16-lane rounding) within 192 columns
#define PSVR_DP_KIND_RING4 14          // extd2_ring_kernel<4>: ... within 256 columns
#define PSVR_DP_NUM_KINDS 15
// kinds only sequences of over kDpLongLen bases reach (the engine has none), for problems the kinds above cannot hold in LDS
#define PSVR_DP_KIND_RING1_3 15        // extd2_ring1_kernel<3>: as RING3, one wavefront per workgroup (query + target image up to 160 KiB)
#define PSVR_DP_KIND_RING1_4 16        // extd2_ring1_kernel<4>
#define PSVR_DP_KIND_HBM 17            // extd2_hbm_kernel<VAR>: any shape, flag and variant
#define PSVR_DP_NUM_HOST_KINDS 18
inline const char *dp_kind_name(int kind, int variant)
{
	static const char *n[PSVR_DP_NUM_KINDS] = {"extd2_lds_kernel", "extd2_reg_kernel<1,lds>", "extd2_reg_kernel<2,lds>", "extd2_reg_kernel<3,lds>", "extd2_reg_kernel<4,lds>",
	                                           "extd2_reg_kernel<5,lds>", "extd2_reg_kernel<1,hbm>", "extd2_reg_kernel<2,hbm>", "extd2_reg_kernel<3,hbm>", "extd2_reg_kernel<4,hbm>",
	                                           "extd2_reg_kernel<5,hbm>", "extd2_tiny_kernel", "extd2_team_kernel", "extd2_ring_kernel<3>", "extd2_ring_kernel<4>"};
	if (kind == 0 && variant == 1) return "extz2_lds_kernel";
	if (kind == PSVR_DP_KIND_RING1_3) return "extd2_ring1_kernel<3>";
	if (kind == PSVR_DP_KIND_RING1_4) return "extd2_ring1_kernel<4>";
	if (kind == PSVR_DP_KIND_HBM) return variant == 0 ? "extd2_hbm_kernel" : "extz2_hbm_kernel";
	return n[kind];
}

// ---- size formulas
#define PSVR_DP_STRIP 16               // extd2_team_kernel: size classes count 16-column strips
#define PSVR_DP_TINY_MAX 16            // extd2_tiny_kernel: qlen, tlen <= 16
// Direction bytes stay in LDS only while the whole footprint is at most this (keeps >= 32 waves per CU resident);
// larger problems stream them to an HBM slab and trace back through L2
#define PSVR_DP_PG_THRESHOLD 4096
static const int kDpWaves = 4;                // alignments (wavefronts) per workgroup of the register-resident kernels
static const int kDpLongLen = 8000;           // the LDS of every kind below PSVR_DP_NUM_KINDS holds a problem whose sequences are at most this long
static const int kDpMaxSeqLen = 1 << 28;      // per-sequence limit: keeps rows, column offsets and extd2_hbm_kernel's ranks in 32 bits
static const int kDpTinySmallLds = 4096;      // merged tiny launches: classes up to this (8 anti-diagonals) share a launch, the larger ones another
// true when the band [(r-w+1)>>1, (r+w)>>1] never clips the DP matrix: then st0/en0 follow the matrix edges only, every
// in-band cell's (r-1,t-1)/(r-1,t) neighbours are in-band or one of the explicit boundary values (ksw2_extd2_sse.c:142-156),
// and the lanes of the 16-rounded blocks outside the band are never read back
PSVR_HD bool dp_band_never_binds(int qlen, int tlen, int w) { return qlen <= w && tlen <= w + 1; }
// the band width in effect: w < 0 means unbanded (ksw2_extd2_sse.c:83)
PSVR_HD int dp_band_w(int qlen, int tlen, int w) { return w < 0 ? (qlen > tlen ? qlen : tlen) : w; }
// 16-byte blocks of one row of direction bytes (:86-87); the row pitch is 16 times this
PSVR_HD int dp_n_col(int qlen, int tlen, int w_in)
{
	int w = dp_band_w(qlen, tlen, w_in);
	int n_col = qlen < tlen ? qlen : tlen;
	n_col = ((n_col < w + 1 ? n_col : w + 1) + 15) / 16 + 1;
	return n_col;
}
PSVR_HD long long dp_reg_lds_need(int qlen, int tlen, int w_in)
{
	return (long long)((qlen + 16 + 15) & ~15) + (long long)(qlen + tlen - 1) * dp_n_col(qlen, tlen, w_in) * 16 + 16;
}
PSVR_HD long long dp_p_bytes(int qlen, int tlen, int w_in)
{
	return ((long long)(qlen + tlen - 1) * dp_n_col(qlen, tlen, w_in) + 1) * 16;
}
PSVR_HD constexpr int dp_lds_kernel_need(int qlen, int tlen, int variant)
{
	int T = (tlen + 15) / 16 * 16, QL = (qlen + 15) / 16 * 16;
	int narr = variant == 0 ? 7 : 5;
	int img = narr * T + T + QL + 16;
	return ((img + 15) & ~15) + 4 * T;
}
static_assert(dp_lds_kernel_need(kDpLongLen, kDpLongLen, 0) <= PSVR_DP_MAX_LDS, "the general kernel's LDS holds every problem that is not long");
// extd2_hbm_kernel's slice of the slab: the direction bytes (none without a CIGAR), then the flat image of extd2_lds_kernel
// (u|v|x|y|x2|y2|s|sf|qr, 16-aligned) and H (int32 per column)
PSVR_HD long long dp_hbm_img_off(int qlen, int tlen, int w_in, bool with_cigar)
{
	return with_cigar ? (dp_p_bytes(qlen, tlen, w_in) + 255) & ~255LL : 0;
}
PSVR_HD long long dp_hbm_img_bytes(int qlen, int tlen, int variant)
{
	const long long T = (tlen + 15LL) / 16 * 16, QL = (qlen + 15LL) / 16 * 16;
	return (((variant == 0 ? 8 : 6) * T + QL + 16 + 15) & ~15LL) + 4 * T;
}

// ---- parameter rules
struct DpParams {
	int32_t m;
	int32_t q, e, q2, e2;       // after the q+e <= q2+e2 swap (ksw2_extd2_sse.c:70)
	int32_t qe_pre;             // q+e BEFORE the swap: only feeds H[0] at r==0 (:60,351)
	int32_t sc_mch, sc_mis, sc_N, m1;
	int32_t w, zdrop, end_bonus, flag;
	int32_t long_thres, long_diff;
	int32_t skip;               // 1: parameter set makes the reference return right after reset (:68,93)
	int32_t nowrap_ok;          // in-band values provably fit int8 for these scoring parameters
	int8_t  mat[25];
};
// parameter preparation (ksw2_extd2_sse.c:60-98); false: the alphabet size is not one of 0..5 (the only error)
inline bool make_dp_params(const psvr_ksw_params_t *par, int variant, DpParams *P)
{
	memset(P, 0, sizeof *P);
	int m = par->m, q = par->q, e = par->e, q2 = par->q2, e2 = par->e2;
	if (m > 5 || m < 0) return false;
	P->m = m;
	P->qe_pre = q + e;
	memcpy(P->mat, par->mat, 25);
	P->w = par->w, P->zdrop = par->zdrop, P->end_bonus = par->end_bonus, P->flag = par->flag;
	if (variant == 0) {
		if (m <= 1) { P->skip = 1; return true; }
		if (q2 + e2 < q + e) { int t = q; q = q2, q2 = t, t = e, e = e2, e2 = t; }   // :70
	} else {
		if (m <= 0) { P->skip = 1; return true; }
		q2 = q, e2 = e;
	}
	P->q = q, P->e = e, P->q2 = q2, P->e2 = e2;
	P->sc_mch = par->mat[0], P->sc_mis = par->mat[1];
	P->sc_N = par->mat[m * m - 1] == 0 ? (int8_t)(-e2) : par->mat[m * m - 1];
	if (variant == 1) P->sc_N = par->mat[m * m - 1] == 0 ? (int8_t)(-e) : par->mat[m * m - 1];
	P->m1 = m - 1;
	int min_sc = par->mat[1];
	for (int t = 1; t < m * m; ++t) min_sc = std::min<int>(min_sc, par->mat[t]);
	if (-min_sc > 2 * (q + e)) { P->skip = 1; return true; }                    // :93
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
	return true;
}
// the z-drop rule cannot trigger whatever the sequences are: a gap of any length costs at most q2 (e2 == 0), so an anti-diagonal's maximum
// is never more than 2 q2 below the running maximum (one insertion + one deletion from the cell that holds it) -- in a matrix whose first
// row and column are charged with the same (post-swap) pairs as its interior.  The reference charges H[0] at r == 0 with q + e taken
// BEFORE the swap (qe_pre, ksw2_extd2_sse.c:60,351): when the caller's pairs arrive in the other order, every H is lower by
// qe_pre - (q + e) than that argument assumes while the running maximum starts at 0, so the threshold rises by that shift (0 for
// pairs in plain order).  The team kernel's LEAN variant (no per-diagonal maximum) is exact then, for a caller that reads neither
// ez.max nor max_q / max_t
inline bool dp_zdrop_inert(const DpParams &P)
{
	return P.e2 == 0 && (P.zdrop < 0 || P.zdrop >= 2 * P.q2 + (P.qe_pre - (P.q + P.e))) && !(P.flag & PSVR_EZ_EXTZ_ONLY);
}
// the flags the register-resident, ring, tiny and team kernels implement (extd2 only); everything else goes to the general kernels
PSVR_HD bool dp_fast_ok(int flag, int variant) { return variant == 0 && (flag & ~(PSVR_EZ_EXTZ_ONLY | PSVR_EZ_REV_CIGAR | PSVR_EZ_SCORE_ONLY)) == 0; }
// the tiny / team kernels need the lean regime (values fit int8, band never clips) and only the flags they implement
PSVR_HD bool dp_tiny_ok(const DpParams &P, bool fast_ok) { return fast_ok && P.nowrap_ok && !P.skip && (P.w < 0 || P.w >= PSVR_DP_TINY_MAX); }

// ---- routing
struct DpRoute {
	int kind, need;     // need: dynamic LDS bytes per alignment, through which the size class is expressed
	int64_t slab;       // bytes of the problem's slice of the slab (DpBatch::pslab: direction bytes, extd2_hbm_kernel's image), a multiple of 256; 0: none
};
// Where a problem goes.  With both sequences of at most kDpLongLen bases: the tiny kernel (need = 512 x anti-diagonals, which bins the
// problems by size), the team kernel, the register-resident kernels, the ring kernels, the general kernel.  Longer ones: the fast-flag
// banded shapes the ring kernels take when the query + target image fits LDS, everything else (wide or no band, the other flags, extz2,
// images beyond LDS) extd2_hbm_kernel; a long problem without a CIGAR has no direction bytes.
// (team_ok = false: a batch too small to fill the chip with 32 alignments per wavefront goes to the wavefront-per-alignment kernels,
// whose sweep is qlen + tlen steps instead of strips x (qlen + 15))
PSVR_HD DpRoute dp_route(int qlen, int tlen, int w, bool fast_ok, int variant, bool skip, bool tiny_ok, bool team_ok, bool with_cigar)
{
	const bool is_long = qlen > kDpLongLen || tlen > kDpLongLen;
	DpRoute R{1, 0, 0};
	if (skip || (!is_long && (qlen <= 0 || tlen <= 0))) return R;      // answered without a sweep (extd2_reg_kernel)
	const bool dirs = with_cigar || !is_long;
	const int64_t p_slab = dirs ? (dp_p_bytes(qlen, tlen, w) + 255) & ~(int64_t)255 : 0;
	if (!is_long) {
		if (tiny_ok && qlen <= PSVR_DP_TINY_MAX && tlen <= PSVR_DP_TINY_MAX) { R.kind = PSVR_DP_KIND_TINY, R.need = (qlen + tlen - 1) * 512; return R; }
		// 16-column strips in registers: whenever the band never clips the matrix (the lean regime).  The size class is the number of
		// strips (1..13), expressed through `need` as that class's byte threshold.
		if (tiny_ok && team_ok && dp_band_never_binds(qlen, tlen, dp_band_w(qlen, tlen, w)) && tlen <= PSVR_DP_STRIP * PSVR_DP_NUM_LDS_CLASSES) {
			R.kind = PSVR_DP_KIND_STRIP, R.need = dp_lds_class_bytes((tlen + PSVR_DP_STRIP - 1) / PSVR_DP_STRIP - 1);
			return R;
		}
		const int T = (tlen + 15) / 16 * 16;
		if (fast_ok && T <= 320) {
			const long long n = dp_reg_lds_need(qlen, tlen, w);
			if (n <= PSVR_DP_PG_THRESHOLD) { R.kind = (T + 63) / 64, R.need = (int)n; return R; }
			R.kind = 5 + (T + 63) / 64, R.need = ((qlen + 16 + 15) & ~15) + 16, R.slab = p_slab;
			return R;
		}
	}
	if (fast_ok) {
		// wider than the register-resident kernels' 320 columns: the ring kernels, when the columns an anti-diagonal can touch -- the band,
		// w + 1 wide at most (and never wider than the shorter sequence), plus the 16-lane rounding at both ends, the stale-score block and
		// the left neighbour of its first column -- fit their ring.  LDS: the query image and the target; four alignments per workgroup
		// while the class of that fits a quarter of LDS (always, up to kDpLongLen bases), one otherwise.
		const int wf = dp_band_w(qlen, tlen, w), sh = qlen < tlen ? qlen : tlen;
		const int span = (wf < sh - 1 ? wf : sh - 1) + 33;
		const long long ring_need = ((qlen + 16 + 15) & ~15LL) + ((tlen + 15) & ~15LL) + 16;
		if (span <= 256 && ring_need <= PSVR_DP_MAX_LDS) {
			const bool four = (long long)dp_lds_class_bytes(dp_lds_class(ring_need)) * kDpWaves <= PSVR_DP_MAX_LDS;
			R.kind = span <= 192 ? (four ? PSVR_DP_KIND_RING3 : PSVR_DP_KIND_RING1_3) : (four ? PSVR_DP_KIND_RING4 : PSVR_DP_KIND_RING1_4);
			R.need = (int)ring_need, R.slab = p_slab;
			return R;
		}
	}
	if (is_long) {
		R.kind = PSVR_DP_KIND_HBM;
		R.slab = dp_hbm_img_off(qlen, tlen, w, with_cigar) + ((dp_hbm_img_bytes(qlen, tlen, variant) + 255) & ~(int64_t)255);
		return R;
	}
	R.kind = 0, R.need = dp_lds_kernel_need(qlen, tlen, variant), R.slab = p_slab;
	return R;
}

// ---- the team kernel's scratch
// A team = kDpTeamLanes lanes, each with kDpTeamCpl target columns of a strip in registers (strip width = their product).
// 4 x 4 was the first shape; 2 x 8 keeps the 16-column strips but spends a step's fixed cost -- neighbour exchange, boundary records,
// per-diagonal maximum -- on eight cells instead of four, and puts 32 alignments in a wavefront.  Other shapes of the row sweep on the
// bench batch (profiles/r03e_team_kernel_row_sweep.txt): 1 x 16 at two wavefronts per SIMD as fast, 4 x 4 and 4 x 8 slower.
static constexpr int kDpTeamLanes = 2, kDpTeamCpl = 8;
// lanes per alignment of the team kernel for the class of problems with n_strips16 16-column strips
PSVR_HD int dp_team_lanes(int n_strips16) { return kDpTeamLanes; }
// scratch bytes one wavefront of the team kernel needs for alignments with at most qmax query bases in that class
PSVR_HD unsigned long long dp_team_ws_bytes(int qmax, int n_strips16, int lanes, int cpl = kDpTeamCpl)
{
	const int sw = cpl * lanes, pb = 64 / lanes, n_strips = (n_strips16 * 16 + sw - 1) / sw;
	// direction bytes (one per cell, 64 x cpl per step), then per row / diagonal and alignment: two boundary dwords (ping-pong), the key D and the
	// dword with the two band-end values (16 bytes; sized for 20: a fifth dword per diagonal is head-room, not used)
	return (unsigned long long)(64 * cpl) * n_strips * (qmax + sw - 1) + (unsigned long long)pb * 20 * (qmax + sw * n_strips + 1);
}
// A class of `count` problems whose longest query has qmax bases: its wavefronts, the scratch slice of each, the scratch of the class.
// The planners size the buffer with the last, TeamLaunch::add hands out the slices: were they to differ, the kernel would report
// through DpBatch::err or write beyond its slice.
PSVR_HD unsigned long long dp_team_waves(int cls, unsigned long long count) { return (count * dp_team_lanes(cls + 1) + 63) / 64; }
PSVR_HD unsigned long long dp_team_wave_ws(int cls, int qmax) { return dp_team_ws_bytes(qmax > 0 ? qmax : 1, cls + 1, dp_team_lanes(cls + 1)); }
PSVR_HD unsigned long long dp_team_class_ws(int cls, unsigned long long count, int qmax) { return dp_team_waves(cls, count) * dp_team_wave_ws(cls, qmax); }

// ---- launch order
// The problem ids of a round are laid out, and the launches go out, kind by kind in this order, each kind with its classes largest
// first: the long problems' kernels, the general kernel, the HBM-direction-byte kernels, the LDS ones, the tiny kernel, and the team
// kernel last (inside a class its longest queries first: the alignments of a wavefront sweep as many steps as the longest of them,
// so neighbours in that order pad least).
PSVR_HD int dp_kind_order(int k)
{
	const int t[PSVR_DP_NUM_HOST_KINDS] = {17, 16, 15, 0, 14, 13, 10, 9, 8, 7, 6, 5, 4, 3, 2, 1, PSVR_DP_KIND_TINY, PSVR_DP_KIND_STRIP};
	return t[k];
}
// The engine's device planner counts a round's problems in buckets: kind * 13 + class for the wavefront / tiny kernels (< 256); the team
// kernel's problems (query of at most 200 bases: the band never clips) have a bucket per (class, query length), 256 + class * 200 +
// (qlen - 1).  Its slots are the buckets in launch order, without the three long kinds, which it never produces.
static const int kDpPlanClasses = PSVR_DP_NUM_LDS_CLASSES, kDpPlanKinds = PSVR_DP_NUM_KINDS, kDpPlanTeamKind = PSVR_DP_KIND_STRIP, kDpPlanQBins = 200;
static const int kDpPlanTeam0 = 256;                                               // first team bucket
static const int kDpPlanBuckets = kDpPlanTeam0 + kDpPlanClasses * kDpPlanQBins;
static const int kDpPlanOtherSlots = (kDpPlanKinds - 1) * kDpPlanClasses;          // slots of the wavefront / tiny kernels
static const int kDpPlanSlots = kDpPlanOtherSlots + kDpPlanClasses * kDpPlanQBins;
static_assert(PSVR_DP_NUM_HOST_KINDS * PSVR_DP_NUM_LDS_CLASSES <= kDpPlanTeam0, "a count per (kind, class) below the team buckets");
PSVR_HD int dp_plan_bucket(int kind, int cls, int qlen)
{
	if (kind == kDpPlanTeamKind) return kDpPlanTeam0 + cls * kDpPlanQBins + (qlen < 1 ? 0 : qlen > kDpPlanQBins ? kDpPlanQBins - 1 : qlen - 1);
	return kind * kDpPlanClasses + cls;
}
// the bucket whose problems come k-th in launch order (0 <= k < kDpPlanSlots)
PSVR_HD int dp_plan_slot_bucket(int k)
{
	if (k < kDpPlanOtherSlots) return dp_kind_order(PSVR_DP_NUM_HOST_KINDS - PSVR_DP_NUM_KINDS + k / kDpPlanClasses) * kDpPlanClasses + (kDpPlanClasses - 1 - k % kDpPlanClasses);
	k -= kDpPlanOtherSlots;
	return kDpPlanTeam0 + (kDpPlanClasses - 1 - k / kDpPlanQBins) * kDpPlanQBins + (kDpPlanQBins - 1 - k % kDpPlanQBins);
}
// bucket counts -> the first position of every bucket (the serial form of what k_dp_plan_starts does with a workgroup); returns the total
inline long long dp_plan_starts(const unsigned int *hist, long long *start)
{
	long long acc = 0;
	for (int b = 0; b < kDpPlanBuckets; ++b) start[b] = 0;
	for (int k = 0; k < kDpPlanSlots; ++k) { const int b = dp_plan_slot_bucket(k); start[b] = acc, acc += hist[b]; }
	return acc;
}

// ---- launch list
struct DpLaunch {
	int kind, cls;          // the launch's LDS bytes / strips are its class's
	long long first, count; // slice of the id list
	int qmax;               // team kernel: the longest query of the class
};
// The launches of a round in launch order from cnt[kind * 13 + class] (every kind but the team kernel's) and the team kernel's
// problems and longest query per class.  merge_tiny: the tiny kernel's classes go out as at most two launches, split at
// kDpTinySmallLds, each at the LDS size of its largest populated class: the two populous classes (up to 4 and up to 8
// anti-diagonals) together at no more than 16 KB a block, the rest at up to 40 KB -- one launch per class was six launches of a
// few hundred wavefronts each, queued one behind the other.
inline std::vector<DpLaunch> dp_launch_list(const unsigned long long *cnt, const unsigned long long *team_cnt, const unsigned long long *team_qmax, bool merge_tiny)
{
	std::vector<DpLaunch> ls;
	long long acc = 0;
	for (int ko = 0; ko < PSVR_DP_NUM_HOST_KINDS; ++ko)
		for (int cls = PSVR_DP_NUM_LDS_CLASSES - 1; cls >= 0; --cls) {
			const int kind = dp_kind_order(ko);
			const bool team = kind == PSVR_DP_KIND_STRIP;
			const long long n = (long long)(team ? team_cnt[cls] : cnt[kind * PSVR_DP_NUM_LDS_CLASSES + cls]);
			if (!n) continue;
			const bool joins = merge_tiny && kind == PSVR_DP_KIND_TINY && !ls.empty() && ls.back().kind == kind &&
			                   (dp_lds_class_bytes(ls.back().cls) > kDpTinySmallLds) == (dp_lds_class_bytes(cls) > kDpTinySmallLds);
			if (joins) ls.back().count += n;
			else ls.push_back(DpLaunch{kind, cls, acc, n, team ? (int)team_qmax[cls] : 0});
			acc += n;
		}
	return ls;
}

// ---- the host planner of seam B2: lengths and parameters -> ids in launch order, slab offsets, launches
struct DpHostPlan {
	std::vector<int32_t> idx;          // problem ids, launch by launch; inside a team class by descending query length (stable)
	std::vector<int64_t> poff;         // per problem: byte offset of its slab slice (the running sum in problem order)
	std::vector<DpLaunch> launches;
	int64_t slab_bytes = 0, ws_bytes = 0;
};
// (the caller has refused sequences of kDpMaxSeqLen bases or more)
inline DpHostPlan dp_plan_host(int64_t n, const int32_t *qlen, const int32_t *tlen, const DpParams &P, int variant)
{
	DpHostPlan out;
	const bool fast_ok = dp_fast_ok(P.flag, variant), tiny_ok = dp_tiny_ok(P, fast_ok), with_cigar = !(P.flag & PSVR_EZ_SCORE_ONLY);
	unsigned long long cnt[PSVR_DP_NUM_HOST_KINDS * PSVR_DP_NUM_LDS_CLASSES] = {}, qmax[PSVR_DP_NUM_LDS_CLASSES] = {};
	std::vector<int> slot(n);
	out.poff.assign(n, 0);
	for (int64_t i = 0; i < n; ++i) {
		const DpRoute R = dp_route(qlen[i], tlen[i], P.w, fast_ok, variant, P.skip != 0, tiny_ok, true, with_cigar);
		if (R.slab) out.poff[i] = out.slab_bytes, out.slab_bytes += R.slab;
		const int cls = dp_lds_class(R.need);
		++cnt[slot[i] = R.kind * PSVR_DP_NUM_LDS_CLASSES + cls];
		if (R.kind == PSVR_DP_KIND_STRIP) qmax[cls] = std::max<unsigned long long>(qmax[cls], qlen[i]);
	}
	out.launches = dp_launch_list(cnt, cnt + PSVR_DP_KIND_STRIP * PSVR_DP_NUM_LDS_CLASSES, qmax, false);
	long long at[PSVR_DP_NUM_HOST_KINDS * PSVR_DP_NUM_LDS_CLASSES] = {};
	for (const DpLaunch &L : out.launches) at[L.kind * PSVR_DP_NUM_LDS_CLASSES + L.cls] = L.first;
	out.idx.resize(n);
	for (int64_t i = 0; i < n; ++i) out.idx[at[slot[i]]++] = (int32_t)i;
	for (const DpLaunch &L : out.launches) {
		if (L.kind != PSVR_DP_KIND_STRIP) continue;
		// alignments of similar query length share a wavefront (their strips take similar numbers of steps)
		std::stable_sort(out.idx.begin() + L.first, out.idx.begin() + L.first + L.count, [&](int32_t x, int32_t y) { return qlen[x] > qlen[y]; });
		out.ws_bytes += (int64_t)dp_team_class_ws(L.cls, (unsigned long long)L.count, L.qmax);
	}
	return out;
}

} // namespace psvr
