// ksw_device.h -- device-side pieces of the banded dual-affine anti-diagonal DP for gfx950.
//
// Replaces ksw_extd2_sse / ksw_extz2_sse (reference: src/kswlib/ksw2_extd2_sse.c:26-396,
// ksw2_extz2_sse.c:23-305) and ksw_backtrack_D / ksw_apply_zdrop (src/kswlib/ksw2.h:119-151,245-261).
//
// Design (MI355X-first, not a port of the SSE code).  Four kernels share the recurrences; the planners route a problem by shape
// (dp_plan.h: the one place the size classes, kinds, routing rules, scratch sizes and launch order live -- this header keeps what the
// kernels themselves need):
//   * extd2_team_kernel<LANES, CPL> + extd2_team_finish_kernel -- the `aln` path's kernel: band never clips the matrix, values fit
//     int8 (dp_band_never_binds && nowrap_ok).  2 lanes per alignment, 32 alignments per wavefront, the matrix swept in strips of
//     16 target columns with the state of 8 columns per lane in registers, a ROW of them per step; see the kernel for the strip
//     boundary / per-diagonal bookkeeping.  The z-drop / end rules and the traceback are the second launch, a thread per alignment.
//   * extd2_tiny_kernel     -- same regime, qlen, tlen <= 16: one thread per alignment, state in LDS.
//   * extd2_reg_kernel<K,PG> -- one 64-lane wavefront per alignment, lane L of chunk c owns target column t = 64c + L, the
//     per-column state (u,v,x,y,x2,y2,s,H) in VGPRs, (r-1,t-1) neighbours by DPP wave_shr:1 with the inter-chunk carry
//     through v_readlane, direction bytes in LDS or an HBM slab, exact max / arg-max by DPP reductions.  Its dp_wave_loop
//     keeps the reference's 16-lane block rounding of [st,en] bit for bit (lanes outside the band but inside the rounded
//     block are computed and read back exactly as the SSE code does, 8-bit wrap included): needed when the band clips.
//   * extd2_lds_kernel<VAR>  -- any shape and flag, and the single-affine extz2 variant: state in LDS in the reference's layout.
//   * extd2_hbm_kernel<VAR>  -- the same recurrence for what LDS cannot hold (long sequences): the flat image and H in a per-problem
//     HBM workspace, a workgroup of kDpHbmWaves wavefronts per alignment.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "../../include/psvr_engine.h"
#include "dp_plan.h"

namespace psvr {

struct DpBatch { // device pointers of one batch
	const int32_t *idx;        // problem ids handled by this launch (one per workgroup)
	const uint8_t *qseq; const int64_t *q_off; const int32_t *qlen;
	const uint8_t *tseq; const int64_t *t_off; const int32_t *tlen;
	psvr_extz_t *ez; uint32_t *cigar;
	uint8_t *pslab; const int64_t *p_off;   // lds kernel only: direction-byte slab, offsets in (1 << p_unit_shift)-byte units
	int32_t p_unit_shift;
	int32_t lds_per_wave;      // reg kernels: dynamic LDS bytes of one wavefront's problem
	long long n;               // problems in this launch
	uint8_t *ws; unsigned long long ws_cap;   // team kernel: per-wavefront scratch, a slice per wavefront (TeamPlan::ws_base)
	int *err;                  // set to 20 if that scratch runs out (cannot happen with the planners' bounds; never silent)
};

template <int K, bool PG> __global__ void extd2_reg_kernel(DpBatch B, DpParams P);   // ksw_kernels.hip
template <int K> __global__ void extd2_ring_kernel(DpBatch B, DpParams P);             // ksw_kernels.hip: the same sweep on a ring of 64 K columns that slides with the band
template <int VAR> __global__ void extd2_lds_kernel(DpBatch B, DpParams P); // ksw_kernels.hip
template <int K> __global__ void extd2_ring1_kernel(DpBatch B, DpParams P);            // ksw_kernels.hip: extd2_ring_kernel<K> with one wavefront per workgroup
template <int VAR> __global__ void extd2_hbm_kernel(DpBatch B, DpParams P); // ksw_kernels.hip
static const int kDpHbmWaves = 8;   // wavefronts per workgroup (= per alignment) of extd2_hbm_kernel
__global__ void extd2_tiny_kernel(DpBatch B, DpParams P, int max_rows);        // ksw_kernels.hip
// all size classes of the team kernel go out in ONE launch (a class alone rarely fills the chip): block b serves class c with
// first_block[c] <= b < first_block[c + 1]; its alignments are idx[first_slot[c] + ...], count[c] of them
struct TeamPlan {
	int32_t n_classes;
	int32_t first_block[PSVR_DP_NUM_LDS_CLASSES + 1];
	int32_t n_strips16[PSVR_DP_NUM_LDS_CLASSES];
	long long first_slot[PSVR_DP_NUM_LDS_CLASSES], count[PSVR_DP_NUM_LDS_CLASSES];
	// scratch of class c's wavefront w at ws_base[c] + w * ws_need[c] (sized by the class's longest query)
	unsigned long long ws_base[PSVR_DP_NUM_LDS_CLASSES], ws_need[PSVR_DP_NUM_LDS_CLASSES];
};
template <int LANES, int CPL, int LEAN> __global__ void extd2_team_kernel(DpBatch B, DpParams P, TeamPlan T);          // ksw_kernels.hip: the sweep, a row per lane and step
template <int LANES, int CPL, int LEAN> __global__ void extd2_team_finish_kernel(DpBatch B, DpParams P, TeamPlan T);   // z-drop / end rules and traceback, a thread per alignment

__device__ __forceinline__ int s8(int v) { return (int)(int8_t)v; }

// u / v of the first cell of row / column r: the gap that reaches it along the matrix edge (ksw2_extd2_sse.c:142-156)
__device__ __forceinline__ int dp_edge_gap(const DpParams &P, int r)
{
	return r == 0 ? s8(-P.q - P.e) : r < P.long_thres ? s8(-P.e) : r == P.long_thres ? s8(P.long_diff) : s8(-P.e2);
}
// last column that gets a fresh score on a diagonal: score groups of 16 from st0 (:159)
__device__ __forceinline__ int dp_fresh_end(int st0, int en0) { return st0 + ((en0 - st0) / 16 + 1) * 16 - 1; }
// The reference's order among cells of one anti-diagonal that tie for the maximum (:322-349): en0 first, then the 4-lane SSE groups
// [st0, en1) lane by lane, then the scalar tail.  Smaller rank = earlier; t - st0 < 1 << RS.  dp_rank_col is the way back.
__device__ __forceinline__ int dp_diag_en1(int st0, int en0) { return st0 + (en0 - st0) / 4 * 4; }
template <int RS>
__device__ __forceinline__ unsigned dp_diag_rank(int t, int st0, int en0, int en1)
{
	return t == en0 ? 0u : t < en1 ? 1u + ((unsigned)((t - st0) & 3) << RS) + (unsigned)(t - st0) : 1u + (4u << RS) + (unsigned)(t - st0);
}
template <int RS>
__device__ __forceinline__ int dp_rank_col(unsigned rk, int st0, int en0) { return rk == 0 ? en0 : st0 + (int)((rk - 1u) & ((1u << RS) - 1u)); }

// mark a value the code knows to be identical in all lanes of the wavefront as uniform (-> SGPR, scalar control flow)
__device__ __forceinline__ int uni(int v) { return __builtin_amdgcn_readfirstlane(v); }
__device__ __forceinline__ long long uni64(long long v)
{
	const unsigned lo = (unsigned)__builtin_amdgcn_readfirstlane((int)(unsigned)v), hi = (unsigned)__builtin_amdgcn_readfirstlane((int)(unsigned)((unsigned long long)v >> 32));
	return (long long)((unsigned long long)hi << 32 | lo);
}

// DPP controls (GFX9): row_shr:n = 0x110+n, wave_shr:1 = 0x138, row_bcast:15 = 0x142, row_bcast:31 = 0x143
__device__ __forceinline__ int dpp_wave_shr1(int v, int carry_in)
{
	return __builtin_amdgcn_update_dpp(carry_in, v, 0x138, 0xf, 0xf, false);
}

// wave-wide max of a signed 32-bit value; result valid in every lane (broadcast from lane 63)
__device__ __forceinline__ int wave_max_i32(int v)
{
	const int idn = (int)0x80000000;
	int t;
	t = __builtin_amdgcn_update_dpp(idn, v, 0x111, 0xf, 0xf, false); v = max(v, t);
	t = __builtin_amdgcn_update_dpp(idn, v, 0x112, 0xf, 0xf, false); v = max(v, t);
	t = __builtin_amdgcn_update_dpp(idn, v, 0x114, 0xf, 0xf, false); v = max(v, t);
	t = __builtin_amdgcn_update_dpp(idn, v, 0x118, 0xf, 0xf, false); v = max(v, t);
	t = __builtin_amdgcn_update_dpp(idn, v, 0x142, 0xa, 0xf, false); v = max(v, t);
	t = __builtin_amdgcn_update_dpp(idn, v, 0x143, 0xc, 0xf, false); v = max(v, t);
	return __builtin_amdgcn_readlane(v, 63);
}

__device__ __forceinline__ unsigned wave_min_u32(unsigned v)
{
	const int idn = (int)0xffffffff;
	unsigned t;
	t = (unsigned)__builtin_amdgcn_update_dpp(idn, (int)v, 0x111, 0xf, 0xf, false); v = min(v, t);
	t = (unsigned)__builtin_amdgcn_update_dpp(idn, (int)v, 0x112, 0xf, 0xf, false); v = min(v, t);
	t = (unsigned)__builtin_amdgcn_update_dpp(idn, (int)v, 0x114, 0xf, 0xf, false); v = min(v, t);
	t = (unsigned)__builtin_amdgcn_update_dpp(idn, (int)v, 0x118, 0xf, 0xf, false); v = min(v, t);
	t = (unsigned)__builtin_amdgcn_update_dpp(idn, (int)v, 0x142, 0xa, 0xf, false); v = min(v, t);
	t = (unsigned)__builtin_amdgcn_update_dpp(idn, (int)v, 0x143, 0xc, 0xf, false); v = min(v, t);
	return (unsigned)__builtin_amdgcn_readlane((int)v, 63);
}

// band limits of anti-diagonal r (ksw2_extd2_sse.c:125-140); returns false when st > en
__device__ __forceinline__ bool band_limits(int r, int qlen, int tlen, int w, int &st0, int &en0, int &st, int &en)
{
	st0 = 0, en0 = tlen - 1;
	if (st0 < r - qlen + 1) st0 = r - qlen + 1;
	if (en0 > r) en0 = r;
	if (st0 < ((r - w + 1) >> 1)) st0 = (r - w + 1) >> 1;
	if (en0 > ((r + w) >> 1)) en0 = (r + w) >> 1;
	st = st0 & ~15;
	en = ((en0 + 16) & ~15) - 1;
	return st0 <= en0;
}

struct EzAcc { // running ksw_extz_t (uniform per wave)
	int max, zdropped, max_q, max_t, mqe, mqe_t, mte, mte_q, score, reach_end;
	__device__ __forceinline__ void reset()
	{
		max_q = max_t = mqe_t = mte_q = -1;
		max = 0, score = mqe = mte = PSVR_KSW_NEG_INF;
		zdropped = 0, reach_end = 0;
	}
	// ksw_apply_zdrop with is_rot=1 (ksw2.h:245-261)
	__device__ __forceinline__ bool apply_zdrop(int H, int r, int t, int zdrop, int e)
	{
		if (H > max) {
			max = H, max_t = t, max_q = r - t;
		} else if (t >= max_t && r - t >= max_q) {
			int tl = t - max_t, ql = (r - t) - max_q;
			int l = tl > ql ? tl - ql : ql - tl;
			if (zdrop >= 0 && max - H > zdrop + l * e) {
				zdropped = 1;
				return true;
			}
		}
		return false;
	}
	// what the reference does with H at the end of anti-diagonal r (ksw2_extd2_sse.c:352-359): the end scores, the z-drop rule
	// (true = stop), the global score.  H_st0 / H_en0: H at the band's ends; `e` the extension cost the rule charges (e2; extz2: e)
	__device__ __forceinline__ bool end_diagonal(int r, int qlen, int tlen, int st0, int en0, int H_st0, int H_en0, int max_H, int max_t, int zdrop, int e)
	{
		if (en0 == tlen - 1 && H_en0 > mte) mte = H_en0, mte_q = r - (((en0 + 16) & ~15) - 1);   // r - en
		if (r - st0 == qlen - 1 && H_st0 > mqe) mqe = H_st0, mqe_t = st0;
		if (apply_zdrop(max_H, r, max_t, zdrop, e)) return true;
		if (r == qlen + tlen - 2 && en0 == tlen - 1) score = H_en0;
		return false;
	}
};

// Where the traceback starts (ksw2_extd2_sse.c:382-391); false = no CIGAR.  Sets ez.reach_end, so it is part of the result.
__device__ __forceinline__ bool trace_start(EzAcc &ez, const DpParams &P, int qlen, int tlen, int &i0, int &j0)
{
	i0 = j0 = -1;
	if (!ez.zdropped && !(P.flag & PSVR_EZ_EXTZ_ONLY)) i0 = tlen - 1, j0 = qlen - 1;
	else if (!ez.zdropped && (P.flag & PSVR_EZ_EXTZ_ONLY) && ez.mqe + P.end_bonus > ez.max) ez.reach_end = 1, i0 = ez.mqe_t, j0 = qlen - 1;
	else if (ez.max_t >= 0 && ez.max_q >= 0) i0 = ez.max_t, j0 = ez.max_q;
	return i0 >= 0 && j0 >= 0;
}

// Traceback over direction bytes (ksw_backtrack_D with is_rot=1, min_intron_len=0; ksw2.h:119-151).
// `P` reads one byte of row r at column offset k; ops are staged through `emit(k, word)`.
// Every lane runs the same (uniform) walk.  Returns the number of CIGAR ops.
template <class ReadP, class Emit>
__device__ __forceinline__ int traceback(int i0, int j0, int qlen, int tlen, int w, ReadP readp, Emit emit)
{
	int i = i0, j = j0, state = 0, n = 0;
	int cur_op = -1, cur_len = 0;
	auto push = [&](int op, int len) {
		if (op == cur_op) cur_len += len;
		else {
			if (cur_op >= 0) emit(n++, (uint32_t)cur_len << 4 | (uint32_t)cur_op);
			cur_op = op, cur_len = len;
		}
	};
	while (i >= 0 && j >= 0) {
		int r = i + j, st0, en0, off, off_end, force_state = -1;
		band_limits(r, qlen, tlen, w, st0, en0, off, off_end);
		if (i < off) force_state = 2;
		if (i > off_end) force_state = 1;
		int tmp = force_state < 0 ? readp(r, i - off) : 0;
		if (state == 0) state = tmp & 7;
		else if (!((tmp >> (state + 2)) & 1)) state = 0;
		if (state == 0) state = tmp & 7;
		if (force_state >= 0) state = force_state;
		if (state == 0) push(0, 1), --i, --j;
		else if (state == 1 || state == 3) push(2, 1), --i;
		else push(1, 1), --j;
	}
	if (i >= 0) push(2, i + 1);
	if (j >= 0) push(1, j + 1);
	if (cur_op >= 0) emit(n++, (uint32_t)cur_len << 4 | (uint32_t)cur_op);
	return n;
}

} // namespace psvr
