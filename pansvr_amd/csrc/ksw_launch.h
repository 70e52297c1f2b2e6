// ksw_launch.h -- one place that maps a DP kind (dp_plan.h) to its kernel instantiation
#pragma once
#include <hip/hip_runtime.h>
#include "ksw_device.h"

namespace psvr {

// (kinds 3..5, extd2_reg_kernel<3..5,lds>, have no kernel: 129 target columns already need more direction bytes than PSVR_DP_PG_THRESHOLD,
// so no planner produces them; one that did would be an internal error)
inline hipError_t dp_launch_kind(int kind, int variant, unsigned count, int lds, hipStream_t stream, const DpBatch &B0, const DpParams &P)
{
	DpBatch B = B0;
	B.n = count, B.lds_per_wave = lds;
	if (kind == PSVR_DP_KIND_TINY) {        // `lds` is the size bin: 512 bytes per anti-diagonal
		const int max_rows = lds / 512;
		hipLaunchKernelGGL(extd2_tiny_kernel, dim3((count + 63) / 64), dim3(64), (size_t)8192 + (size_t)max_rows * 1024, stream, B, P, max_rows);
		return hipSuccess;
	}
	if (kind == PSVR_DP_KIND_RING1_3 || kind == PSVR_DP_KIND_RING1_4) {   // a workgroup per alignment
		if (kind == PSVR_DP_KIND_RING1_3) hipLaunchKernelGGL(extd2_ring1_kernel<3>, dim3(count), dim3(64), lds, stream, B, P);
		else hipLaunchKernelGGL(extd2_ring1_kernel<4>, dim3(count), dim3(64), lds, stream, B, P);
		return hipSuccess;
	}
	if (kind == PSVR_DP_KIND_HBM) {
		if (variant == 0) hipLaunchKernelGGL(extd2_hbm_kernel<0>, dim3(count), dim3(64 * kDpHbmWaves), 0, stream, B, P);
		else hipLaunchKernelGGL(extd2_hbm_kernel<1>, dim3(count), dim3(64 * kDpHbmWaves), 0, stream, B, P);
		return hipSuccess;
	}
	const bool reg = kind >= 1;
	dim3 g(reg ? (count + kDpWaves - 1) / kDpWaves : count), b(reg ? 64 * kDpWaves : 64);
	if (reg) lds *= kDpWaves;
	switch (kind) {
	case 1: hipLaunchKernelGGL((extd2_reg_kernel<1, false>), g, b, lds, stream, B, P); break;
	case 2: hipLaunchKernelGGL((extd2_reg_kernel<2, false>), g, b, lds, stream, B, P); break;
	case 3: case 4: case 5: return hipErrorInvalidDeviceFunction;
	case 6: hipLaunchKernelGGL((extd2_reg_kernel<1, true>), g, b, lds, stream, B, P); break;
	case 7: hipLaunchKernelGGL((extd2_reg_kernel<2, true>), g, b, lds, stream, B, P); break;
	case 8: hipLaunchKernelGGL((extd2_reg_kernel<3, true>), g, b, lds, stream, B, P); break;
	case 9: hipLaunchKernelGGL((extd2_reg_kernel<4, true>), g, b, lds, stream, B, P); break;
	case 10: hipLaunchKernelGGL((extd2_reg_kernel<5, true>), g, b, lds, stream, B, P); break;
	case PSVR_DP_KIND_RING3: hipLaunchKernelGGL(extd2_ring_kernel<3>, g, b, lds, stream, B, P); break;
	case PSVR_DP_KIND_RING4: hipLaunchKernelGGL(extd2_ring_kernel<4>, g, b, lds, stream, B, P); break;
	default:
		if (variant == 0) hipLaunchKernelGGL(extd2_lds_kernel<0>, g, b, lds, stream, B, P);
		else hipLaunchKernelGGL(extd2_lds_kernel<1>, g, b, lds, stream, B, P);
	}
	return hipSuccess;
}

// the team kernel: every class in one launch (largest classes first, their wavefronts run longest), then the launch that turns what
// the sweep left in scratch into ksw_extz_t records and CIGARs
struct TeamLaunch {
	TeamPlan T;
	TeamLaunch() { T.n_classes = 0; T.first_block[0] = 0; }
	unsigned long long ws_next = 0;
	// a class (cls + 1 strips of 16 columns) and the longest query among its `count` problems (a wavefront's scratch slice is sized by it)
	void add(int cls, long long first_slot, long long count, int qmax)
	{
		const int c = T.n_classes++;
		T.n_strips16[c] = cls + 1, T.first_slot[c] = first_slot, T.count[c] = count;
		T.first_block[c + 1] = T.first_block[c] + (int)dp_team_waves(cls, (unsigned long long)count);
		T.ws_need[c] = dp_team_wave_ws(cls, qmax);
		T.ws_base[c] = ws_next;
		ws_next += dp_team_class_ws(cls, (unsigned long long)count, qmax);
	}
	// lean: the variant without the per-diagonal maximum -- only for a caller that has checked dp_zdrop_inert(P) and reads neither ez.max nor max_q / max_t
	void launch_sweep(hipStream_t stream, const DpBatch &B, const DpParams &P, bool lean = false) const
	{
		if (!T.n_classes) return;
		if (lean) hipLaunchKernelGGL((extd2_team_kernel<kDpTeamLanes, kDpTeamCpl, 1>), dim3((unsigned)T.first_block[T.n_classes]), dim3(64), 0, stream, B, P, T);
		else hipLaunchKernelGGL((extd2_team_kernel<kDpTeamLanes, kDpTeamCpl, 0>), dim3((unsigned)T.first_block[T.n_classes]), dim3(64), 0, stream, B, P, T);
	}
	void launch_finish(hipStream_t stream, const DpBatch &B, const DpParams &P, bool lean = false) const
	{
		if (!T.n_classes) return;
		const unsigned blocks = (unsigned)T.first_block[T.n_classes], pb = 64u / kDpTeamLanes;
		if (lean) hipLaunchKernelGGL((extd2_team_finish_kernel<kDpTeamLanes, kDpTeamCpl, 1>), dim3((blocks * pb + 63u) / 64u), dim3(64), 0, stream, B, P, T);
		else hipLaunchKernelGGL((extd2_team_finish_kernel<kDpTeamLanes, kDpTeamCpl, 0>), dim3((blocks * pb + 63u) / 64u), dim3(64), 0, stream, B, P, T);
	}
	void launch(hipStream_t stream, const DpBatch &B, const DpParams &P, bool lean = false) const { launch_sweep(stream, B, P, lean), launch_finish(stream, B, P, lean); }
};
inline hipError_t dp_allow_big_lds()
{
	hipError_t e = hipSuccess;
#define PSVR_ATTR(k) do { hipError_t x = hipFuncSetAttribute((const void *)(k), hipFuncAttributeMaxDynamicSharedMemorySize, PSVR_DP_MAX_LDS); if (x != hipSuccess) e = x; } while (0)
	PSVR_ATTR((extd2_reg_kernel<1, false>)); PSVR_ATTR((extd2_reg_kernel<2, false>));
	PSVR_ATTR(extd2_lds_kernel<0>); PSVR_ATTR(extd2_lds_kernel<1>); PSVR_ATTR(extd2_ring_kernel<3>); PSVR_ATTR(extd2_ring_kernel<4>);
	PSVR_ATTR(extd2_ring1_kernel<3>); PSVR_ATTR(extd2_ring1_kernel<4>);
#undef PSVR_ATTR
	return e;
}

} // namespace psvr
