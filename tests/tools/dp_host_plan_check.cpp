// dp_host_plan_check -- TEST-ONLY: the host planner of seam B2 (dp_plan_host, dp_plan.h) without a device.
// stdin: batches "variant m q e q2 e2 w zdrop end_bonus flag n", 25 matrix entries, n pairs "qlen tlen".
// stdout per batch: "plan rc slab_bytes ws_bytes launches" (rc: 0, or -1 when the parameters are refused), a line "kind class first count qmax name" per launch, "idx" + n ids, "poff" + n offsets.
#include <cstdio>
#include <vector>
#include "../../pansvr_amd/csrc/dp_plan.h"

int main()
{
	using namespace psvr;
	int variant, v[9];
	long long n;
	while (scanf("%d %d %d %d %d %d %d %d %d %d %lld", &variant, &v[0], &v[1], &v[2], &v[3], &v[4], &v[5], &v[6], &v[7], &v[8], &n) == 11) {
		psvr_ksw_params_t par;
		memset(&par, 0, sizeof par);
		par.m = (int8_t)v[0], par.q = (int8_t)v[1], par.e = (int8_t)v[2], par.q2 = (int8_t)v[3], par.e2 = (int8_t)v[4];
		par.w = v[5], par.zdrop = v[6], par.end_bonus = v[7], par.flag = v[8];
		for (int k = 0; k < 25; ++k) { int x; if (scanf("%d", &x) != 1) return 1; par.mat[k] = (int8_t)x; }
		std::vector<int32_t> ql((size_t)n), tl((size_t)n);
		for (long long i = 0; i < n; ++i) if (scanf("%d %d", &ql[(size_t)i], &tl[(size_t)i]) != 2) return 1;
		DpParams P;
		if (!make_dp_params(&par, variant, &P)) { printf("plan -1 0 0 0\nidx\npoff\n"); continue; }
		const DpHostPlan hp = dp_plan_host(n, ql.data(), tl.data(), P, variant);
		printf("plan 0 %lld %lld %zu\n", (long long)hp.slab_bytes, (long long)hp.ws_bytes, hp.launches.size());
		for (const DpLaunch &L : hp.launches) printf("%d %d %lld %lld %d %s\n", L.kind, L.cls, L.first, L.count, L.qmax, dp_kind_name(L.kind, variant));
		printf("idx");
		for (int32_t i : hp.idx) printf(" %d", i);
		printf("\npoff");
		for (size_t i = 0; i < hp.poff.size(); ++i) printf(" %lld", (long long)hp.poff[i]);
		printf("\n");
	}
	return 0;
}
