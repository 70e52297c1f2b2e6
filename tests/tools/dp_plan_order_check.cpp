// dp_plan_order_check -- TEST-ONLY: the launch order and the launch lists of the DP planners (dp_plan.h) and the team kernel's scratch
// slices (TeamLaunch::add, ksw_launch.h) on the host.  Compiled for the host only (ksw_launch.h needs the HIP headers); no device call is made.
// stdin: lines "kind class qlen count"; stdout: for every line "bucket start", then "total N", then the launch list with the tiny
// classes merged and the one without ("launches merged|plain M", M lines "kind class first count qmax"), then for the latter the team
// kernel's scratch: "ws shared X" (the sum of dp_team_class_ws) and "ws next Y" (what TeamLaunch::add accumulates).
#include <cstdio>
#include <vector>
#include "../../pansvr_amd/csrc/ksw_launch.h"

int main()
{
	using namespace psvr;
	std::vector<unsigned int> hist(kDpPlanBuckets, 0);
	std::vector<int> asked;
	unsigned long long cnt[kDpPlanTeam0] = {}, team_cnt[PSVR_DP_NUM_LDS_CLASSES] = {}, team_qmax[PSVR_DP_NUM_LDS_CLASSES] = {};
	int kind, cls, qlen;
	unsigned int count;
	while (scanf("%d %d %d %u", &kind, &cls, &qlen, &count) == 4) {
		const int b = dp_plan_bucket(kind, cls, qlen);
		if (b < 0 || b >= kDpPlanBuckets || cls < 0 || cls >= PSVR_DP_NUM_LDS_CLASSES) { fprintf(stderr, "bucket %d out of range\n", b); return 1; }
		hist[(size_t)b] += count;
		asked.push_back(b);
		if (kind != PSVR_DP_KIND_STRIP) cnt[b] += count;
		else {
			team_cnt[cls] += count;
			if ((unsigned long long)qlen > team_qmax[cls]) team_qmax[cls] = (unsigned long long)qlen;
		}
	}
	std::vector<long long> start(kDpPlanBuckets, 0);
	const long long total = dp_plan_starts(hist.data(), start.data());
	for (int b : asked) printf("%d %lld\n", b, start[(size_t)b]);
	printf("total %lld\n", total);
	for (int merge = 1; merge >= 0; --merge) {
		const std::vector<DpLaunch> ls = dp_launch_list(cnt, team_cnt, team_qmax, merge != 0);
		printf("launches %s %zu\n", merge ? "merged" : "plain", ls.size());
		TeamLaunch team;
		unsigned long long shared = 0;
		for (const DpLaunch &L : ls) {
			printf("%d %d %lld %lld %d\n", L.kind, L.cls, L.first, L.count, L.qmax);
			if (L.kind != PSVR_DP_KIND_STRIP) continue;
			team.add(L.cls, L.first, L.count, L.qmax);
			shared += dp_team_class_ws(L.cls, (unsigned long long)L.count, L.qmax);
		}
		if (!merge) printf("ws shared %llu\nws next %llu\n", shared, team.ws_next);
	}
	return 0;
}
