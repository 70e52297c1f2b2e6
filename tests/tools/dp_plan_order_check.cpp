// dp_plan_order_check -- TEST-ONLY: the launch order of the engine's device DP planner (engine_core.h) on the host.
// stdin: lines "kind class qlen count"; stdout: for every line "bucket start", then "total N".
#include <cstdio>
#include <vector>
#include "../../pansvr_amd/csrc/engine_core.h"

int main()
{
	using namespace psvr;
	std::vector<unsigned int> hist(kDpPlanBuckets, 0);
	std::vector<int> asked;
	int kind, cls, qlen;
	unsigned int count;
	while (scanf("%d %d %d %u", &kind, &cls, &qlen, &count) == 4) {
		const int b = dp_plan_bucket(kind, cls, qlen);
		if (b < 0 || b >= kDpPlanBuckets) { fprintf(stderr, "bucket %d out of range\n", b); return 1; }
		hist[(size_t)b] += count;
		asked.push_back(b);
	}
	std::vector<long long> start(kDpPlanBuckets, 0);
	const long long total = dp_plan_starts(hist.data(), start.data());
	for (int b : asked) printf("%d %lld\n", b, start[(size_t)b]);
	printf("total %lld\n", total);
	return 0;
}
