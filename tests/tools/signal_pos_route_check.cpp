// signal_pos_route_check -- `panSVR signal --mate-device` without a GPU: signal_mate_route (pansvr_amd/csrc/signal_device_route.h) over
// signal_route_host.h's host-memory backend.  The command line is `panSVR signal`'s (tests/test_signal_pos_route.py compares with the
// command's host route); the variables are that header's (tests/test_signal_mate_gpu.py reads the PSVR_CHECK_DUMP files).
// An error state that the route returns (4, 5) ends the program with status 30 + state instead of SignalStep::run's abort().
#include "signal_route_host.h"

int main(int argc, char **argv)
{
	return signal_main(argc, argv, nullptr, [](SignalStep &S, long long *pairs_done) {
		HostBackend be;
		const int rc = signal_mate_route(be, S, pairs_done);
		return route_status(rc, *pairs_done, S.out);
	});
}
