// signal_device_route_check -- `panSVR signal -N --signal-device` without a GPU: signal_device_route (pansvr_amd/csrc/signal_device_route.h) over
// signal_route_host.h's host-memory backend.  The command line is `panSVR signal`'s (tests/test_signal_device_route.py compares with the
// command's host route); on top of that header's variables:
//   PSVR_CHECK_ROUTE_INPUT=f   the route reads f instead: a damaged copy of the input whose front is the input's (the step samples the first
//                              100 000 records before the route begins, so a small damaged input never reaches it; this way the route meets
//                              the damage in mid-file, and what takes over reads the whole input)
// An error state that the route returns (3, 4, 5) ends the program with status 30 + state instead of SignalStep::run's abort().
#include "signal_route_host.h"

int main(int argc, char **argv)
{
	return signal_main(argc, argv, [](SignalStep &S, long long *pairs_done) {
		HostBackend be;
		const std::string input = S.o.input;
		if (const char *e = getenv("PSVR_CHECK_ROUTE_INPUT")) S.o.input = e;
		const int rc = signal_device_route(be, S, pairs_done);
		S.o.input = input;
		return route_status(rc, *pairs_done, S.out);
	});
}
