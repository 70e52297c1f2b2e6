// bam_device_route_check -- `panSVR aln -N --bam-device`'s route without a GPU: signal_device_route (pansvr_amd/csrc/signal_device_route.h) in
// window mode over signal_route_host.h's host-memory backend and its reader, which takes every run's window in pieces and prints what each
// piece used.  So stdout is the text of the pairs that were handed over, followed -- when the route is left -- by what the host route writes
// for the rest.  The command line is `panSVR signal -N --signal-device`'s (tests/test_bam_device_route.py compares with `panSVR signal -N`);
// the variables are that header's and signal_device_route_check's PSVR_CHECK_ROUTE_INPUT.
// An error state that the route returns (3, 4, 5) ends the program with status 30 + state instead of SignalStep::run's abort().
#include "signal_route_host.h"

int main(int argc, char **argv)
{
	return signal_main(argc, argv, [](SignalStep &S, long long *pairs_done) {
		HostBackend be;
		PrintingReader reader(be);
		const std::string input = S.o.input;
		if (const char *e = getenv("PSVR_CHECK_ROUTE_INPUT")) S.o.input = e;
		const int rc = signal_device_route(be, S, pairs_done, nullptr, &reader);
		S.o.input = input;
		return route_status(rc, *pairs_done, stdout);
	});
}
