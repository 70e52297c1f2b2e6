// mate_window_route_check -- `panSVR aln --mate-device`'s route without a GPU: signal_mate_route (pansvr_amd/csrc/signal_device_route.h) in window
// mode over signal_route_host.h's host-memory backend and its reader, which takes every offered kept window in pieces and prints what each
// piece used.  So stdout is the text of the pairs that were handed over, followed -- when the route is left -- by what the host route writes
// for the rest.  The command line is `panSVR signal --mate-device`'s (tests/test_mate_window_route.py compares with `panSVR signal`); on top
// of that header's variables:
//   PSVR_CHECK_WINDOW_PAIRS=n  the route's window_pairs (default 1 << 20)
//   PSVR_CHECK_WINDOW_BYTES=n  the bytes a kept window must stay below, for the route and for the backend's add (default 2^32)
// An error state that the route returns (4, 5) ends the program with status 30 + state instead of SignalStep::run's abort().
#include "signal_route_host.h"

int main(int argc, char **argv)
{
	return signal_main(argc, argv, nullptr, [](SignalStep &S, long long *pairs_done) {
		HostBackend be;
		PrintingReader reader(be);
		const long long window_pairs = getenv("PSVR_CHECK_WINDOW_PAIRS") ? atoll(getenv("PSVR_CHECK_WINDOW_PAIRS")) : 1 << 20;
		if (const char *e = getenv("PSVR_CHECK_WINDOW_BYTES")) be.window_bytes_max = atoll(e);
		const int rc = signal_mate_route(be, S, pairs_done, nullptr, &reader, window_pairs, be.window_bytes_max);
		fflush(stdout);
		fprintf(stderr, "the reader was offered %lld windows and took %lld pieces\n", reader.offers, reader.pieces);
		return route_status(rc, *pairs_done, stdout);
	});
}
