// bam_device_route_check -- `panSVR aln -N --bam-device`'s route without a GPU: pansvr_amd/csrc/signal_device_route.h in window mode over
// signal_device_route_check.cpp's host-memory backend (included as it is, its main renamed), with the window put together by the one-lane host
// build of signal_window_device.h and a reader that takes it in pieces: fastq_device.h's host parser with a pair limit, walking the window by
// used_bytes as FastqReader::read_window does, and printing what each piece used.  So stdout is the text of the pairs that were handed over,
// followed -- when the route is left -- by what the host route writes for the rest.  The command line is `panSVR signal -N --signal-device`'s
// (tests/test_bam_device_route.py compares with `panSVR signal -N`); on top of that file's variables:
//   PSVR_CHECK_PIECE_PAIRS=n   the reader's pair limit per piece (default 1 << 20)
//   PSVR_CHECK_FAIL=call:n     also for signal_window (the backend's call) and window_parse (the reader's n-th piece fails)
#define main signal_device_route_check_main
#include "signal_device_route_check.cpp"
#undef main
#include "../../pansvr_amd/csrc/fastq_device.h"
#include "../../pansvr_amd/csrc/signal_window_device.h"

struct WindowBackend : HostBackend {
	std::string window;
	int signal_window(const void *host, int64_t host_bytes, const int64_t *host_off, int64_t n_host, psvr_signal_window_info_t *info)
	{
		if (failing("signal_window")) return 3;
		int64_t n_front = 0, declined = 0, written = 0;
		while (n_front < (int64_t)tab.size() && tab[(size_t)n_front].state < 3) ++n_front;
		std::vector<uint8_t> state((size_t)n_front + 1);
		std::vector<int64_t> toff((size_t)n_front + 1);
		for (int64_t p = 0; p < n_front; ++p) state[(size_t)p] = tab[(size_t)p].state, toff[(size_t)p] = tab[(size_t)p].text_off, declined += state[(size_t)p] == 2, written += state[(size_t)p] == 1;
		if (const char *bad = sw_args_bad(host_bytes, host_off, n_host, declined)) { err = bad; return 1; }
		window.assign(text.size() + (size_t)host_bytes, '\xEE');
		sw_window_host(state.data(), toff.data(), n_front, (const uint8_t *)text.data(), (int64_t)text.size(), (const uint8_t *)host, host_off, n_host, (uint8_t *)&window[0]);
		info->n_bytes = (int64_t)window.size(), info->n_pairs = written + declined, info->n_host_pairs = n_host;
		return 0;
	}
};

struct PrintingReader : SignalWindowTaker {
	WindowBackend &be;
	long long piece_pairs = 1 << 20;
	explicit PrintingReader(WindowBackend &b) : be(b) { if (const char *e = getenv("PSVR_CHECK_PIECE_PAIRS")) piece_pairs = atoll(e); }
	long long offer(const psvr_signal_window_info_t &info, std::string *why) override
	{
		long long taken = 0;
		uint64_t at = 0;
		while (taken < info.n_pairs) {
			if (be.failing("window_parse")) { *why = be.err; return taken; }
			FqHostResult r;
			fq_parse_host(be.window.data() + at, be.window.size() - at, 1, piece_pairs, (int64_t)1 << 60, &r);
			if (r.info.n_pairs < 1 || taken + r.info.n_pairs > info.n_pairs) { *why = "the window's text does not hold the pairs the run counted"; return taken; }
			fwrite(be.window.data() + at, 1, (size_t)r.info.used_bytes, stdout);
			at += (uint64_t)r.info.used_bytes, taken += r.info.n_pairs;
		}
		if (at != be.window.size()) { *why = "text behind the window's last pair"; return taken - 1; }
		return taken;
	}
};

int main(int argc, char **argv)
{
	return signal_main(argc, argv, [](SignalStep &S, long long *pairs_done) {
		WindowBackend be;
		PrintingReader reader(be);
		const std::string input = S.o.input;
		if (const char *e = getenv("PSVR_CHECK_ROUTE_INPUT")) S.o.input = e;
		const int rc = signal_device_route(be, S, pairs_done, nullptr, &reader);
		S.o.input = input;
		if (rc > 0) {                                            // (SignalStep::run would abort(): the code is what the test looks at)
			fflush(stdout);
			fprintf(stderr, "route returned state %d behind %lld pairs\n", rc, *pairs_done);
			exit(30 + rc);
		}
		return rc;
	});
}
