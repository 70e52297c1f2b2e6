// mate_window_route_check -- `panSVR aln --mate-device`'s route without a GPU: signal_mate_route (pansvr_amd/csrc/signal_device_route.h) in window
// mode over signal_pos_route_check.cpp's host-memory backend (included as it is; it lies in a namespace of its own here, so its main is
// pos_route_check::main), with the kept window grown by the one-lane host build of the add rule of signal_window_device.h and a reader that
// takes every offered window in pieces: fastq_device.h's host parser with a pair limit, walking the window by used_bytes as
// FastqReader::read_window does, and printing what each piece used.  So stdout is the text of the pairs that were handed over, followed --
// when the route is left -- by what the host route writes for the rest.  The command line is `panSVR signal --mate-device`'s
// (tests/test_mate_window_route.py compares with `panSVR signal`); on top of signal_pos_route_check's variables:
//   PSVR_CHECK_WINDOW_PAIRS=n  the route's window_pairs (default 1 << 20)
//   PSVR_CHECK_WINDOW_BYTES=n  the bytes a kept window must stay below, for the route and for the backend's add (default 2^32)
//   PSVR_CHECK_PIECE_PAIRS=n   the reader's pair limit per piece (default 1 << 20)
//   PSVR_CHECK_FAIL=call:n     also for signal_window_add (the backend's call) and window_parse (the reader's n-th piece fails)
// An error state that the route returns (4, 5) ends the program with status 30 + state instead of SignalStep::run's abort().
#include <zlib.h>
#include <map>
#include <memory>
#include <string>
#include <vector>
#include "../../pansvr_amd/csrc/signal_device_route.h"
#include "../../pansvr_amd/csrc/signal_device.h"
#include "../../pansvr_amd/csrc/inflate_layout.h"
#include "../../pansvr_amd/csrc/fastq_device.h"
#include "../../pansvr_amd/csrc/signal_window_device.h"
#include "signal_mate_host.h"
namespace pos_route_check {
#include "signal_pos_route_check.cpp"
}
using namespace psvr;

struct MateWindowBackend : pos_route_check::PosBackend {
	std::string window;
	long long win_pairs = 0, win_host_pairs = 0, window_bytes_max = (long long)1 << 32;
	int signal_window_add(const void *host, int64_t host_bytes, const int64_t *host_off, int64_t n_host, int32_t restart, psvr_signal_window_info_t *info)
	{
		if (failing("signal_window_add")) return 3;
		int64_t n_front = 0, declined = 0, written = 0;
		while (n_front < (int64_t)tab.size() && tab[(size_t)n_front].state < 3) ++n_front;
		std::vector<uint8_t> state((size_t)n_front + 1);
		std::vector<int64_t> toff((size_t)n_front + 1);
		for (int64_t p = 0; p < n_front; ++p) state[(size_t)p] = tab[(size_t)p].state, toff[(size_t)p] = tab[(size_t)p].text_off, declined += state[(size_t)p] == 2, written += state[(size_t)p] == 1;
		if (const char *bad = sw_args_bad(host_bytes, host_off, n_host, declined)) { err = bad; return 1; }
		const size_t base = restart ? 0 : window.size(), n_out = text.size() + (size_t)host_bytes;
		if ((long long)(base + n_out) >= window_bytes_max) { err = "a window of " + std::to_string(base + n_out) + " bytes"; return 2; }
		if (restart) window.clear(), win_pairs = win_host_pairs = 0;
		window.resize(base + n_out, '\xEE');
		sw_window_add_host(state.data(), toff.data(), n_front, (const uint8_t *)text.data(), (int64_t)text.size(), (const uint8_t *)host, host_off, n_host, (uint8_t *)&window[0], (int64_t)base);
		win_pairs += written + declined, win_host_pairs += n_host;
		info->n_bytes = (int64_t)window.size(), info->n_pairs = win_pairs, info->n_host_pairs = win_host_pairs;
		return 0;
	}
};

struct PrintingReader : SignalWindowTaker {
	MateWindowBackend &be;
	long long piece_pairs = 1 << 20, offers = 0, pieces = 0;
	explicit PrintingReader(MateWindowBackend &b) : be(b) { if (const char *e = getenv("PSVR_CHECK_PIECE_PAIRS")) piece_pairs = atoll(e); }
	long long offer(const psvr_signal_window_info_t &info, std::string *why) override
	{
		long long taken = 0;
		uint64_t at = 0;
		++offers;
		if ((size_t)info.n_bytes != be.window.size()) { *why = "the offer is not the kept window"; return 0; }
		while (taken < info.n_pairs) {
			if (be.failing("window_parse")) { *why = be.err; return taken; }
			FqHostResult r;
			fq_parse_host(be.window.data() + at, be.window.size() - at, 1, piece_pairs, (int64_t)1 << 60, &r);
			if (r.info.n_pairs < 1 || taken + r.info.n_pairs > info.n_pairs) { *why = "the window's text does not hold the pairs the route counted"; return taken; }
			fwrite(be.window.data() + at, 1, (size_t)r.info.used_bytes, stdout);
			at += (uint64_t)r.info.used_bytes, taken += r.info.n_pairs, ++pieces;
		}
		if (at != be.window.size()) { *why = "text behind the window's last pair"; return taken - 1; }
		return taken;
	}
};

int main(int argc, char **argv)
{
	return signal_main(argc, argv, nullptr, [](SignalStep &S, long long *pairs_done) {
		MateWindowBackend be;
		PrintingReader reader(be);
		const long long window_pairs = getenv("PSVR_CHECK_WINDOW_PAIRS") ? atoll(getenv("PSVR_CHECK_WINDOW_PAIRS")) : 1 << 20;
		if (const char *e = getenv("PSVR_CHECK_WINDOW_BYTES")) be.window_bytes_max = atoll(e);
		const int rc = signal_mate_route(be, S, pairs_done, nullptr, &reader, window_pairs, be.window_bytes_max);
		fflush(stdout);
		fprintf(stderr, "the reader was offered %lld windows and took %lld pieces\n", reader.offers, reader.pieces);
		if (rc > 0) {                                            // (SignalStep::run would abort(): the code is what the test looks at)
			fprintf(stderr, "route returned state %d behind %lld pairs\n", rc, *pairs_done);
			exit(30 + rc);
		}
		return rc;
	});
}
