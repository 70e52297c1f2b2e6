// signal_window_add_check -- the one-lane host build of the add rule of pansvr_amd/csrc/signal_window_device.h (what psvr_signal_window_add's
// kernels run: a run's window written behind the bytes a kept window holds) on a sequence of runs from files.  A program of its own, built
// plain and with -fsanitize=address,undefined (tests/test_signal_window_add_rules.py compares the kept window with plain concatenation of
// the runs' windows).  The window buffer has exactly the bytes the accepted adds need and lies between two guard blocks; it is filled with
// the guard byte, and after every add everything outside the add's own bytes must be what it was.
//   signal_window_add_check out.bin {restart case.txt text.bin host.bin}...
// case.txt is signal_window_check's: "n_front text_bytes host_bytes n_host", n_front lines "state toff", n_host + 1 offsets (none when 0).
// stdout, a line per add: "refused: <reason>" (psvr_signal_window_add's PSVR_ERR_ARG; the window stays as it is), or
// "added <base> <n_out> <total bytes> <total pairs> <total host pairs>".  Exit status 4: an add touched a byte that is not its own.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <vector>
#include "../../pansvr_amd/csrc/signal_window_device.h"

using namespace psvr;

static const uint8_t kGuard = 0xEE;
static const long long kGuardBytes = 64;

struct Run {
	int restart = 0;
	long long n_front = 0, text_bytes = 0, host_bytes = 0, n_host = 0, declined = 0, written = 0;
	std::unique_ptr<uint8_t[]> state, text, host;
	std::unique_ptr<int64_t[]> toff, hoff;
	const char *bad = nullptr;
};

static std::unique_ptr<uint8_t[]> slurp(const char *path, long long n)
{
	std::unique_ptr<uint8_t[]> b(new uint8_t[(size_t)n]);        // (exactly n bytes)
	FILE *f = fopen(path, "rb");
	if (!f || (n && fread(b.get(), 1, (size_t)n, f) != (size_t)n)) { fprintf(stderr, "cannot read %lld bytes of %s\n", n, path); exit(2); }
	fclose(f);
	return b;
}

static void read_run(Run &r, char **argv)
{
	r.restart = atoi(argv[0]);
	FILE *c = fopen(argv[1], "r");
	if (!c || fscanf(c, "%lld %lld %lld %lld", &r.n_front, &r.text_bytes, &r.host_bytes, &r.n_host) != 4 || r.n_front < 0 || r.text_bytes < 0) { fprintf(stderr, "cannot read %s\n", argv[1]); exit(2); }
	r.state.reset(new uint8_t[(size_t)r.n_front]), r.toff.reset(new int64_t[(size_t)r.n_front]);
	for (long long p = 0; p < r.n_front; ++p) {
		long long s, t;
		if (fscanf(c, "%lld %lld", &s, &t) != 2) { fprintf(stderr, "pair %lld\n", p); exit(2); }
		r.state[(size_t)p] = (uint8_t)s, r.toff[(size_t)p] = t, r.declined += s == 2, r.written += s == 1;
	}
	if (r.n_host > 0) {
		r.hoff.reset(new int64_t[(size_t)r.n_host + 1]);
		for (long long i = 0; i <= r.n_host; ++i) {
			long long v;
			if (fscanf(c, "%lld", &v) != 1) {
				if (i == 0) { r.hoff.reset(); break; }               // (host pairs and not one offset: the call's null pointer)
				fprintf(stderr, "offset %lld\n", i);
				exit(2);
			}
			r.hoff[(size_t)i] = v;
		}
	}
	fclose(c);
	r.bad = sw_args_bad(r.host_bytes, r.hoff.get(), r.n_host, r.declined);
	if (r.bad) return;
	r.text = slurp(argv[2], r.text_bytes), r.host = slurp(argv[3], r.host_bytes);
}

int main(int argc, char **argv)
{
	if (argc < 2 || (argc - 2) % 4) { fprintf(stderr, "usage: signal_window_add_check out.bin {restart case.txt text.bin host.bin}...\n"); return 2; }
	std::vector<Run> runs((size_t)(argc - 2) / 4);
	long long cap = 0, at = 0;                                   // the largest window the accepted adds make
	for (size_t k = 0; k < runs.size(); ++k) {
		read_run(runs[k], argv + 2 + 4 * k);
		if (runs[k].bad) continue;
		if (runs[k].restart) at = 0;
		at += runs[k].text_bytes + runs[k].host_bytes;
		if (at > cap) cap = at;
	}
	// guard | window[cap] | guard in one allocation, and a copy to compare with
	std::unique_ptr<uint8_t[]> buf(new uint8_t[(size_t)(cap + 2 * kGuardBytes)]), was(new uint8_t[(size_t)(cap + 2 * kGuardBytes)]);
	memset(buf.get(), kGuard, (size_t)(cap + 2 * kGuardBytes));
	uint8_t *win = buf.get() + kGuardBytes;
	long long bytes = 0, pairs = 0, host_pairs = 0;
	for (const Run &r : runs) {
		if (r.bad) { printf("refused: %s\n", r.bad); continue; }
		if (r.restart) bytes = pairs = host_pairs = 0, memset(win, kGuard, (size_t)cap);
		memcpy(was.get(), buf.get(), (size_t)(cap + 2 * kGuardBytes));
		const long long base = bytes, n_out = r.text_bytes + r.host_bytes;
		sw_window_add_host(r.state.get(), r.toff.get(), r.n_front, r.text.get(), r.text_bytes, r.host.get(), r.hoff.get(), r.n_host, win, base);
		for (long long i = 0; i < cap + 2 * kGuardBytes; ++i) {
			const long long w = i - kGuardBytes;
			if (w >= base && w < base + n_out) continue;
			if (buf[(size_t)i] != was[(size_t)i]) { fprintf(stderr, "the add at %lld of %lld bytes changed window byte %lld\n", base, n_out, w); return 4; }
		}
		bytes += n_out, pairs += r.written + r.declined, host_pairs += r.n_host;
		printf("added %lld %lld %lld %lld %lld\n", base, n_out, bytes, pairs, host_pairs);
	}
	FILE *o = fopen(argv[1], "wb");
	if (!o || (bytes && fwrite(win, 1, (size_t)bytes, o) != (size_t)bytes) || fclose(o)) { fprintf(stderr, "cannot write %s\n", argv[1]); return 2; }
	return 0;
}
