// signal_window_check -- the one-lane host build of pansvr_amd/csrc/signal_window_device.h (what k_sg_wflag, k_sg_wcut, k_sg_wseg and
// k_sg_window of signal.hip run) on a pair table and two texts from files.  A program of its own, built plain and with
// -fsanitize=address,undefined (tests/test_signal_window_rules.py compares the window with plain concatenation); every buffer has exactly its
// size, so a byte read or written outside one is the sanitizer's to report.
//   signal_window_check case.txt text.bin host.bin out.bin
// case.txt:  "n_front text_bytes host_bytes n_host"     then n_front lines "state toff"     then n_host + 1 offsets (none when n_host is 0)
// stdout: "refused: <reason>" (exit status 3: psvr_signal_window's PSVR_ERR_ARG), or the segment table, a line "src off len out" per segment.
#include <cstdio>
#include <cstdlib>
#include <memory>
#include <vector>
#include "../../pansvr_amd/csrc/signal_window_device.h"

using namespace psvr;

static std::unique_ptr<uint8_t[]> slurp(const char *path, long long n)
{
	std::unique_ptr<uint8_t[]> b(new uint8_t[(size_t)n]);        // (exactly n bytes, 16-byte aligned as the device's buffers are)
	FILE *f = fopen(path, "rb");
	if (!f || (n && fread(b.get(), 1, (size_t)n, f) != (size_t)n)) { fprintf(stderr, "cannot read %lld bytes of %s\n", n, path); exit(2); }
	fclose(f);
	return b;
}

int main(int argc, char **argv)
{
	if (argc != 5) { fprintf(stderr, "usage: signal_window_check case.txt text.bin host.bin out.bin\n"); return 2; }
	FILE *c = fopen(argv[1], "r");
	long long n_front, text_bytes, host_bytes, n_host;
	if (!c || fscanf(c, "%lld %lld %lld %lld", &n_front, &text_bytes, &host_bytes, &n_host) != 4 || n_front < 0 || text_bytes < 0) { fprintf(stderr, "cannot read %s\n", argv[1]); return 2; }
	std::unique_ptr<uint8_t[]> state(new uint8_t[(size_t)n_front]);
	std::unique_ptr<int64_t[]> toff(new int64_t[(size_t)n_front]);
	long long declined = 0;
	for (long long p = 0; p < n_front; ++p) {
		long long s, t;
		if (fscanf(c, "%lld %lld", &s, &t) != 2) { fprintf(stderr, "pair %lld\n", p); return 2; }
		state[(size_t)p] = (uint8_t)s, toff[(size_t)p] = t, declined += s == 2;
	}
	std::unique_ptr<int64_t[]> hoff;
	if (n_host > 0) {
		hoff.reset(new int64_t[(size_t)n_host + 1]);
		for (long long i = 0; i <= n_host; ++i) { long long v; if (fscanf(c, "%lld", &v) != 1) { fprintf(stderr, "offset %lld\n", i); return 2; } hoff[(size_t)i] = v; }
	}
	fclose(c);
	if (const char *bad = sw_args_bad(host_bytes, hoff.get(), n_host, declined)) { printf("refused: %s\n", bad); return 3; }
	const std::unique_ptr<uint8_t[]> text = slurp(argv[2], text_bytes), host = slurp(argv[3], host_bytes);
	const long long n_out = text_bytes + host_bytes;
	std::unique_ptr<uint8_t[]> out(new uint8_t[(size_t)n_out]);
	for (long long i = 0; i < n_out; ++i) out[(size_t)i] = 0xEE;
	const std::vector<SwSeg> seg = sw_window_host(state.get(), toff.get(), n_front, text.get(), text_bytes, host.get(), hoff.get(), n_host, out.get());
	for (const SwSeg &s : seg) printf("%d %lld %lld %lld\n", s.src, (long long)s.off, (long long)s.len, (long long)s.out);
	FILE *o = fopen(argv[4], "wb");
	if (!o || (n_out && fwrite(out.get(), 1, (size_t)n_out, o) != (size_t)n_out) || fclose(o)) { fprintf(stderr, "cannot write %s\n", argv[4]); return 2; }
	return 0;
}
