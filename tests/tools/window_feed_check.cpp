// window_feed_check -- `panSVR aln -N --bam-device`'s hand-over without a GPU and without the engine library: WindowFeed, FastqReader::read_window /
// fail_windows and the signal step's thread (signal_step_thread, SignalStep::run) as cli_main.cpp puts them together, on two threads.  The calls
// read_window makes (psvr_fastq_parse_signal / download / text) are answered here by the host build of fastq_device.h, over a window that is a
// string in host memory.  Every mode must END (tests/test_window_feed.py runs each under a time limit: a hang is the failure this is about)
// and print what it saw.
//   window_feed_check feed <case>          WindowFeed alone: producer_ends, consumer_fails_first, consumer_fails_mid, consumer_aborts,
//                                          two_windows, closed_twice
//   window_feed_check step <in.bam> <signal.fq> <window pairs> <piece pairs> [<call>:<n>]
//       the signal step's thread over <in.bam> (-N -D) with a device route that offers <signal.fq> (the text of `panSVR signal -N -D`) in
//       windows of <window pairs> pairs; the reader takes pieces of <piece pairs> pairs and prints their text; <call> of the reader's side
//       (create: before the reader's first piece, n is ignored; parse_signal, download, text: at its n-th occurrence) fails.  stdout must be
//       <signal.fq> whatever fails; stderr says how the step ended ("step rc R, P pairs handed over before the route was left: WHY").
#include <atomic>
#include <string>
#include <thread>
#include <vector>
#include "../../pansvr_amd/csrc/signal_step.h"
#include "../../pansvr_amd/csrc/fastq_device.h"

using namespace psvr;

// ---- the engine library's calls, as far as this program's code reaches them
struct psvr_signal { std::string window; };
struct psvr_fastq { FqHostResult r; std::string text; };
static std::string g_err;
static std::string g_fail_call;
static long long g_fail_nth = 0;
static bool failing(const char *call)
{
	static std::atomic<long long> seen[3];
	const int k = !strcmp(call, "parse_signal") ? 0 : !strcmp(call, "download") ? 1 : 2;
	if (g_fail_call != call || ++seen[k] != g_fail_nth) return false;
	g_err = std::string("injected failure of ") + call;
	return true;
}
extern "C" {
const char *psvr_last_error(void) { return g_err.c_str(); }
void *psvr_host_alloc(size_t n) { return malloc(n); }
void psvr_host_free(void *p) { free(p); }
int psvr_fastq_parse(psvr_fastq_t *, const char *, int64_t, int, int64_t, int64_t, psvr_fastq_info_t *) { g_err = "not in this program"; return PSVR_ERR_UNSUPPORTED; }
int psvr_fastq_parse_signal(psvr_fastq_t *fq, const psvr_signal_t *sg, int64_t first_byte, int64_t max_pairs, int64_t max_bases, psvr_fastq_info_t *info)
{
	if (failing("parse_signal")) return PSVR_ERR_DEVICE;
	if (first_byte < 0 || first_byte > (int64_t)sg->window.size()) { g_err = "first_byte outside the window"; return PSVR_ERR_ARG; }
	fq->text.assign(sg->window, (size_t)first_byte, std::string::npos);
	fq_parse_host(fq->text.data(), fq->text.size(), 1, max_pairs, max_bases, &fq->r);
	*info = fq->r.info;
	return 0;
}
int psvr_fastq_download(const psvr_fastq_t *fq, uint64_t *line_start, uint16_t *name_end, int64_t *base_off, psvr_ori_t *ori, char *)
{
	if (failing("download")) return PSVR_ERR_DEVICE;
	const size_t R = (size_t)fq->r.info.n_pairs * 2;
	memcpy(line_start, fq->r.line_start.data(), (4 * R + 1) * 8);
	memcpy(name_end, fq->r.name_end.data(), R * 2);
	memcpy(base_off, fq->r.base_off.data(), (R + 1) * 8);
	memcpy(ori, fq->r.ori.data(), R * sizeof(psvr_ori_t));
	return 0;
}
int psvr_fastq_text(const psvr_fastq_t *fq, void *dst, int64_t first, int64_t n)
{
	if (failing("text")) return PSVR_ERR_DEVICE;
	memcpy(dst, fq->text.data() + first, (size_t)n);
	return 0;
}
}

// ---- WindowFeed alone
static int feed_case(const std::string &name)
{
	WindowFeed w;
	psvr_signal sg;
	const psvr_signal_t *got = nullptr;
	long long at = -1, left = -1;
	if (name == "producer_ends") {                           // the signal step ended in front of the route: the reader must not wait
		std::thread producer([&] { w.close(true); });
		const int r = w.next(&got, &at, &left);
		producer.join();
		printf("next %d\n", r);
	} else if (name == "consumer_fails_first") {             // the reader's parser could not be made: the first offer comes back at once
		std::string why;
		long long taken = -1;
		std::thread producer([&] { taken = w.offer(&sg, 10, &why); w.close(true); });
		w.fail("no parser");
		producer.join();
		printf("offer %lld (%s) next %d\n", taken, why.c_str(), w.next(&got, &at, &left));
	} else if (name == "consumer_fails_mid") {
		std::string why;
		long long taken = -1;
		std::thread producer([&] { taken = w.offer(&sg, 10, &why); w.close(true); });
		const int r1 = w.next(&got, &at, &left);
		printf("next %d at %lld left %lld same %d\n", r1, at, left, got == &sg);
		w.took(100, 4);
		const int r2 = w.next(&got, &at, &left);
		printf("next %d at %lld left %lld\n", r2, at, left);
		w.fail("piece 2");
		producer.join();
		printf("offer %lld (%s) next %d\n", taken, why.c_str(), w.next(&got, &at, &left));
	} else if (name == "consumer_aborts") {                  // the reader stopped early: the producer runs to its end unheard
		std::string why;
		long long first = -1, second = -1;
		std::thread producer([&] { first = w.offer(&sg, 10, &why); second = w.offer(&sg, 7, &why); w.close(false); });
		const int r1 = w.next(&got, &at, &left);
		w.took(30, 3);
		w.abort();
		producer.join();
		printf("next %d offers %lld %lld (%s)\n", r1, first, second, why.c_str());
	} else if (name == "two_windows") {
		std::string why;
		long long a = -1, b = -1, none = -1;
		std::thread producer([&] { a = w.offer(&sg, 5, &why); none = w.offer(&sg, 0, &why); b = w.offer(&sg, 3, &why); w.close(false); });
		int r;
		while ((r = w.next(&got, &at, &left)) == 1) { printf("at %lld left %lld\n", at, left); w.took(11, left > 2 ? 2 : left); }
		producer.join();
		printf("next %d offers %lld %lld %lld (%s)\n", r, a, none, b, why.c_str());
	} else if (name == "closed_twice") {                     // the route's word stands: the thread's close behind it changes nothing
		w.close(false), w.close(true);
		printf("next %d\n", w.next(&got, &at, &left));
	} else return 2;
	return 0;
}

// ---- the signal step's thread, a device route that offers windows, and the reader as aln's read stage runs it
static std::string read_file(const char *path)
{
	std::string s;
	FILE *f = fopen(path, "rb");
	if (!f) { fprintf(stderr, "cannot open %s\n", path); exit(2); }
	char buf[1 << 16];
	for (size_t n; (n = fread(buf, 1, sizeof buf, f)) > 0;) s.append(buf, n);
	fclose(f);
	return s;
}

static int step_case(int argc, char **argv)
{
	const std::string text = read_file(argv[3]);
	const long long window_pairs = atoll(argv[4]), piece_pairs = atoll(argv[5]);
	if (argc > 6) { const char *c = strchr(argv[6], ':'); g_fail_call.assign(argv[6], c ? (size_t)(c - argv[6]) : strlen(argv[6])); g_fail_nth = c ? atoll(c + 1) : 1; }
	std::vector<size_t> pair_at(1, 0);                       // where every pair's text starts (8 lines each)
	for (size_t i = 0, lines = 0; i < text.size(); ++i) if (text[i] == '\n' && ++lines % 8 == 0) pair_at.push_back(i + 1);
	const long long n_pairs = (long long)pair_at.size() - 1;
	SignalStep sig;
	PairFeed feed;
	WindowFeed windows;
	sig.o.sort_by_name = true, sig.o.not_use_filter = true, sig.o.input = argv[2], sig.o.status_fn = std::string(argv[3]) + ".status", sig.o.header_fn = std::string(argv[3]) + ".sam", sig.o.bam_device = true;
	sig.feed = &feed;
	long long handed = -1;
	std::string left_why;
	sig.signal_device_fn = [&](SignalStep &, long long *pairs_done) {
		psvr_signal sg;
		*pairs_done = 0;
		for (long long p = 0; p < n_pairs; p += window_pairs) {
			const long long n = p + window_pairs < n_pairs ? window_pairs : n_pairs - p;
			sg.window.assign(text, pair_at[(size_t)p], pair_at[(size_t)(p + n)] - pair_at[(size_t)p]);
			const long long taken = windows.offer(&sg, n, &left_why);
			*pairs_done += taken;
			if (taken != n) { handed = *pairs_done; windows.close(true); return -1; }
		}
		windows.close(false);
		return 0;
	};
	int sig_rc = -1;
	std::thread sig_thread = signal_step_thread(sig, feed, &windows, &sig_rc);
	FastqReader rd;
	rd.open_windows(&windows), rd.open_feed(&feed);
	FastqBatch B;
	HostBuf stage;
	psvr_fastq fq;
	bool on = true;                                          // aln_pipeline.h's parse_route.on
	long long pieces_dev = 0, pieces_host = 0;
	for (;;) {                                               // EngineDriver::parse_window and AlnPipeline::read_stage, without the engine
		bool ok = false;
		if (on) {
			std::string why;
			int r;
			if (g_fail_call == "create") rd.fail_windows("fastq create: injected failure of create"), r = -1;
			else r = rd.read_window(B, piece_pairs, (long long)1 << 60, &fq, stage, &why);
			if (r < 0) on = false;
			else ok = r > 0;
		}
		if (!on) ok = rd.read(B, piece_pairs, (long long)1 << 60, 1);
		if (!ok) break;
		++(B.dev ? pieces_dev : pieces_host);
		fwrite(B.text, 1, (size_t)B.ls[(size_t)(4 * B.R)], stdout);
	}
	windows.abort(), feed.abort();
	sig_thread.join();
	fflush(stdout);
	fprintf(stderr, "step rc %d, %lld pairs handed over before the route was left: %s\n", sig_rc, handed, left_why.c_str());
	fprintf(stderr, "pieces: %lld from windows, %lld from the feed\n", pieces_dev, pieces_host);
	return sig_rc ? 10 + sig_rc : 0;
}

int main(int argc, char **argv)
{
	if (argc == 3 && !strcmp(argv[1], "feed")) return feed_case(argv[2]);
	if (argc >= 6 && !strcmp(argv[1], "step")) return step_case(argc, argv);
	fprintf(stderr, "usage: window_feed_check feed <case> | step <in.bam> <signal.fq> <window pairs> <piece pairs> [<call>:<n>]\n");
	return 2;
}
