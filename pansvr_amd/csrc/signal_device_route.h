// signal_device_route.h -- `panSVR signal -N --signal-device`: the name-sorted signal step with its records in GPU memory.  Host C++ only, a
// template over the backend, as bam_sort.h's sort_device_route is: cli_main.cpp has the product's (psvr_bam_store_* and psvr_signal_*);
// tests/tools/signal_device_route_check.cpp has one that keeps the store in host memory and runs the rules of signal_device.h with one lane,
// so every rule in here runs without a GPU (tests/test_signal_device_route.py).
//
// The file's own BGZF members go to the device a piece of PSVR_INFLATE_BATCH compressed bytes at a time (bgzf_pieces.h).  Per piece:
//   store_append_bgzf     the members inflated into the record store, the records found there
//   signal_run            from the first record no earlier run consumed: pairs, states, notes, text (include/psvr_engine.h)
//   signal_pairs / text / side   the per-pair table, the text and -- in one piece -- the records of the pairs the host has to look at come back;
//                         the state-1 ranges go to S.out in pair order, a state-2 pair is formatted by SignalStep::pair from its downloaded
//                         records at its place; the wrong-ISIZE lines and the progress lines
//   store_drop            everything the run consumed ceases to exist: the store holds a piece's records and a carried one, whatever the file's length
// A pair in an error state (3, 4, 5): what lies in front of it is written and flushed, the device objects are destroyed, the host route's
// message for that state is printed, and the state is returned: SignalStep::run calls abort() on it as the host loop does.
// Leaving the route: a backend call fails, there is no device, the input is a pipe, a member is corrupt, a record is malformed, the end is
// truncated -- one line names the call and the reason, *pairs_done says how many pairs' text is on S.out, and -1 is returned: SignalStep::run
// reads the file from its beginning on the host route, muted for those pairs, so the statistics, the messages and the exit status are the
// host route's by construction.  0: done; S.bs holds the device's histograms and the count, the caller prints the last line.
//
// What a backend offers (every int is 0 or a status whose text last_error() gives):
//   int store_create() / void store_destroy() / int store_append_bgzf(const void *, int64_t n, int64_t skip, int32_t n_ref, int64_t *used, int64_t *bad_member)
//   int store_chain_info(psvr_bam_chain_info_t *) / int store_drop(int64_t n_front) / int store_footprint(int64_t *chunks, int64_t *bytes)
//   int signal_create(const psvr_signal_opt_t *) / void signal_destroy() / int signal_run(int64_t first_record, int finish, psvr_signal_info_t *)
//   int signal_text(void *, int64_t cap) / int signal_pairs(psvr_signal_pair_t *, int64_t cap)
//   int signal_side(void *bytes, int64_t cap) / int signal_stats(uint64_t *isize_n, uint64_t *len_n)
//   void *host_alloc(size_t) / void host_free(void *) / const char *last_error()
//
// The route has two consumers, and one body for both.  `panSVR signal` takes text: what is described above.  `panSVR aln -N --bam-device`
// takes windows (SignalWindowTaker below, window mode): the run's text is not downloaded; SignalStep::pair formats the state-2 pairs into a
// buffer with offsets instead of S.out; the backend's
//   int signal_window(const void *host_text, int64_t host_bytes, const int64_t *host_off, int64_t n_host, psvr_signal_window_info_t *)
// puts both together where the run's text lies (include/psvr_engine.h), and the taker is offered the window: it returns when the reader
// stage has taken every pair of it (or could not: the route is left then, like after any failing call).  *pairs_done counts the pairs, of any
// state, in front of which everything has been handed over.  The messages carry the command's name; everything else is one code.
#pragma once
#include <sys/stat.h>
#include <chrono>
#include <string>
#include <vector>
#include "../../include/psvr_engine.h"
#include "bgzf_pieces.h"
#include "signal_step.h"

namespace psvr {

// window mode: who takes the windows.  offer() blocks until the pairs are taken and returns how many were (info.n_pairs: all; fewer: *why
// says what failed on the taker's side).  The backend is the taker's to know: it reads the window out of the backend's signal object.
struct SignalWindowTaker {
	virtual ~SignalWindowTaker() {}
	virtual long long offer(const psvr_signal_window_info_t &info, std::string *why) = 0;
};

struct SignalRouteStats {
	long long pairs = 0, written = 0, declined = 0, runs = 0, text_bytes = 0, peak_chunks = 0, peak_bytes = 0;
	long long left_pairs = 0, last_chunks = 0, last_bytes = 0;   // --mate-device: pairs of the by-name pass; the store's footprint behind the last block
	double append_s = 0, mate_s = 0, fetch_s = 0, write_s = 0;   // --mate-device: wall seconds of the route's phases
	long long windows = 0, window_bytes = 0;                     // aln --mate-device: kept windows offered to the taker, and their bytes
};

inline psvr_signal_opt_t signal_device_options(const SignalStep &S)
{
	psvr_signal_opt_t o;
	o.gap_open = S.o.gap_open, o.gap_ex = S.o.gap_ex, o.gap_open2 = S.o.gap_open2, o.gap_ex2 = S.o.gap_ex2, o.match = S.o.match, o.mismatch = S.o.mismatch;
	o.max_tid = S.o.max_tid, o.not_use_filter = S.o.not_use_filter, o.discard_full_match = S.o.discard_full_match, o.isize_min = S.isize_min, o.isize_max = S.isize_max;
	o.stat[0] = S.bs.read_len, o.stat[1] = (int32_t)S.bs.min_i, o.stat[2] = (int32_t)S.bs.mid_i, o.stat[3] = (int32_t)S.bs.max_i;
	return o;
}

// the backend's window call, where it has one (the text consumer's backend needs none)
template <class Backend> auto signal_route_window(Backend &be, const void *t, int64_t n, const int64_t *off, int64_t n_host, psvr_signal_window_info_t *i, int) -> decltype(be.signal_window(t, n, off, n_host, i))
{
	return be.signal_window(t, n, off, n_host, i);
}
template <class Backend> int signal_route_window(Backend &, const void *, int64_t, const int64_t *, int64_t, psvr_signal_window_info_t *, long) { return PSVR_ERR_UNSUPPORTED; }

// the same for the add to the kept window (signal_mate_route in window mode)
template <class Backend> auto signal_route_window_add(Backend &be, const void *t, int64_t n, const int64_t *off, int64_t n_host, int32_t restart, psvr_signal_window_info_t *i, int)
	-> decltype(be.signal_window_add(t, n, off, n_host, restart, i))
{
	return be.signal_window_add(t, n, off, n_host, restart, i);
}
template <class Backend> int signal_route_window_add(Backend &, const void *, int64_t, const int64_t *, int64_t, int32_t, psvr_signal_window_info_t *, long) { return PSVR_ERR_UNSUPPORTED; }

// window mode of both routes: SignalStep::pair writes a state-2 pair's text here, with offsets (the fused command's S.feed and S.out are put
// back when the route ends)
struct SignalHostText {
	SignalStep &S; FILE *out; PairFeed *feed; char *buf = nullptr; size_t len = 0; FILE *mem = nullptr;
	std::vector<int64_t> off;
	SignalHostText(SignalStep &s, bool on) : S(s), out(s.out), feed(s.feed) { if (on && (mem = open_memstream(&buf, &len))) S.out = mem, S.feed = nullptr; }
	void restart() { fflush(mem); rewind(mem); off.assign(1, 0); }
	void pair_done() { fflush(mem); off.push_back((int64_t)ftello(mem)); }
	~SignalHostText() { S.out = out, S.feed = feed; if (mem) fclose(mem), free(buf); }
};

template <class Backend> int signal_device_route(Backend &be, SignalStep &S, long long *pairs_done, SignalRouteStats *stats = nullptr, SignalWindowTaker *taker = nullptr)
{
	*pairs_done = 0;
	SignalRouteStats R;
	auto left = [&](const std::string &call, const std::string &why) {
		if (taker) fprintf(stderr, "[panSVR-amd] aln --bam-device: %s failed (%s): %lld pairs are handed over, the host fused route reads the file from its beginning, silent up to there\n", call.c_str(),
		                   why.c_str(), *pairs_done);
		else fprintf(stderr, "[panSVR-amd] signal --signal-device: %s failed (%s): %lld pairs are written, the host route reads the file from its beginning, silent up to there\n", call.c_str(), why.c_str(),
		             *pairs_done);
		return -1;
	};
	struct stat sb;
	if (S.o.input == "-" || stat(S.o.input.c_str(), &sb) != 0 || !S_ISREG(sb.st_mode)) return left("opening the input", "a pipe cannot be read twice");
	size_t header_bytes = 0, n_ref = 0;
	{
		BamReader rd;                                            // the serial reader: how many inflated bytes the header took
		if (!rd.open(S.o.input.c_str())) return left("reading the header", rd.error());
		header_bytes = rd.header_bytes, n_ref = rd.refs.size();
	}
	FILE *f = fopen(S.o.input.c_str(), "rb");
	if (!f) return left("opening the input", "cannot open " + S.o.input);
	struct Closer {
		FILE *f; Backend &be; uint8_t *text, *side;
		~Closer() { fclose(f); if (text) be.host_free(text); if (side) be.host_free(side); be.signal_destroy(); be.store_destroy(); }
	} guard{f, be, nullptr, nullptr};
	PieceFail fail;
	long long skip = 0;
	if (!bgzf_seek_first_record(f, header_bytes, &skip, &fail)) return left(fail.call, fail.why);
	if (be.store_create()) return left("store create", be.last_error());
	const psvr_signal_opt_t opt = signal_device_options(S);
	if (be.signal_create(&opt)) return left("signal create", be.last_error());
	size_t text_cap = 0, side_cap = 0;
	std::vector<psvr_signal_pair_t> tab;
	int64_t side_bytes = 0;
	long long total = 0;                                         // S.bs.total of the host loop: two per pair
	int error_state = 0;
	bool any_written = false;
	// the two records of pair p of the last run as the host's reader holds them, out of the run's side records
	auto fetch = [&](int64_t p, BamRecord *a, BamRecord *b, PieceFail *why) {
		const int64_t at = tab[(size_t)p].side_off;
		const char *bad = at < 0 || at > side_bytes ? "the pair has no side records" : bam_record_from_bytes(guard.side + at, (size_t)(side_bytes - at), *a);
		const size_t n1 = bad ? 0 : 4 + (size_t)bam_u32(guard.side + at);
		if (!bad) bad = bam_record_from_bytes(guard.side + at + n1, (size_t)(side_bytes - at) - n1, *b);
		if (bad) { *why = {"signal side", bad}; return false; }
		return true;
	};
	// a page-locked buffer of at least n bytes
	auto room = [&](uint8_t **buf, size_t *cap, size_t n, PieceFail *why) {
		if (n <= *cap) return true;
		if (*buf) be.host_free(*buf), *buf = nullptr, *cap = 0;
		if (!(*buf = (uint8_t *)be.host_alloc(n + n / 4))) { *why = {"host_alloc", be.last_error()}; return false; }
		*cap = n + n / 4;
		return true;
	};
	auto write_out = [&](const uint8_t *p, size_t n) { if (n) fwrite(p, 1, n, S.out); };
	SignalHostText host_text(S, taker != nullptr);
	if (taker && !host_text.mem) return left("open_memstream", "out of memory");
	const bool walked = bgzf_for_pieces(be, f, skip, &fail, [&](const uint8_t *p, size_t have, long long skip_now, int64_t *used, PieceFail *why) {
		int64_t bad = -1;
		if (be.store_append_bgzf(p, (int64_t)have, skip_now, (int32_t)n_ref, used, &bad)) { *why = {"append_bgzf", be.last_error()}; return false; }
		int64_t chunks = 0, bytes = 0;
		if (be.store_footprint(&chunks, &bytes)) { *why = {"store footprint", be.last_error()}; return false; }
		if (chunks > R.peak_chunks) R.peak_chunks = chunks;
		if (bytes > R.peak_bytes) R.peak_bytes = bytes;
		psvr_signal_info_t info;
		// (the store's front is what no run has consumed: a lone last primary record and what lies behind it)
		if (be.signal_run(0, 0, &info)) { *why = {"signal run", be.last_error()}; return false; }
		++R.runs;
		tab.resize((size_t)info.pairs);
		if (info.pairs && be.signal_pairs(tab.data(), info.pairs)) { *why = {"signal pairs", be.last_error()}; return false; }
		if ((!taker && !room(&guard.text, &text_cap, (size_t)info.text_bytes, why)) || !room(&guard.side, &side_cap, (size_t)info.side_bytes, why)) return false;
		if (!taker && info.text_bytes && be.signal_text(guard.text, (int64_t)text_cap)) { *why = {"signal text", be.last_error()}; return false; }
		if (taker) host_text.restart();
		if (info.side_bytes && be.signal_side(guard.side, (int64_t)side_cap)) { *why = {"signal side", be.last_error()}; return false; }
		side_bytes = info.side_bytes;
		// the pairs in order: text ranges of state-1 pairs as they lie, a state-2 pair from the host formatter at its place
		const int64_t n_front = info.first_error >= 0 ? info.first_error : info.pairs;
		int64_t flushed = 0;                                     // text bytes of this run that are on S.out
		BamRecord a, b;
		auto flush_to = [&](int64_t q) {                         // the text in front of pair q is on S.out, and *pairs_done says so
			if (taker) return;                                   // (window mode: nothing is handed over before the window is)
			const int64_t upto = q < info.pairs ? tab[(size_t)q].text_off : info.text_bytes;
			write_out(guard.text + flushed, (size_t)(upto - flushed)), flushed = upto;
			*pairs_done = R.pairs + q;
		};
		for (int64_t q = 0; q < n_front; ++q) {
			const psvr_signal_pair_t &t = tab[(size_t)q];
			total += 2;
			if (total % 100000 == 0) fprintf(stderr, "%ld\r", (long)total);
			if (t.state == 2) {
				flush_to(q);
				if (!fetch(q, &a, &b, why)) return false;
				S.stat_written = any_written;
				S.pair(a, b, true);
				any_written = true, ++R.declined;
				if (taker) host_text.pair_done();
				else *pairs_done = R.pairs + q + 1;
				continue;
			}
			if (t.note & 1) {
				flush_to(q);
				if (!fetch(q, &a, &b, why)) return false;
				fprintf(stderr, " wrong ISIZE: %d  %d \n", a.isize, b.isize);
			}
			if (t.state == 1) any_written = true, ++R.written;
		}
		flush_to(n_front);
		if (taker) {                                             // the window: the run's text and the host's, in pair order, offered to the reader
			psvr_signal_window_info_t wi;
			const int64_t n_host = (int64_t)host_text.off.size() - 1, host_bytes = host_text.off.back();
			if (signal_route_window(be, host_text.buf, host_bytes, host_text.off.data(), n_host, &wi, 0)) { *why = {"signal window", be.last_error()}; return false; }
			std::string taker_why;
			const long long taken = taker->offer(wi, &taker_why);
			if (taken != wi.n_pairs) {                           // the pairs in front of the first one that was not taken are handed over
				long long seen = 0;
				int64_t q = 0;
				for (; q < n_front && seen < taken; ++q) seen += tab[(size_t)q].state == 1 || tab[(size_t)q].state == 2;
				*pairs_done = R.pairs + q;
				*why = {"taking a window", taker_why};
				return false;
			}
			*pairs_done = R.pairs + n_front;
			R.text_bytes += wi.n_bytes - info.text_bytes;
		}
		R.pairs += n_front, R.text_bytes += info.text_bytes;
		if (info.first_error >= 0) {                             // the pair the host loop aborts on
			const psvr_signal_pair_t &t = tab[(size_t)info.first_error];
			fflush(S.out);
			error_state = t.state;
			std::string n1 = "?", n2 = "?";
			int i1 = 0, i2 = 0;
			PieceFail ignored;
			if (fetch(info.first_error, &a, &b, &ignored)) n1 = a.qname(), n2 = b.qname(), i1 = a.isize, i2 = b.isize;
			if (t.state == 3) fprintf(stderr, "[panSVR-amd] signal: consecutive records [%s] [%s] are not a pair: is the input sorted by name?\n", n1.c_str(), n2.c_str());
			else if (t.state == 4) fprintf(stderr, "[panSVR-amd] signal: records of [%s] are not first/second in template\n", n1.c_str());
			else {
				total += 2;
				if (total % 100000 == 0) fprintf(stderr, "%ld\r", (long)total);
				if (t.note & 1) fprintf(stderr, " wrong ISIZE: %d  %d \n", i1, i2);
				fprintf(stderr, "[panSVR-amd] signal: read longer than 2047 bases\n");
			}
			*why = {"", ""};
			return false;
		}
		if (be.store_drop(info.consumed)) { *why = {"store drop", be.last_error()}; return false; }
		return true;
	});
	if (error_state) return error_state;
	if (!walked) return left(fail.call, fail.why);
	psvr_bam_chain_info_t ci;
	if (be.store_chain_info(&ci)) return left("chain_info", be.last_error());
	if (ci.tail_bytes) return left("the end of the input", "truncated BAM stream: the file ends " + std::to_string((long long)ci.tail_bytes) + " bytes into a record");
	if (be.signal_stats(S.bs.isize_n.data(), S.bs.len_n.data())) return left("signal stats", be.last_error());
	S.bs.total = (uint64_t)total;
	if (taker) fprintf(stderr, "[panSVR-amd] aln --bam-device: %lld pairs, %lld formatted on the device, %lld formatted by the host, %lld runs, %lld window bytes, peak footprint %lld chunks (%lld bytes)\n", R.pairs,
	                   R.written, R.declined, R.runs, R.text_bytes, R.peak_chunks, R.peak_bytes);
	else fprintf(stderr, "[panSVR-amd] signal --signal-device: %lld pairs, %lld written on the device, %lld declined to the host, %lld runs, %lld text bytes, peak footprint %lld chunks (%lld bytes)\n", R.pairs, R.written,
	             R.declined, R.runs, R.text_bytes, R.peak_chunks, R.peak_bytes);
	if (stats) *stats = R;
	return 0;
}

// ---- `panSVR signal --mate-device`: the position-sorted mode (SignalStep::run_pos_sorted) over the same backend plus
//   int signal_run_pos(int64_t first_record, int finish, const psvr_signal_pos_opt_t *, psvr_signal_info_t *, psvr_signal_pos_info_t *)
//   int signal_mate_notes(psvr_signal_mate_note_t *, int64_t cap)
//   int signal_run_left(int64_t first_pair, int64_t max_pairs, psvr_signal_info_t *, psvr_signal_left_info_t *) / int signal_left_errors(int64_t *, int64_t cap)
// Pieces are appended until signal_run_pos reports a complete block (a piece may hold several); behind the last piece it is asked with
// finish = 1 until fewer than two primaries are left.  Per block: the "Mate failed" lines from the notes, the WARNING line from the counts,
// the pairs as on the -N route (progress in the position mode's form, and counted in front of the template test as that loop does),
// store_drop; the unmated records stay on the device, in the signal object's left store.  Behind the last block the two `phase 2:` lines,
// then signal_run_left slice by slice (--block-records pairs a slice at the most; the call takes fewer where the text would reach 2 GiB), the pairing-error lines at their
// places from signal_left_errors.  *pairs_done counts SignalStep::pair calls, which is what run_pos_sorted is muted by; leaving and the
// error states 4 and 5 work as above.  An odd number of left-overs is the call's to decline: the host route reads the file and ends as it does.
// R (and the summary line) carries the phases' wall times: append (read, upload, inflate, chain), mate (run_pos, run_left), fetch (tables,
// text, side records), write (S.out, the host-formatted pairs).
//
// The route has the same two consumers as the one above, and one body for both.  `panSVR aln --mate-device` takes windows: a run's text is
// not downloaded; SignalStep::pair formats the state-2 pairs into SignalHostText; the backend's
//   int signal_window_add(const void *host_text, int64_t host_bytes, const int64_t *host_off, int64_t n_host, int32_t restart, psvr_signal_window_info_t *)
// writes the run's window behind what the kept window holds (include/psvr_engine.h), so the many small blocks of a position-sorted file
// become few windows.  The kept window is offered to the taker when it holds window_pairs pairs, before an add that would take it to 2^32
// bytes (window_bytes_max: that add restarts it), in front of an error pair, and behind the last slice -- not between phase 1 and phase 2.  *pairs_done
// advances only when an offer returns; after a partial take it is translated back through the added runs' pairs (Kept::has_text).
template <class Backend> int signal_mate_route(Backend &be, SignalStep &S, long long *pairs_done, SignalRouteStats *stats = nullptr, SignalWindowTaker *taker = nullptr, long long window_pairs = 1,
                                               long long window_bytes_max = (long long)1 << 32)
{
	*pairs_done = 0;
	SignalRouteStats R;
	auto left_route = [&](const std::string &call, const std::string &why) {
		if (taker) fprintf(stderr, "[panSVR-amd] aln --mate-device: %s failed (%s): %lld pairs are handed over, the host fused route reads the file from its beginning, silent up to there\n", call.c_str(),
		                   why.c_str(), *pairs_done);
		else fprintf(stderr, "[panSVR-amd] signal --mate-device: %s failed (%s): %lld pairs are written, the host route reads the file from its beginning, silent up to there\n", call.c_str(), why.c_str(),
		             *pairs_done);
		return -1;
	};
	struct Clock {
		double *into; std::chrono::steady_clock::time_point t0 = std::chrono::steady_clock::now();
		~Clock() { *into += std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count(); }
	};
	struct stat sb;
	if (S.o.input == "-" || stat(S.o.input.c_str(), &sb) != 0 || !S_ISREG(sb.st_mode)) return left_route("opening the input", "a pipe cannot be read twice");
	size_t header_bytes = 0, n_ref = 0;
	{
		BamReader rd;
		if (!rd.open(S.o.input.c_str())) return left_route("reading the header", rd.error());
		header_bytes = rd.header_bytes, n_ref = rd.refs.size();
	}
	FILE *f = fopen(S.o.input.c_str(), "rb");
	if (!f) return left_route("opening the input", "cannot open " + S.o.input);
	struct Closer {
		FILE *f; Backend &be; uint8_t *text, *side;
		~Closer() { fclose(f); if (text) be.host_free(text); if (side) be.host_free(side); be.signal_destroy(); be.store_destroy(); }
	} guard{f, be, nullptr, nullptr};
	PieceFail fail;
	long long skip = 0;
	if (!bgzf_seek_first_record(f, header_bytes, &skip, &fail)) return left_route(fail.call, fail.why);
	if (be.store_create()) return left_route("store create", be.last_error());
	const psvr_signal_opt_t opt = signal_device_options(S);
	if (be.signal_create(&opt)) return left_route("signal create", be.last_error());
	const psvr_signal_pos_opt_t popt = {S.o.block_records, 0};
	size_t text_cap = 0, side_cap = 0;
	std::vector<psvr_signal_pair_t> tab;
	std::vector<psvr_signal_mate_note_t> notes;
	std::vector<int64_t> errs;
	int64_t side_bytes = 0;
	long long total = 0, errs_printed = 0;
	int error_state = 0;
	bool any_written = false;
	auto fetch = [&](int64_t p, BamRecord *a, BamRecord *b, PieceFail *why) {
		const int64_t at = tab[(size_t)p].side_off;
		const char *bad = at < 0 || at > side_bytes ? "the pair has no side records" : bam_record_from_bytes(guard.side + at, (size_t)(side_bytes - at), *a);
		const size_t n1 = bad ? 0 : 4 + (size_t)bam_u32(guard.side + at);
		if (!bad) bad = bam_record_from_bytes(guard.side + at + n1, (size_t)(side_bytes - at) - n1, *b);
		if (bad) { *why = {"signal side", bad}; return false; }
		return true;
	};
	auto room = [&](uint8_t **buf, size_t *cap, size_t n, PieceFail *why) {
		if (n <= *cap) return true;
		if (*buf) be.host_free(*buf), *buf = nullptr, *cap = 0;
		if (!(*buf = (uint8_t *)be.host_alloc(n + n / 4))) { *why = {"host_alloc", be.last_error()}; return false; }
		*cap = n + n / 4;
		return true;
	};
	SignalHostText host_text(S, taker != nullptr);
	if (taker && !host_text.mem) return left_route("open_memstream", "out of memory");
	// window mode: the kept window -- the pairs in front of it, and per pair added since its restart whether the window holds text of it
	struct Kept {
		bool open = false;
		psvr_signal_window_info_t info = {0, 0, 0};
		long long first_pair = 0;
		std::vector<uint8_t> has_text;
	} kept;
	// the kept window goes to the taker; behind it the next add restarts.  false: fewer pairs were taken, *pairs_done says how far
	auto offer = [&](PieceFail *why) {
		if (!kept.open) return true;
		std::string taker_why;
		const long long taken = kept.info.n_pairs > 0 ? taker->offer(kept.info, &taker_why) : 0;
		if (kept.info.n_pairs > 0) ++R.windows, R.window_bytes += kept.info.n_bytes;
		if (taken != kept.info.n_pairs) {                        // the pairs in front of the first one that was not taken are handed over
			long long seen = 0;
			size_t q = 0;
			for (; q < kept.has_text.size() && seen < taken; ++q) seen += kept.has_text[q];
			*pairs_done = kept.first_pair + (long long)q;
			*why = {"taking a window", taker_why};
			return false;
		}
		*pairs_done = kept.first_pair + (long long)kept.has_text.size();
		kept.open = false;
		return true;
	};
	auto progress = [&]() { total += 2; if (total % 100000 == 0) fprintf(stderr, "%ld\n", (long)total); };
	// the pairing-error steps in front of pair q of a slice (errs: signal_left_errors; empty for a block)
	auto error_steps = [&](long long upto) {
		for (; errs_printed < upto; ++errs_printed) {
			progress();
			fprintf(stderr, "Read Pairing error!, reads names are not same, please confirm the completeness of BAM/CRAM file.\n");
		}
	};
	// the pairs of the last run (a block's or a slice's): table, text and side records come back, the text goes out in pair order with the
	// host-formatted pairs at their places.  false: *why says which call failed, or error_state is set (and *why is empty)
	auto pairs_out = [&](const psvr_signal_info_t &info, bool slice, PieceFail *why) {
		{
			Clock clock{&R.fetch_s};
			tab.resize((size_t)info.pairs);
			if (info.pairs && be.signal_pairs(tab.data(), info.pairs)) { *why = {"signal pairs", be.last_error()}; return false; }
			errs.assign(slice ? (size_t)info.pairs : 0, 0);
			if (slice && info.pairs && be.signal_left_errors(errs.data(), info.pairs)) { *why = {"signal left_errors", be.last_error()}; return false; }
			if ((!taker && !room(&guard.text, &text_cap, (size_t)info.text_bytes, why)) || !room(&guard.side, &side_cap, (size_t)info.side_bytes, why)) return false;
			if (!taker && info.text_bytes && be.signal_text(guard.text, (int64_t)text_cap)) { *why = {"signal text", be.last_error()}; return false; }
			if (info.side_bytes && be.signal_side(guard.side, (int64_t)side_cap)) { *why = {"signal side", be.last_error()}; return false; }
			side_bytes = info.side_bytes;
		}
		Clock clock{&R.write_s};
		if (taker) host_text.restart();
		const int64_t n_front = info.first_error >= 0 ? info.first_error : info.pairs;
		int64_t flushed = 0;
		BamRecord a, b;
		auto flush_to = [&](int64_t q) {
			if (taker) return;                                   // (window mode: nothing is handed over before a window is)
			const int64_t upto = q < info.pairs ? tab[(size_t)q].text_off : info.text_bytes;
			if (upto > flushed) fwrite(guard.text + flushed, 1, (size_t)(upto - flushed), S.out);
			flushed = upto;
			*pairs_done = R.pairs + q;
		};
		for (int64_t q = 0; q < n_front; ++q) {
			const psvr_signal_pair_t &t = tab[(size_t)q];
			if (slice) error_steps(errs[(size_t)q]);
			progress();
			if (t.state == 2) {
				flush_to(q);
				if (!fetch(q, &a, &b, why)) return false;
				S.stat_written = any_written;
				S.pair(a, b, true);
				any_written = true, ++R.declined;
				if (taker) host_text.pair_done();
				else *pairs_done = R.pairs + q + 1;
				continue;
			}
			if (t.note & 1) {
				flush_to(q);
				if (!fetch(q, &a, &b, why)) return false;
				fprintf(stderr, " wrong ISIZE: %d  %d \n", a.isize, b.isize);
			}
			if (t.state == 1) any_written = true, ++R.written;
		}
		flush_to(n_front);
		if (taker) {                                             // the run's window behind what the kept window holds
			const int64_t n_host = (int64_t)host_text.off.size() - 1, host_bytes = host_text.off.back();
			if (kept.open && kept.info.n_bytes + info.text_bytes + host_bytes >= window_bytes_max && !offer(why)) return false;
			const bool restart = !kept.open;
			psvr_signal_window_info_t wi;
			if (signal_route_window_add(be, host_text.buf, host_bytes, host_text.off.data(), n_host, restart ? 1 : 0, &wi, 0)) { *why = {"signal window_add", be.last_error()}; return false; }
			if (restart) kept.first_pair = R.pairs, kept.has_text.clear();
			kept.open = true, kept.info = wi;
			for (int64_t q = 0; q < n_front; ++q) kept.has_text.push_back(tab[(size_t)q].state == 1 || tab[(size_t)q].state == 2);
		}
		R.pairs += n_front, R.text_bytes += info.text_bytes;
		if (slice) R.left_pairs += n_front;
		if (taker && (kept.info.n_pairs >= window_pairs || info.first_error >= 0) && !offer(why)) return false;
		if (info.first_error < 0) return true;
		const psvr_signal_pair_t &t = tab[(size_t)info.first_error];   // the pair the host loop aborts on
		fflush(S.out);
		error_state = t.state;
		std::string n1 = "?";
		int i1 = 0, i2 = 0;
		PieceFail ignored;
		if (fetch(info.first_error, &a, &b, &ignored)) n1 = a.qname(), i1 = a.isize, i2 = b.isize;
		if (slice) error_steps(errs[(size_t)info.first_error]);
		progress();
		if (t.state == 5) {
			if (t.note & 1) fprintf(stderr, " wrong ISIZE: %d  %d \n", i1, i2);
			fprintf(stderr, "[panSVR-amd] signal: read longer than 2047 bases\n");
		} else fprintf(stderr, "[panSVR-amd] signal: records of [%s] are not first/second in template\n", n1.c_str());
		*why = {"", ""};
		return false;
	};
	// the blocks that are complete in the store
	auto blocks = [&](int finish, PieceFail *why) {
		for (;;) {
			psvr_signal_info_t info;
			psvr_signal_pos_info_t pi;
			{
				Clock clock{&R.mate_s};
				if (be.signal_run_pos(0, finish, &popt, &info, &pi)) { *why = {"signal run_pos", be.last_error()}; return false; }
			}
			if (!pi.complete) return true;
			if (pi.primaries < 2) {
				if (be.store_drop(pi.consumed)) { *why = {"store drop", be.last_error()}; return false; }
				return true;
			}
			++R.runs;
			notes.resize((size_t)pi.notes);
			if (pi.notes && be.signal_mate_notes(notes.data(), pi.notes)) { *why = {"signal mate_notes", be.last_error()}; return false; }
			for (const psvr_signal_mate_note_t &t : notes)
				fprintf(stderr, "NUM: [%lld]: Mate failed, index:[%d] in [%d] size block, tid: [ %d ], pos [%d] name [%s]\n", (long long)t.number, t.index, t.block, t.tid, t.pos, t.name);
			if (pi.unmated * 20 > pi.primaries) fprintf(stderr, "WARNING, too many total_unmated_read![ %d %d %f]\n", (int)pi.unmated, (int)pi.primaries, (float)(int)pi.unmated / (float)(int)pi.primaries);
			if (!pairs_out(info, false, why)) return false;
			if (be.store_drop(pi.consumed)) { *why = {"store drop", be.last_error()}; return false; }
			int64_t chunks = 0, bytes = 0;
			if (be.store_footprint(&chunks, &bytes)) { *why = {"store footprint", be.last_error()}; return false; }
			R.last_chunks = chunks, R.last_bytes = bytes;
		}
	};
	const bool walked = bgzf_for_pieces(be, f, skip, &fail, [&](const uint8_t *p, size_t have, long long skip_now, int64_t *used, PieceFail *why) {
		int64_t bad = -1;
		{
			Clock clock{&R.append_s};
			if (be.store_append_bgzf(p, (int64_t)have, skip_now, (int32_t)n_ref, used, &bad)) { *why = {"append_bgzf", be.last_error()}; return false; }
		}
		int64_t chunks = 0, bytes = 0;
		if (be.store_footprint(&chunks, &bytes)) { *why = {"store footprint", be.last_error()}; return false; }
		if (chunks > R.peak_chunks) R.peak_chunks = chunks;
		if (bytes > R.peak_bytes) R.peak_bytes = bytes;
		return blocks(0, why);
	});
	if (error_state) return error_state;
	if (!walked) return left_route(fail.call, fail.why);
	psvr_bam_chain_info_t ci;
	if (be.store_chain_info(&ci)) return left_route("chain_info", be.last_error());
	if (ci.tail_bytes) return left_route("the end of the input", "truncated BAM stream: the file ends " + std::to_string((long long)ci.tail_bytes) + " bytes into a record");
	if (!blocks(1, &fail)) return error_state ? error_state : left_route(fail.call, fail.why);
	// phase 2: the left store in the host comparator's order, a slice of its pairs at a time
	psvr_signal_left_info_t li;
	for (int64_t first = 0;;) {
		psvr_signal_info_t info;
		{
			Clock clock{&R.mate_s};
			if (be.signal_run_left(first, S.o.block_records, &info, &li)) return left_route("signal run_left", be.last_error());
		}
		if (first == 0) fprintf(stderr, "phase 2:\nSort all unpaired records: [%zu] in total\n", (size_t)li.records);
		if (!pairs_out(info, true, &fail)) return error_state ? error_state : left_route(fail.call, fail.why);
		if (!li.more) break;
		first += li.n_pairs;
	}
	error_steps(li.errors);
	if (taker && !offer(&fail)) return left_route(fail.call, fail.why);   // what the kept window still holds
	if (be.signal_stats(S.bs.isize_n.data(), S.bs.len_n.data())) return left_route("signal stats", be.last_error());
	S.bs.total = (uint64_t)total;
	if (taker) fprintf(stderr, "[panSVR-amd] aln --mate-device: %lld pairs, %lld formatted on the device, %lld formatted by the host, %lld paired by name, %lld blocks, %lld windows offered, %lld window bytes, peak footprint %lld chunks (%lld bytes), %lld chunks (%lld bytes) behind the last block; append %.3f s, mate %.3f s, fetch %.3f s, write %.3f s\n",
	                   R.pairs, R.written, R.declined, R.left_pairs, R.runs, R.windows, R.window_bytes, R.peak_chunks, R.peak_bytes, R.last_chunks, R.last_bytes, R.append_s, R.mate_s, R.fetch_s, R.write_s);
	else fprintf(stderr, "[panSVR-amd] signal --mate-device: %lld pairs, %lld written on the device, %lld declined to the host, %lld paired by name, %lld blocks, %lld text bytes, peak footprint %lld chunks (%lld bytes), %lld chunks (%lld bytes) behind the last block; append %.3f s, mate %.3f s, fetch %.3f s, write %.3f s\n",
	        R.pairs, R.written, R.declined, R.left_pairs, R.runs, R.text_bytes, R.peak_chunks, R.peak_bytes, R.last_chunks, R.last_bytes, R.append_s, R.mate_s, R.fetch_s, R.write_s);
	if (stats) *stats = R;
	return 0;
}

} // namespace psvr
