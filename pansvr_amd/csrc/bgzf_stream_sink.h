// bgzf_stream_sink.h -- the writer of `panSVR aln --stream-device`'s main file: the BAM stream is gathered in a device-resident BGZF stream
// (psvr_bgzf_stream_*, include/psvr_engine.h) instead of in BgzfWriter's page-locked buffer, so that the records the device encoded go from
// the encoder to the compressor without leaving HBM.  Host C++ only, a template over the stream backend: cli_main.cpp has the product's, over
// psvr_bgzf_stream_* and the pipeline slots' emitters; tests/tools/sink_host.h has one that keeps the stream in host memory
// and makes the members with the encoder's host build, so every rule in here runs without a GPU (tests/test_bgzf_stream_sink.py).
//
// The sink owns the file.  What reaches it, in stream order: the BAM header (open), then per piece its chunks -- device_chunks(slot, p0, p1)
// for a run of adjacent chunks whose records lie in the slot's emitter, host_chunk(bytes) for a chunk the host formatted -- and piece_done(),
// which waits for the queued appends (the slot's emitter is free again) and, once take_members or more members are pending, takes them into
// page-locked memory and writes them.  close() takes the tail as a last, shorter member and writes the EOF block.
//
// Leaving the device route.  Any failed stream call ends it for the rest of the run, in this order: the pending bytes are recovered; they
// go to the host members route (a BgzfWriter on the same file: psvr_bgzf_compress_members or zlib), which continues at the member boundary
// the last take ended on; then the bytes of the failed call itself (a host chunk as given, device chunks fetched from the slot's emitter);
// then everything that comes later, in the order it comes.  Nothing is written out of order because nothing is written from two places: up
// to the failure only takes write, after it only the BgzfWriter does.  If the pending bytes cannot be recovered, or the records of a device
// chunk cannot be fetched, the file could only be written with bytes missing: the call says why and returns false, and the command ends
// with a non-zero status.
//
// What a backend offers (every int is 0 or a status whose text last_error() gives):
//   int stream_create() / void stream_destroy()                the stream, at members of kBgzfBlock bytes
//   int stream_append(const void *, int64_t) / int stream_append_emit(int slot, int64_t first_pair, int64_t n_pairs)
//   int64_t stream_pending()                                   (< 0: failed)
//   int64_t bound(int64_t n)                                   room that the members of n pending bytes never exceed
//   int take(int finish, void *out, int64_t cap, int64_t *got, int64_t *member_off, int64_t member_cap, int64_t *n_members, int64_t *used)
//   int stream_recover(void *bytes, int64_t cap, int64_t *n)   cap too small: kOverflow and *n is set
//   int emit_view(int slot, int64_t P, const int64_t **off, const uint8_t **state)   offsets and states of the slot's emitted piece
//   int emit_fetch(int slot, int64_t p0, int64_t p1, std::vector<uint8_t> *out)      the records of pairs [p0, p1) of the slot's piece
//   void *host_alloc(size_t) / void host_free(void *)          page-locked where that exists (member_take.h, which makes the takes)
//   void host_route(BgzfWriter &)                              how the writer that takes over compresses (set_device_members, or nothing)
//   const char *last_error()
#pragma once
#include <stdint.h>
#include <stdio.h>
#include <atomic>
#include <deque>
#include <string>
#include <utility>
#include <vector>
#include "bam_writer.h"
#include "member_take.h"

namespace psvr {

struct StreamSinkStats {
	long long device_bytes = 0, host_bytes = 0;          // stream bytes that never left HBM before they were compressed / that came from the host (the BAM header is the first of them)
	long long members = 0;                               // members the device stream made
	long long device_chunks = 0, host_chunks = 0;        // runs of device chunks / host chunks taken in (the header is not a chunk)
	bool left = false;                                   // the device route was given up
};

template <class Backend> class BgzfStreamSink {
public:
	static const int kOverflow = 6;                      // PSVR_ERR_OVERFLOW
	StreamSinkStats st;
	explicit BgzfStreamSink(Backend &be, size_t take_members = 1024) : be_(be), take_(be), take_members_(take_members < 1 ? 1 : take_members) {}

	// the file and the stream; the BAM header is the stream's first bytes.  false: the file cannot be opened
	bool open(const char *fn, const std::string &header_text, const std::vector<BamRef> &refs, int threads)
	{
		f_ = fopen(fn, "wb");
		if (!f_) return false;
		threads_ = threads;
		on_ = true;
		if (be_.stream_create()) {
			fprintf(stderr, "[panSVR-amd] BGZF stream on the device failed (create: %s): the main file is compressed through the host members route\n", be_.last_error());
			on_ = false, st.left = true;
			start_host_route();
		}
		const std::vector<uint8_t> h = bam_header_block(header_text, refs);
		return host_bytes(h.data(), h.size(), false);
	}
	bool on() const { return on_; }                      // the device route is still on (a piece formatted while it was may still hand in device chunks)
	bool ok() const { return !fatal_; }

	int emit_view(int slot, int64_t P, const int64_t **off, const uint8_t **state) { return be_.emit_view(slot, P, off, state); }
	const char *last_error() { return be_.last_error(); }

	// records of pairs [p0, p1) of the slot's emitted piece: device to device while the route is on, fetched from the emitter after it
	bool device_chunks(int slot, int64_t p0, int64_t p1, int64_t n_bytes)
	{
		if (fatal_) return false;
		if (p1 <= p0 || n_bytes == 0) return true;
		if (on_) {
			if (be_.stream_append_emit(slot, p0, p1 - p0) == 0) {
				++st.device_chunks, st.device_bytes += n_bytes, segs_.push_back({true, n_bytes});
				return true;
			}
			if (!leave("append from the emitter")) return false;
		}
		if (be_.emit_fetch(slot, p0, p1, &fetched_)) return fatal("the records of a device chunk could not be fetched from the emitter");
		++st.host_chunks, st.host_bytes += (long long)fetched_.size();
		host_.write(fetched_.data(), fetched_.size());
		return true;
	}
	bool host_chunk(const void *p, size_t n) { return host_bytes(p, n, true); }

	// after a piece: the queued appends are through (the slot's emitter may run again); enough members pending: taken and written
	bool piece_done()
	{
		if (fatal_) return false;
		if (!on_) return true;
		const int64_t n = be_.stream_pending();
		if (n < 0) return leave("pending");
		if ((size_t)(n / (int64_t)kBgzfBlock) < take_members_) return true;
		return take(0, n) || leave("take");
	}
	// the tail as a last member, the EOF block, the file closed.  false: something failed in compressing or writing, or earlier
	bool close()
	{
		if (!f_) return false;
		if (on_ && !fatal_) {
			const int64_t n = be_.stream_pending();
			if (n < 0 || !take(1, n)) leave(n < 0 ? "pending" : "the last take");
		}
		be_.stream_destroy();
		if (fatal_) {                                        // (no EOF block: the file is not whole, and does not look it)
			fclose(f_);
			f_ = nullptr;
			return false;
		}
		if (host_open_) {
			const bool fine = host_.close();                 // (its EOF block, its fclose)
			f_ = nullptr;
			return fine && !fatal_ && take_.wrote;
		}
		if (fwrite(kBgzfEof, 1, sizeof kBgzfEof, f_) != sizeof kBgzfEof) take_.wrote = false;
		if (fclose(f_) != 0) take_.wrote = false;
		f_ = nullptr;
		return take_.wrote && !fatal_;
	}

private:
	Backend &be_;
	MemberTake<Backend> take_;
	FILE *f_ = nullptr;
	int threads_ = 1;
	size_t take_members_;
	std::atomic<bool> on_{false};                        // (the formatter's thread asks, the writer's thread answers)
	bool fatal_ = false, host_open_ = false;
	BgzfWriter host_;                                    // the host members route, once the device route is left
	std::vector<uint8_t> fetched_;
	std::deque<std::pair<bool, int64_t>> segs_;          // what is pending, in order: (from the device, bytes)

	bool fatal(const char *what)
	{
		fprintf(stderr, "[panSVR-amd] --stream-device: %s (%s): the main file would have bytes missing, giving up\n", what, be_.last_error());
		fatal_ = true;
		return false;
	}
	void start_host_route()
	{
		host_.adopt(f_, threads_);
		be_.host_route(host_);
		host_open_ = true;
	}
	bool host_bytes(const void *p, size_t n, bool is_chunk)
	{
		if (fatal_) return false;
		if (n == 0) return true;
		if (on_) {
			if (be_.stream_append(p, (int64_t)n) == 0) {
				st.host_chunks += is_chunk, st.host_bytes += (long long)n, segs_.push_back({false, (int64_t)n});
				return true;
			}
			if (!leave("append")) return false;
		}
		st.host_chunks += is_chunk, st.host_bytes += (long long)n;
		host_.write(p, n);
		return true;
	}
	bool take(int finish, int64_t pending)               // false: the take failed; otherwise it consumed the first `used` pending bytes
	{
		int64_t used = 0;
		if (!take_(f_, finish, pending, &used)) return false;
		st.members = take_.members;
		while (used > 0 && !segs_.empty()) {
			const int64_t m = segs_.front().second < used ? segs_.front().second : used;
			used -= m, segs_.front().second -= m;
			if (segs_.front().second == 0) segs_.pop_front();
		}
		return true;
	}
	// the device route ends here: what is pending goes to the host members route first.  false: it could not be recovered
	bool leave(const char *what)
	{
		fprintf(stderr, "[panSVR-amd] BGZF stream on the device failed (%s: %s): the main file is compressed through the host members route from here on\n", what, be_.last_error());
		on_ = false, st.left = true;
		int64_t n = 0;
		int rc = be_.stream_recover(nullptr, 0, &n);
		std::vector<uint8_t> back;
		if (rc == kOverflow && n > 0) {
			back.resize((size_t)n);
			rc = be_.stream_recover(back.data(), n, &n);
		}
		if (rc) return fatal("the pending bytes of the stream could not be recovered");
		for (const auto &s : segs_) if (s.first) st.device_bytes -= s.second, st.host_bytes += s.second;   // (they left HBM after all)
		segs_.clear();
		start_host_route();
		host_.write(back.data(), (size_t)n);
		return true;
	}
};

} // namespace psvr
