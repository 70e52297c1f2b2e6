// sort_store_sink.h -- the writer of `panSVR aln --sort-device`'s main file: the records are kept in a device-resident store (psvr_bam_store_*,
// include/psvr_engine.h) until the input ends, ordered there, gathered in sorted order into a device-resident BGZF stream (psvr_bgzf_stream_*)
// and compressed there, so that only the compressed members and the table the .bai is built from come to the host.  Host C++ only, a template
// over the backend, as bgzf_stream_sink.h is: cli_main.cpp has the product's; tests/tools/sort_store_sink_check.cpp has one that keeps store and
// stream in host memory by the same rules, so every rule in here runs without a GPU (tests/test_sort_store_sink.py).
//
// What reaches the sink, in input order: per piece its chunks -- device_chunks(slot, p0, p1) for a run of adjacent chunks whose records lie in
// the slot's emitter, host_chunk(bytes) for a chunk the host formatted -- and piece_done(), which waits for the queued appends (the slot's
// emitter is free again).  finish() orders the store and writes the file and its index:
//   the BAM header with SO:coordinate (sorted_header_text) into a fresh BGZF stream; then windows of sorted ranks -- as many as fill
//   take_members members -- gathered into the stream (store_stream), taken (the last window with finish, so the tail becomes the last, shorter
//   member), written, their starts logged; the EOF block; the .bai from the store's meta table and the member starts (build_bai, sorted_bam.h).
// Both this route and `--sort --deflate-device` cut the same stream every 0xff00 bytes, and a member's bytes depend on its input bytes alone:
// the files are the same, byte for byte.
//
// Leaving the device route.  A failed backend call never loses a record:
//   before the file is begun   the store is downloaded into a SortRecords; the failed call's own bytes (a host chunk as given, device chunks
//                              fetched from the slot's emitter) and all later pieces go there too; the end is the host's sorted writer
//   after the file is begun    (order, meta, a stream call, a take) the store is downloaded, the file is begun anew (truncated) and written by
//                              the host's sorted writer
//   the download fails         the call says why and returns false: the command ends with status 2, and no partial .bai is left behind
// The host's sorted writer is the caller's (`write_host`: the command hands in write_sorted_main, i.e. coordinate_order + write_sorted_bam on the
// --deflate-device route).
//
// What a backend offers (every int is 0 or a status whose text last_error() gives):
//   int store_create() / void store_destroy()
//   int store_append(const void *, int64_t) / int store_append_emit(int slot, int64_t first_pair, int64_t n_pairs)
//   int store_info(int64_t *n_records, int64_t *n_bytes)       waits for the queued appends
//   int store_order() / int store_meta(int64_t first_rank, int64_t n, psvr_bam_rec_meta_t *)
//   int store_order_names()                                    optional: what adopt(..., by_name) orders by (tests/tools/nsort_sink_check.cpp has one)
//   int store_stream(int64_t first_rank, int64_t n)            those ranks' records behind the stream's pending bytes
//   int store_download(void *bytes, int64_t cap, int64_t *n)
//   int stream_create() / void stream_destroy() / int stream_append(const void *, int64_t)
//   int64_t bound(int64_t n)                                   room that the members of n pending bytes never exceed
//   int take(int finish, void *out, int64_t cap, int64_t *got, int64_t *member_off, int64_t member_cap, int64_t *n_members, int64_t *used)
//   int emit_view(int slot, int64_t P, const int64_t **off, const uint8_t **state) / int emit_fetch(int slot, int64_t p0, int64_t p1, std::vector<uint8_t> *out)
//   void *host_alloc(size_t) / void host_free(void *) / const char *last_error()
#pragma once
#include <stdint.h>
#include <stdio.h>
#include <time.h>
#include <atomic>
#include <functional>
#include <string>
#include <type_traits>
#include <utility>
#include <vector>
#include "sorted_bam.h"

namespace psvr {

struct SortSinkStats {
	long long device_bytes = 0, host_bytes = 0;          // record bytes that never left HBM / bytes appended from the host (the BAM header among them) or kept there after the route was left
	long long records = 0, members = 0;                  // records in the sorted file; members the device stream made
	long long device_chunks = 0, host_chunks = 0;
	double t_order = 0;                                  // the order's own time
	bool left = false;                                   // the device route was given up
};

// a backend that offers int store_order_names(): the store ordered by name (psvr_bam_store_order_names); only such a backend instantiates the call
template <class B, class = void> struct HasStoreOrderNames : std::false_type {};
template <class B> struct HasStoreOrderNames<B, std::void_t<decltype(std::declval<B &>().store_order_names())>> : std::true_type {};

template <class Backend> class SortStoreSink {
public:
	SortSinkStats st;
	// write_host: the host's sorted writer over the records (0, or the command's exit status); it says itself what fails
	typedef std::function<int(const SortRecords &)> WriteHost;
	SortStoreSink(Backend &be, WriteHost write_host, size_t take_members = 1024) : be_(be), write_host_(std::move(write_host)), take_members_(take_members < 1 ? 1 : take_members) {}
	~SortStoreSink() { if (pin_) be_.host_free(pin_); }

	void open(const char *fn, const std::string &header_text, const std::vector<BamRef> &refs)
	{
		fn_ = fn, text_ = sorted_header_text(header_text, false), refs_ = refs;
		on_ = true;
		if (be_.store_create()) {
			fprintf(stderr, "[panSVR-amd] record store on the device failed (create: %s): the main file's records are kept and sorted on the host\n", be_.last_error());
			on_ = false, st.left = true;
		}
	}
	// A store that the caller has created through the backend and fills itself (`panSVR sort --sort-device`, bam_sort.h, from the file's own
	// members): finish_store() writes the sorted file and its index from it.  The caller has its input still, so a failed call downloads nothing.
	// by_name (`panSVR sort --nsort-device`): the header says SO:queryname, the store is ordered by store_order_names(), and there is no .bai;
	// the windows, the takes and the EOF block are the same
	void adopt(const char *fn, const std::string &header_text, const std::vector<BamRef> &refs, bool by_name = false)
	{
		fn_ = fn, text_ = sorted_header_text(header_text, by_name), refs_ = refs;
		on_ = foreign_ = true, by_name_ = by_name;
	}
	// 0: written; -1: a backend call failed and has been named, the caller starts over from its input; 2: the file cannot be written.  The store is destroyed
	int finish_store()
	{
		const bool done = on_ && foreign_ && write_device();
		be_.store_destroy();
		return done ? 0 : fatal_ ? 2 : -1;
	}
	bool on() const { return on_; }
	bool ok() const { return !fatal_; }
	const char *sorter() const { return st.left ? "device+host" : "device"; }   // the e2e_json line's "sorter" (host: the option was not in effect)
	int emit_view(int slot, int64_t P, const int64_t **off, const uint8_t **state) { return be_.emit_view(slot, P, off, state); }
	const char *last_error() { return be_.last_error(); }

	bool device_chunks(int slot, int64_t p0, int64_t p1, int64_t n_bytes)
	{
		if (fatal_) return false;
		if (p1 <= p0 || n_bytes == 0) return true;
		if (on_) {
			if (be_.store_append_emit(slot, p0, p1 - p0) == 0) {
				++st.device_chunks, st.device_bytes += n_bytes;
				return true;
			}
			if (!leave("append from the emitter")) return false;
		}
		if (be_.emit_fetch(slot, p0, p1, &fetched_)) return fatal("the records of a device chunk could not be fetched from the emitter");
		++st.host_chunks, st.host_bytes += (long long)fetched_.size();
		return keep(fetched_.data(), fetched_.size());
	}
	bool host_chunk(const void *p, size_t n)
	{
		if (fatal_) return false;
		if (n == 0) return true;
		if (on_) {
			if (be_.store_append(p, (int64_t)n) == 0) {
				++st.host_chunks, st.host_bytes += (long long)n;
				return true;
			}
			if (!leave("append")) return false;
		}
		++st.host_chunks, st.host_bytes += (long long)n;
		return keep(p, n);
	}
	// after a piece: the queued appends are through (the slot's emitter may run again)
	bool piece_done()
	{
		if (fatal_) return false;
		if (!on_) return true;
		int64_t nr = 0, nb = 0;
		return be_.store_info(&nr, &nb) == 0 || leave("info");
	}
	// the end of the input: the sorted file and its index.  0, or the command's exit status (what failed has been said)
	int finish()
	{
		if (fatal_) return 2;
		if (on_) {
			if (write_device()) { be_.store_destroy(); return 0; }
			if (fatal_) { be_.store_destroy(); return 2; }
		}
		be_.store_destroy();
		st.records = (long long)host_.size();
		return write_host_(host_);
	}

private:
	Backend &be_;
	WriteHost write_host_;
	size_t take_members_;
	std::string fn_, text_;
	std::vector<BamRef> refs_;
	std::atomic<bool> on_{false};                        // (the formatter's thread asks, the writer's thread answers)
	bool fatal_ = false, foreign_ = false;               // foreign_: the store was adopted, its records are not this sink's to rescue
	bool by_name_ = false;                               // (adopt) name order, no index
	SortRecords host_;                                   // the records, once the device route is left
	uint8_t *pin_ = nullptr;
	size_t pin_cap_ = 0;
	std::vector<uint8_t> fetched_;

	bool fatal(const char *what)
	{
		fprintf(stderr, "[panSVR-amd] --sort-device: %s (%s): the main file would have records missing, giving up\n", what, be_.last_error());
		fatal_ = true;
		return false;
	}
	bool keep(const void *p, size_t n)
	{
		if (host_.add_stream((const uint8_t *)p, n)) return true;
		fprintf(stderr, "[panSVR-amd] --sort-device: malformed record from the formatter\n");
		fatal_ = true;
		return false;
	}
	// the device route ends here: every record of the store goes to the host's SortRecords, in append order.  false: they could not be had
	bool leave(const char *what)
	{
		if (foreign_) {
			fprintf(stderr, "[panSVR-amd] record store on the device failed (%s: %s): the input is read again and sorted by the host's route\n", what, be_.last_error());
			on_ = false, st.left = true, st.members = 0;
			return true;
		}
		fprintf(stderr, "[panSVR-amd] record store on the device failed (%s: %s): the main file's records are kept and sorted on the host from here on\n", what, be_.last_error());
		on_ = false, st.left = true, st.members = 0;
		int64_t n = 0;
		int rc = be_.store_download(nullptr, 0, &n);
		std::vector<uint8_t> back;
		if (rc != 0 && n > 0) {                              // (the size came with the refusal)
			back.resize((size_t)n);
			rc = be_.store_download(back.data(), n, &n);
		}
		if (rc) return fatal("the records of the store could not be downloaded");
		st.host_bytes += st.device_bytes, st.device_bytes = 0;   // (they left HBM after all)
		return keep(back.data(), (size_t)n);
	}
	bool take(FILE *f, int finish, int64_t pending, std::vector<uint64_t> *starts, uint64_t *fpos, bool *wrote)
	{
		if (pending == 0) return true;
		const size_t need = (size_t)be_.bound(pending);
		if (need > pin_cap_) {
			if (pin_) be_.host_free(pin_);
			pin_ = (uint8_t *)be_.host_alloc(need + need / 4), pin_cap_ = pin_ ? need + need / 4 : 0;
			if (!pin_) return false;
		}
		const int64_t cap_m = pending / (int64_t)kBgzfBlock + 1;
		moff_.assign((size_t)cap_m + 1, 0);
		int64_t got = 0, nm = 0, used = 0;
		if (be_.take(finish, pin_, (int64_t)pin_cap_, &got, moff_.data(), cap_m, &nm, &used)) return false;
		for (int64_t m = 0; m < nm; ++m) starts->push_back(*fpos + (uint64_t)moff_[(size_t)m]);
		if (fwrite(pin_, 1, (size_t)got, f) != (size_t)got) *wrote = false;
		*fpos += (uint64_t)got, st.members += nm, pending_ -= used;
		return true;
	}
	std::vector<int64_t> moff_;
	int64_t pending_ = 0;
	// order, header, windows, EOF block, .bai.  false: the device route failed (left: the host writer takes over) or the run cannot go on (fatal_)
	bool write_device()
	{
		const double t0 = now();
		if (order_store()) { leave("order"); return false; }
		st.t_order = now() - t0;
		int64_t n = 0, nb = 0;
		if (be_.store_info(&n, &nb)) { leave("info"); return false; }
		std::vector<psvr_bam_rec_meta_t> meta((size_t)n);
		if (n && be_.store_meta(0, n, meta.data())) { leave("meta"); return false; }
		FILE *f = fopen(fn_.c_str(), "wb");
		if (!f) { fprintf(stderr, "fail to open file '%s'\n", fn_.c_str()); fatal_ = true; return false; }
		const std::vector<uint8_t> head = bam_header_block(text_, refs_);
		std::vector<uint64_t> starts;
		uint64_t fpos = 0;
		bool wrote = true;
		const char *failed = nullptr;
		pending_ = 0;
		if (be_.stream_create()) failed = "stream create";
		else {
			if (be_.stream_append(head.data(), (int64_t)head.size())) failed = "stream append";
			else pending_ = (int64_t)head.size();
			const int64_t want = (int64_t)take_members_ * (int64_t)kBgzfBlock;
			for (int64_t a = 0; !failed && a < n;) {
				int64_t b = a, bytes = 0;
				while (b < n && pending_ + bytes < want) bytes += meta[(size_t)b++].len;
				if (be_.store_stream(a, b - a)) { failed = "stream from the store"; break; }
				pending_ += bytes;
				if (!take(f, b == n, pending_, &starts, &fpos, &wrote)) failed = b == n ? "the last take" : "take";
				a = b;
			}
			if (!failed && n == 0 && !take(f, 1, pending_, &starts, &fpos, &wrote)) failed = "the last take";
			be_.stream_destroy();
		}
		if (failed) {
			fclose(f);
			if (!leave(failed)) { remove((fn_ + ".bai").c_str()); return false; }
			return false;                                    // (write_host begins the file anew)
		}
		starts.push_back(fpos);
		if (fwrite(kBgzfEof, 1, sizeof kBgzfEof, f) != sizeof kBgzfEof) wrote = false;
		if (fclose(f) != 0) wrote = false;
		if (!wrote) { fprintf(stderr, "fail to write file '%s'\n", fn_.c_str()); fatal_ = true; return false; }
		if (!by_name_) {                                     // (a name-sorted file has no index)
			std::string err;
			const std::vector<uint8_t> bai = build_bai(refs_.size(), (size_t)n, head.size(), starts, [&](size_t i) {
				const psvr_bam_rec_meta_t &m = meta[i];
				return BaiRecord{m.tid, m.pos, m.end, m.bin, m.flag, m.len};
			});
			if (!write_bai(fn_, bai, &err)) { fprintf(stderr, "%s\n", err.c_str()); fatal_ = true; return false; }
		}
		st.records = n, st.host_bytes += (long long)head.size();   // (the BAM header is the stream's first host append)
		return true;
	}
	int order_store()
	{
		if constexpr (HasStoreOrderNames<Backend>::value) { if (by_name_) return be_.store_order_names(); }
		else if (by_name_) return -1;                        // (last_error() is the backend's: it has said nothing of a call it does not have)
		return be_.store_order();
	}
	static double now()
	{
		struct timespec ts;
		clock_gettime(CLOCK_MONOTONIC, &ts);
		return ts.tv_sec + 1e-9 * ts.tv_nsec;
	}
};

} // namespace psvr
