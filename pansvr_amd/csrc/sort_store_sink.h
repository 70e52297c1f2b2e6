// sort_store_sink.h -- the chunk intake of `panSVR aln --sort-device`'s main file: the records are kept in a device-resident store (psvr_bam_store_*,
// include/psvr_engine.h) until the input ends; then sorted_bam.h's write_sorted_store orders them there, gathers them into a device-resident
// BGZF stream and writes the file and its .bai, so that only the compressed members and the table the .bai is built from come to the host.
// Host C++ only, a template over the backend, as bgzf_stream_sink.h is: cli_main.cpp has the product's; tests/tools/sink_host.h has one that
// keeps store and stream in host memory by the same rules, so every rule in here runs without a GPU (tests/test_sort_store_sink.py).
//
// What reaches the sink, in input order: per piece its chunks -- device_chunks(slot, p0, p1) for a run of adjacent chunks whose records lie in
// the slot's emitter, host_chunk(bytes) for a chunk the host formatted -- and piece_done(), which waits for the queued appends (the slot's
// emitter is free again).  finish() has the store written.  Both this route and `--sort --deflate-device` cut the same stream every 0xff00
// bytes, and a member's bytes depend on its input bytes alone: the files are the same, byte for byte.
//
// Leaving the device route.  A failed backend call never loses a record:
//   before the file is begun   the store is downloaded into a SortRecords; the failed call's own bytes (a host chunk as given, device chunks
//                              fetched from the slot's emitter) and all later pieces go there too; the end is the host's sorted writer
//   after the file is begun    (the writer names order, meta, a stream call or a take) the store is downloaded, the file is begun anew
//                              (truncated) and written by the host's sorted writer
//   the download fails         the call says why and returns false: the command ends with status 2, and no partial .bai is left behind
// The host's sorted writer is the caller's (`write_host`: the command hands in write_sorted_main, i.e. coordinate_order + write_sorted_bam on the
// --deflate-device route).
//
// What a backend offers (every int is 0 or a status whose text last_error() gives), besides what write_sorted_store asks (sorted_bam.h):
//   int store_create() / void store_destroy()
//   int store_append(const void *, int64_t) / int store_append_emit(int slot, int64_t first_pair, int64_t n_pairs)
//   int store_info(int64_t *n_records, int64_t *n_bytes)       waits for the queued appends
//   int store_download(void *bytes, int64_t cap, int64_t *n)
//   int emit_view(int slot, int64_t P, const int64_t **off, const uint8_t **state) / int emit_fetch(int slot, int64_t p0, int64_t p1, std::vector<uint8_t> *out)
//   const char *last_error()
#pragma once
#include <stdint.h>
#include <stdio.h>
#include <atomic>
#include <functional>
#include <string>
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

template <class Backend> class SortStoreSink {
public:
	SortSinkStats st;
	// write_host: the host's sorted writer over the records (0, or the command's exit status); it says itself what fails
	typedef std::function<int(const SortRecords &)> WriteHost;
	SortStoreSink(Backend &be, WriteHost write_host, size_t take_members = 1024) : be_(be), write_host_(std::move(write_host)), take_members_(take_members < 1 ? 1 : take_members) {}

	void open(const char *fn, const std::string &header_text, const std::vector<BamRef> &refs)
	{
		fn_ = fn, text_ = header_text, refs_ = refs;
		on_ = true;
		if (be_.store_create()) {
			fprintf(stderr, "[panSVR-amd] record store on the device failed (create: %s): the main file's records are kept and sorted on the host\n", be_.last_error());
			on_ = false, st.left = true;
		}
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
			const StoreWritten w = write_sorted_store(be_, fn_, text_, refs_, false, take_members_);
			if (w.status == 0) {
				st.records = w.records, st.members = w.members, st.t_order = w.t_order;
				st.host_bytes += w.header_bytes;                 // (the BAM header is the stream's first host append)
			}
			else if (w.status > 0) fatal_ = true;
			else if (!leave(w.failed) && w.begun) remove((fn_ + ".bai").c_str());   // (no partial index beside a file that was begun)
		}
		be_.store_destroy();
		if (fatal_) return 2;
		if (!st.left) return 0;
		st.records = (long long)host_.size();
		return write_host_(host_);                           // (it begins the file anew)
	}

private:
	Backend &be_;
	WriteHost write_host_;
	size_t take_members_;
	std::string fn_, text_;
	std::vector<BamRef> refs_;
	std::atomic<bool> on_{false};                        // (the formatter's thread asks, the writer's thread answers)
	bool fatal_ = false;
	SortRecords host_;                                   // the records, once the device route is left
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
		fprintf(stderr, "[panSVR-amd] record store on the device failed (%s: %s): the main file's records are kept and sorted on the host from here on\n", what, be_.last_error());
		on_ = false, st.left = true;
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
};

} // namespace psvr
