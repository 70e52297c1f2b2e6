// aln_pipeline.h -- the four overlapped stages of `panSVR aln` (classify_pipeline, rr.cpp:100-131, kt_pipeline): load_reads | align |
// output_results, the last one as two stages, format | write, because formatting (or BGZF deflate) and the file write each take about as
// long as the parse.  Host C++ only: the engine is reached through a driver type (cli_main.cpp has the product's, over psvr_engine_*,
// psvr_fastq_* and psvr_bam_emit_*; tests/tools/aln_pipeline_check.cpp has one over the CPU emulation), so every rule in here -- the pieces,
// -R, the slot ring, the block split, the draw-order exchange, the splice of device-encoded records, the order of what reaches the two
// files -- runs without a GPU (tests/test_aln_pipeline.py).
//
// What a driver offers (no virtual functions: the pipeline is a template over it; every int is 0 or an error whose text last_error()
// gives on the calling thread; the pipeline calls the per-device operations from one host thread per device):
//   int create(const psvr_aln_params_t &, int64_t pos[3])        the engines of all devices; pos: where a fresh engine stands
//   int load(int d, const int64_t pos[3], const FastqBatch &, long long lo, long long n)    set the stream position + upload pairs [lo, lo + n)
//   int run(int d, bool trace) / int stream_end(int d, int64_t end[3]) / int rebase(int d, const int64_t pos[3])
//   int download(int d, Block &, bool full, long long *bytes)    the block's ResultView (+ the fixed ABI records for --records)
//   const char *last_error() / bool hbm_used(size_t *)
//   the two device routes, kNotAvailable from a driver without them (the pipeline then takes the host route without a word):
//   int parse_window(int slot, FastqReader &, FastqBatch &, long long pairs, long long bases, int threads, std::string *why)   1 / 0 (input ended) / -1
//   int emit_encode(int slot, const FastqBatch &, bool not_ori) / int emit_download(int slot, long long P, EmitView *)
// --stream-device does not add to that list: who writes the main file then (MainSink below) reaches the pipeline as an optional last
// constructor argument, and it is the sink, not the driver, that is asked for the offsets and states of a slot's emitted piece.
// --ori-device does not either: who encodes the second file's records (OriSource below) is the constructor's argument behind the sink.
#pragma once
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <sys/time.h>
#include <unistd.h>
#include <atomic>
#include <condition_variable>
#include <functional>
#include <mutex>
#include <new>
#include <string>
#include <thread>
#include <vector>
#include "host_io.h"
#include "fastq_batch.h"
#include "sam_emit.h"
#include "bam_writer.h"

namespace psvr {
namespace aln {

inline double walltime()
{
	struct timeval tv;
	gettimeofday(&tv, nullptr);
	return tv.tv_sec + 1e-6 * tv.tv_usec;
}

// the options the stages read (the command's Opt adds its own)
struct PipeOpt {
	int thread_n = 4;
	bool not_ori = false, trace = false;
	long long max_use_read = 0x7fffffff;
	std::vector<int> devices = {0};
	long long batch_pairs = 2000000;       // N_NEEDED, rr.cpp:24
	long long batch_bases = 100000000;     // MAX_read_size, rr.cpp:109 (333 334 pairs of 150 bp: the limit that actually binds)
	long long sub_pairs = 65536;           // a batch travels through the four stages in pieces of this many pairs (0 = whole batches): three
	                                       // reference-sized batches do not fill a four-stage pipeline, forty pieces do
	bool parse_device = false;             // FASTQ input: every window parsed on the first device, the bases handed to the engine device to device
	bool emit_device = false;              // ... and the main BAM file's records encoded there; implies parse_device
	bool ori_device = false;               // ... and the second file's records; implies emit_device.  A piece both encoders took whole is resident: its results and text stay in HBM
};

// one output file: SAM text (-S) or BAM (default, like the reference's init_run)
struct OutFile {
	FILE *sam = nullptr;
	BamWriter bam;
	bool is_bam = false;
	bool open(const std::string &fn, bool as_bam, const HeaderInfo &H, const std::vector<BamRef> &refs, int threads, int level = -1)
	{
		is_bam = as_bam;
		if (!as_bam) { sam = fopen(fn.c_str(), "w"); if (sam) { setvbuf(sam, nullptr, _IOFBF, 1 << 22); fputs(H.text.c_str(), sam); } return sam != nullptr; }
		return bam.open(fn.c_str(), H.text, refs, threads, level);
	}
	// formatted records (SAM lines or encoded BAM records) of a run of pairs, in order
	void write_raw(const Bytes &b) { if (b.empty()) return; if (is_bam) bam.write_raw(b.data(), b.size()); else fwrite(b.data(), 1, b.size(), sam); }
	bool close() { if (is_bam) return bam.close(); return fclose(sam) == 0; }
};
static const char *const kSortNoMem = "[panSVR-amd] --sort: out of host memory for the main file's records; run `panSVR aln` without --sort, then `panSVR sort` on its output\n";

// The reference's batch: N_NEEDED pairs or MAX_read_size bases, whichever comes first (rr.cpp:24,109,126); it is read in pieces that end
// where it ends (a piece stops at what is left of both limits), so the batches are the reference's.  No I/O.
struct PieceRule {
	long long batch_pairs, batch_bases, sub_pairs, max_use_read;
	long long loaded = 0, n_pieces = 0, in_batch_pairs = 0, in_batch_bases = 0;
	static constexpr long long kFirstPiece = 8192;
	long long want() const                               // pairs the next piece wants (<= 0: -R is reached)
	{
		long long w = batch_pairs - in_batch_pairs;
		if (sub_pairs > 0 && sub_pairs < w) w = sub_pairs;
		// the first pieces are short ones: the later stages have something to do after a millisecond of reading instead of ten, and the
		// engine's first batch -- mostly set-up that does not depend on its size -- is through sooner
		if (sub_pairs > 0 && n_pieces < 3 && (kFirstPiece << n_pieces) < w) w = kFirstPiece << n_pieces;
		return max_use_read - loaded < w ? max_use_read - loaded : w;
	}
	long long bases_left() const { return batch_bases - in_batch_bases; }
	long long took(long long pairs, long long bases)     // after a piece: the pairs of the reference-sized batch that has just ended, or 0
	{
		++n_pieces, loaded += pairs, in_batch_pairs += pairs, in_batch_bases += bases;
		if (in_batch_pairs < batch_pairs && in_batch_bases < batch_bases) return 0;
		const long long done = in_batch_pairs;
		in_batch_pairs = in_batch_bases = 0;
		return done;
	}
};

// A slot keeps its buffers (like the reference's Classify_buff_pool): the raw text + line index of its batch, the page-locked upload
// arrays, per device the page-locked compact results, and the formatted records.
struct Block {                       // the share of one device
	long long lo = 0, hi = 0;
	HostBuf hdr_buf, pair_buf, cand_buf, cig_buf;
	ResultView V;
	std::vector<psvr_read_result_t> full; std::vector<uint32_t> full_cig;   // --records only (the fixed-size ABI form)
};
struct Job {
	FastqBatch fb;
	int slot = 0;                      // (the driver keeps what its device routes need per slot)
	bool emitted = false;              // --emit-device: this piece's main records were encoded on the device
	bool ori_emitted = false;          // --ori-device: ... and the second file's
	bool resident = false;             // ... and neither encoder declined a pair: the piece's results were not downloaded, its window text may not be here
	std::vector<uint8_t> from_dev;     // --stream-device, per chunk: its main records stay in the slot's emitter (mb[ci] is empty) ...
	const int64_t *dev_off = nullptr;  // ... at [dev_off[p0], dev_off[p1]) of its bytes
	std::vector<Block> blk;
	long long pair_base = 0;
	std::vector<Bytes> mb, ob;         // formatted records of both files, per chunk of pairs
	int state = 0;              // 0 free, 1 loaded, 2 aligned, 3 formatted
	bool last = false;          // end-of-input marker travelling through the stages
	long long batch_pairs_done = 0;   // > 0 on the last piece of a reference-sized batch: that batch's pairs (the progress line)
};
// Job slots cycle through the stages in input order, so the output order is the input order.
constexpr int kSlots = 5;
struct SlotRing {
	Job jobs[kSlots];
	std::mutex mu;
	std::condition_variable cv;
	explicit SlotRing(int D) { for (int s = 0; s < kSlots; ++s) jobs[s].slot = s, jobs[s].blk = std::vector<Block>((size_t)D); }
	void wait_state(Job &J, int st) { std::unique_lock<std::mutex> lk(mu); cv.wait(lk, [&] { return J.state == st; }); }
	void set_state(Job &J, int st) { { std::lock_guard<std::mutex> lk(mu); J.state = st; } cv.notify_all(); }
};

// a device route that is on until it fails once (--emit-device is looked at by the engine stage and by the formatter: atomic)
constexpr int kNotAvailable = -1000;
struct DeviceRoute {
	std::atomic<bool> on;
	const char *message;               // what fail() prints, with the reason
	DeviceRoute(bool start, const char *m) : on(start), message(m) {}
	void fail(int rc, const char *why) { if (rc != kNotAvailable) fprintf(stderr, message, why); on = false; }
};
struct EmitView { const uint8_t *bytes = nullptr, *state = nullptr; const int64_t *off = nullptr; };   // a piece's device-encoded records: [off[p], off[p + 1]) of pair p; state 2 = declined
// --stream-device: who writes the main file instead of `fo` (cli_main.cpp has the product's, over bgzf_stream_sink.h).  The formatter asks it
// for a piece's offsets and states only (the records stay in HBM); the writer hands it the piece's chunks in order.  A bool that is false:
// the file cannot be written whole, the sink has said why, and the command ends.
struct MainSink {
	virtual ~MainSink() {}
	virtual bool on() const = 0;                                             // the device route is on (off after a failure: later pieces take the splice path)
	virtual int piece_view(int slot, long long P, EmitView *v) = 0;           // off and state of the slot's emitted piece; bytes stays null
	virtual const char *last_error() = 0;
	virtual bool device_chunks(int slot, long long p0, long long p1, long long n_bytes) = 0;   // the records of pairs [p0, p1), from the slot's emitter
	virtual bool host_chunk(const uint8_t *p, size_t n) = 0;
	virtual bool piece_done() = 0;                                           // the slot's emitter is free again when this returns
	virtual const char *option() const { return "--stream-device"; }         // the option that put the sink there (--sort-device has one too), for messages
};

// --ori-device: who encodes the second file's records of a slot's piece (cli_main.cpp has the product's: a second emitter per slot over
// psvr_bam_emit_ori_engine; tests/tools/aln_ori_pipeline_check.cpp has one over the host build of the rules).  The engine stage calls encode
// right after the driver's emit_encode, before the engine gets its next piece, and decides there whether the piece is resident; the
// formatter calls download.  Every int is 0 or an error whose text last_error() gives.
struct OriSource {
	virtual ~OriSource() {}
	virtual int encode(int slot, const FastqBatch &fb, long long *declined) = 0;   // *declined: pairs of the piece in state 2
	virtual long long main_declined(int slot) = 0;                                  // ... and of the slot's last main-file encode (the driver's emit_encode)
	virtual int download(int slot, long long P, EmitView *v) = 0;                   // bytes, off and state of the slot's encoded piece, in host memory
	virtual int fetch_text(FastqBatch &fb) = 0;                                     // the window text of a piece that is not resident (fb.text_pending bytes), into fb.text
	virtual const char *last_error() = 0;
};

// every timer and counter of the `wall:` line and of e2e_json, by the stage that writes it
struct RunStats {
	int devices = 1, threads = 1;      // the command: what surrounds the pipeline
	bool sam = false;
	double wall0 = 0, wall = 0, t_index = 0, t_idx_first = 0, t_idx_clone = 0, t_sort = 0, t_sort_order = 0, t_teardown = 0;
	double t_read = 0;                 // reader
	long long n_dev_pieces = 0, n_host_pieces = 0;       // pieces parsed on the device / on the host threads
	double t_engine = 0, t_exchange = 0;                 // engine stage
	long long n_batches = 0, total_pairs = 0, rebase_iters = 0, d2h_bytes = 0;   // (n_batches: pieces run by the engine)
	size_t hbm_first = 0, hbm_last = 0;
	double t_format = 0;               // formatter
	long long n_ref_batches = 0;       // reference-sized batches
	long long n_emit_pieces = 0, n_emit_host_pieces = 0;   // pieces whose main records came from the device / from the host formatter
	// pairs the encoder took (state 0 or 1) / declined (state 2) / whose chunk was spliced in from the device's bytes (a chunk with a declined pair is formatted on the host whole)
	long long emit_device_pairs = 0, emit_declined_pairs = 0, emit_spliced_pairs = 0;
	EmitStats emit;
	double t_write = 0;                // writer
	bool stream_fields = false;        // the command's line ends with the four fields below (it can have a main-file sink; a pipeline built without one prints the line as it was)
	const char *streamer = "host";     // --stream-device: where the main file's stream was gathered (device / host / device+host) ...
	long long stream_device_bytes = 0, stream_host_bytes = 0, stream_members = 0;   // ... its bytes that never left HBM / that came from the host, the members the device stream made
	bool sort_fields = false;          // ... and with the five fields below behind them
	const char *sorter = "host";       // --sort-device: where the main file's records were kept and sorted (device / host / device+host when the route was left) ...
	long long sort_device_bytes = 0, sort_host_bytes = 0, sort_records = 0, sort_members = 0;   // ... record bytes that never left HBM / bytes appended from the host, records and members of the sorted file
	bool effort_field = false;         // ... and with the field below behind them
	int deflate_effort = 0;            // --deflate-effort: the wavefront BGZF encoder's effort on the routes that compress through it
	bool ori_fields = false;           // --ori-device was given: ... and with the six fields below behind it
	long long n_ori_pieces = 0, n_ori_host_pieces = 0;   // pieces whose second-file records came from the device / from the host formatter
	long long ori_device_pairs = 0, ori_declined_pairs = 0, ori_spliced_pairs = 0;   // as the three emit_ counters, for the second file
	long long resident_pieces = 0, text_d2h_bytes = 0;   // pieces whose results and text never came to the host; window text fetched from the device
	// PSVR_CLI_TIMING: when each stage had each piece (ms from the first FASTQ byte), printed at the end
	const bool timing = getenv("PSVR_CLI_TIMING") != nullptr;
	struct Span { double a = 0, b = 0; };
	std::vector<Span> tl[4];
	RunStats() { if (timing) for (auto &v : tl) v.resize(1 << 16); }
	void mark(int stage, long long piece, double a, double b) { if (timing && piece < (1 << 16)) tl[stage][(size_t)piece].a = a, tl[stage][(size_t)piece].b = b; }
	void print(double cpu_s) const
	{
		if (timing) {
			static const char *nm[4] = {"read", "engine", "format", "write"};
			for (long long i = 0; i <= n_batches && i < (1 << 16); ++i) {
				fprintf(stderr, "[panSVR-amd] piece %lld:", i);
				for (int st = 0; st < 4; ++st) fprintf(stderr, "  %s %.1f-%.1f", nm[st], (tl[st][(size_t)i].a - wall0) * 1e3, (tl[st][(size_t)i].b - wall0) * 1e3);
				fprintf(stderr, "\n");
			}
			fprintf(stderr, "[panSVR-amd] files closed at %.1f ms, engine and index released %.1f ms later\n", wall * 1e3, t_teardown * 1e3);
		}
		fprintf(stderr, "Classify CPU: %.3f sec\n", cpu_s);
		const long long dropped = (long long)emit.dropped;
		if (dropped) fprintf(stderr, "[panSVR-amd] %lld records were refused by the record rules of sam_parse1 and not written (see the ERROR lines above)\n", dropped);
		fprintf(stderr, "[panSVR-amd] wall: read+parse %.3f s, engine (upload+run+download) %.3f s, format %.3f s, write%s %.3f s\n", t_read, t_engine, t_format, sam ? "" : "+compress", t_write);
		fprintf(stderr, "[panSVR-amd] e2e_json {\"pairs\":%lld,\"batches\":%lld,\"pieces\":%lld,\"devices\":%d,\"threads\":%d,\"wall_s\":%.4f,", total_pairs, n_ref_batches, n_batches, devices, threads, wall);
		fprintf(stderr, "\"index_s\":%.4f,\"index_first_s\":%.4f,\"index_clone_s\":%.4f,\"read_parse_s\":%.4f,\"engine_s\":%.4f,\"exchange_s\":%.4f,\"rebase_iterations\":%lld,", t_index, t_idx_first, t_idx_clone, t_read, t_engine, t_exchange, rebase_iters);
		fprintf(stderr, "\"format_s\":%.4f,\"write_s\":%.4f,\"sort_s\":%.4f,\"sort_order_s\":%.4f,\"d2h_bytes\":%lld,\"hbm_used_first\":%zu,\"hbm_used_last\":%zu,", t_format, t_write, t_sort, t_sort_order, d2h_bytes, hbm_first, hbm_last);
		fprintf(stderr, "\"dropped\":%lld,\"teardown_s\":%.4f,\"parser\":\"%s\",\"emitter\":\"%s\",", dropped, t_teardown, n_dev_pieces ? (n_host_pieces ? "device+host" : "device") : "host", n_emit_pieces ? (n_emit_host_pieces ? "device+host" : "device") : "host");
		fprintf(stderr, "\"emit_device_pairs\":%lld,\"emit_declined_pairs\":%lld,\"emit_spliced_pairs\":%lld%s", emit_device_pairs, emit_declined_pairs, emit_spliced_pairs, stream_fields ? "," : "}\n");
		if (stream_fields) fprintf(stderr, "\"streamer\":\"%s\",\"stream_device_bytes\":%lld,\"stream_host_bytes\":%lld,\"stream_members\":%lld%s", streamer, stream_device_bytes, stream_host_bytes, stream_members, sort_fields ? "," : "}\n");
		if (stream_fields && sort_fields) fprintf(stderr, "\"sorter\":\"%s\",\"sort_device_bytes\":%lld,\"sort_host_bytes\":%lld,\"sort_records\":%lld,\"sort_members\":%lld%s", sorter, sort_device_bytes, sort_host_bytes, sort_records, sort_members, effort_field ? "," : "}\n");
		if (stream_fields && sort_fields && effort_field) fprintf(stderr, "\"deflate_effort\":%d%s", deflate_effort, ori_fields ? "," : "}\n");
		if (stream_fields && sort_fields && effort_field && ori_fields)
			fprintf(stderr, "\"ori_emitter\":\"%s\",\"ori_device_pairs\":%lld,\"ori_declined_pairs\":%lld,\"ori_spliced_pairs\":%lld,\"resident_pieces\":%lld,\"text_d2h_bytes\":%lld}\n",
			        n_ori_pieces ? (n_ori_host_pieces ? "device+host" : "device") : "host", ori_device_pairs, ori_declined_pairs, ori_spliced_pairs, resident_pieces, text_d2h_bytes);
	}
};

template <class Driver> struct AlnPipeline {
	const PipeOpt &o;
	Driver &drv;
	FastqReader &fq;
	psvr_aln_params_t &par;            // the reader completes it from the first read (STAT_), before the first piece is aligned
	SamEmitter &em;
	OutFile &fo, &fo_ori;
	std::function<bool(const uint8_t *, size_t)> keep_main;   // --sort: takes the main file's records (they are kept until the input ends) instead of `fo`; false: malformed
	MainSink *sink;                    // --stream-device: writes the main file instead of `fo` (null: none)
	OriSource *ori;                    // --ori-device: encodes the second file's records (null: the host formatter does)
	FILE *frec;                        // --records
	RunStats &st;
	const int D;
	SlotRing ring;
	DeviceRoute parse_route, emit_route, ori_route;
	int64_t pos[3] = {0, 0, 0};        // where the next piece starts in the three draw streams
	std::vector<int> rcs;              // per device: what its thread's last driver call answered ...
	std::vector<std::string> errs;     // ... and the driver's text for it
	int block_id = 0;

	AlnPipeline(const PipeOpt &opt, Driver &d, FastqReader &r, psvr_aln_params_t &p, SamEmitter &e, OutFile &main, OutFile &ori, std::function<bool(const uint8_t *, size_t)> keep, FILE *rec, RunStats &stats, bool device_routes,
	            MainSink *main_sink = nullptr, OriSource *ori_source = nullptr)
	    : o(opt), drv(d), fq(r), par(p), em(e), fo(main), fo_ori(ori), keep_main(std::move(keep)), sink(main_sink), ori(ori_source), frec(rec), st(stats), D((int)opt.devices.size()), ring(D),
	      parse_route(opt.parse_device && device_routes, "[panSVR-amd] FASTQ parse on the device failed (%s): parsing on the host threads from here on\n"),
	      emit_route(opt.emit_device && device_routes, "[panSVR-amd] BAM records on the device failed (%s): formatting on the host threads from here on\n"),
	      ori_route(opt.ori_device && device_routes && ori_source, "[panSVR-amd] ori BAM records on the device failed (%s): formatting the second file on the host threads from here on\n"),
	      rcs((size_t)D, 0), errs((size_t)D) {}

	// reader, formatter and writer on a thread of their own (thread_pool() is per calling thread), the engine stage on this one
	void run()
	{
		std::thread reader([this] { read_stage(); }), formatter([this] { format_stage(); }), writer([this] { write_stage(); });
		engine_stage();
		reader.join(), formatter.join(), writer.join();
	}

	// ---- step 0: pieces of the reference's batches
	void read_stage()
	{
		PieceRule rule{o.batch_pairs, o.batch_bases, o.sub_pairs, o.max_use_read};
		long long pair_base = 0, n_read_pieces = 0;
		for (int slot = 0;; slot = (slot + 1) % kSlots) {
			Job &J = ring.jobs[slot];
			ring.wait_state(J, 0);
			const long long want = rule.want();
			double tw = walltime();
			bool ok = false;
			if (want > 0 && parse_route.on) {
				std::string why;
				const int r = drv.parse_window(slot, fq, J.fb, want, rule.bases_left(), o.thread_n, &why);
				if (r < 0) parse_route.fail(r, why.c_str());
				else ok = r > 0;
			}
			if (want > 0 && !parse_route.on) ok = fq.read(J.fb, want, rule.bases_left(), o.thread_n);
			if (ok) ++(J.fb.dev ? st.n_dev_pieces : st.n_host_pieces);
			st.t_read += walltime() - tw;
			st.mark(0, n_read_pieces++, tw, walltime());
			if (!ok) { J.last = true; J.batch_pairs_done = rule.in_batch_pairs; ring.set_state(J, 1); return; }
			if (rule.loaded == 0) fq.stat_params(&par);      // STAT_ of the very first read (rr.cpp:134-148), before the first batch is aligned
			J.pair_base = pair_base, pair_base += J.fb.n_pairs();
			J.batch_pairs_done = rule.took(J.fb.n_pairs(), J.fb.base_off[J.fb.R]);
			ring.set_state(J, 1);
		}
	}

	// ---- step 1: the engine(s)
	[[noreturn]] void die(const char *what)
	{
		fprintf(stderr, "[panSVR-amd] %s: %s\n", what, drv.last_error());
		abort();                                            // the reference's xassert / xopen end the same way
	}
	template <class F> void each_device(F &&fn)           // one host thread per device (an engine has one owner at a time); a failed call ends the run
	{
		auto call = [&](int d) { const int rc = fn(d); if (rc) rcs[(size_t)d] = rc, errs[(size_t)d] = drv.last_error(); };
		std::vector<std::thread> th;
		for (int d = 1; d < D; ++d) th.emplace_back(call, d);
		call(0);
		for (std::thread &t : th) t.join();
		fail_check();
	}
	void fail_check()
	{
		for (int d = 0; d < D; ++d)
			if (rcs[(size_t)d]) { fprintf(stderr, "[panSVR-amd] engine error %d on device %d: %s\n", rcs[(size_t)d], o.devices[(size_t)d], errs[(size_t)d].c_str()); abort(); }
	}
	void engine_stage()
	{
		bool created = false;
		for (int slot = 0;; slot = (slot + 1) % kSlots) {
			Job &J = ring.jobs[slot];
			ring.wait_state(J, 1);
			if (J.last) { ring.set_state(J, 2); break; }
			const double tw = walltime();
			if (!created) {
				fprintf(stderr, "Current used read status: READ_LEN=%d; ISIZE_MIN=%d; ISIZE_MID=%d; ISIZE_MAX=%d; filter_score_full_match=%d\n", par.normal_read_length, par.isize_min, 0,
				        par.isize_max, par.min_filter_score);
				if (drv.create(par, pos)) die("engine");        // (pos: a fresh engine stands where the reference's generators stand after init_run)
				created = true;
			}
			align_piece(J, tw);
			size_t hbm;                                         // steady footprint: HBM in use on the first device after the first and after the latest batch
			if (drv.hbm_used(&hbm)) { st.hbm_last = hbm; if (st.n_batches <= 3) st.hbm_first = hbm; }   // (first: after the first piece of full size -- the three before it are short ones)
			++st.n_batches, st.total_pairs += J.fb.n_pairs();
			st.t_engine += walltime() - tw;
			st.mark(1, st.n_batches - 1, tw, walltime());
			ring.set_state(J, 2);
		}
	}
	// pair i of P goes to device floor(i * D / P); every block runs from `pos`, is moved to where the one before it ended, and comes back
	void align_piece(Job &J, double tw)
	{
		const long long P = J.fb.n_pairs();
		for (int d = 0; d < D; ++d) { J.blk[(size_t)d].lo = (P * d + D - 1) / D, J.blk[(size_t)d].hi = (P * (d + 1) + D - 1) / D; }
		each_device([&](int d) {
			const Block &bk = J.blk[(size_t)d];
			const double t0 = walltime();
			int rc = drv.load(d, pos, J.fb, bk.lo, bk.hi - bk.lo);   // block 0 starts there; the others are moved by the exchange
			const double t1 = walltime();
			if (!rc) rc = drv.run(d, o.trace);
			if (st.timing && d == 0) fprintf(stderr, "[panSVR-amd] batch %lld: engine ready %.1f ms after the batch, upload %.1f ms, run %.1f ms\n", st.n_batches, (t0 - tw) * 1e3, (t1 - t0) * 1e3, (walltime() - t1) * 1e3);
			return rc;
		});
		// --emit-device: the main file's records of the piece, encoded right after the run where the window's text and the results lie (one device: no exchange below), before either is given its next piece
		J.emitted = false;
		if (emit_route.on && J.fb.dev) {
			const int rc = drv.emit_encode(J.slot, J.fb, o.not_ori);
			if (rc) emit_route.fail(rc, drv.last_error());
			else J.emitted = true;
		}
		// --ori-device: the second file's records the same way.  When both encoders ran and neither declined a pair (and --records is off),
		// nothing on the host will look at the piece's results or text: the piece is resident, its results are not downloaded and its window
		// text, where the reader left it on the device, is not fetched.  The decision is made here because the engine's results go with its
		// next run.  Any other piece takes the usual path in full.
		J.ori_emitted = J.resident = false;
		long long ori_declined = 0;
		if (ori_route.on && J.fb.dev) {
			const int rc = ori->encode(J.slot, J.fb, &ori_declined);
			if (rc) ori_route.fail(rc, ori->last_error());
			else J.ori_emitted = true;
		}
		const bool full = frec != nullptr;                      // the parity tests read the fixed-size ABI records
		J.resident = J.emitted && J.ori_emitted && !full && ori_declined == 0 && ori->main_declined(J.slot) == 0;
		if (J.fb.text_pending && !J.resident) {
			if (ori->fetch_text(J.fb)) { fprintf(stderr, "[panSVR-amd] window text: %s\n", ori->last_error()); abort(); }
		}
		st.text_d2h_bytes += J.fb.text_fetched;                  // (what the reader fetched with the piece, or the fetch above)
		if (D > 1) exchange_draw_order();
		if (drv.stream_end(D - 1, pos)) die("engine");
		if (J.resident) { ++st.resident_pieces; return; }
		each_device([&](int d) {
			long long bytes = 0;
			const int rc = drv.download(d, J.blk[(size_t)d], full, &bytes);
			if (!rc) { std::lock_guard<std::mutex> lk(ring.mu); st.d2h_bytes += bytes; }
			return rc;
		});
	}
	// The draw-order exchange: the reference draws from ONE sequence in input order, so block d starts where block d-1 ended.  A block's
	// draw count almost never depends on where it starts, so one pass of moves normally settles it; the loop covers the rest.
	void exchange_draw_order()
	{
		const double tx = walltime();
		std::vector<int64_t> start((size_t)D * 3), end((size_t)D * 3);
		for (int d = 0; d < D; ++d) for (int k = 0; k < 3; ++k) start[(size_t)d * 3 + k] = pos[k];
		for (int it = 0;; ++it) {
			for (int d = 0; d < D; ++d) if (drv.stream_end(d, &end[(size_t)d * 3])) die("engine");
			std::vector<int> moved;
			int64_t acc[3] = {pos[0], pos[1], pos[2]};
			for (int d = 0; d < D; ++d) {
				int64_t used[3];
				for (int k = 0; k < 3; ++k) used[k] = end[(size_t)d * 3 + k] - start[(size_t)d * 3 + k];
				bool mv = false;
				for (int k = 0; k < 3; ++k) if (start[(size_t)d * 3 + k] != acc[k]) mv = true, start[(size_t)d * 3 + k] = acc[k];
				if (mv) moved.push_back(d);
				for (int k = 0; k < 3; ++k) acc[k] += used[k];
			}
			if (moved.empty()) break;
			if (it > 64) { fprintf(stderr, "[panSVR-amd] draw-order exchange did not converge\n"); abort(); }
			std::vector<std::thread> th;
			for (int d : moved) th.emplace_back([&, d]() { if (drv.rebase(d, &start[(size_t)d * 3])) rcs[(size_t)d] = 1, errs[(size_t)d] = drv.last_error(); });
			for (std::thread &t : th) t.join();
			fail_check();
			++st.rebase_iters;
		}
		st.t_exchange += walltime() - tx;
	}

	// ---- step 2: records of both files, formatted for runs of pairs on -t threads and written in input order
	void progress(const Job &J)                           // output_results, rr.cpp:166
	{
		if (J.batch_pairs_done > 0) fprintf(stderr, "Processing %d reads, at block ID %d\n", (int)J.batch_pairs_done, block_id++), ++st.n_ref_batches;
	}
	void format_stage()
	{
		long long n_fmt_pieces = 0;
		for (int slot = 0;; slot = (slot + 1) % kSlots) {
			Job &J = ring.jobs[slot];
			ring.wait_state(J, 2);
			if (J.last) { progress(J); ring.set_state(J, 3); return; }     // (a line here: the input ended inside a batch)
			const double tw = walltime();
			progress(J);
			em.min_filter_score = par.min_filter_score;
			if (frec) write_records(J);
			format_piece(J);
			st.t_format += walltime() - tw;
			st.mark(2, n_fmt_pieces++, tw, walltime());
			ring.set_state(J, 3);
		}
	}
	void write_records(const Job &J)
	{
		for (const Block &bk : J.blk)
			for (long long p = bk.lo; p < bk.hi; ++p) {
				const char *t; int lens[2];
				J.fb.seq(2 * p, t, lens[0]), J.fb.seq(2 * p + 1, t, lens[1]);
				fprintf(frec, "%s\n", record_json(J.pair_base + p, &bk.full[(size_t)(2 * (p - bk.lo))], bk.V.pairs[p - bk.lo], &J.fb.ori[2 * p], lens, bk.full_cig.data(), o.trace).c_str());
			}
	}
	void format_piece(Job &J)
	{
		const long long P = J.fb.n_pairs(), chunk = 4096, nchunk = (P + chunk - 1) / chunk;
		std::vector<Bytes> &mb = J.mb, &ob = J.ob;
		mb.resize((size_t)nchunk), ob.resize((size_t)nchunk);
		for (auto &v : mb) v.clear();        // (capacity is kept from the slot's previous batch: no growth copies in steady state)
		for (auto &v : ob) v.clear();
		// --emit-device: the piece's main records come from the device; a chunk with a declined pair goes through the host formatter whole, so
		// what it reports and drops is what it always did
		// --stream-device: only the offsets and the states are fetched; a chunk without a declined pair is marked "from the device" and its records
		// stay where the encoder wrote them (write_stage hands the range to the sink)
		EmitView dev;
		const bool streamed = J.emitted && sink && sink->on();
		if (J.emitted) {
			const int rc = streamed ? sink->piece_view(J.slot, P, &dev) : drv.emit_download(J.slot, P, &dev);
			if (rc) { emit_route.fail(rc, streamed ? sink->last_error() : drv.last_error()); J.emitted = false, dev = EmitView(); }
		}
		// --ori-device: the second file's chunks by the same rule, decided on their own; its bytes are downloaded and go through fo_ori
		EmitView odev;
		if (J.ori_emitted) {
			const int rc = ori->download(J.slot, P, &odev);
			if (rc) { ori_route.fail(rc, ori->last_error()); J.ori_emitted = false, odev = EmitView(); }
		}
		if (J.resident && !(J.emitted && J.ori_emitted)) { fprintf(stderr, "[panSVR-amd] the records of a piece whose results stayed on the device cannot be fetched: the run ends here\n"); abort(); }
		if (ori) ++(J.ori_emitted ? st.n_ori_pieces : st.n_ori_host_pieces);
		J.from_dev.assign((size_t)nchunk, 0), J.dev_off = dev.off;
		++(J.emitted ? st.n_emit_pieces : st.n_emit_host_pieces);
		std::atomic<long long> next(0), n_dev_pairs(0), n_declined(0), n_spliced(0), o_dev_pairs(0), o_declined(0), o_spliced(0);
		auto work = [&]() {
			for (long long ci = next++; ci < nchunk; ci = next++) {
				const long long p0 = ci * chunk, p1 = p0 + chunk < P ? p0 + chunk : P;
				bool host_main = !dev.state;
				if (dev.state) {
					long long nd = 0;
					for (long long p = p0; p < p1; ++p) nd += dev.state[p] == 2;
					n_declined += nd, n_dev_pairs += (p1 - p0) - nd;
					if (nd) host_main = true;
					else if (!dev.bytes) J.from_dev[(size_t)ci] = 1, n_spliced += p1 - p0;
					else mb[(size_t)ci].insert(mb[(size_t)ci].end(), dev.bytes + dev.off[p0], dev.bytes + dev.off[p1]), n_spliced += p1 - p0;
				}
				bool host_ori = !odev.state;
				if (odev.state) {
					long long nd = 0;
					for (long long p = p0; p < p1; ++p) nd += odev.state[p] == 2;
					o_declined += nd, o_dev_pairs += (p1 - p0) - nd;
					if (nd) host_ori = true;
					else ob[(size_t)ci].insert(ob[(size_t)ci].end(), odev.bytes + odev.off[p0], odev.bytes + odev.off[p1]), o_spliced += p1 - p0;
				}
				if (!host_main && !host_ori) continue;
				size_t bi = 0;
				for (long long p = p0; p < p1; ++p) {
					while (p >= J.blk[bi].hi) ++bi;
					if (host_main) em.main_pair(J.fb, J.blk[bi].V, p, mb[(size_t)ci]);
					if (host_ori) em.ori_pair(J.fb, J.blk[bi].V, p, ob[(size_t)ci]);
				}
			}
		};
		thread_pool().run((int)(o.thread_n < nchunk ? o.thread_n : nchunk), [&](int) { work(); });
		st.emit_device_pairs += n_dev_pairs, st.emit_declined_pairs += n_declined, st.emit_spliced_pairs += n_spliced;
		st.ori_device_pairs += o_dev_pairs, st.ori_declined_pairs += o_declined, st.ori_spliced_pairs += o_spliced;
	}
	// --stream-device: the chunks in order, adjacent device chunks joined into one range of the slot's emitter
	void write_to_sink(Job &J)
	{
		const long long P = J.fb.n_pairs(), chunk = 4096, nchunk = (long long)J.mb.size();
		bool fine = true;
		long long run0 = -1;                                // first pair of the run of device chunks that is open
		auto flush = [&](long long p1) {
			if (run0 >= 0 && fine) fine = sink->device_chunks(J.slot, run0, p1, (long long)(J.dev_off[p1] - J.dev_off[run0]));
			run0 = -1;
		};
		for (long long ci = 0; ci < nchunk && fine; ++ci) {
			const long long p0 = ci * chunk;
			if (J.from_dev[(size_t)ci]) { if (run0 < 0) run0 = p0; continue; }
			flush(p0);
			if (fine) fine = sink->host_chunk(J.mb[(size_t)ci].data(), J.mb[(size_t)ci].size());
		}
		flush(P);
		if (fine) fine = sink->piece_done();
		if (!fine) { fprintf(stderr, "[panSVR-amd] %s: the main file cannot be written whole; the run ends here with status 2 and BOTH output files (-o and -p) are incomplete\n", sink->option()); _exit(2); }
	}
	void write_stage()
	{
		long long n_wr_pieces = 0;
		for (int slot = 0;; slot = (slot + 1) % kSlots) {
			Job &J = ring.jobs[slot];
			ring.wait_state(J, 3);
			if (J.last) return;
			const double tw = walltime();
			if (sink) {
				write_to_sink(J);
				for (size_t ci = 0; ci < J.ob.size(); ++ci) fo_ori.write_raw(J.ob[ci]);
			} else if (keep_main) {
				try {
					for (size_t ci = 0; ci < J.mb.size(); ++ci)
						if (!keep_main(J.mb[ci].data(), J.mb[ci].size())) { fprintf(stderr, "[panSVR-amd] --sort: malformed record from the formatter\n"); abort(); }
				} catch (const std::bad_alloc &) { fputs(kSortNoMem, stderr); _exit(2); }
				for (size_t ci = 0; ci < J.ob.size(); ++ci) fo_ori.write_raw(J.ob[ci]);
			} else
				for (size_t ci = 0; ci < J.mb.size(); ++ci) fo.write_raw(J.mb[ci]), fo_ori.write_raw(J.ob[ci]);
			st.t_write += walltime() - tw;
			st.mark(3, n_wr_pieces++, tw, walltime());
			ring.set_state(J, 0);
		}
	}
};

} // namespace aln
} // namespace psvr
