// bam_sort.h -- `panSVR sort`: what panSVR_run.sh does after the `aln` step with `samtools sort` + `samtools index`
// (panSVR_run.sh:53-54), so the drop-in does not depend on an external binary.  Host C++ only.
//   panSVR sort [-n] [-t threads] [-o out.bam] [--inflate-device | --inflate-threads N] [--deflate-device] in.bam      coordinate order (default) + out.bam.bai, or name order (-n)
//   panSVR sort --sort-device [-t threads] [-o out.bam] in.bam          the same files as with --deflate-device, the records kept in GPU memory (below)
// Coordinate order is samtools' (bam_sort.c bam1_lt): reference id as unsigned (unplaced records last), position, forward strand
// before reverse, ties in input order; name order compares the names with strcmp, first read before second.  The whole file is held
// in memory (the aln step's output is the signal subset of a run, not the full BAM).  The order and the writing are sorted_bam.h's, which
// `panSVR aln --sort` shares: the coordinate order is computed on the device when one is visible.
// --sort-device (sort_device_route): the file's own BGZF members go to the device as they are read, a piece of PSVR_INFLATE_BATCH compressed
// bytes at a time while the next piece is read; they are inflated into a device-resident record store and cut into records there
// (psvr_bam_store_append_bgzf, include/psvr_engine.h), and at the end of the file the store is ordered, gathered, compressed and indexed by
// sorted_bam.h's store writer: no inflated byte and no record visits the host.  Whatever fails -- no device, memory, a position the key cannot
// hold, a corrupt member, a malformed record, a truncated file -- is named on one line, the store is destroyed, and the --deflate-device
// route below runs on the same file from its beginning: its messages and its exit status are the command's.
//   panSVR sort --nsort-device [-t threads] [-o out.bam] in.bam         name order by the same route: the store is ordered by psvr_bam_store_order_names,
// the header says SO:queryname and no index is written; the file is that of -n --deflate-device, which is also what takes over.  Plain -n
// computes its order on the device as well when one is visible (name_order_device: the names in one blob, psvr_sort_order_names).
#pragma once
#include <stdint.h>
#include <stdio.h>
#include <string.h>
#include <time.h>
#include <string>
#include <vector>
#include <functional>
#include <future>
#include "bam_reader.h"
#include "bgzf_pieces.h"
#include "name_key.h"
#include "sorted_bam.h"

namespace psvr {

// The device route of `panSVR sort --sort-device` over a backend (cli_main.cpp: psvr_bam_store_* and psvr_bgzf_stream_*): what
// finish_sorted_store asks (sorted_bam.h), int store_create(), and int store_append_bgzf(const void *, int64_t n, int64_t skip, int32_t n_ref, int64_t *used, int64_t *bad_member),
// int store_chain_info(psvr_bam_chain_info_t *).  0: out_fn and its .bai are written; -1: the route was left (one line said why), the caller
// sorts the file its other way; 2: the output cannot be written.  by_name (--nsort-device): name order, no index; the backend has store_order_names().
template <class Backend> int sort_device_route(Backend &be, const std::string &in_fn, const std::string &out_fn, bool by_name = false)
{
	const char *opt = by_name ? "--nsort-device" : "--sort-device";
	auto left = [&](const char *call, const std::string &why) {
		fprintf(stderr, "[panSVR-amd] sort %s: %s failed (%s): the file is read again and sorted by the %s--deflate-device route\n", opt, call, why.c_str(), by_name ? "-n " : "");
		return -1;
	};
	if (in_fn == "-") return left("opening the input", "a pipe cannot be read twice");
	std::string text;
	std::vector<BamRef> refs;
	size_t header_bytes = 0;
	{
		BamReader rd;                                            // the serial reader: the header's text, the references, and how many inflated bytes they took
		if (!rd.open(in_fn.c_str())) return left("reading the header", rd.error());
		text = rd.header_text, header_bytes = rd.header_bytes;
		for (auto &rf : rd.refs) refs.push_back({rf.first, (uint32_t)rf.second});
	}
	FILE *f = fopen(in_fn.c_str(), "rb");
	if (!f) return left("opening the input", "cannot open " + in_fn);
	struct Closer { FILE *f; Backend &be; ~Closer() { fclose(f); be.store_destroy(); } } guard{f, be};
	// the first member to send is the one that holds the first record's first byte; `skip` bytes of it are the header's (bgzf_pieces.h)
	PieceFail fail;
	long long skip = 0;
	if (!bgzf_seek_first_record(f, header_bytes, &skip, &fail)) return left(fail.call.c_str(), fail.why);
	if (be.store_create()) return left("store create", be.last_error());
	auto now = [] { struct timespec ts; clock_gettime(CLOCK_MONOTONIC, &ts); return ts.tv_sec + 1e-9 * ts.tv_nsec; };
	const double t0 = now();
	long long members_in = 0;
	const bool walked = bgzf_for_pieces(be, f, skip, &fail, [&](const uint8_t *p, size_t have, long long skip_now, int64_t *used, PieceFail *why) {
		int64_t bad = -1;
		if (be.store_append_bgzf(p, (int64_t)have, skip_now, (int32_t)refs.size(), used, &bad)) { *why = {"append_bgzf", be.last_error()}; return false; }
		for (size_t at = 0; at < (size_t)*used;) {               // the members the call took, for the statistics line
			uint32_t bsize = 0, xlen = 0;
			if (bgzf_member_header(p + at, (uint64_t)*used - at, &bsize, &xlen) != 0) break;
			at += bsize, ++members_in;
		}
		return true;
	});
	if (!walked) return left(fail.call.c_str(), fail.why);
	psvr_bam_chain_info_t ci;
	if (be.store_chain_info(&ci)) return left("chain_info", be.last_error());
	if (ci.tail_bytes) return left("the end of the input", "truncated BAM stream: the file ends " + std::to_string((long long)ci.tail_bytes) + " bytes into a record");
	int64_t n_rec = 0, n_bytes = 0;
	if (be.store_info(&n_rec, &n_bytes)) return left("info", be.last_error());
	const double t1 = now();
	StoreWritten w;
	if (const int rc = finish_sorted_store(be, out_fn, text, refs, by_name, kDeflateDeviceBlocks, &w)) return rc;
	const double t2 = now();
	fprintf(stderr, "[panSVR-amd] sort: %lld records -> %s (%s order, ordered on the device, records kept on the device)\n", w.records, out_fn.c_str(), by_name ? "name" : "coordinate");
	fprintf(stderr, "[panSVR-amd] sort %s: %lld records, %lld record bytes, %lld members in, %lld members out, %lld segments: %lld without a guess, %lld wrong guesses, %lld walked again; append %.3f s, order %.3f s, write %.3f s\n",
	        opt, (long long)n_rec, (long long)n_bytes, members_in, w.members, (long long)ci.segments, (long long)ci.no_guess, (long long)ci.wrong_guess, (long long)ci.rewalked,
	        t1 - t0, w.t_order, t2 - t1 - w.t_order);
	return 0;
}

// what bam_sort_main's --sort-device and --nsort-device call: (in.bam, out.bam, by_name, --deflate-effort) -> sort_device_route's answer over the
// caller's backend, whose stream compresses at that effort
typedef std::function<int(const std::string &, const std::string &, bool, int)> SortDeviceFn;
// the compressor of --deflate-device at an effort of 0..3 (the CLI hands in adapters over psvr_bgzf_compress_members_effort)
typedef BgzfMembersFn (*BgzfMembersAtFn)(int effort);

// `panSVR sort -n` on the device: the names of R in one blob (each up to its first NUL inside the name field), flag & 0xc0 as the tie key,
// ordered by psvr_sort_order_names: name_order's order.  false with the reason: the caller orders with name_order
inline bool name_order_device(const SortRecords &R, int device, std::vector<uint32_t> &ord, std::string *err)
{
	const size_t n = R.size();
	std::vector<uint8_t> blob, tie(n);
	std::vector<int64_t> off(n);
	blob.reserve(n * 32);
	for (size_t i = 0; i < n; ++i) {
		const uint8_t *r = R.rec(i);
		off[i] = (int64_t)blob.size(), tie[i] = (uint8_t)name_tie_key(r[18]);
		blob.insert(blob.end(), r + 36, r + 36 + name_len_rec(r));
		blob.push_back(0);
	}
	ord.resize(n);
	if (psvr_sort_order_names(device, (int64_t)n, blob.data(), (int64_t)blob.size(), off.data(), tie.data(), ord.data())) { *err = psvr_last_error(); return false; }
	return true;
}

// what --sort-device's usage text says about its speed
#define PSVR_SORT_CMD_DEVICE_MEASURED \
	"Measured on the 1.6 M records of\n" \
	"                                1 M pairs, -t 16 (three interleaved runs, median wall): 0.522 s against 2.359 s for --deflate-device, 1.303 s with\n" \
	"                                --inflate-device and 1.162 s with --inflate-threads 16 on top (DESIGN.md section 8 f3)"

// what --nsort-device's usage text says about its speed
#define PSVR_NSORT_CMD_DEVICE_MEASURED \
	"Measured on the 1.6 M records of 1 M pairs,\n" \
	"                                -t 16 (three interleaved runs, median wall): 0.520 s against 2.361 s for -n --deflate-device with the order on one\n" \
	"                                host thread and 1.188 s with --inflate-threads 16 on top (ahead: the ranges do not overlap); plain -n --deflate-device\n" \
	"                                with its order from the GPU 2.079 s (DESIGN.md section 8 f3)"

// what --deflate-effort's usage text says about its sizes and speed
#define PSVR_DEFLATE_EFFORT_MEASURED \
	"Measured on the 1.6 M records\n" \
	"                                 of 1 M pairs (-t 16, three interleaved runs): the sorted file 118.5 MB at effort 0 (+22.9 %% on zlib's default\n" \
	"                                 level, 96.4 MB), 99.8 MB at 1 (+3.5 %%), 97.6 MB at 2 (+1.2 %%), 96.3 MB at 3 (-0.1 %%); sort --sort-device's write\n" \
	"                                 phase 0.16 s at effort 0 (the parent build: 0.16 s, unchanged), 0.24 / 0.33 / 0.49 s at 1 / 2 / 3, aln\n" \
	"                                 --sort-device's sort part 0.16 s (parent 0.16) / 0.24-0.26 / 0.33 / 0.49 s: every effort stays ahead of the host\n" \
	"                                 routes.  A call of 201 MB with its copies: 14.8 / 23.5 / 37.0 / 58.4 ms (parent 14.9), the member kernel alone\n" \
	"                                 7.7 / 16.3 / 29.9 / 51.3 ms (parent 7.7) (DESIGN.md section 4 (6))"

// --deflate-effort's argument: "0" .. "3" and nothing else; -1 for anything else (no argument, text, a number with a tail), which the commands refuse
inline int parse_deflate_effort(const char *s) { return s && s[0] >= '0' && s[0] <= '3' && !s[1] ? s[0] - '0' : -1; }

// deflate_fn: the compressor --deflate-device uses (the CLI hands in &psvr_bgzf_compress_members); deflate_at: the same per --deflate-effort
// (null: the option is refused, this build has one effort)
inline int bam_sort_main(int argc, char **argv, BgzfMembersFn deflate_fn = nullptr, SortDeviceFn sort_device_fn = nullptr, BgzfMembersAtFn deflate_at = nullptr)
{
	bool by_name = false;
	int threads = 4, inflate_device = -1, inflate_threads = 0;
	bool bad_arg = false, deflate_device = false, sort_device = false, nsort_device = false, effort_given = false;
	int effort = 0;
	std::string out_fn, in_fn;
	for (int i = 2; i < argc; ++i) {
		if (!strcmp(argv[i], "-n")) by_name = true;
		else if (!strcmp(argv[i], "--nsort-device")) nsort_device = deflate_device = true;
		else if ((!strcmp(argv[i], "-t") || !strcmp(argv[i], "-@")) && i + 1 < argc) threads = atoi(argv[++i]);
		else if (!strcmp(argv[i], "-o") && i + 1 < argc) out_fn = argv[++i];
		else if (!strcmp(argv[i], "--inflate-device")) inflate_device = 0;
		else if (!strcmp(argv[i], "--deflate-device")) deflate_device = true;
		else if (!strcmp(argv[i], "--sort-device")) sort_device = deflate_device = true;
		else if (!strcmp(argv[i], "--deflate-effort")) effort = parse_deflate_effort(i + 1 < argc ? argv[++i] : nullptr), effort_given = true;
		else if (!strcmp(argv[i], "--inflate-threads") && i + 1 < argc) { inflate_threads = atoi(argv[++i]); bad_arg |= inflate_threads < 1; }
		else in_fn = argv[i];
	}
	if (bad_arg) fprintf(stderr, "--inflate-threads wants a positive number\n");
	if (in_fn.empty() || bad_arg) {
		fprintf(stderr, "usage: panSVR sort [-n] [-t threads] [-o out.bam] [--inflate-device | --inflate-threads N] [--deflate-device | --sort-device | --nsort-device] [--deflate-effort N] in.bam\n"
		                "         -n                     name order (the names as strcmp compares them, first read before second, ties in input order), no index;\n"
		                "                                the order is computed on the GPU (device 0) when one is visible, on one host thread otherwise\n"
		                "         --inflate-device       inflate the input's BGZF members on the GPU (device 0), a chunk of the file at a time\n"
		                "                                (faster than the default reader; it does not win against --inflate-threads 16)\n"
		                "         --inflate-threads INT  inflate them with zlib on INT host threads (also what takes over when the device route fails)\n"
		                "         --deflate-device       compress the output's BGZF members on the GPU (device 0), a wavefront per member of 0xff00 bytes, 1024\n"
		                "                                members a call.  Measured on the 2 M records of 1 M pairs, -t 16: 2.24-2.28 s against 2.45-3.04 s by\n"
		                "                                default (reading the input is most of both), the file 23 %% larger than zlib's default level makes it (--deflate-effort);\n"
		                "                                a call of 201 MB: 14.9 ms = 13.5 GB/s with its copies, zlib's default level on 16 threads 491 ms\n"
		                "         --deflate-effort INT   0-3: how hard that encoder searches; with --deflate-device, --sort-device or --nsort-device only [0].\n"
		                "                                0: one hash-table candidate per position and the distances 1 and 2, every match taken (greedy).  1 / 2 / 3: a\n"
		                "                                hash chain of 4 / 8 / 16 candidates and lazy matching, zlib's means.  " PSVR_DEFLATE_EFFORT_MEASURED "\n"
		                "         --sort-device          coordinate order only; implies --deflate-device.  The file's BGZF members are inflated on the GPU (device 0)\n"
		                "                                into a record store in its memory, the records are found, ordered, gathered and compressed there: the files\n"
		                "                                are those of --deflate-device, byte for byte.  Whatever the device route cannot do (no device, memory, a\n"
		                "                                malformed or truncated file) is named, and the --deflate-device route sorts the file.  " PSVR_SORT_CMD_DEVICE_MEASURED "\n"
		                "         --nsort-device         name order by the same route; implies -n and --deflate-device.  The store is ordered by name on the GPU (the\n"
		                "                                names cut into 8-byte chunks, a stable radix sort per chunk); the file is that of -n --deflate-device, byte\n"
		                "                                for byte, and no index is written.  Whatever the device route cannot do is named, and the -n --deflate-device\n"
		                "                                route sorts the file.  Not with --sort-device.  " PSVR_NSORT_CMD_DEVICE_MEASURED "\n");
		return 1;
	}
	if (effort_given && (effort < 0 || effort > 3)) { fprintf(stderr, "--deflate-effort wants 0 .. 3\n"); return 1; }
	if (effort_given && (!deflate_device || !deflate_at)) { fprintf(stderr, "--deflate-effort cannot be given without --deflate-device, --sort-device or --nsort-device: it is the effort of the GPU's BGZF encoder (a wavefront per member), which only those routes use\n"); return 1; }
	if (sort_device && nsort_device) { fprintf(stderr, "--nsort-device cannot be combined with --sort-device: a file has one order, name (--nsort-device) or coordinate (--sort-device)\n"); return 1; }
	if (sort_device && by_name) { fprintf(stderr, "--sort-device cannot be combined with -n: name order is not built on the device by this option; --nsort-device is the name order's device route\n"); return 1; }
	if (nsort_device) by_name = true;
	if (out_fn.empty()) out_fn = in_fn + (by_name ? ".nsorted.bam" : ".sorted.bam");
	if (threads < 1) threads = 1;
	if (sort_device || nsort_device) {
		const int rc = sort_device_fn ? sort_device_fn(in_fn, out_fn, nsort_device, effort) : -1;
		if (!sort_device_fn) fprintf(stderr, "[panSVR-amd] sort %s: this build has no device route: the file is sorted by the %s--deflate-device route\n", nsort_device ? "--nsort-device" : "--sort-device", nsort_device ? "-n " : "");
		if (rc >= 0) return rc;
	}
	BamReader rd;
	if (inflate_device >= 0 || inflate_threads > 0) rd.set_batched(inflate_device, inflate_threads);
	if (!rd.open(in_fn.c_str())) { fprintf(stderr, "[panSVR-amd] sort: %s\n", rd.error().c_str()); return 2; }
	// every record as it stands in the file (block_size + body, the fixed part re-encoded), one buffer
	SortRecords R;
	BamRecord r;
	while (rd.next(r)) {
		uint8_t f[32];
		auto p32 = [&](int o, uint32_t v) { for (int k = 0; k < 4; ++k) f[o + k] = (uint8_t)(v >> (8 * k)); };
		p32(0, (uint32_t)r.tid), p32(4, (uint32_t)r.pos);
		f[8] = r.l_qname, f[9] = r.mapq, f[10] = f[11] = 0;                    // (the bin: recomputed from the CIGAR's span by add)
		f[12] = (uint8_t)r.n_cigar, f[13] = (uint8_t)(r.n_cigar >> 8), f[14] = (uint8_t)r.flag, f[15] = (uint8_t)(r.flag >> 8);
		p32(16, (uint32_t)r.l_qseq), p32(20, (uint32_t)r.mtid), p32(24, (uint32_t)r.mpos), p32(28, (uint32_t)r.isize);
		R.add(f, r.data.data(), r.data.size());
	}
	if (!rd.error().empty()) { fprintf(stderr, "[panSVR-amd] sort: %s\n", rd.error().c_str()); return 2; }
	std::vector<uint32_t> ord;
	bool on_device = false;
	std::string err;
	if (by_name) {
		// on the device when one is visible, as coordinate_order; a call that fails says so and the host orders (name_order is the rule either way)
		if (R.size() > 0 && R.size() < ((size_t)1 << 32) && psvr_device_count() > 0) {
			on_device = name_order_device(R, 0, ord, &err);
			if (!on_device) fprintf(stderr, "[panSVR-amd] sort: device name order failed (%s): the names are ordered on the host\n", err.c_str());
		}
		if (!on_device) name_order(R, ord);
	}
	else if (!coordinate_order(R, 0, ord, &on_device, &err)) { fprintf(stderr, "[panSVR-amd] sort: device order: %s\n", err.c_str()); return 2; }
	if (!write_sorted_bam(out_fn, rd.header_text, rd.refs, R, ord, by_name, threads, &err, deflate_device ? (deflate_at ? deflate_at(effort) : deflate_fn) : nullptr, 0)) { fprintf(stderr, "%s\n", err.c_str()); return 2; }
	fprintf(stderr, "[panSVR-amd] sort: %zu records -> %s (%s order%s)\n", ord.size(), out_fn.c_str(), by_name ? "name" : "coordinate", on_device ? ", ordered on the device" : "");
	return 0;
}

} // namespace psvr
