// cli_main.cpp -- the `panSVR` command on the MI355X engine: the sub-command dispatch and `panSVR aln` / `fc_aln`, the host side of the
// reference's three-stage pipeline (load_reads -> [engine] -> output_results; src/PanSVgenerateVCF/read_realignment.cpp:26-176) above
// the C ABI of include/psvr_engine.h.  Same options, positional arguments, stderr progress lines and SAM/BAM records as the reference.
//
// aln_main is a list of steps: options, header, index, the pipeline, the --sort tail, teardown, statistics.  The pipeline itself -- the
// four overlapped stages, the pieces, the block split over devices and the draw-order exchange -- is aln_pipeline.h, host C++ over a
// driver type; EngineDriver below is the product's driver, the only place that calls psvr_engine_*, psvr_fastq_* and psvr_bam_emit_*
// (tests/tools/aln_pipeline_check.cpp runs the same pipeline over the CPU emulation).  Other host-side pieces: fastq_batch.h (step 0:
// batches parsed straight into page-locked upload buffers), sam_emit.h + bam_writer.h (step 2: records of the pairs that are written).
//
// Multi-GPU (`--devices 0,1,...`): the index is resident on every device (one host upload, then device-to-device copies),
// every batch is cut into contiguous blocks -- pair i of n goes to device floor(i * D / n), kt_for's contract of independent
// items (clib/kthread.c:43-86) with the order kept -- and because the reference draws from ONE rand()/random_r sequence in input
// order, block d is moved to start where block d-1 ended (psvr_engine_rebase) before the ordered gather into step 2.
#define PSVR_BGZF_ON_DEVICE 1
#include <getopt.h>
#include <signal.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <sys/stat.h>
#include <time.h>
#include <unistd.h>
#include <memory>
#include <string>
#include <thread>
#include <vector>
#include "../../include/psvr_engine.h"
#include "aln_pipeline.h"
#include "index_build.h"
#include "signal_step.h"
#include "signal_device_route.h"
#include "bam_sort.h"
#include "sorted_bam.h"
#include "bgzf_stream_sink.h"
#include "sort_store_sink.h"

using namespace psvr;
using aln::walltime;

struct Opt : aln::PipeOpt {
	int gap_open = 16, gap_ex = 1, gap_open2 = 32, gap_ex2 = 0, match = 2, mismatch = 12, zdrop = 400, bw = 500;
	std::string out = "./output.bam", out_ori = "./output_ori.bam";
	bool sam = false;
	std::string index_dir, reads, header;
	std::string records;      // --records FILE: one JSON line per pair (what the parity tests compare)
	bool sig_all = false, sig_discard = false, sig_by_name = false;   // BAM input: fc_signal's -D / -U / -N
	bool from_bam = false;                       // <reads> is a *.bam
	int bam_level = -1;                          // zlib level of the BGZF blocks (-1 = zlib's default, what htslib's "wb" uses)
	bool bgzf_device = false;                    // the main file's BGZF blocks compressed on the first device (psvr_bgzf_compress)
	bool deflate_device = false;                 // the BAM files' BGZF members (the sorted file's too) compressed on the first device, a wavefront per member (psvr_bgzf_compress_members)
	bool inflate_device = false;                 // BAM input: its BGZF members inflated on the first device (psvr_bgzf_decompress) ...
	int inflate_threads = 0;                     // ... or with zlib on this many host threads (bam_reader.h's batched mode)
	int deflate_effort = 0;                      // --deflate-effort: the wavefront encoder's effort, 0..3 (deflate_wave_device.h); wants one of the routes that compress through it
	bool deflate_effort_given = false;
	bool stream_device = false;                  // the main BAM file's stream gathered in HBM: records from the encoder to the member compressor device to device (implies emit_device and deflate_device)
	bool sort = false;                           // --sort: the main file coordinate-sorted + its .bai (sorted_bam.h), ordered on the first device
	bool bam_device = false;                     // a name-sorted *.bam read file: the signal step's device route hands windows of FASTQ text in HBM to the reader stage
	bool mate_device = false;                    // a position-sorted *.bam read file: the same through the position-sorted mode's route, the runs of its blocks added to one kept window
	int block_records = 0;                       // --block-records: the signal step's block limit on both routes (0: its default)
	bool sort_device = false;                    // ... with the records kept, ordered and compressed in HBM (sort_store_sink.h; implies sort, emit_device and deflate_device)
};

// what --parse-device's usage text says about its speed
#define PSVR_PARSE_DEVICE_MEASURED \
	"Measured (1 M pairs = 830 MB of text, -t 16, three interleaved runs): it LOSES to the host parser: read stage\n" \
	"                                 0.21-0.27 s against 0.08-0.12 s, SAM wall 0.36-0.44 s against 0.29-0.32 s, BAM with --deflate-device 0.44-0.55 s\n" \
	"                                 against 0.44-0.46 s.  The kernels are not the cost (a 65 536-pair piece, 62 MB: newline passes 16 + 18 us, extract\n" \
	"                                 116 us, all launches ~0.3 ms); the staging copy, the upload and the downloads are"

// what --stream-device's usage text says about its speed
#define PSVR_STREAM_DEVICE_MEASURED \
	"Measured (1 M pairs, -t 16, three\n" \
	"                                 interleaved runs, median wall): 0.390 s against 0.525 s for --emit-device --deflate-device and 0.373 s for plain\n" \
	"                                 --deflate-device (on par: the ranges overlap; DESIGN.md section 8 f3)"

// what --ori-device's usage text says about its speed
#define PSVR_ORI_DEVICE_MEASURED \
	"Measured\n" \
	"                                 (1 M pairs, -t 16, three interleaved runs, median wall): behind --mate-device\n" \
	"                                 --stream-device 0.526 s against 0.582 s without it, behind --stream-device on FASTQ 0.488 s against 0.406 s (the\n" \
	"                                 ranges overlap in both: no gain shown); format_s 0.05-0.06 s against 0.09 s, engine_s 0.31 / 0.34 s against 0.35 /\n" \
	"                                 0.30 s, d2h_bytes 0 against 211 MB, text_d2h_bytes 6.7 MB of 830 MB (DESIGN.md section 8 f3)"

// what --sort-device's usage text says about its speed
#define PSVR_SORT_DEVICE_MEASURED \
	"Measured (1 M pairs, -t 16,\n" \
	"                                 three interleaved runs, median wall): 0.587 s against 1.036 s for --sort --deflate-device and 1.300 s with --emit-device\n" \
	"                                 on top (ahead: the ranges do not overlap); its sort part 0.169 s against 0.645 s (DESIGN.md section 8 f3)"

static int usage()
{
	fprintf(stderr,
	        "\n  Usage:     panSVR  aln|fc_aln  [Options] <IndexDir> [ReadFiles.fa][ori_header_fn.sam]>\n"
	        "  Basic:   \n"
	        "    <IndexDir>      FOLDER   the directory contains index (or the anchor FASTA: the index is then built in GPU memory)\n"
	        "    [ReadFiles.fa]  FILES    reads files, FASTQ(A) format (or fq.gz), read 1 and 2 of a pair stored together ('-' = stdin),\n"
	        "                             or a *.bam: the signal step then runs in-process ([ori_header.sam] is written;\n"
	        "                             -N / -D / -U as in fc_signal: name-sorted input / all pairs are signals / drop fully matching pairs)\n"
	        "                             Using [signal] command to generate this type of file\n"
	        "    [ori_header.sam]  FILES  Header file of original BAM/CRAM file\n"
	        "  Options:\n"
	        "    -t, --thread            INT  host threads for parsing / formatting / compression (the alignment runs on the GPU) [4]\n"
	        "    -O, --gap-open1         INT  Gap open penalty 1 [16]\n"
	        "    -P, --gap-open2         INT  Gap open penalty 2 [32]\n"
	        "    -E, --gap-extension1    INT  Gap extension penalty 1 [1]\n"
	        "    -F, --gap-extension2    INT  Gap extension penalty 2 [0]\n"
	        "    -M, --match-score       INT  Match score [2]\n"
	        "    -m, --mis-score         INT  Mismatch score [12]\n"
	        "    -z, --zdrop             INT  Z-drop score [400]\n"
	        "    -w, --band-width        INT  parsed and ignored like the reference (DP band is fixed at 200) [500]\n"
	        "    -o, --output            STR  Output file [./output.bam]\n"
	        "    -p, --output_signal_ori STR  Reads not fully aligned by aligner nor re-aligner [./output_ori.bam]\n"
	        "    -Q, --not-ori                NOT output original result when score of ORI is bigger\n"
	        "    -S, --SAM                    Output as SAM, default is BAM\n"
	        "    -R, --max_use_read      INT  Max number of read pairs to align\n"
	        "        --devices           LIST HIP devices, e.g. 0,1,2,3 or 0-7: every batch is split over them in input order [0]\n"
	        "        --device            INT  the same for one device\n"
	        "        --batch             INT  read pairs per batch [2000000]\n"
	        "        --batch-bases       INT  bases per batch (the reference stops a batch at 100 MB of bases) [100000000]\n"
	        "        --sub-batch         INT  pairs per pipeline piece of a batch, 0 = whole batches (results do not depend on it) [65536]\n"
	        "        --compress-level    INT  zlib level of the BAM output's BGZF blocks, 0-9 (1 is ~3x faster than the default) [-1 = default, like htslib]\n"
	        "        --bgzf-fast              BGZF blocks from the built-in encoder on the -t threads (1.6x the speed of level 1, blocks ~10%% larger)\n"
	        "        --bgzf-device            compress the BAM output's BGZF blocks on the GPU (a lane per block; ~10 %% larger than zlib level 1,\n"
	        "                                 the host's deflate is what bounds the BAM route otherwise)\n"
	        "        --sort                   write the main output (-o) coordinate-sorted with its index <out>.bai, as `panSVR sort`\n"
	        "                                 would from the unsorted file (ordered on the first device of --devices; not with -S,\n"
	        "                                 --compress-level, --bgzf-fast or --bgzf-device)\n"
	        "        --deflate-device         compress the BAM output's BGZF members on the GPU (the first device), a wavefront per member of 0xff00\n"
	        "                                 bytes: both files, and with --sort the sorted file (not with -S, --compress-level, --bgzf-fast or\n"
	        "                                 --bgzf-device).  Measured: a call of 201 MB of records 14.9 ms = 13.5 GB/s with its copies (--bgzf-device\n"
	        "                                 34.6 ms; zlib level 1 / default level / --bgzf-fast on 16 threads 222 / 491 / 161 ms), members 0.7 %% larger\n"
	        "                                 than zlib level 1's and 4.8 %% larger than the default level's on those records.  1 M pairs, -t 16:\n"
	        "                                 `aln` 0.44 s against 1.05-1.12 s by default and 0.47 s with --bgzf-fast; `aln --sort` 1.03-1.17 s against\n"
	        "                                 1.33-1.83 s (its sort part 0.65-0.74 s against 0.91-1.35 s), the sorted file 23 %% larger than the default\n"
	        "                                 level's (--deflate-effort closes that gap).  Whether the engine's launches queue behind the deflate calls (a stream of the lowest priority\n"
	        "                                 beside the engine's) has not been looked at\n"
	        "        --deflate-effort    INT  0-3: how hard that encoder searches; with --deflate-device, --stream-device or --sort-device only [0].\n"
	        "                                 0: one hash-table candidate per position and the distances 1 and 2, every match taken (greedy).  1 / 2 / 3: a\n"
	        "                                 hash chain of 4 / 8 / 16 candidates and lazy matching, zlib's means.  " PSVR_DEFLATE_EFFORT_MEASURED "\n"
	        "        --inflate-device         a *.bam read file: inflate its BGZF members on the GPU (the first device; a wavefront per member,\n"
	        "                                 a chunk of the file at a time, on a stream of its own; faster than the default reader, but it\n"
	        "                                 does not win against --inflate-threads 16.  Whether the engine's launches queue behind the inflate\n"
	        "                                 calls on the shared GPU has not been measured)\n"
	        "        --inflate-threads   INT  ... or with zlib on INT host threads (also what takes over when the device route fails)\n"
	        "        --parse-device           FASTQ input (a file, '-' or fq.gz): parse every window on the GPU (the only device of --devices): line index,\n"
	        "                                 sequence lengths, bases and the comments' numbers; the window is staged in page-locked memory on the -t\n"
	        "                                 threads, the bases reach the engine device to device, the pieces and the records are the same.  A call\n"
	        "                                 that fails (a window of 4 GiB or more, a device error) leaves the rest of the input to the host threads.\n"
	        "                                 " PSVR_PARSE_DEVICE_MEASURED "\n"
	        "        --emit-device            FASTQ input: implies --parse-device; the main BAM file's records are encoded on the GPU as well (a chunk with\n"
	        "                                 a pair the encoder declines is formatted on the host threads, and so is the second file unless --ori-device\n"
	        "                                 is given)\n"
	        "        --ori-device             FASTQ input: implies --emit-device; the second (-p) file's records are encoded on the GPU as well, from the\n"
	        "                                 FLAG_ / CIGAR_ / MATE_ / TAG_ text of the comments (a chunk with a pair that encoder declines is formatted on the\n"
	        "                                 host threads).  A piece of which neither encoder declined a pair is resident: its results are not downloaded and,\n"
	        "                                 behind --bam-device / --mate-device, its text is not fetched.  Not with -S or more than one entry in --devices.\n"
	        "                                 A failed call leaves the second file to the host threads from there on.  Combines with --stream-device,\n"
	        "                                 --sort-device, --deflate-device, --bam-device, --mate-device and --sort.  " PSVR_ORI_DEVICE_MEASURED "\n"
	        "        --stream-device          FASTQ input: implies --emit-device and --deflate-device; the main BAM file's records go from the encoder to\n"
	        "                                 the BGZF member compressor inside GPU memory (a device-resident stream cut every 0xff00 bytes) and only the\n"
	        "                                 compressed members come to the host; chunks the host formatted are uploaded into the same stream.  Not with\n"
	        "                                 --sort, -S or more than one entry in --devices.  A failed stream call hands what is pending and everything\n"
	        "                                 after it to the host members route, in order.  " PSVR_STREAM_DEVICE_MEASURED "\n"
	        "        --sort-device            FASTQ input: implies --sort, --emit-device and --deflate-device; the main file's records stay in GPU memory until\n"
	        "                                 the input ends (a record store in chunks that never move), are ordered there, gathered in sorted order into the\n"
	        "                                 device-resident BGZF stream and compressed: only the members and the index's table come to the host.  The three\n"
	        "                                 files are those of --sort --deflate-device, byte for byte.  Not with -S, --stream-device, --compress-level,\n"
	        "                                 --bgzf-fast, --bgzf-device or more than one entry in --devices.  A failed store call downloads the records and\n"
	        "                                 leaves the rest to the host's sorted writer.  " PSVR_SORT_DEVICE_MEASURED "\n"
	        "        --bam-device             with -N and a *.bam read file: the file's members are inflated, paired, judged and formatted as FASTQ text in GPU\n"
	        "                                 memory (the route of `signal -N --signal-device`), and the reader stage parses that text where it lies: only\n"
	        "                                 the compressed members of the input cross to the device.  Implies --parse-device; --emit-device, --stream-device\n"
	        "                                 and --sort-device then apply to the BAM input.  Whatever the route cannot do (no device, a pipe, a corrupt or\n"
	        "                                 truncated file, a failing call on either side) is named on one line, and the host fused route reads the file\n"
	        "                                 again, silent for the pairs already handed over.  Not with more than one entry in --devices\n"
	        "        --mate-device            without -N and a *.bam read file sorted by position: the same through the route of `signal --mate-device` (blocks mated\n"
	        "                                 in GPU memory, the left-overs paired by name there).  The windows of consecutive blocks and slices are put\n"
	        "                                 together on the device until they hold --sub-batch pairs (0: a batch's pair limit), so a file with many small\n"
	        "                                 blocks does not become as many pieces.  Implies --parse-device; --emit-device, --stream-device and --sort-device\n"
	        "                                 apply as behind --bam-device, and the route is left the same way.  Not with -N (that is --bam-device), not with\n"
	        "                                 more than one entry in --devices\n"
	        "        --block-records     INT  BAM input without -N: primary records of a block of the position-sorted mode at the most, on both routes [1000000]\n"
	        "        --records           STR  dump per-pair decision records (JSON lines) for parity checks\n"
	        "        --trace                  add per-strand seed/chain hashes to --records\n\n");
	return 1;
}

static double cputime() { return (double)clock() / CLOCKS_PER_SEC; }
struct IndexSvNames : SvNames {
	const psvr_index_t *idx = nullptr;
	const char *print_string(int sv) const override { return psvr_index_sv_print_string(idx, sv); }
	const char *vcf_id(int sv) const override { return psvr_index_sv_vcf_id(idx, sv); }
};

// `panSVR index [-k 22] [--sparse-hash] <anchors.fa> <IndexDir>`: what `deBGA index -k 22 <anchors.fa> <IndexDir>` builds
// (panSVR_run.sh runs it on the SV anchor reference before `aln`).  Host only.
static int index_main(int argc, char **argv)
{
	bool dense = true;
	std::vector<std::string> pos;
	for (int i = 2; i < argc; ++i) {
		if (!strcmp(argv[i], "-k") && i + 1 < argc) { if (atoi(argv[++i]) != 22) { fprintf(stderr, "panSVR aln probes a k = 22 index: -k must be 22\n"); return 1; } }
		else if (!strcmp(argv[i], "--sparse-hash")) dense = false;
		else pos.push_back(argv[i]);
	}
	if (pos.size() != 2) { fprintf(stderr, "usage: panSVR index [-k 22] [--sparse-hash] <anchors.fa> <IndexDir>\n"); return 1; }
	psvr::IndexBuilder b;
	psvr::BuiltIndex ix;
	if (!b.build(pos[0].c_str(), &ix)) { fprintf(stderr, "[panSVR-amd] index: %s\n", b.error().c_str()); return 2; }
	std::string dir = pos[1], err;
	while (dir.size() > 1 && dir.back() == '/') dir.pop_back();
	if (!psvr::IndexBuilder::write_dir(ix, dir, dense, &err)) { fprintf(stderr, "[panSVR-amd] index: %s\n", err.c_str()); return 2; }
	fprintf(stderr, "[panSVR-amd] index: %zu unipaths, %llu distinct 22-mers, %zu positions\n", ix.seqf.size() - 1, (unsigned long long)ix.n_kmer, ix.pos.size());
	return 0;
}

static bool parse_devices(const char *s, std::vector<int> *out)
{
	out->clear();
	const char *p = s;
	while (*p) {
		char *e;
		long a = strtol(p, &e, 10), b = a;
		if (e == p || a < 0) return false;
		if (*e == '-') { const char *q = e + 1; b = strtol(q, &e, 10); if (e == q || b < a) return false; }
		for (long d = a; d <= b; ++d) out->push_back((int)d);
		if (*e == ',') ++e; else if (*e) return false;
		p = e;
	}
	return !out->empty() && out->size() <= 64;
}

[[noreturn]] static void die(const char *what)
{
	fprintf(stderr, "[panSVR-amd] %s: %s\n", what, psvr_last_error());
	abort();                                                // the reference's xassert / xopen end the same way
}


// The product's engine driver of aln_pipeline.h (the operations are described there): one index per DISTINCT device, one engine per entry of
// --devices, and per pipeline slot what the two device routes keep between stages.
struct EngineDriver {
	const std::vector<int> devices;
	std::vector<int> first;            // per entry of --devices: the first entry that names the same device (itself: it owns that device's index)
	std::vector<psvr_index_t *> idx;
	std::vector<psvr_engine_t *> eng;
	psvr_fastq_t *fq[aln::kSlots] = {};       // --parse-device: the slot's parser (its device buffers hold the batch until the engine has taken it) ...
	HostBuf stage[aln::kSlots];               // ... and the page-locked copy of the window it parses
	psvr_bam_emit_t *bem[aln::kSlots] = {};   // --emit-device: the slot's record encoder; the piece's records, offsets and states once downloaded (page-locked)
	HostBuf em_bytes[aln::kSlots], em_off[aln::kSlots], em_state[aln::kSlots];
	psvr_bam_emit_info_t em_info[aln::kSlots] = {};   // ... and the totals of its last run
	psvr_bam_emit_t *bem_ori[aln::kSlots] = {};   // --ori-device: the same for the second file (DriverOriSource below)
	HostBuf ori_bytes[aln::kSlots], ori_off[aln::kSlots], ori_state[aln::kSlots];
	// PSVR_PARSE_DEVICE_MAX_BYTES: the largest window that goes to the device (the tests send every window to the fallback with it)
	const size_t parse_max_window = getenv("PSVR_PARSE_DEVICE_MAX_BYTES") ? (size_t)strtoull(getenv("PSVR_PARSE_DEVICE_MAX_BYTES"), nullptr, 10) : ~(size_t)0;

	explicit EngineDriver(const std::vector<int> &dv) : devices(dv), first(dv.size()), idx(dv.size(), nullptr), eng(dv.size(), nullptr)
	{
		for (size_t d = 0; d < dv.size(); ++d) for (first[d] = 0; dv[(size_t)first[d]] != dv[d];) ++first[d];
	}
	// the first index comes from the files (or is built from the anchor FASTA), the others from it, device to device
	void load_indexes(const Opt &o, aln::RunStats *st)
	{
		const double t_idx0 = walltime();
		for (int dev : devices) (void)psvr_device_warmup(dev, 4);     // the engines' queues are set up while the index loads
		for (size_t d = 0; d < devices.size(); ++d) {
			if (first[d] != (int)d) { idx[d] = idx[(size_t)first[d]]; continue; }
			const double t0 = walltime();
			if (d == 0) {
				// <IndexDir> may also be the anchor FASTA itself: the index is then built straight into HBM (no `index` step, no files)
				struct stat sb;
				const bool is_fasta = stat(o.index_dir.c_str(), &sb) == 0 && S_ISREG(sb.st_mode);
				if (is_fasta ? psvr_index_build(o.index_dir.c_str(), o.header.c_str(), devices[0], &idx[0]) : psvr_index_load(o.index_dir.c_str(), o.header.c_str(), devices[0], &idx[0])) die("index");
				st->t_idx_first = walltime() - t0;
			}
			else { if (psvr_index_clone(idx[0], devices[d], &idx[d])) die("index clone"); st->t_idx_clone += walltime() - t0; }
		}
		st->t_index = walltime() - t_idx0;
	}
	void release()
	{
		for (auto &b : bem) if (b) psvr_bam_emit_destroy(b), b = nullptr;
		for (auto &b : bem_ori) if (b) psvr_bam_emit_destroy(b), b = nullptr;
		for (auto &f : fq) if (f) psvr_fastq_destroy(f), f = nullptr;
		for (psvr_engine_t *e : eng) if (e) psvr_engine_destroy(e);
		for (size_t d = 0; d < idx.size(); ++d) if (first[d] == (int)d) psvr_index_destroy(idx[d]);
	}

	const char *last_error() { return psvr_last_error(); }
	int create(const psvr_aln_params_t &par, int64_t pos[3])
	{
		for (size_t d = 0; d < eng.size(); ++d) if (int rc = psvr_engine_create(idx[d], &par, &eng[d])) return rc;
		return psvr_engine_stream_end(eng[0], pos);
	}
	int load(int d, const int64_t pos[3], const FastqBatch &fb, long long lo, long long n)
	{
		if (int rc = psvr_engine_set_stream_pos(eng[(size_t)d], pos)) return rc;
		return fb.dev ? psvr_engine_upload_fastq(eng[(size_t)d], fb.dev, lo, n) : psvr_engine_upload(eng[(size_t)d], n, fb.bases, fb.base_off + 2 * lo, fb.ori + 2 * lo);
	}
	int run(int d, bool trace) { return psvr_engine_run(eng[(size_t)d], trace ? 1 : 0, nullptr); }
	int stream_end(int d, int64_t end[3]) { return psvr_engine_stream_end(eng[(size_t)d], end); }
	int rebase(int d, const int64_t pos[3]) { return psvr_engine_rebase(eng[(size_t)d], pos, nullptr); }
	static int sizes_only(int rc) { return rc == PSVR_ERR_OVERFLOW ? 0 : rc; }   // a download call that is given no room answers with the sizes: that was the question
	int download(int d, aln::Block &bk, bool full, long long *bytes)
	{
		psvr_engine_t *e = eng[(size_t)d];
		const long long n = bk.hi - bk.lo;
		int64_t nc = 0, nw = 0, used = 0;
		int rc = sizes_only(psvr_engine_download_compact(e, nullptr, nullptr, nullptr, 0, &nc, nullptr, 0, &nw));
		psvr_read_hdr_t *hdr = (psvr_read_hdr_t *)bk.hdr_buf.reserve((size_t)(2 * n + 1) * sizeof(psvr_read_hdr_t));
		psvr_pair_result_t *prs = (psvr_pair_result_t *)bk.pair_buf.reserve((size_t)(n + 1) * sizeof(psvr_pair_result_t));
		psvr_cand_t *cands = (psvr_cand_t *)bk.cand_buf.reserve((size_t)(nc + 1) * sizeof(psvr_cand_t));
		uint32_t *cig = (uint32_t *)bk.cig_buf.reserve((size_t)(nw + 1) * 4);
		if (!rc) rc = psvr_engine_download_compact(e, hdr, prs, cands, nc + 1, &nc, cig, nw + 1, &nw);
		bk.V.hdr = hdr, bk.V.pairs = prs, bk.V.cands = cands, bk.V.cig = cig, bk.V.pair0 = bk.lo;
		if (!rc && full) rc = sizes_only(psvr_engine_download(e, nullptr, nullptr, nullptr, 0, &used));
		if (!rc && full) {
			bk.full.resize((size_t)(2 * n)), bk.full_cig.resize((size_t)used + 1);
			rc = psvr_engine_download(e, bk.full.data(), nullptr, bk.full_cig.data(), used + 1, &used);
		}
		*bytes = (long long)(2 * n * sizeof(psvr_read_hdr_t) + n * sizeof(psvr_pair_result_t) + nc * sizeof(psvr_cand_t) + nw * 4);
		return rc;
	}
	bool hbm_used(size_t *out)         // HBM in use on the first device, from the engine's own statistics
	{
		char sb[8192];
		const char *q = psvr_engine_stats(eng[0], sb, sizeof sb) ? nullptr : strstr(sb, "\"hbm_used_bytes\":");
		if (q) *out = strtoull(q + 17, nullptr, 10);
		return q != nullptr;
	}
	int parse_window(int slot, FastqReader &rd, FastqBatch &fb, long long pairs, long long bases, int threads, std::string *why)
	{
		const bool made = fq[slot] || !psvr_fastq_create(devices[0], &fq[slot]);
		if (rd.has_windows()) {
			// --bam-device: the text is in the signal object's memory.  Whichever side fails, the route's producer knows, and its one line
			// names the call, the reason and the pairs handed over: the pipeline goes over to the PairFeed without a line of its own
			if (!made) { rd.fail_windows(*why = std::string("fastq create: ") + psvr_last_error()); return aln::kNotAvailable; }
			const int r = rd.read_window(fb, pairs, bases, fq[slot], stage[slot], why);
			return r < 0 ? aln::kNotAvailable : r;
		}
		if (!made) { *why = psvr_last_error(); return -1; }
		return rd.read_device(fb, pairs, bases, threads, fq[slot], stage[slot], parse_max_window, why);
	}
	int emit_encode(int slot, const FastqBatch &fb, bool not_ori)
	{
		if (!bem[slot]) if (int rc = psvr_bam_emit_create(idx[0], &bem[slot])) return rc;
		return psvr_bam_emit_engine(bem[slot], eng[0], fb.dev, not_ori ? PSVR_EMIT_NOT_ORI : 0, &em_info[slot]);
	}
	// an emitter's piece into page-locked memory, in two steps: offsets and states (they say how many bytes), then the bytes
	static int emitter_view(psvr_bam_emit_t *em, long long P, HostBuf &ho, HostBuf &hs, aln::EmitView *v)
	{
		int64_t *off = (int64_t *)ho.reserve((size_t)(P + 1) * 8);
		uint8_t *stt = (uint8_t *)hs.reserve((size_t)P + 1);
		v->bytes = nullptr, v->off = off, v->state = stt;
		return psvr_bam_emit_download(em, nullptr, 0, off, stt);
	}
	static int emitter_bytes(psvr_bam_emit_t *em, long long P, HostBuf &hb, aln::EmitView *v)
	{
		uint8_t *bytes = (uint8_t *)hb.reserve((size_t)v->off[P] + 1);
		v->bytes = bytes;
		return psvr_bam_emit_download(em, bytes, v->off[P], nullptr, nullptr);
	}
	static int emitter_download(psvr_bam_emit_t *em, long long P, HostBuf &hb, HostBuf &ho, HostBuf &hs, aln::EmitView *v)
	{
		if (int rc = emitter_view(em, P, ho, hs, v)) return rc;
		return emitter_bytes(em, P, hb, v);
	}
	int emit_download(int slot, long long P, aln::EmitView *v) { return emitter_download(bem[slot], P, em_bytes[slot], em_off[slot], em_state[slot], v); }
};

// --ori-device: the second file's encoder as the pipeline sees it: a second emitter per slot, run on the engine's results where they lie
struct DriverOriSource : aln::OriSource {
	EngineDriver &drv;
	explicit DriverOriSource(EngineDriver &d) : drv(d) {}
	int encode(int slot, const FastqBatch &fb, long long *declined) override
	{
		if (!drv.bem_ori[slot]) if (int rc = psvr_bam_emit_create(drv.idx[0], &drv.bem_ori[slot])) return rc;
		psvr_bam_emit_info_t info;
		const int rc = psvr_bam_emit_ori_engine(drv.bem_ori[slot], drv.eng[0], fb.dev, &info);
		if (!rc) *declined = info.n_declined_pairs;
		return rc;
	}
	long long main_declined(int slot) override { return drv.em_info[slot].n_declined_pairs; }
	int download(int slot, long long P, aln::EmitView *v) override { return EngineDriver::emitter_download(drv.bem_ori[slot], P, drv.ori_bytes[slot], drv.ori_off[slot], drv.ori_state[slot], v); }
	int fetch_text(FastqBatch &fb) override { return FastqReader::fetch_window_text(fb); }
	const char *last_error() override { return psvr_last_error(); }
};

// The backends of the device routes (bgzf_stream_sink.h, sort_store_sink.h, sorted_bam.h's store writer, bam_sort.h and signal_device_route.h
// say what each asks), in one vocabulary: every call is named once and shared by inheritance.
// what every backend says of the library and of page-locked memory
struct HostCalls {
	const char *last_error() { return psvr_last_error(); }
	void *host_alloc(size_t n) { return psvr_host_alloc(n); }
	void host_free(void *p) { psvr_host_free(p); }
};
// what both sinks' backends ask of the pipeline slots' emitters (EngineDriver::bem[]): emitter_download's two steps, apart
struct EmitterAccess {
	EngineDriver &drv;
	long long view_pairs[aln::kSlots] = {};    // pairs of the piece emit_view last looked at, per slot
	aln::EmitView view[aln::kSlots];
	explicit EmitterAccess(EngineDriver &d) : drv(d) {}
	int emit_view(int slot, int64_t P, const int64_t **off, const uint8_t **state)
	{
		const int rc = EngineDriver::emitter_view(drv.bem[slot], P, drv.em_off[slot], drv.em_state[slot], &view[slot]);
		view_pairs[slot] = P, *off = view[slot].off, *state = view[slot].state;
		return rc;
	}
	int emit_fetch(int slot, int64_t p0, int64_t p1, std::vector<uint8_t> *out)   // (the failure path: the whole piece comes down for one range of it)
	{
		const aln::EmitView &v = view[slot];
		if (int rc = EngineDriver::emitter_bytes(drv.bem[slot], view_pairs[slot], drv.em_bytes[slot], &view[slot])) return rc;
		out->assign(v.bytes + v.off[p0], v.bytes + v.off[p1]);
		return 0;
	}
};
// --deflate-effort: the members call at one effort, in the shape the writers take their compressor in (BgzfMembersFn, bam_writer.h)
template <int EFFORT> static int members_at_effort(int device, const void *in, int64_t n, int32_t mb, void *out, int64_t cap, int64_t *got, int64_t *off, int64_t off_cap, int64_t *nm)
{
	return psvr_bgzf_compress_members_effort(device, in, n, mb, out, cap, got, off, off_cap, nm, EFFORT);
}
static psvr::BgzfMembersFn members_fn(int effort)
{
	static const psvr::BgzfMembersFn at[4] = {&psvr_bgzf_compress_members, &members_at_effort<1>, &members_at_effort<2>, &members_at_effort<3>};
	return at[effort];
}
// a device stream at the command's effort
static int stream_create_at(int device, int effort, psvr_bgzf_stream_t **s)
{
	if (int rc = psvr_bgzf_stream_create(device, (int32_t)kBgzfBlock, s)) return rc;
	return effort ? psvr_bgzf_stream_set_effort(*s, effort) : 0;
}
// the device BGZF stream at the command's effort
struct StreamCalls : HostCalls {
	const int device, effort;
	psvr_bgzf_stream_t *s = nullptr;
	explicit StreamCalls(int dev, int eff = 0) : device(dev), effort(eff) {}
	int stream_create() { return stream_create_at(device, effort, &s); }
	void stream_destroy() { if (s) psvr_bgzf_stream_destroy(s), s = nullptr; }
	int stream_append(const void *p, int64_t n) { return psvr_bgzf_stream_append(s, p, n); }
	int64_t bound(int64_t n) { return psvr_bgzf_members_bound(n, (int32_t)kBgzfBlock); }
	int take(int finish, void *out, int64_t cap, int64_t *got, int64_t *member_off, int64_t member_cap, int64_t *nm, int64_t *used)
	{
		return psvr_bgzf_stream_take(s, finish, out, cap, got, member_off, member_cap, nm, used);
	}
};
// a record store filled from a BAM file's own members
struct StoreFill {
	const int store_device;
	psvr_bam_store_t *store = nullptr;
	explicit StoreFill(int dev) : store_device(dev) {}
	int store_create() { return psvr_bam_store_create(store_device, &store); }
	void store_destroy() { if (store) psvr_bam_store_destroy(store), store = nullptr; }
	int store_append_bgzf(const void *p, int64_t n, int64_t skip, int32_t n_ref, int64_t *used, int64_t *bad) { return psvr_bam_store_append_bgzf(store, p, n, skip, n_ref, used, bad); }
	int store_chain_info(psvr_bam_chain_info_t *i) { return psvr_bam_store_chain_info(store, i); }
};
// --stream-device: bgzf_stream_sink.h's backend
struct StreamBackend : EmitterAccess, StreamCalls {
	StreamBackend(EngineDriver &d, int dev, int eff = 0) : EmitterAccess(d), StreamCalls(dev, eff) {}
	int stream_append_emit(int slot, int64_t first, int64_t n) { return psvr_bgzf_stream_append_emit(s, drv.bem[slot], first, n); }
	int64_t stream_pending() { return psvr_bgzf_stream_pending(s); }
	int stream_recover(void *bytes, int64_t cap, int64_t *n) { return psvr_bgzf_stream_recover(s, bytes, cap, n); }
	void host_route(BgzfWriter &w) { w.set_device_members(device, members_fn(effort), psvr::kDeflateDeviceBlocks); }
};
// `panSVR sort --sort-device` (bam_sort.h: sort_device_route): the store filled from the file's own members, ordered and written through the stream
struct SortCmdBackend : StoreFill, StreamCalls {
	explicit SortCmdBackend(int dev, int eff = 0) : StoreFill(dev), StreamCalls(dev, eff) {}
	int store_append(const void *p, int64_t n) { return psvr_bam_store_append(store, p, n); }
	int store_info(int64_t *n_records, int64_t *n_bytes)
	{
		psvr_bam_store_info_t i;
		if (int rc = psvr_bam_store_info(store, &i)) return rc;
		*n_records = i.n_records, *n_bytes = i.n_bytes;
		return 0;
	}
	int store_order() { return psvr_bam_store_order(store); }
	int store_order_names() { return psvr_bam_store_order_names(store); }
	int store_meta(int64_t first, int64_t n, psvr_bam_rec_meta_t *m) { return psvr_bam_store_meta(store, first, n, m); }
	int store_stream(int64_t first, int64_t n) { return psvr_bam_store_stream(store, s, first, n); }
	int store_download(void *bytes, int64_t cap, int64_t *n) { return psvr_bam_store_download(store, bytes, cap, n); }
};
// --sort-device: sort_store_sink.h's backend: the same store and stream, filled from the pipeline slots' emitters
struct SortBackend : EmitterAccess, SortCmdBackend {
	SortBackend(EngineDriver &d, int dev, int eff = 0) : EmitterAccess(d), SortCmdBackend(dev, eff) {}
	int store_append_emit(int slot, int64_t first, int64_t n) { return psvr_bam_store_append_emit(store, drv.bem[slot], first, n); }
};
// `panSVR signal -N --signal-device` (signal_device_route.h): the store filled from the file's own members, and psvr_signal_* over it
struct SignalCmdBackend : StoreFill, HostCalls {
	psvr_signal_t *sg = nullptr;
	explicit SignalCmdBackend(int dev) : StoreFill(dev) {}
	int store_drop(int64_t n) { return psvr_bam_store_drop(store, n); }
	int store_footprint(int64_t *chunks, int64_t *bytes) { return psvr_bam_store_footprint(store, chunks, bytes); }
	int signal_create(const psvr_signal_opt_t *o) { return psvr_signal_create(store_device, o, &sg); }   // (beside the store)
	void signal_destroy() { if (sg) psvr_signal_destroy(sg), sg = nullptr; }
	int signal_run(int64_t first, int finish, psvr_signal_info_t *i) { return psvr_signal_run(sg, store, first, finish, i); }
	int signal_text(void *t, int64_t cap) { return psvr_signal_text(sg, t, cap); }
	int signal_pairs(psvr_signal_pair_t *t, int64_t cap) { return psvr_signal_pairs(sg, t, cap); }
	int signal_side(void *b, int64_t cap) { return psvr_signal_side(sg, b, cap); }
	int signal_stats(uint64_t *isize_n, uint64_t *len_n) { return psvr_signal_stats(sg, isize_n, len_n); }
	// --mate-device
	int signal_run_pos(int64_t first, int finish, const psvr_signal_pos_opt_t *o, psvr_signal_info_t *i, psvr_signal_pos_info_t *pi) { return psvr_signal_run_pos(sg, store, first, finish, o, i, pi); }
	int signal_mate_notes(psvr_signal_mate_note_t *t, int64_t cap) { return psvr_signal_mate_notes(sg, t, cap); }
	int signal_run_left(int64_t first, int64_t max_pairs, psvr_signal_info_t *i, psvr_signal_left_info_t *li) { return psvr_signal_run_left(sg, first, max_pairs, i, li); }
	int signal_left_errors(int64_t *e, int64_t cap) { return psvr_signal_left_errors(sg, e, cap); }
	int signal_window(const void *t, int64_t n, const int64_t *off, int64_t n_host, psvr_signal_window_info_t *i) { return psvr_signal_window(sg, t, n, off, n_host, i); }
	int signal_window_add(const void *t, int64_t n, const int64_t *off, int64_t n_host, int32_t restart, psvr_signal_window_info_t *i) { return psvr_signal_window_add(sg, t, n, off, n_host, restart, i); }
};
// either sink as the pipeline sees it; option: the one that put it there
template <class Sink> struct DeviceMainSink : aln::MainSink {
	Sink &k;
	const char *const opt;
	DeviceMainSink(Sink &sink, const char *option) : k(sink), opt(option) {}
	bool on() const override { return k.on(); }
	int piece_view(int slot, long long P, aln::EmitView *v) override { v->bytes = nullptr; return k.emit_view(slot, P, &v->off, &v->state); }
	const char *last_error() override { return k.last_error(); }
	bool device_chunks(int slot, long long p0, long long p1, long long n_bytes) override { return k.device_chunks(slot, p0, p1, n_bytes); }
	bool host_chunk(const uint8_t *p, size_t n) override { return k.host_chunk(p, n); }
	bool piece_done() override { return k.piece_done(); }
	const char *option() const override { return opt; }
};

// what an option combination is refused with (true: a message went out); sort_conflict: the first option on the line that --sort cannot go with
static bool option_conflict(const Opt &o, const char *sort_conflict)
{
	if (o.deflate_effort_given && (o.deflate_effort < 0 || o.deflate_effort > 3))
		fprintf(stderr, "--deflate-effort wants 0 .. 3\n");
	else if (o.deflate_effort_given && !o.deflate_device)
		fprintf(stderr, "--deflate-effort cannot be given without --deflate-device, --stream-device or --sort-device: it is the effort of the GPU's BGZF encoder (a wavefront per member), which only those routes use\n");
	else if (o.sort_device && o.stream_device)
		fprintf(stderr, "--sort-device cannot be combined with --stream-device: the stream compresses the main file's records in input order as they leave the encoder, a sorted file needs all of them first\n");
	else if (o.sort_device && sort_conflict)
		fprintf(stderr, "--sort-device cannot be combined with %s: the sorted file is BAM, its members compressed on the GPU from records that stay in its memory\n", sort_conflict);
	else if (o.sort_device && o.devices.size() > 1)
		fprintf(stderr, "--sort-device cannot be combined with more than one entry in --devices: the records are encoded, kept, ordered and compressed inside the first device's memory\n");
	else if (o.stream_device && o.sort)
		fprintf(stderr, "--stream-device cannot be combined with --sort: the stream compresses the main file's records in input order as they leave the encoder, a sorted file needs all of them first\n");
	else if (o.stream_device && o.sam)
		fprintf(stderr, "--stream-device cannot be combined with -S: it hands BAM records from the device's encoder to the device's BGZF compressor, SAM text is formatted and written on the host threads\n");
	else if (o.stream_device && sort_conflict)
		fprintf(stderr, "--stream-device cannot be combined with %s: it implies --deflate-device, a compression route of its own for BAM output (a wavefront per BGZF member on the GPU)\n", sort_conflict);
	else if (o.stream_device && o.devices.size() > 1)
		fprintf(stderr, "--stream-device cannot be combined with more than one entry in --devices: the records go from the encoder to the compressor inside the first device's memory\n");
	else if (o.sort && sort_conflict)
		fprintf(stderr, "--sort cannot be combined with %s: the sorted file is BAM compressed as `panSVR sort` compresses it\n", sort_conflict);
	else if (o.deflate_device && sort_conflict)
		fprintf(stderr, "--deflate-device cannot be combined with %s: it is a compression route of its own for BAM output (a wavefront per BGZF member on the GPU)\n", sort_conflict);
	else if (o.ori_device && o.devices.size() > 1)
		fprintf(stderr, "--ori-device cannot be combined with more than one entry in --devices: the second file's records are encoded from the text and the results in the first device's memory\n");
	else if (o.ori_device && o.sam)
		fprintf(stderr, "--ori-device cannot be combined with -S: the device encodes BAM records, SAM text is formatted on the host threads\n");
	else if (o.emit_device && o.devices.size() > 1)
		fprintf(stderr, "--emit-device cannot be combined with more than one entry in --devices: the records are encoded from the text and the results in the first device's memory\n");
	else if (o.emit_device && o.sam)
		fprintf(stderr, "--emit-device cannot be combined with -S: the device encodes BAM records, SAM text is formatted on the host threads\n");
	else if (o.bam_device && o.devices.size() > 1)
		fprintf(stderr, "--bam-device cannot be combined with more than one entry in --devices: the text is made and parsed in the first device's memory\n");
	else if (o.mate_device && o.devices.size() > 1)
		fprintf(stderr, "--mate-device cannot be combined with more than one entry in --devices: the text is made and parsed in the first device's memory\n");
	else if (o.parse_device && o.devices.size() > 1)
		fprintf(stderr, "--parse-device cannot be combined with more than one entry in --devices: the parsed bases stay in the first device's memory and would have to travel between devices\n");
	else return false;
	return true;
}

// -1: go on; otherwise the command's exit status
static int parse_aln_options(int argc, char **argv, Opt *op)
{
	Opt &o = *op;
	static struct option lo[] = {{"thread", 1, 0, 't'}, {"gap-open1", 1, 0, 'O'}, {"gap-open2", 1, 0, 'P'}, {"gap-extension1", 1, 0, 'E'}, {"gap-extension2", 1, 0, 'F'},
	                             {"match-score", 1, 0, 'M'}, {"mis-score", 1, 0, 'm'}, {"zdrop", 1, 0, 'z'}, {"band-width", 1, 0, 'w'}, {"output", 1, 0, 'o'},
	                             {"output_signal_ori", 1, 0, 'p'}, {"not-ori", 0, 0, 'Q'}, {"SAM", 0, 0, 'S'}, {"max_use_read", 1, 0, 'R'}, {"device", 1, 0, 1000},
	                             {"records", 1, 0, 1001}, {"trace", 0, 0, 1002}, {"batch", 1, 0, 1003}, {"devices", 1, 0, 1004}, {"batch-bases", 1, 0, 1005}, {"compress-level", 1, 0, 1006}, {"sub-batch", 1, 0, 1007}, {"bgzf-device", 0, 0, 1008}, {"bgzf-fast", 0, 0, 1009}, {"sort", 0, 0, 1010}, {"inflate-device", 0, 0, 1011}, {"inflate-threads", 1, 0, 1012}, {"deflate-device", 0, 0, 1013}, {"parse-device", 0, 0, 1014}, {"emit-device", 0, 0, 1015}, {"stream-device", 0, 0, 1016}, {"sort-device", 0, 0, 1017}, {"signal-device", 0, 0, 1018}, {"bam-device", 0, 0, 1019}, {"mate-device", 0, 0, 1020}, {"block-records", 1, 0, 1021}, {"deflate-effort", 1, 0, 1022}, {"ori-device", 0, 0, 1023},
	                             {"not-use-filter", 0, 0, 'D'}, {"discard-full-match", 0, 0, 'U'}, {"sort-by-name", 0, 0, 'N'}, {0, 0, 0, 0}};
	int c;
	const char *sort_conflict = nullptr;               // the first option that --sort cannot go with
	optind = 2;
	while ((c = getopt_long(argc, argv, "t:O:P:E:F:M:m:z:w:o:p:QSR:DUN", lo, NULL)) >= 0) {
		switch (c) {
		case 't': o.thread_n = atoi(optarg); break;
		case 'O': o.gap_open = atoi(optarg); break;
		case 'P': o.gap_open2 = atoi(optarg); break;
		case 'E': o.gap_ex = atoi(optarg); break;
		case 'F': o.gap_ex2 = atoi(optarg); break;
		case 'M': o.match = atoi(optarg); break;
		case 'm': o.mismatch = atoi(optarg); break;
		case 'z': o.zdrop = atoi(optarg); break;
		case 'w': o.bw = atoi(optarg); break;
		case 'o': o.out = optarg; break;
		case 'p': o.out_ori = optarg; break;
		case 'Q': o.not_ori = true; break;
		case 'S': o.sam = true; if (!sort_conflict) sort_conflict = "-S"; break;
		case 'R': o.max_use_read = atoll(optarg); break;
		case 1000: o.devices = {atoi(optarg)}; break;
		case 1001: o.records = optarg; break;
		case 1002: o.trace = true; break;
		case 1003: o.batch_pairs = atoll(optarg); break;
		case 1004: if (!parse_devices(optarg, &o.devices)) { fprintf(stderr, "bad --devices list '%s'\n", optarg); return 1; } break;
		case 1005: o.batch_bases = atoll(optarg); break;
		case 1007: o.sub_pairs = atoll(optarg); break;
		case 1008: o.bgzf_device = true; if (!sort_conflict) sort_conflict = "--bgzf-device"; break;
		case 1009: o.bam_level = psvr::BgzfWriter::kLevelFast; if (!sort_conflict) sort_conflict = "--bgzf-fast"; break;
		case 1006: o.bam_level = atoi(optarg); if (o.bam_level < -1 || o.bam_level > 9) { fprintf(stderr, "--compress-level wants -1 .. 9\n"); return 1; } if (!sort_conflict) sort_conflict = "--compress-level"; break;
		case 1010: o.sort = true; break;
		case 1011: o.inflate_device = true; break;
		case 1013: o.deflate_device = true; break;
		case 1014: o.parse_device = true; break;
		case 1015: o.emit_device = o.parse_device = true; break;
		case 1023: o.ori_device = o.emit_device = o.parse_device = true; break;
		case 1017: o.sort_device = o.sort = o.emit_device = o.parse_device = o.deflate_device = true; break;
		case 1016: o.stream_device = o.emit_device = o.parse_device = o.deflate_device = true; break;
		case 1018: fprintf(stderr, "[panSVR-amd] --signal-device is `panSVR signal -N`'s route to FASTQ text: ignored by aln (a *.bam read file hands its pairs over on the host threads)\n"); break;
		case 1019: o.bam_device = true; break;
		case 1020: o.mate_device = true; break;
		case 1021: o.block_records = atoi(optarg); if (o.block_records < 2) { fprintf(stderr, "--block-records wants a number of at least 2\n"); return 1; } break;
		case 1022: o.deflate_effort = psvr::parse_deflate_effort(optarg), o.deflate_effort_given = true; break;
		case 1012: o.inflate_threads = atoi(optarg); if (o.inflate_threads < 1) { fprintf(stderr, "--inflate-threads wants a positive number\n"); return 1; } break;
		case 'D': o.sig_all = true; break;
		case 'U': o.sig_discard = true; break;
		case 'N': o.sig_by_name = true; break;
		default: return usage();
		}
	}
	if (option_conflict(o, sort_conflict)) return 1;
	if (argc - optind < 3) return usage();
	if (!(o.thread_n >= 1 && o.thread_n <= 48)) { fprintf(stderr, "Input error: thread_n cannot be less than 1 or more than 48\n"); abort(); }   // xassert, rr.hpp:121
	if (o.batch_pairs < 1) o.batch_pairs = 1;
	o.index_dir = argv[optind], o.reads = argv[optind + 1], o.header = argv[optind + 2];
	o.from_bam = o.reads.size() > 4 && o.reads.compare(o.reads.size() - 4, 4, ".bam") == 0;
	if (!o.from_bam && (o.inflate_device || o.inflate_threads > 0)) fprintf(stderr, "[panSVR-amd] --inflate-device / --inflate-threads apply to a *.bam read file: ignored for [%s]\n", o.reads.c_str());
	if (o.bam_device && !o.from_bam) fprintf(stderr, "[panSVR-amd] --bam-device applies to a *.bam read file: ignored for [%s]\n", o.reads.c_str()), o.bam_device = false;
	if (o.bam_device && !o.sig_by_name) fprintf(stderr, "[panSVR-amd] aln --bam-device: refused (it is the name-sorted mode's route: give -N): the host fused route runs\n"), o.bam_device = false;
	if (o.mate_device && !o.from_bam) fprintf(stderr, "[panSVR-amd] --mate-device applies to a *.bam read file: ignored for [%s]\n", o.reads.c_str()), o.mate_device = false;
	if (o.mate_device && o.sig_by_name) fprintf(stderr, "[panSVR-amd] aln --mate-device: refused (it is the position-sorted mode's route: -N has --bam-device): the host fused route runs\n"), o.mate_device = false;
	if (o.bam_device || o.mate_device) { o.parse_device = true; return -1; }   // (the device stages behind the reader apply to the BAM input)
	if (o.from_bam && o.parse_device) fprintf(stderr, "[panSVR-amd] --parse-device applies to FASTQ text: ignored for [%s] (a *.bam read file hands its pairs over without text)\n", o.reads.c_str());
	if (o.from_bam && o.sort_device) fprintf(stderr, "[panSVR-amd] --sort-device applies to FASTQ text: ignored for [%s] (the records of a *.bam read file are formatted on the host threads; the run is that of --sort --deflate-device)\n", o.reads.c_str());
	else if (o.from_bam && o.stream_device) fprintf(stderr, "[panSVR-amd] --stream-device applies to FASTQ text: ignored for [%s] (the records of a *.bam read file are formatted on the host threads; the files are compressed as with --deflate-device)\n", o.reads.c_str());
	else if (o.from_bam && o.emit_device) fprintf(stderr, "[panSVR-amd] --emit-device applies to FASTQ text: ignored for [%s] (the records of a *.bam read file are formatted on the host threads)\n", o.reads.c_str());
	if (o.from_bam && o.ori_device) fprintf(stderr, "[panSVR-amd] --ori-device applies to FASTQ text: ignored for [%s] (the second file's records of a *.bam read file are formatted on the host threads)\n", o.reads.c_str());
	return -1;
}

// <reads> may be a BAM (*.bam): the signal step then runs in this process (options of fc_signal: -N for name-sorted input,
// position-sorted otherwise) and hands its pairs to the reader stage; <header.sam> is WRITTEN from the BAM's header
static void load_header(const Opt &o, HeaderInfo *H, std::vector<BamRef> *refs)
{
	if (o.from_bam) {
		psvr::BamReader rd;
		if (!rd.open(o.reads.c_str())) { fprintf(stderr, "[panSVR-amd] %s\n", rd.error().c_str()); abort(); }
		FILE *h = fopen(o.header.c_str(), "w");
		if (!h) { fprintf(stderr, "fail to open file '%s'\n", o.header.c_str()); abort(); }
		fwrite(rd.header_text.data(), 1, rd.header_text.size(), h);
		fclose(h);
	}
	fprintf(stderr, "Open original header file [%s]\n", o.header.c_str());
	if (!H->load(o.header)) { fprintf(stderr, "fail to open file '%s'\n", o.header.c_str()); abort(); }
	for (size_t i = 0; i < H->names.size(); ++i) refs->push_back({H->names[i], H->lens[i]});
}

// f2 fused: the signal step's thread hands its pairs straight to the batch being built (PairFeed, fastq_batch.h) -- no FASTQ text, no pipe
static std::thread start_signal_step(const Opt &o, psvr::SignalStep &sig, PairFeed &feed, WindowFeed *windows, int *sig_rc)
{
	sig.o.sort_by_name = o.sig_by_name, sig.o.input = o.reads, sig.o.header_fn = o.header, sig.o.status_fn = o.header + ".status";
	sig.o.not_use_filter = o.sig_all, sig.o.discard_full_match = o.sig_discard;
	sig.o.inflate_device = o.inflate_device ? o.devices[0] : -1, sig.o.inflate_threads = o.inflate_threads;
	sig.o.match = o.match, sig.o.mismatch = o.mismatch, sig.o.gap_open = o.gap_open, sig.o.gap_ex = o.gap_ex, sig.o.gap_open2 = o.gap_open2, sig.o.gap_ex2 = o.gap_ex2;
	if (o.block_records) sig.o.block_records = o.block_records;
	sig.feed = &feed;
	return psvr::signal_step_thread(sig, feed, windows, sig_rc);
}

// --bam-device, --mate-device: who takes the windows of the signal step's device route -- the reader stage, through the WindowFeed
struct ReaderWindowTaker : psvr::SignalWindowTaker {
	SignalCmdBackend &be;
	WindowFeed &windows;
	ReaderWindowTaker(SignalCmdBackend &b, WindowFeed &w) : be(b), windows(w) {}
	long long offer(const psvr_signal_window_info_t &info, std::string *why) override { return windows.offer(be.sg, info.n_pairs, why); }
};
// the fused command's device route: route(be, S, pairs_done, &taker) is signal_device_route or signal_mate_route in window mode
template <class Route> static std::function<int(psvr::SignalStep &, long long *)> window_route_fn(const Opt &o, WindowFeed &windows, Route route)
{
	return [&o, &windows, route](psvr::SignalStep &S, long long *pairs_done) {
		SignalCmdBackend be(o.devices[0]);
		ReaderWindowTaker taker(be, windows);
		const int rc = route(be, S, pairs_done, &taker);
		windows.close(rc != 0);                              // (left: the host fused route hands the rest over through the PairFeed)
		return rc;
	};
}
// `panSVR signal`'s: route(be, S, pairs_done) is one of the two with text for its consumer
template <class Route> static std::function<int(psvr::SignalStep &, long long *)> text_route_fn(Route route)
{
	return [route](psvr::SignalStep &S, long long *pairs_done) {
		SignalCmdBackend be(0);
		return route(be, S, pairs_done);
	};
}

// --sort: the main file, its records ordered on the first device, written with the index.  0, or the command's exit status
static int write_sorted_main(const Opt &o, const HeaderInfo &H, const std::vector<BamRef> &bam_refs, const SortRecords &sorted, aln::RunStats *st)
{
	const double ts = walltime();
	try {
		std::vector<uint32_t> ord;
		bool on_device = false;
		std::string err;
		if (!coordinate_order(sorted, o.devices[0], ord, &on_device, &err)) { fprintf(stderr, "[panSVR-amd] --sort: device order: %s\n", err.c_str()); return 2; }
		st->t_sort_order = walltime() - ts;
		fprintf(stderr, "[panSVR-amd] --sort: %zu records (%.1f MB) ordered %s in %.1f ms\n", sorted.size(), sorted.bytes / 1e6, on_device ? "on the device" : "on the host",
		        st->t_sort_order * 1e3);
		std::vector<std::pair<std::string, int32_t>> refs;
		for (const BamRef &r : bam_refs) refs.push_back({r.name, (int32_t)r.len});
		if (!write_sorted_bam(o.out, H.text, refs, sorted, ord, false, o.thread_n, &err, o.deflate_device ? members_fn(o.deflate_effort) : nullptr, o.devices[0], psvr::kDeflateDeviceBlocks)) { fprintf(stderr, "%s\n", err.c_str()); return 2; }
	} catch (const std::bad_alloc &) { fputs(aln::kSortNoMem, stderr); return 2; }
	st->t_sort = walltime() - ts;
	return 0;
}

static int aln_main(int argc, char **argv)
{
	Opt o;
	const int status = parse_aln_options(argc, argv, &o);
	if (status >= 0) return status;
	HeaderInfo H;
	std::vector<BamRef> refs;
	load_header(o, &H, &refs);
	aln::RunStats st;
	st.devices = (int)o.devices.size(), st.threads = o.thread_n, st.sam = o.sam, st.deflate_effort = o.deflate_effort, st.stream_fields = st.sort_fields = st.effort_field = true;
	EngineDriver drv(o.devices);
	fprintf(stderr, "Begin loading index @%s\n", o.index_dir.c_str());
	drv.load_indexes(o, &st);
	fprintf(stderr, "End loading index\n");

	fprintf(stderr, "Start classify\n");
	const double cpu0 = cputime();
	st.wall0 = walltime();
	psvr::SignalStep sig;
	std::thread sig_thread;
	int sig_rc = 0;
	PairFeed feed;
	WindowFeed windows;
	if (o.bam_device) {
		sig.o.bam_device = true;
		sig.signal_device_fn = window_route_fn(o, windows, [](SignalCmdBackend &be, psvr::SignalStep &S, long long *pairs_done, ReaderWindowTaker *taker) {
			return psvr::signal_device_route(be, S, pairs_done, nullptr, taker);
		});
	}
	if (o.mate_device) {
		sig.o.mate_fused = true;
		sig.mate_device_fn = window_route_fn(o, windows, [&o](SignalCmdBackend &be, psvr::SignalStep &S, long long *pairs_done, ReaderWindowTaker *taker) {
			// (a kept window is offered when it holds a piece's pairs: the reader cuts it by the piece rule, and few pieces end short at a window's end)
			return psvr::signal_mate_route(be, S, pairs_done, nullptr, taker, o.sub_pairs > 0 ? o.sub_pairs : o.batch_pairs);
		});
	}
	const bool device_input = o.bam_device || o.mate_device;   // the reader stage takes windows of text in HBM
	if (o.from_bam) sig_thread = start_signal_step(o, sig, feed, device_input ? &windows : nullptr, &sig_rc);
	FastqReader fq;
	if (device_input) fq.open_windows(&windows);
	if (o.from_bam) fq.open_feed(&feed);
	else if (!fq.open(o.reads.c_str())) { fprintf(stderr, "%s\n", fq.error().c_str()); abort(); }
	aln::OutFile fo, fo_ori;
	// --stream-device: the main file is the sink's, not `fo`'s (PSVR_STREAM_TAKE_MEMBERS: members pending before a take; the tests take small files in pieces with it)
	const bool device_routes = !o.from_bam || device_input;
	const bool streaming = o.stream_device && device_routes;
	std::unique_ptr<StreamBackend> stream_backend;
	std::unique_ptr<BgzfStreamSink<StreamBackend>> stream_sink;
	std::unique_ptr<aln::MainSink> main_sink;
	if (streaming) {
		stream_backend.reset(new StreamBackend(drv, o.devices[0], o.deflate_effort));
		stream_sink.reset(new BgzfStreamSink<StreamBackend>(*stream_backend, getenv("PSVR_STREAM_TAKE_MEMBERS") ? (size_t)atoll(getenv("PSVR_STREAM_TAKE_MEMBERS")) : psvr::kDeflateDeviceBlocks));
		main_sink.reset(new DeviceMainSink<BgzfStreamSink<StreamBackend>>(*stream_sink, "--stream-device"));
		if (!stream_sink->open(o.out.c_str(), H.text, refs, o.thread_n)) { fprintf(stderr, "fail to open output file\n"); abort(); }
	}
	// --sort-device: the main file's records go to the sink's store; the file is written when the input has ended
	const bool sorting_device = o.sort_device && device_routes;
	std::unique_ptr<SortBackend> sort_backend;
	std::unique_ptr<SortStoreSink<SortBackend>> sort_sink;
	if (sorting_device) {
		sort_backend.reset(new SortBackend(drv, o.devices[0], o.deflate_effort));
		sort_sink.reset(new SortStoreSink<SortBackend>(*sort_backend, [&](const SortRecords &R) { return write_sorted_main(o, H, refs, R, &st); },
		                                               getenv("PSVR_STREAM_TAKE_MEMBERS") ? (size_t)atoll(getenv("PSVR_STREAM_TAKE_MEMBERS")) : psvr::kDeflateDeviceBlocks));
		main_sink.reset(new DeviceMainSink<SortStoreSink<SortBackend>>(*sort_sink, "--sort-device"));
		sort_sink->open(o.out.c_str(), H.text, refs);
	}
	if ((!o.sort && !streaming && !fo.open(o.out, !o.sam, H, refs, o.thread_n, o.bam_level)) || !fo_ori.open(o.out_ori, !o.sam, H, refs, o.thread_n, o.bam_level)) { fprintf(stderr, "fail to open output file\n"); abort(); }
	SortRecords sorted;                                  // --sort: the main file's records, kept until the input ends
	if (o.bgzf_device && !o.sam) fo.bam.bgzf().set_device(o.devices[0]), fo_ori.bam.bgzf().set_device(o.devices[0]);
	if (o.deflate_device && !streaming) fo.bam.bgzf().set_device_members(o.devices[0], members_fn(o.deflate_effort), psvr::kDeflateDeviceBlocks);
	if (o.deflate_device) fo_ori.bam.bgzf().set_device_members(o.devices[0], members_fn(o.deflate_effort), psvr::kDeflateDeviceBlocks);
	FILE *frec = o.records.empty() ? nullptr : fopen(o.records.c_str(), "w");
	fprintf(stderr, "Processing file: [%s].\n", o.reads.c_str());

	psvr_aln_params_t par;
	psvr_aln_params_default(&par);
	par.match = o.match, par.mismatch = o.mismatch, par.gap_open = o.gap_open, par.gap_ex = o.gap_ex, par.gap_open2 = o.gap_open2, par.gap_ex2 = o.gap_ex2, par.zdrop = o.zdrop;
	IndexSvNames svn;
	svn.idx = drv.idx[0];
	SamEmitter em;
	em.H = &H, em.sv = &svn, em.as_bam = !o.sam, em.not_ori = o.not_ori, em.stats = &st.emit;
	std::function<bool(const uint8_t *, size_t)> keep_main;
	if (o.sort) keep_main = [&sorted](const uint8_t *p, size_t n) { return sorted.add_stream(p, n); };
	DriverOriSource ori_source(drv);                     // --ori-device: the second file's records from the device; the window routes then leave a piece's text there until it is asked for
	if (o.ori_device && device_routes) fq.set_lazy_window_text(true);
	st.ori_fields = o.ori_device;
	aln::AlnPipeline<EngineDriver> pipe(o, drv, fq, par, em, fo, fo_ori, keep_main, frec, st, device_routes, main_sink.get(), o.ori_device && device_routes ? &ori_source : nullptr);
	pipe.run();
	windows.abort();
	feed.abort();                                        // (a reader that stopped at -R leaves the signal step to run to its end unheard)
	if (sig_thread.joinable()) {
		sig_thread.join();
		if (sig_rc) { fprintf(stderr, "[panSVR-amd] the signal step failed\n"); abort(); }
	}
	if (streaming) {
		const double tc = walltime();
		if (!stream_sink->close()) { fprintf(stderr, "[panSVR-amd] --stream-device: fail to write output file: the main file [%s] is incomplete, and the ori file [%s] was not closed and is incomplete too\n", o.out.c_str(), o.out_ori.c_str()); return 2; }
		st.t_write += walltime() - tc;
		const StreamSinkStats &ss = stream_sink->st;
		st.streamer = ss.device_chunks == 0 ? "host" : ss.host_chunks || ss.left ? "device+host" : "device";
		st.stream_device_bytes = ss.device_bytes, st.stream_host_bytes = ss.host_bytes, st.stream_members = ss.members;
	}
	if ((!o.sort && !streaming && !fo.close()) || !fo_ori.close()) { fprintf(stderr, "fail to write output file\n"); abort(); }
	if (sorting_device) {
		const double ts = walltime();
		const int rc = sort_sink->finish();
		const SortSinkStats &ss = sort_sink->st;
		if (rc) { if (!sort_sink->ok()) fprintf(stderr, "[panSVR-amd] --sort-device: the main file [%s] was not written\n", o.out.c_str()); return rc; }
		if (!ss.left) {
			st.t_sort_order = ss.t_order;
			fprintf(stderr, "[panSVR-amd] --sort-device: %lld records (%.1f MB) ordered on the device in %.1f ms, %lld members\n", ss.records, (ss.device_bytes + ss.host_bytes) / 1e6, ss.t_order * 1e3, ss.members);
		}
		st.t_sort = walltime() - ts;
		st.sorter = sort_sink->sorter();
		st.sort_device_bytes = ss.device_bytes, st.sort_host_bytes = ss.host_bytes, st.sort_records = ss.records, st.sort_members = ss.members;
	} else if (o.sort) if (const int rc = write_sorted_main(o, H, refs, sorted, &st)) return rc;
	if (frec) fclose(frec);
	st.wall = walltime() - st.wall0;                     // first FASTQ byte to the files closed; giving the HBM back is reported beside it, like the index load
	drv.release();
	st.t_teardown = walltime() - st.wall0 - st.wall;
	st.print(cputime() - cpu0);
	return 0;
}

int main(int argc, char **argv)
{
	if (argc >= 2 && !strcmp(argv[1], "index")) return index_main(argc, argv);
	if (argc >= 2 && (!strcmp(argv[1], "signal") || !strcmp(argv[1], "fc_signal"))) return psvr::signal_main(argc, argv,
			text_route_fn([](SignalCmdBackend &be, psvr::SignalStep &S, long long *pairs_done) { return psvr::signal_device_route(be, S, pairs_done); }),
			text_route_fn([](SignalCmdBackend &be, psvr::SignalStep &S, long long *pairs_done) { return psvr::signal_mate_route(be, S, pairs_done); }));
	if (argc >= 2 && !strcmp(argv[1], "sort"))
		return psvr::bam_sort_main(argc, argv, &psvr_bgzf_compress_members, [](const std::string &in, const std::string &out, bool by_name, int effort) {
			SortCmdBackend be(0, effort);
			return psvr::sort_device_route(be, in, out, by_name);
		}, &members_fn);
	if (argc >= 2 && (!strcmp(argv[1], "aln") || !strcmp(argv[1], "fc_aln"))) return aln_main(argc, argv);
	fprintf(stderr, "panSVR (MI355X engine): the read re-alignment step and its two neighbours.\n  usage: panSVR aln|fc_aln [options] <IndexDir> <reads.fq|-> <header.sam>\n         panSVR index [-k 22] <anchors.fa> <IndexDir>\n         panSVR signal [-N] [options] <in.bam> > reads.fq\n         panSVR sort [-n] [-t threads] [-o out.bam] in.bam      (coordinate order + .bai, or -n name order)\n         panSVR sort --sort-device [-t threads] [-o out.bam] in.bam      (the same files, the records inflated, kept, ordered and compressed in GPU memory)\n         panSVR sort --nsort-device [-t threads] [-o out.bam] in.bam     (name order by the same route: the file of sort -n --deflate-device, no index)\n         signal, sort and aln <in.bam>: --inflate-device | --inflate-threads N  (the input's BGZF members inflated in batches)\n         aln, aln --sort and sort: --deflate-device  (the output's BGZF members compressed on the GPU, a wavefront per member)\n         aln <reads.fq>: --parse-device  (the FASTQ text parsed on the GPU, the bases handed to the engine device to device)\n         aln <reads.fq>: --emit-device   (implies --parse-device; the main BAM file's records encoded on the GPU as well)\n"
	                "         aln <reads.fq>: --ori-device    (implies --emit-device; the second file's records encoded on the GPU too, pieces both encoders took whole stay there)\n"
                "         aln <reads.fq>: --stream-device (implies --emit-device and --deflate-device; the records go from the encoder to the compressor in GPU memory)\n"
	                "         aln <reads.fq>: --sort-device   (implies --sort, --emit-device and --deflate-device; the records are kept, ordered and compressed in GPU memory)\n"
	                "         panSVR aln --sort ...    (the same coordinate-sorted BAM + .bai straight from the aln step)\n");
	return 1;
}
