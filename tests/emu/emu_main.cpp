// tests/emu/emu_main.cpp -- TEST INFRASTRUCTURE ONLY.
//
// emu_aln: the host backend for pansvr_amd/csrc/engine_core.h (CpuBE, cpu_backend.h) runs the very same stage functions
// (aln_device.h) and batch orchestration the GPU engine uses, but as plain loops on the CPU, with the
// oracle's DP (oracle/ksw_oracle.c) standing in for the HIP DP kernel.  It exists so the stage logic
// and the speculative rand()-offset loop can be checked against the golden records in `-m "not gpu"`
// tests.  It is never linked into libpsvr_engine.so.
//
// With --sam / --ori-sam it also runs the PRODUCT's host-side formatter (pansvr_amd/csrc/sam_emit.h, fastq_batch.h) over these
// results, so the SAM text can be compared with the reference's own files without a GPU.
//
// With --bam / --ori-bam (next to --sam / --ori-sam) the two files are written once more as whole BAM files through the product's
// BamWriter (header, records of the direct encoder -- or of BamWriter::encode with --bam-via-text -- and BGZF), as `panSVR aln` does.
//
// Usage: emu_aln <fixture_index_dir> <reads.fq> <header.sam> [--trace] [--batch N] [--sam FILE --ori-sam FILE [--bam FILE --ori-bam FILE]]
//                [--threads N]
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>
#include "../../pansvr_amd/csrc/engine_core.h"
#include "../../pansvr_amd/csrc/host_io.h"
#include "../../pansvr_amd/csrc/fastq_batch.h"
#include "../../pansvr_amd/csrc/sam_emit.h"
#include "../../pansvr_amd/csrc/signal_step.h"
#include <thread>
#include "cpu_backend.h"

using namespace psvr;

struct HostSvNames : SvNames {
	const HostIndex *h;
	const char *print_string(int sv) const override { return sv >= 0 && sv < (int)h->svh.size() ? h->svh[(size_t)sv].vcf_print_string.c_str() : nullptr; }
	const char *vcf_id(int sv) const override { return sv >= 0 && sv < (int)h->svh.size() ? h->svh[(size_t)sv].vcf_id.c_str() : nullptr; }
};

int main(int argc, char **argv)
{
	if (argc < 4) { fprintf(stderr, "usage: emu_aln <index_dir> <reads.fq> <header.sam> [--trace] [--batch N] [--sam FILE --ori-sam FILE]\n"); return 1; }
	bool trace = false, quiet = false, not_ori = false, sig_n = false, sig_d = false, sig_u = false;
	long long batch = 1 << 20;
	int threads = 1;
	const char *sam_fn = nullptr, *ori_fn = nullptr, *bam_fn = nullptr, *bam_out = nullptr, *bam_ori_out = nullptr;
	bool bam_text = false;
	int format_reps = 0;
	long long pos[3] = {-1, -1, -1}, from[3] = {-1, -1, -1};
	int score[7] = {0};
	bool have_score = false;
	for (int i = 4; i < argc; ++i) {
		if (!strcmp(argv[i], "--trace")) trace = true;
		else if (!strcmp(argv[i], "--no-records")) quiet = true;
		else if (!strcmp(argv[i], "-Q")) not_ori = true;            // --not-ori (read_realignment.cpp:485)
		else if (!strcmp(argv[i], "-N")) sig_n = true;
		else if (!strcmp(argv[i], "-D")) sig_d = true;
		else if (!strcmp(argv[i], "-U")) sig_u = true;
		else if (!strcmp(argv[i], "--batch") && i + 1 < argc) batch = atoll(argv[++i]);
		else if (!strcmp(argv[i], "--threads") && i + 1 < argc) threads = atoi(argv[++i]);
		else if (!strcmp(argv[i], "--sam") && i + 1 < argc) sam_fn = argv[++i];
		else if (!strcmp(argv[i], "--ori-sam") && i + 1 < argc) ori_fn = argv[++i];
		else if (!strcmp(argv[i], "--bam") && i + 1 < argc) bam_out = argv[++i];                 // both files as BAM through BamWriter (needs --sam / --ori-sam)
		else if (!strcmp(argv[i], "--ori-bam") && i + 1 < argc) bam_ori_out = argv[++i];
		else if (!strcmp(argv[i], "--bam-records") && i + 1 < argc) bam_fn = argv[++i];      // the main file's records as BAM bytes (uncompressed, no header): direct encoder
		else if (!strcmp(argv[i], "--format-reps") && i + 1 < argc) format_reps = atoi(argv[++i]);   // host stages timed on one thread: the batch formatted this many times (stderr)
		else if (!strcmp(argv[i], "--bam-via-text")) bam_text = true;                          // ... through the SAM-line strings and BamWriter::encode instead
		else if (!strcmp(argv[i], "--stream-pos") && i + 1 < argc) sscanf(argv[++i], "%lld,%lld,%lld", &pos[0], &pos[1], &pos[2]);       // start of this shard in the three draw streams
		else if (!strcmp(argv[i], "--rebase-from") && i + 1 < argc) sscanf(argv[++i], "%lld,%lld,%lld", &from[0], &from[1], &from[2]);  // run there first, then rebase to --stream-pos
		else if (!strcmp(argv[i], "--score") && i + 1 < argc) {                                // -M -m -O -E -P -F -z of the CLI, in that order
			if (sscanf(argv[++i], "%d,%d,%d,%d,%d,%d,%d", &score[0], &score[1], &score[2], &score[3], &score[4], &score[5], &score[6]) != 7) { fprintf(stderr, "--score wants M,m,O,E,P,F,z\n"); return 1; }
			have_score = true;
		}
	}
	const size_t rl = strlen(argv[2]);
	const bool from_bam = rl > 4 && !strcmp(argv[2] + rl - 4, ".bam");
	if (from_bam) {                // the header file is WRITTEN from the BAM's header, like the CLI does
		psvr::BamReader br;
		if (!br.open(argv[2])) { fprintf(stderr, "%s\n", br.error().c_str()); return 2; }
		FILE *h = fopen(argv[3], "w");
		if (!h) return 2;
		fwrite(br.header_text.data(), 1, br.header_text.size(), h);
		fclose(h);
	}
	HostIndex hi;
	hi.keep_sparse = true;       // PSVR_EMU_SPARSE_HASH build: no 2 GiB table on the CPU
	std::string err;
	if (!hi.load_dir(argv[1], argv[3], &err)) { fprintf(stderr, "%s\n", err.c_str()); return 2; }
	DevIndex ix = hi.view();       // host pointers: the CPU backend's "device" is host memory
	psvr_aln_params_t par;
	aln_params_default(&par);
	if (have_score) par.match = score[0], par.mismatch = score[1], par.gap_open = score[2], par.gap_ex = score[3], par.gap_open2 = score[4], par.gap_ex2 = score[5], par.zdrop = score[6];
	CpuBE be;
	EngineCore<CpuBE> core(be);
	FastqReader rd;
	FastqBatch fb;
	// <reads> = *.bam: the signal step in this process, its pairs handed to the batch reader without FASTQ text (PairFeed: what `panSVR aln x.bam` does)
	psvr::SignalStep sig;
	psvr::PairFeed feed;
	std::thread sig_thread;
	int sig_rc = 0;
	if (from_bam) {
		sig.o.sort_by_name = sig_n, sig.o.not_use_filter = sig_d, sig.o.discard_full_match = sig_u;
		sig.o.input = argv[2], sig.o.header_fn = argv[3], sig.o.status_fn = std::string(argv[3]) + ".status";
		sig.feed = &feed;
		sig_thread = std::thread([&]() { sig_rc = sig.run(); feed.close(); });
		rd.open_feed(&feed);
	} else if (!rd.open(argv[2])) { fprintf(stderr, "%s\n", rd.error().c_str()); return 2; }
	HeaderInfo H;
	HostSvNames svn;
	svn.h = &hi;
	SamEmitter em;
	FILE *fsam = nullptr, *fori = nullptr, *fbam = nullptr;
	if (bam_fn && !(fbam = fopen(bam_fn, "wb"))) { fprintf(stderr, "cannot open %s\n", bam_fn); return 2; }
	if (sam_fn && ori_fn) {
		if (!H.load(argv[3])) { fprintf(stderr, "cannot read %s\n", argv[3]); return 2; }
		fsam = fopen(sam_fn, "w"), fori = fopen(ori_fn, "w");
		if (!fsam || !fori) { fprintf(stderr, "cannot open the SAM outputs\n"); return 2; }
		fputs(H.text.c_str(), fsam), fputs(H.text.c_str(), fori);
		em.H = &H, em.sv = &svn, em.not_ori = not_ori;
	}
	BamWriter bw[2];
	const bool whole_bam = bam_out && bam_ori_out && fsam;
	if (whole_bam) {
		std::vector<BamRef> refs;
		for (size_t i = 0; i < H.names.size(); ++i) refs.push_back({H.names[i], H.lens[i]});
		if (!bw[0].open(bam_out, H.text, refs) || !bw[1].open(bam_ori_out, H.text, refs)) { fprintf(stderr, "cannot open the BAM outputs\n"); return 2; }
	}
	bool first = true;
	long long pair_base = 0;
	while (rd.read(fb, batch, 100000000, threads)) {
		if (first) {
			rd.stat_params(&par);
			core.init(ix, par);
			first = false;
			em.min_filter_score = par.min_filter_score;
			const long long *st = from[0] >= 0 ? from : pos;
			if (st[0] >= 0) core.grand_pos = st[0], core.hrand_pos[0] = st[1], core.hrand_pos[1] = st[2];
		}
		int rc = core.upload(fb.n_pairs(), fb.bases, fb.base_off, fb.ori);
		if (!rc) rc = core.run(trace, true);
		if (!rc && from[0] >= 0 && pos[0] >= 0) { rc = core.rebase(pos[0], pos[1], pos[2], trace, true); from[0] = -1; }
		if (rc) { fprintf(stderr, "emu error %d: %s\n", rc, core.err.c_str()); return 3; }
		for (long long p = 0; p < fb.n_pairs() && !quiet; ++p) {
			const char *t; int lens[2];
			fb.seq(2 * p, t, lens[0]), fb.seq(2 * p + 1, t, lens[1]);
			psvr_read_result_t rr[2];
			materialize_read(core.c, 2 * p, &rr[0]), materialize_read(core.c, 2 * p + 1, &rr[1]);
			puts(record_json(pair_base + p, rr, core.c.pres[p], &fb.ori[2 * p], lens, core.c.cig.base, trace).c_str());
		}
		if (fsam) {       // the engine's arrays ARE the compact form (headers + candidate list + CIGAR arena)
			ResultView V;
			V.hdr = core.c.rh, V.pairs = core.c.pres, V.cands = core.c.cand, V.cig = core.c.cig.base;
			Bytes a, b;
			if (format_reps > 0) {
				auto now = [] { return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count(); };
				for (int mode = 0; mode < 2; ++mode) {
					SamEmitter e2 = em;
					e2.as_bam = mode == 1;
					size_t bytes = 0;
					const double t0 = now();
					for (int rep = 0; rep < format_reps; ++rep) {
						a.clear(), b.clear();
						for (long long p = 0; p < fb.n_pairs(); ++p) e2.main_pair(fb, V, p, a), e2.ori_pair(fb, V, p, b);
						bytes = a.size() + b.size();
					}
					const double dt = (now() - t0) / format_reps;
					fprintf(stderr, "[emu] format (%s): %.1f ns per read, %.2f GB/s of output, %zu bytes\n", mode ? "BAM records" : "SAM text", dt * 1e9 / (2.0 * fb.n_pairs()), bytes / dt / 1e9, bytes);
				}
				a.clear(), b.clear();
			}
			for (long long p = 0; p < fb.n_pairs(); ++p) em.main_pair(fb, V, p, a), em.ori_pair(fb, V, p, b);
			fwrite(a.data(), 1, a.size(), fsam), fwrite(b.data(), 1, b.size(), fori);
			if (fbam) {
				SamEmitter eb = em;
				eb.as_bam = true, eb.bam_via_text = bam_text;
				Bytes m;
				for (long long p = 0; p < fb.n_pairs(); ++p) eb.main_pair(fb, V, p, m);
				fwrite(m.data(), 1, m.size(), fbam);
			}
			if (whole_bam) {
				SamEmitter eb = em;
				eb.as_bam = true, eb.bam_via_text = bam_text;
				Bytes m, o;
				for (long long p = 0; p < fb.n_pairs(); ++p) eb.main_pair(fb, V, p, m), eb.ori_pair(fb, V, p, o);
				bw[0].write_raw(m.data(), m.size()), bw[1].write_raw(o.data(), o.size());
			}
		}
		core.commit();
		fprintf(stderr, "[emu] stream_end %lld %lld %lld\n", core.grand_pos, core.hrand_pos[0], core.hrand_pos[1]);
		fprintf(stderr, "[emu] chain+select: %lld reads by the small case, %lld by the generic pair\n", be.n_small, be.n_generic);
		pair_base += fb.n_pairs();
		fprintf(stderr, "[emu] batch of %lld pairs: %lld rounds, %lld pair-runs (+%lld pairing-only, +%lld shadow, %lld sensitive, %lld window misses), %lld DP problems, %lld candidates\n", fb.n_pairs(), core.stats.rounds,
		        core.stats.pairs_run, core.stats.pair_only, core.stats.shadow_runs, core.stats.sensitive, core.stats.window_miss, core.stats.dp_problems, core.stats.cands);
	}
	if (fsam) fclose(fsam), fclose(fori);
	if (fbam) fclose(fbam);
	if (whole_bam && (!bw[0].close() || !bw[1].close())) { fprintf(stderr, "cannot write the BAM outputs\n"); return 2; }
	feed.abort();
	if (sig_thread.joinable()) sig_thread.join();
	if (sig_rc) { fprintf(stderr, "the signal step failed\n"); return 4; }
	return 0;
}
