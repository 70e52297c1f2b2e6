// bam_sort.h -- `panSVR sort`: what panSVR_run.sh does after the `aln` step with `samtools sort` + `samtools index`
// (panSVR_run.sh:53-54), so the drop-in does not depend on an external binary.  Host C++ only.
//   panSVR sort [-n] [-t threads] [-o out.bam] [--inflate-device | --inflate-threads N] [--deflate-device] in.bam      coordinate order (default) + out.bam.bai, or name order (-n)
// Coordinate order is samtools' (bam_sort.c bam1_lt): reference id as unsigned (unplaced records last), position, forward strand
// before reverse, ties in input order; name order compares the names with strcmp, first read before second.  The whole file is held
// in memory (the aln step's output is the signal subset of a run, not the full BAM).  The order and the writing are sorted_bam.h's, which
// `panSVR aln --sort` shares: the coordinate order is computed on the device when one is visible.
#pragma once
#include <stdint.h>
#include <stdio.h>
#include <string.h>
#include <string>
#include <vector>
#include "bam_reader.h"
#include "sorted_bam.h"

namespace psvr {

// deflate_fn: the compressor --deflate-device uses (the CLI hands in &psvr_bgzf_compress_members)
inline int bam_sort_main(int argc, char **argv, BgzfMembersFn deflate_fn = nullptr)
{
	bool by_name = false;
	int threads = 4, inflate_device = -1, inflate_threads = 0;
	bool bad_arg = false, deflate_device = false;
	std::string out_fn, in_fn;
	for (int i = 2; i < argc; ++i) {
		if (!strcmp(argv[i], "-n")) by_name = true;
		else if ((!strcmp(argv[i], "-t") || !strcmp(argv[i], "-@")) && i + 1 < argc) threads = atoi(argv[++i]);
		else if (!strcmp(argv[i], "-o") && i + 1 < argc) out_fn = argv[++i];
		else if (!strcmp(argv[i], "--inflate-device")) inflate_device = 0;
		else if (!strcmp(argv[i], "--deflate-device")) deflate_device = true;
		else if (!strcmp(argv[i], "--inflate-threads") && i + 1 < argc) { inflate_threads = atoi(argv[++i]); bad_arg |= inflate_threads < 1; }
		else in_fn = argv[i];
	}
	if (bad_arg) fprintf(stderr, "--inflate-threads wants a positive number\n");
	if (in_fn.empty() || bad_arg) {
		fprintf(stderr, "usage: panSVR sort [-n] [-t threads] [-o out.bam] [--inflate-device | --inflate-threads N] [--deflate-device] in.bam\n"
		                "         --inflate-device       inflate the input's BGZF members on the GPU (device 0), a chunk of the file at a time\n"
		                "                                (faster than the default reader; it does not win against --inflate-threads 16)\n"
		                "         --inflate-threads INT  inflate them with zlib on INT host threads (also what takes over when the device route fails)\n"
		                "         --deflate-device       compress the output's BGZF members on the GPU (device 0), a wavefront per member of 0xff00 bytes, 1024\n"
		                "                                members a call.  Measured on the 2 M records of 1 M pairs, -t 16: 2.24-2.28 s against 2.45-3.04 s by\n"
		                "                                default (reading the input is most of both), the file 23 %% larger than zlib's default level makes it;\n"
		                "                                a call of 201 MB: 14.9 ms = 13.5 GB/s with its copies, zlib's default level on 16 threads 491 ms\n");
		return 1;
	}
	if (out_fn.empty()) out_fn = in_fn + (by_name ? ".nsorted.bam" : ".sorted.bam");
	if (threads < 1) threads = 1;
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
	if (by_name) name_order(R, ord);
	else if (!coordinate_order(R, 0, ord, &on_device, &err)) { fprintf(stderr, "[panSVR-amd] sort: device order: %s\n", err.c_str()); return 2; }
	if (!write_sorted_bam(out_fn, rd.header_text, rd.refs, R, ord, by_name, threads, &err, deflate_device ? deflate_fn : nullptr, 0)) { fprintf(stderr, "%s\n", err.c_str()); return 2; }
	fprintf(stderr, "[panSVR-amd] sort: %zu records -> %s (%s order%s)\n", ord.size(), out_fn.c_str(), by_name ? "name" : "coordinate", on_device ? ", ordered on the device" : "");
	return 0;
}

} // namespace psvr
