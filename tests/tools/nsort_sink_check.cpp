// nsort_sink_check.cpp -- the by-name mode of sorted_bam.h's store writer (what `panSVR sort --nsort-device` ends with: finish_sorted_store(...,
// by_name)) over a stand-in backend without a GPU (sink_host.h's StoreHost: the store is a SortRecords in host memory whose store_order_names()
// is name_order(), the BGZF stream a byte vector whose members the encoder's host build makes, and the first call of one kind can be made to
// fail).  The yardstick is write_sorted_bam(..., by_name = true) on the same records, its members from the same build.
// usage: nsort_sink_check <records> <out.bam> <ref.bam> <take_members> <fail>
//   records       BAM records back to back (block_size first): what the caller has put into the store
//   take_members  members pending before a take (the yardstick's window is the same)
//   fail          the call whose first use fails: order | info | meta | "stream create" | "stream append" | stream | take | "the last take" | none
// prints "rc <finish_sorted_store's answer> records <n> members <n> calls <n>"; exit status 0, or 9 on a mistake of the check's own.
#include "sink_host.h"

int main(int argc, char **argv)
{
	if (argc != 6) { fprintf(stderr, "usage: nsort_sink_check <records> <out.bam> <ref.bam> <take_members> <fail>\n"); return 9; }
	std::vector<uint8_t> bytes;
	{
		FILE *f = fopen(argv[1], "rb");
		if (!f) return 9;
		uint8_t b[65536];
		for (size_t k; (k = fread(b, 1, sizeof b, f)) > 0;) bytes.insert(bytes.end(), b, b + k);
		fclose(f);
	}
	const size_t take_members = (size_t)atoll(argv[4]);
	const std::string text = "@HD\tVN:1.6\tSO:unsorted\n@SQ\tSN:chr1\tLN:250000000\n@SQ\tSN:chr2\tLN:250000000\n@SQ\tSN:chr3\tLN:250000000\n";
	const std::vector<BamRef> refs = {{"chr1", 250000000}, {"chr2", 250000000}, {"chr3", 250000000}};
	const std::vector<std::pair<std::string, int32_t>> prefs = {{"chr1", 250000000}, {"chr2", 250000000}, {"chr3", 250000000}};
	StoreHost be;
	if (!be.R.add_stream(bytes.data(), bytes.size())) { fprintf(stderr, "nsort_sink_check: %s is no record stream\n", argv[1]); return 9; }
	be.fail_kind = argv[5];
	StoreWritten w;
	const int rc = finish_sorted_store(be, argv[2], text, refs, true, take_members, &w);
	if (!be.destroyed) { fprintf(stderr, "nsort_sink_check: the store was not destroyed\n"); return 9; }
	if (be.ordered == 1) { fprintf(stderr, "nsort_sink_check: the by-name writer asked for the coordinate order\n"); return 9; }
	// the yardstick: the host's name order and sorted writer, the members from the host build, the same window
	SortRecords all;
	all.add_stream(bytes.data(), bytes.size());
	std::vector<uint32_t> ord;
	std::string err;
	name_order(all, ord);
	if (!write_sorted_bam(argv[3], text, prefs, all, ord, true, 2, &err, &host_members, 0, take_members)) { fprintf(stderr, "%s\n", err.c_str()); return 9; }
	printf("rc %d records %lld members %lld calls %lld\n", rc, w.records, w.members, be.calls);
	return 0;
}
