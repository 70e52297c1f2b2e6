// nsort_sink_check.cpp -- the by-name mode of sort_store_sink.h's writer (`panSVR sort --nsort-device`: adopt(..., by_name) + finish_store())
// over a stand-in backend without a GPU, in the manner of sort_store_sink_check.cpp: the adopted store is a SortRecords in host memory with a
// store_order_names() that is name_order(), the BGZF stream a byte vector whose members the encoder's host build makes, and the first call
// of one kind can be made to fail.  The yardstick is write_sorted_bam(..., by_name = true) on the same records, its members from the same build.
// usage: nsort_sink_check <records> <out.bam> <ref.bam> <take_members> <fail>
//   records       BAM records back to back (block_size first): what the caller has put into the store
//   take_members  members pending before a take (the yardstick's window is the same)
//   fail          the call whose first use fails: order | info | meta | "stream create" | "stream append" | stream | take | "the last take" | none
// prints "rc <finish_store's answer> records <n> members <n> calls <n>"; exit status 0, or 9 on a mistake of the check's own.
#define PSVR_BGZF_ON_DEVICE 1
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <algorithm>
#include <string>
#include <vector>
#include "../../pansvr_amd/csrc/deflate_wave_device.h"
#include "../../pansvr_amd/csrc/sort_store_sink.h"
using namespace psvr;

// the engine library's symbols that the included headers name (no device here)
extern "C" {
const char *psvr_last_error(void) { return "stand-in"; }
int psvr_device_count(void) { return 0; }
int psvr_sort_order_u64(int, int64_t, const uint64_t *, uint32_t *) { abort(); }
void *psvr_host_alloc(size_t n) { return malloc(n); }
void psvr_host_free(void *p) { free(p); }
int64_t psvr_bgzf_bound(int64_t n) { return n; }
int psvr_bgzf_compress(int, const void *, int64_t, void *, int64_t, int64_t *) { abort(); }
}

// members of 0xff00 bytes from the encoder's host build, in the shape of psvr_bgzf_compress_members
static int host_members(int, const void *in, int64_t n, int32_t member_bytes, void *out, int64_t cap, int64_t *got, int64_t *off, int64_t off_cap, int64_t *nm)
{
	static DfwLds *lds = new DfwLds;
	const size_t mb = (size_t)member_bytes;
	int64_t at = 0, k = 0;
	for (size_t o = 0; o < (size_t)n; o += mb, ++k) {
		const uint32_t m = (uint32_t)((size_t)n - o < mb ? (size_t)n - o : mb);
		std::vector<uint8_t> src((const uint8_t *)in + o, (const uint8_t *)in + o + m);
		std::vector<uint32_t> slot(dfw_slot_bytes(m) / 4), tok(m + 1);
		memset(lds, 0xa5, sizeof *lds);
		const uint32_t size = dfw_member<1>(src.data(), m, (uint8_t *)slot.data(), tok.data(), lds, 0);
		if (size > dfw_member_max(m) || at + size > cap || (off && k >= off_cap)) { fprintf(stderr, "nsort_sink_check: a member of %u bytes from %u\n", size, m); exit(9); }
		if (off) off[k] = at;
		memcpy((uint8_t *)out + at, slot.data(), size), at += size;
	}
	if (off) off[k] = at;
	if (nm) *nm = k;
	*got = at;
	return 0;
}

struct StandIn {
	SortRecords R;                                                     // the adopted store
	std::vector<uint32_t> ord;
	int ordered = 0;
	bool stream_on = false, destroyed = false;
	std::vector<uint8_t> pend;                                         // the stream
	long long calls = 0;
	std::string fail, err;
	bool failing(const char *what)
	{
		++calls;
		if (fail != what) return false;
		fail = "spent", err = std::string("stand-in failure in ") + what;
		return true;
	}
	const char *last_error() { return err.c_str(); }
	int store_create() { return 0; }
	void store_destroy() { destroyed = true; }
	int store_append(const void *, int64_t) { abort(); }               // (an adopted store is the caller's to fill)
	int store_append_emit(int, int64_t, int64_t) { abort(); }
	int store_download(void *, int64_t, int64_t *) { abort(); }        // (and the caller has its input still: nothing is downloaded)
	int emit_view(int, int64_t, const int64_t **, const uint8_t **) { abort(); }
	int emit_fetch(int, int64_t, int64_t, std::vector<uint8_t> *) { abort(); }
	int store_info(int64_t *nr, int64_t *nb)
	{
		if (failing("info")) return 3;
		*nr = (int64_t)R.size(), *nb = (int64_t)R.bytes;
		return 0;
	}
	int store_order() { err = "the by-name sink asked for the coordinate order"; return 1; }
	int store_order_names()
	{
		if (failing("order")) return 3;
		name_order(R, ord);
		ordered = 2;
		return 0;
	}
	int store_meta(int64_t first, int64_t n, psvr_bam_rec_meta_t *m)
	{
		if (failing("meta")) return 3;
		if (ordered != 2 || first < 0 || n < 0 || first + n > (int64_t)R.size()) { err = "ranks"; return 1; }
		for (int64_t r = 0; r < n; ++r) {
			const uint8_t *h = R.rec(ord[(size_t)(first + r)]);
			bam_rec_derived(h, &m[r]);
			m[r].index = ord[(size_t)(first + r)], m[r].pad = 0;
		}
		return 0;
	}
	int store_stream(int64_t first, int64_t n)
	{
		if (failing("stream")) return 3;
		if (ordered != 2 || !stream_on || first < 0 || n < 0 || first + n > (int64_t)R.size()) { err = "ranks"; return 1; }
		for (int64_t r = first; r < first + n; ++r) {
			const uint8_t *h = R.rec(ord[(size_t)r]);
			pend.insert(pend.end(), h, h + 4 + bam_u32(h));
		}
		return 0;
	}
	int stream_create()
	{
		if (failing("stream create")) return 3;
		stream_on = true, pend.clear();
		return 0;
	}
	void stream_destroy() { stream_on = false; }
	int stream_append(const void *p, int64_t n)
	{
		if (failing("stream append")) return 3;
		pend.insert(pend.end(), (const uint8_t *)p, (const uint8_t *)p + n);
		return 0;
	}
	int64_t bound(int64_t n) { return n > 0 ? bgzf_members_max(n, kBgzfBlock) : 0; }
	int take(int finish, void *out, int64_t cap, int64_t *got, int64_t *off, int64_t off_cap, int64_t *nm, int64_t *used)
	{
		if (failing(finish ? "the last take" : "take")) return 3;
		*got = *nm = *used = 0;
		if (cap < bound((int64_t)pend.size())) { err = "no room"; return 6; }
		const size_t mb = kBgzfBlock, whole = finish ? pend.size() : pend.size() / mb * mb;
		if (whole) host_members(0, pend.data(), (int64_t)whole, (int32_t)mb, out, cap, got, off, off_cap, nm);
		pend.erase(pend.begin(), pend.begin() + (long)whole);
		*used = (int64_t)whole;
		return 0;
	}
	void *host_alloc(size_t n) { return malloc(n); }
	void host_free(void *p) { free(p); }
};

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
	StandIn be;
	if (!be.R.add_stream(bytes.data(), bytes.size())) { fprintf(stderr, "nsort_sink_check: %s is no record stream\n", argv[1]); return 9; }
	be.fail = argv[5];
	SortStoreSink<StandIn> sink(be, [](const SortRecords &) { return 2; }, take_members);
	sink.adopt(argv[2], text, refs, true);
	const int rc = sink.finish_store();
	if (!be.destroyed) { fprintf(stderr, "nsort_sink_check: the store was not destroyed\n"); return 9; }
	// the yardstick: the host's name order and sorted writer, the members from the host build, the same window
	SortRecords all;
	all.add_stream(bytes.data(), bytes.size());
	std::vector<uint32_t> ord;
	std::string err;
	name_order(all, ord);
	if (!write_sorted_bam(argv[3], text, prefs, all, ord, true, 2, &err, &host_members, 0, take_members)) { fprintf(stderr, "%s\n", err.c_str()); return 9; }
	printf("rc %d records %lld members %lld calls %lld\n", rc, sink.st.records, sink.st.members, be.calls);
	return 0;
}
