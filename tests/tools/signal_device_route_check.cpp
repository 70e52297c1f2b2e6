// signal_device_route_check -- `panSVR signal -N --signal-device` without a GPU: pansvr_amd/csrc/signal_device_route.h over a backend that keeps
// the record store in host memory (the members inflated with zlib, the record chain walked serially by the reader's rules, chunks that are
// filled, released and spared as psvr_bam_store_drop does) and runs the rules of signal_device.h with one lane, by psvr_signal_run's steps.
// The command line is `panSVR signal`'s (tests/test_signal_device_route.py compares with the command's host route); on top:
//   PSVR_CHECK_FAIL=call:n     the n-th call of that name fails (store_create, store_append_bgzf, store_footprint, store_drop, store_chain_info,
//                              signal_create, signal_run, signal_pairs, signal_text, signal_side, signal_stats, host_alloc)
//   PSVR_CHECK_CHUNK=bytes     the store's chunk size (default 256 MiB: never more than one chunk in the tests)
//   PSVR_CHECK_ROUTE_INPUT=f   the route reads f instead: a damaged copy of the input whose front is the input's (the step samples the first
//                              100 000 records before the route begins, so a small damaged input never reaches it; this way the route meets
//                              the damage in mid-file, and what takes over reads the whole input)
// An error state that the route returns (3, 4, 5) ends the program with status 30 + state instead of SignalStep::run's abort().
#include <zlib.h>
#include <map>
#include <memory>
#include <string>
#include <vector>
#include "../../pansvr_amd/csrc/signal_device_route.h"
#include "../../pansvr_amd/csrc/signal_device.h"
#include "../../pansvr_amd/csrc/inflate_layout.h"

using namespace psvr;

struct HostBackend {
	struct Rec { std::shared_ptr<std::vector<uint8_t>> chunk; size_t off; };
	std::string err, fail_call;
	long long fail_at = 0;
	std::map<std::string, long long> calls;
	size_t chunk_bytes = (size_t)256 << 20;
	// the store
	bool have_store = false, bad = false;
	std::vector<std::shared_ptr<std::vector<uint8_t>>> chunks;
	std::shared_ptr<std::vector<uint8_t>> spare;
	size_t fill = 0, tail = 0;                               // of the last chunk: bytes of whole records, then the tail
	std::vector<Rec> recs;
	// the signal object
	bool have_sg = false, spent = false;
	psvr_signal_opt_t opt;
	std::vector<uint64_t> isize_n = std::vector<uint64_t>(kSgMaxIsize, 0), len_n = std::vector<uint64_t>(kSgMaxLen, 0);
	std::vector<psvr_signal_pair_t> tab;
	std::string text, side;

	HostBackend()
	{
		if (const char *e = getenv("PSVR_CHECK_FAIL")) {
			const std::string s = e;
			const size_t c = s.find(':');
			fail_call = s.substr(0, c), fail_at = c == std::string::npos ? 1 : atoll(s.c_str() + c + 1);
		}
		if (const char *e = getenv("PSVR_CHECK_CHUNK")) chunk_bytes = (size_t)atoll(e);
	}
	bool failing(const char *call)
	{
		if (++calls[call] == fail_at && fail_call == call) { err = std::string("injected failure of ") + call; return true; }
		return false;
	}
	const char *last_error() { return err.c_str(); }
	void *host_alloc(size_t n) { return failing("host_alloc") ? nullptr : malloc(n ? n : 1); }
	void host_free(void *p) { free(p); }

	int store_create() { if (failing("store_create")) return 3; have_store = true; return 0; }
	void store_destroy() { have_store = false, chunks.clear(), spare.reset(), recs.clear(); }
	const uint8_t *rec(size_t i) const { return recs[i].chunk->data() + recs[i].off; }
	int store_append_bgzf(const void *in_, int64_t n, int64_t skip, int32_t, int64_t *used, int64_t *bad_member)
	{
		*used = 0, *bad_member = -1;
		if (failing("store_append_bgzf")) return 3;
		if (bad) { err = "the store is unusable"; return 3; }
		const uint8_t *in = (const uint8_t *)in_;
		std::vector<InfMember> mem;
		long long in_used = 0, total = 0;
		const long long bad_m = inf_layout(in, n, mem, &in_used, &total);
		if (bad_m >= 0) { *bad_member = bad_m, err = "corrupt BGZF block"; return 5; }
		if (mem.empty()) return 0;
		std::vector<uint8_t> inflated((size_t)total);
		for (size_t i = 0; i < mem.size(); ++i) {
			const InfMember &m = mem[i];
			const uint8_t *p = in + m.in_off;
			z_stream zs;
			memset(&zs, 0, sizeof zs);
			if (inflateInit2(&zs, -15) != Z_OK) { err = "zlib"; return 3; }
			zs.next_in = (Bytef *)(p + m.hdr), zs.avail_in = m.bsize - m.hdr - 8, zs.next_out = inflated.data() + m.out_off, zs.avail_out = m.isize;
			const int rc = inflate(&zs, Z_FINISH);
			const uint32_t want = p[m.bsize - 8] | (uint32_t)p[m.bsize - 7] << 8 | (uint32_t)p[m.bsize - 6] << 16 | (uint32_t)p[m.bsize - 5] << 24;
			const bool fine = rc == Z_STREAM_END && zs.total_out == m.isize && (uint32_t)crc32(crc32(0L, Z_NULL, 0), inflated.data() + m.out_off, m.isize) == want;
			inflateEnd(&zs);
			if (!fine) { *bad_member = (int64_t)i, err = "corrupt BGZF block"; return 5; }
		}
		*used = in_used;
		// the call's stream: the tail, then the members' bytes less the skipped ones -- in the last chunk if it has room, else in a fresh one
		const size_t add = (size_t)(total - skip), need = tail + add;
		if (chunks.empty() || chunks.back()->size() - fill < need) {
			std::shared_ptr<std::vector<uint8_t>> c;
			if (spare && spare->size() >= need) c = std::move(spare), spare.reset();
			else c = std::make_shared<std::vector<uint8_t>>(need > chunk_bytes ? need : chunk_bytes);
			if (tail) memcpy(c->data(), chunks.back()->data() + fill, tail);
			chunks.push_back(c), fill = 0;
		}
		uint8_t *base = chunks.back()->data() + fill;
		memcpy(base + tail, inflated.data() + skip, add);
		size_t at = 0;
		const size_t end = tail + add;
		for (;;) {                                               // the chain, by the reader's rules
			const size_t avail = end - at;
			if (avail < 4) break;
			const uint32_t bs = bam_u32(base + at);
			if (bs < kBamRecMinBlock || bs > kBamRecStoreMaxBlock) { bad = true, err = "malformed BAM record"; return 3; }
			if (avail < kBamRecHead || (size_t)bs + 4 > avail) break;
			if (!bam_rec_reader_fits(base + at) || !bam_rec_name_ends(base + at)) { bad = true, err = "malformed BAM record"; return 3; }
			recs.push_back({chunks.back(), fill + at});
			at += 4 + (size_t)bs;
		}
		fill += at, tail = end - at;
		return 0;
	}
	int store_chain_info(psvr_bam_chain_info_t *i) { if (failing("store_chain_info")) return 3; memset(i, 0, sizeof *i); i->tail_bytes = (int64_t)tail; return 0; }
	int store_drop(int64_t n_front)
	{
		if (failing("store_drop")) return 3;
		if (n_front < 0 || n_front > (int64_t)recs.size()) { err = "drop outside the store"; return 1; }
		recs.erase(recs.begin(), recs.begin() + n_front);
		size_t keep_from = chunks.empty() ? 0 : chunks.size() - 1;
		if (!recs.empty()) for (size_t k = 0; k < chunks.size(); ++k) if (chunks[k] == recs[0].chunk) { keep_from = k; break; }
		for (size_t k = 0; k < keep_from; ++k) if (!spare && chunks[k]->size() == chunk_bytes) spare = chunks[k];
		chunks.erase(chunks.begin(), chunks.begin() + (long)keep_from);
		return 0;
	}
	int store_footprint(int64_t *n, int64_t *bytes)
	{
		if (failing("store_footprint")) return 3;
		*n = (int64_t)chunks.size() + (spare ? 1 : 0), *bytes = spare ? (int64_t)spare->size() : 0;
		for (auto &c : chunks) *bytes += (int64_t)c->size();
		return 0;
	}

	int signal_create(const psvr_signal_opt_t *o) { if (failing("signal_create")) return 3; opt = *o, have_sg = true; return 0; }
	void signal_destroy() { have_sg = false; }
	int signal_run(int64_t first, int, psvr_signal_info_t *info)      // psvr_signal_run's steps, serially
	{
		if (failing("signal_run")) return 3;
		const FqGroup g;
		std::vector<int64_t> prim;
		for (size_t i = (size_t)first; i < recs.size(); ++i) if (sg_primary(rec(i))) prim.push_back((int64_t)i);
		const int64_t P = (int64_t)prim.size() / 2;
		tab.assign((size_t)P, psvr_signal_pair_t());
		int64_t first_err = -1, first_written = -1;
		for (int64_t p = 0; p < P; ++p) {
			psvr_signal_pair_t &t = tab[(size_t)p];
			uint32_t note = 0;
			t.rec1 = prim[(size_t)(2 * p)], t.rec2 = prim[(size_t)(2 * p + 1)];
			t.state = (uint8_t)sg_pair_size(g, opt, rec((size_t)t.rec1), rec((size_t)t.rec2), &t.bytes, &note);
			t.note = (uint8_t)note, t.pad = 0;
			if (t.state >= 3 && first_err < 0) first_err = p;
			if ((t.state == 1 || t.state == 2) && first_written < 0) first_written = p;
		}
		const int64_t n_front = first_err >= 0 ? first_err : P;
		int64_t stat_pair = -1;
		if (!spent && first_written >= 0 && first_written < n_front) {
			stat_pair = first_written, spent = true;
			if (tab[(size_t)stat_pair].state == 1) tab[(size_t)stat_pair].bytes += sg_stat_bytes(g, opt);
		}
		int64_t off = 0;
		info->written = info->declined = 0;
		for (int64_t p = 0; p < P; ++p) {
			if (p >= n_front) tab[(size_t)p].bytes = 0;
			tab[(size_t)p].text_off = off, off += tab[(size_t)p].bytes;
			if (p < n_front) info->written += tab[(size_t)p].state == 1, info->declined += tab[(size_t)p].state == 2;
		}
		text.assign((size_t)off, '\xEE');
		for (int64_t p = 0; p < n_front; ++p) {
			const psvr_signal_pair_t &t = tab[(size_t)p];
			for (int k = 0; k < 2; ++k) {
				int32_t ib, lb;
				sg_collect_bins(rec((size_t)(k ? t.rec2 : t.rec1)), &ib, &lb);
				if (ib >= 0) isize_n[(size_t)ib]++;
				if (lb >= 0) len_n[(size_t)lb]++;
			}
			if (t.state != 1) continue;
			BeWrite w;
			w.out = (uint8_t *)&text[0], w.pos = (uint64_t)t.text_off;
			uint32_t note = 0;
			if (sg_pair(g, opt, rec((size_t)t.rec1), rec((size_t)t.rec2), p == stat_pair, w, &note) != 1 || w.pos != (uint64_t)(t.text_off + t.bytes)) { err = "the passes disagree"; return 3; }
		}
		side.clear();                                            // the records of the pairs the host looks at, and of the error pair
		for (int64_t p = 0; p < P; ++p) {
			psvr_signal_pair_t &t = tab[(size_t)p];
			t.side_off = -1;
			if (!(p == first_err || (p < n_front && (t.state == 2 || t.note)))) continue;
			t.side_off = (int64_t)side.size();
			for (int k = 0; k < 2; ++k) {
				const uint8_t *r = rec((size_t)(k ? t.rec2 : t.rec1));
				side.append((const char *)r, 4 + (size_t)bam_u32(r));
			}
		}
		info->side_bytes = (int64_t)side.size();
		info->pairs = P, info->first_error = first_err, info->text_bytes = off;
		info->consumed = prim.size() & 1 ? prim.back() : (int64_t)recs.size();
		return 0;
	}
	int signal_text(void *t, int64_t cap)
	{
		if (failing("signal_text")) return 3;
		if (cap < (int64_t)text.size()) { err = "text overflow"; return 6; }
		memcpy(t, text.data(), text.size());
		return 0;
	}
	int signal_pairs(psvr_signal_pair_t *t, int64_t cap)
	{
		if (failing("signal_pairs")) return 3;
		if (cap < (int64_t)tab.size()) { err = "table overflow"; return 6; }
		for (size_t i = 0; i < tab.size(); ++i) t[i] = tab[i];
		return 0;
	}
	int signal_side(void *bytes, int64_t cap)
	{
		if (failing("signal_side")) return 3;
		if (cap < (int64_t)side.size()) { err = "side overflow"; return 6; }
		memcpy(bytes, side.data(), side.size());
		return 0;
	}
	int signal_stats(uint64_t *a, uint64_t *b)
	{
		if (failing("signal_stats")) return 3;
		memcpy(a, isize_n.data(), isize_n.size() * 8), memcpy(b, len_n.data(), len_n.size() * 8);
		return 0;
	}
};

int main(int argc, char **argv)
{
	return signal_main(argc, argv, [](SignalStep &S, long long *pairs_done) {
		HostBackend be;
		const std::string input = S.o.input;
		if (const char *e = getenv("PSVR_CHECK_ROUTE_INPUT")) S.o.input = e;
		const int rc = signal_device_route(be, S, pairs_done);
		S.o.input = input;
		if (rc > 0) {                                            // (SignalStep::run would abort(): the code is what the test looks at)
			fflush(S.out);
			fprintf(stderr, "route returned state %d behind %lld pairs\n", rc, *pairs_done);
			exit(30 + rc);
		}
		return rc;
	});
}
