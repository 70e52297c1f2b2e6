// signal_route_host.h -- the routes of pansvr_amd/csrc/signal_device_route.h without a GPU: what the four route checkers
// (signal_device_route_check.cpp, bam_device_route_check.cpp, signal_pos_route_check.cpp, mate_window_route_check.cpp) share.  One backend that
// keeps the record store in host memory (the members inflated with zlib, the record chain walked serially by the reader's rules, chunks that
// are filled, released and spared as psvr_bam_store_drop does) and runs the device's rules with one lane: signal_device.h's per pair, by
// psvr_signal_run's passes (pairs_pass: over consecutive primaries for signal_run, over a block's mates and a slice of the by-name pass for
// the position-sorted mode's calls, which take the mate rules from signal_mate_host.h), and signal_window_device.h's add rule for the
// window.  And the reader of the window consumers: it takes every offered window in pieces (fastq_device.h's host parser with a pair limit,
// walking the window by used_bytes as FastqReader::read_window does) and prints what each piece used.
//   PSVR_CHECK_FAIL=call:n     the n-th call of that name fails (store_create, store_append_bgzf, store_footprint, store_drop, store_chain_info,
//                              signal_create, signal_run, signal_pairs, signal_text, signal_side, signal_stats, host_alloc; signal_run_pos,
//                              signal_mate_notes, signal_run_left, signal_left_errors; signal_window, signal_window_add; window_parse: the
//                              reader's n-th piece)
//   PSVR_CHECK_CHUNK=bytes     the store's chunk size (default 256 MiB: never more than one chunk in the tests)
//   PSVR_CHECK_PIECE_PAIRS=n   the reader's pair limit per piece (default 1 << 20)
//   PSVR_CHECK_DUMP=prefix     what every call of the position-sorted mode answered, for tests/test_signal_mate_gpu.py to hold the device to.
//                              prefix.calls has per call
//     O <the 15 numbers of psvr_signal_opt_t>                                            (signal_create)
//     B primaries consumed unmated left_bytes mate_failed notes replayed | L records pairs errors first_pair n_pairs more
//     I pairs written declined first_error text_bytes side_bytes
//     P state note bytes rec1 rec2 side_off text_off errors_in_front   (per pair; the last is 0 for a block)
//     N number index block tid pos name                                  (per note)
//                              and prefix.<call>.text / .side / .left hold the call's bytes.
#pragma once
#include <zlib.h>
#include <algorithm>
#include <map>
#include <memory>
#include <string>
#include <vector>
#include "../../pansvr_amd/csrc/signal_device_route.h"
#include "../../pansvr_amd/csrc/signal_device.h"
#include "../../pansvr_amd/csrc/inflate_layout.h"
#include "../../pansvr_amd/csrc/fastq_device.h"
#include "../../pansvr_amd/csrc/signal_window_device.h"
#include "signal_mate_host.h"

using namespace psvr;

struct HostBackend {
	struct Rec { std::shared_ptr<std::vector<uint8_t>> chunk; size_t off; };
	typedef std::vector<const uint8_t *> Recs;
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
	// the position-sorted mode
	long long mate_failed = 0;
	std::vector<psvr_signal_mate_note_t> notes;
	std::string left;
	std::vector<std::string> left_store;                     // the unmated records of all blocks, in append order
	std::vector<size_t> left_ord;
	std::vector<std::pair<size_t, size_t>> left_pairs;       // indices into left_store
	std::vector<int64_t> left_errs, slice_errs;              // per pair: the error steps in front of it
	int64_t left_err_total = 0;
	bool left_ordered = false;
	FILE *dump_f = nullptr;
	std::string dump_prefix;
	long long dump_calls = 0;
	// the window
	std::string window;
	long long win_pairs = 0, win_host_pairs = 0, window_bytes_max = (long long)1 << 32;

	HostBackend()
	{
		if (const char *e = getenv("PSVR_CHECK_FAIL")) {
			const std::string s = e;
			const size_t c = s.find(':');
			fail_call = s.substr(0, c), fail_at = c == std::string::npos ? 1 : atoll(s.c_str() + c + 1);
		}
		if (const char *e = getenv("PSVR_CHECK_CHUNK")) chunk_bytes = (size_t)atoll(e);
		if (const char *e = getenv("PSVR_CHECK_DUMP")) dump_prefix = e, dump_f = fopen((dump_prefix + ".calls").c_str(), "w");
	}
	~HostBackend() { if (dump_f) fclose(dump_f); }
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

	int signal_create(const psvr_signal_opt_t *o)
	{
		if (failing("signal_create")) return 3;
		opt = *o, have_sg = true;
		if (dump_f) {
			const int32_t *v = (const int32_t *)o;
			fprintf(dump_f, "O");
			for (size_t k = 0; k < sizeof *o / 4; ++k) fprintf(dump_f, " %d", v[k]);
			fprintf(dump_f, "\n");
		}
		return 0;
	}
	void signal_destroy() { have_sg = false; }
	// psvr_signal_run's passes over a pair list: r1 / r2 the records, i1 / i2 what the table says about them (everything of *info but consumed)
	int pairs_pass(const Recs &r1, const Recs &r2, const std::vector<int64_t> &i1, const std::vector<int64_t> &i2, psvr_signal_info_t *info)
	{
		const FqGroup g;
		const int64_t P = (int64_t)r1.size();
		tab.assign((size_t)P, psvr_signal_pair_t());
		text.clear(), side.clear();
		int64_t first_err = -1, first_written = -1;
		for (int64_t p = 0; p < P; ++p) {
			psvr_signal_pair_t &t = tab[(size_t)p];
			uint32_t note = 0;
			t.rec1 = i1[(size_t)p], t.rec2 = i2[(size_t)p];
			t.state = (uint8_t)sg_pair_size(g, opt, r1[(size_t)p], r2[(size_t)p], &t.bytes, &note);
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
				sg_collect_bins(k ? r2[(size_t)p] : r1[(size_t)p], &ib, &lb);
				if (ib >= 0) isize_n[(size_t)ib]++;
				if (lb >= 0) len_n[(size_t)lb]++;
			}
			if (t.state != 1) continue;
			BeWrite w;
			w.out = (uint8_t *)&text[0], w.pos = (uint64_t)t.text_off;
			uint32_t note = 0;
			if (sg_pair(g, opt, r1[(size_t)p], r2[(size_t)p], p == stat_pair, w, &note) != 1 || w.pos != (uint64_t)(t.text_off + t.bytes)) { err = "the passes disagree"; return 3; }
		}
		for (int64_t p = 0; p < P; ++p) {                        // the records of the pairs the host looks at, and of the error pair
			psvr_signal_pair_t &t = tab[(size_t)p];
			t.side_off = -1;
			if (!(p == first_err || (p < n_front && (t.state == 2 || t.note)))) continue;
			t.side_off = (int64_t)side.size();
			for (int k = 0; k < 2; ++k) {
				const uint8_t *r = k ? r2[(size_t)p] : r1[(size_t)p];
				side.append((const char *)r, 4 + (size_t)bam_u32(r));
			}
		}
		info->side_bytes = (int64_t)side.size(), info->pairs = P, info->first_error = first_err, info->text_bytes = off;
		return 0;
	}
	int signal_run(int64_t first, int, psvr_signal_info_t *info)      // the pairs are the consecutive primaries
	{
		if (failing("signal_run")) return 3;
		std::vector<int64_t> prim, i1, i2;
		Recs r1, r2;
		for (size_t i = (size_t)first; i < recs.size(); ++i) if (sg_primary(rec(i))) prim.push_back((int64_t)i);
		for (size_t p = 0; p + 1 < prim.size(); p += 2) i1.push_back(prim[p]), i2.push_back(prim[p + 1]), r1.push_back(rec((size_t)prim[p])), r2.push_back(rec((size_t)prim[p + 1]));
		if (int rc = pairs_pass(r1, r2, i1, i2, info)) return rc;
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

	// ---- the position-sorted mode, by psvr_signal_run_pos's and psvr_signal_run_left's steps
	void dump_blob(const char *what, const std::string &b)
	{
		FILE *f = fopen((dump_prefix + "." + std::to_string(dump_calls) + "." + what).c_str(), "wb");
		if (f) fwrite(b.data(), 1, b.size(), f), fclose(f);
	}
	void dump_call(const std::string &head, const psvr_signal_info_t &info, const std::vector<int64_t> *errs)
	{
		if (!dump_f) return;
		fprintf(dump_f, "%s\nI %lld %lld %lld %lld %lld %lld\n", head.c_str(), (long long)info.pairs, (long long)info.written, (long long)info.declined, (long long)info.first_error, (long long)info.text_bytes,
		        (long long)info.side_bytes);
		for (size_t p = 0; p < tab.size(); ++p)
			fprintf(dump_f, "P %d %d %d %lld %lld %lld %lld %lld\n", tab[p].state, tab[p].note, tab[p].bytes, (long long)tab[p].rec1, (long long)tab[p].rec2, (long long)tab[p].side_off, (long long)tab[p].text_off,
			        errs ? (long long)(*errs)[p] : 0ll);
		for (const psvr_signal_mate_note_t &t : notes) fprintf(dump_f, "N %lld %d %d %d %d %s\n", (long long)t.number, t.index, t.block, t.tid, t.pos, t.name);
		dump_blob("text", text), dump_blob("side", side), dump_blob("left", left);
		fflush(dump_f);
		++dump_calls;
	}
	int signal_run_pos(int64_t first, int finish, const psvr_signal_pos_opt_t *po, psvr_signal_info_t *info, psvr_signal_pos_info_t *pi)
	{
		if (failing("signal_run_pos")) return 3;
		memset(info, 0, sizeof *info), memset(pi, 0, sizeof *pi);
		info->first_error = -1, pi->mate_failed = mate_failed;
		std::vector<int64_t> where;
		Recs prim;
		for (size_t i = (size_t)first; i < recs.size(); ++i) if (sg_primary(rec(i))) where.push_back((int64_t)i), prim.push_back(rec(i));
		const SmHostBlock B = sm_host_block(prim, po && po->block_records ? po->block_records : kSmRecords, po && po->block_span ? po->block_span : kSmSpan, finish != 0);
		if (!B.complete) return 0;
		pi->complete = 1, pi->primaries = B.n;
		tab.clear(), text.clear(), side.clear(), left.clear(), notes.clear();
		if (B.n < 2) { pi->consumed = info->consumed = (int64_t)recs.size(); return 0; }
		if (B.bad) { err = B.bad == 1 ? "positions decrease inside a block (is the input sorted by position?)" : "a position of the block overflows the host loop's position index"; return 7; }
		Recs r1, r2;
		std::vector<int64_t> i1, i2;
		for (const auto &p : B.pairs) r1.push_back(prim[(size_t)p.first]), r2.push_back(prim[(size_t)p.second]), i1.push_back(where[(size_t)p.first]), i2.push_back(where[(size_t)p.second]);
		if (int rc = pairs_pass(r1, r2, i1, i2, info)) return rc;
		// the unmated records (into the left store) and the notes
		for (int32_t i : B.left) {
			left.append((const char *)prim[(size_t)i], 4 + (size_t)bam_u32(prim[(size_t)i]));
			left_store.emplace_back((const char *)prim[(size_t)i], 4 + (size_t)bam_u32(prim[(size_t)i]));
		}
		left_ordered = false;
		long long rank = 0;
		for (int64_t i = 0; i < B.n; ++i) {
			if (!B.fail[(size_t)i]) continue;
			const long long turn = mate_failed + ++rank;
			if (sm_note_slot(mate_failed, turn) < 0) continue;
			psvr_signal_mate_note_t t;
			memset(&t, 0, sizeof t);
			const uint8_t *r = prim[(size_t)i];
			t.number = turn, t.index = (int32_t)i, t.block = (int32_t)B.n, t.tid = bam_i32(r + 4), t.pos = bam_i32(r + 8);
			strncpy(t.name, (const char *)r + kBamRecHead, 255);
			notes.push_back(t);
		}
		mate_failed += B.fails;
		pi->consumed = info->consumed = where[(size_t)B.n - 1] + 1;
		pi->unmated = (int64_t)B.left.size(), pi->left_bytes = (int64_t)left.size(), pi->mate_failed = mate_failed, pi->notes = (int64_t)notes.size(), pi->replayed = B.replayed;
		char head[256];
		snprintf(head, sizeof head, "B %lld %lld %lld %lld %lld %lld %lld", (long long)pi->primaries, (long long)pi->consumed, (long long)pi->unmated, (long long)pi->left_bytes, (long long)pi->mate_failed,
		         (long long)pi->notes, (long long)pi->replayed);
		dump_call(head, *info, nullptr);
		return 0;
	}
	int signal_mate_notes(psvr_signal_mate_note_t *t, int64_t cap)
	{
		if (failing("signal_mate_notes")) return 3;
		if (cap < (int64_t)notes.size()) { err = "note overflow"; return 6; }
		for (size_t i = 0; i < notes.size(); ++i) t[i] = notes[i];
		return 0;
	}
	const uint8_t *lrec(size_t i) const { return (const uint8_t *)left_store[i].data(); }
	int signal_run_left(int64_t first_pair, int64_t max_pairs, psvr_signal_info_t *info, psvr_signal_left_info_t *li)
	{
		if (failing("signal_run_left")) return 3;
		memset(info, 0, sizeof *info), memset(li, 0, sizeof *li);
		info->first_error = -1;
		if (left_store.size() & 1) { err = "an odd number of records found no mate: the host loop ends there"; return 7; }
		const FqGroup g;
		if (!left_ordered) {
			left_ord.resize(left_store.size());
			for (size_t i = 0; i < left_ord.size(); ++i) left_ord[i] = i;
			// (the device sorts by 8-byte chunks of the name and sm_left_tie; the order is the one this comparator gives)
			std::stable_sort(left_ord.begin(), left_ord.end(), [&](size_t a, size_t b) {
				const int c = strcmp((const char *)lrec(a) + kBamRecHead, (const char *)lrec(b) + kBamRecHead);
				if (c) return c < 0;
				return sm_left_tie(bam_u16(lrec(a) + 18)) < sm_left_tie(bam_u16(lrec(b) + 18));
			});
			left_pairs.clear(), left_errs.clear();
			int64_t errs = 0;
			for (const auto &ev : sm_phase2_events(left_ord.size(), [&](size_t a, size_t b) { return sg_same_name(g, lrec(left_ord[a]), lrec(left_ord[b])); })) {
				if (!ev.second) { ++errs; continue; }
				left_pairs.push_back({left_ord[ev.first], left_ord[ev.first + 1]}), left_errs.push_back(errs);
			}
			left_err_total = errs;
			left_ordered = true;
		}
		const int64_t P = (int64_t)left_pairs.size();
		if (first_pair < 0 || first_pair > P || max_pairs < 1) { err = "slice outside the pair list"; return 1; }
		const int64_t cnt = std::min(max_pairs, P - first_pair);
		li->records = (int64_t)left_store.size(), li->pairs = P, li->errors = left_err_total, li->first_pair = first_pair, li->n_pairs = cnt, li->more = first_pair + cnt < P;
		Recs r1, r2;
		std::vector<int64_t> i1, i2;
		slice_errs.clear();
		for (int64_t p = first_pair; p < first_pair + cnt; ++p) {
			r1.push_back(lrec(left_pairs[(size_t)p].first)), r2.push_back(lrec(left_pairs[(size_t)p].second));
			i1.push_back((int64_t)left_pairs[(size_t)p].first), i2.push_back((int64_t)left_pairs[(size_t)p].second), slice_errs.push_back(left_errs[(size_t)p]);
		}
		notes.clear(), left.clear();
		if (int rc = pairs_pass(r1, r2, i1, i2, info)) return rc;
		char head[256];
		snprintf(head, sizeof head, "L %lld %lld %lld %lld %lld %lld", (long long)li->records, (long long)li->pairs, (long long)li->errors, (long long)li->first_pair, (long long)li->n_pairs, (long long)li->more);
		dump_call(head, *info, &slice_errs);
		return 0;
	}
	int signal_left_errors(int64_t *e, int64_t cap)
	{
		if (failing("signal_left_errors")) return 3;
		if (cap < (int64_t)slice_errs.size()) { err = "error table overflow"; return 6; }
		for (size_t i = 0; i < slice_errs.size(); ++i) e[i] = slice_errs[i];
		return 0;
	}

	// ---- the window: the last run's text and the host's in pair order, behind what the window holds (restart: at base 0)
	int window_add(const void *host, int64_t host_bytes, const int64_t *host_off, int64_t n_host, int32_t restart, psvr_signal_window_info_t *info)
	{
		int64_t n_front = 0, declined = 0, written = 0;
		while (n_front < (int64_t)tab.size() && tab[(size_t)n_front].state < 3) ++n_front;
		std::vector<uint8_t> state((size_t)n_front + 1);
		std::vector<int64_t> toff((size_t)n_front + 1);
		for (int64_t p = 0; p < n_front; ++p) state[(size_t)p] = tab[(size_t)p].state, toff[(size_t)p] = tab[(size_t)p].text_off, declined += state[(size_t)p] == 2, written += state[(size_t)p] == 1;
		if (const char *bad = sw_args_bad(host_bytes, host_off, n_host, declined)) { err = bad; return 1; }
		const size_t base = restart ? 0 : window.size(), n_out = text.size() + (size_t)host_bytes;
		if ((long long)(base + n_out) >= window_bytes_max) { err = "a window of " + std::to_string(base + n_out) + " bytes"; return 2; }
		if (restart) window.clear(), win_pairs = win_host_pairs = 0;
		window.resize(base + n_out, '\xEE');
		sw_window_add_host(state.data(), toff.data(), n_front, (const uint8_t *)text.data(), (int64_t)text.size(), (const uint8_t *)host, host_off, n_host, (uint8_t *)&window[0], (int64_t)base);
		win_pairs += written + declined, win_host_pairs += n_host;
		info->n_bytes = (int64_t)window.size(), info->n_pairs = win_pairs, info->n_host_pairs = win_host_pairs;
		return 0;
	}
	int signal_window(const void *host, int64_t host_bytes, const int64_t *host_off, int64_t n_host, psvr_signal_window_info_t *info)
	{
		return failing("signal_window") ? 3 : window_add(host, host_bytes, host_off, n_host, 1, info);
	}
	int signal_window_add(const void *host, int64_t host_bytes, const int64_t *host_off, int64_t n_host, int32_t restart, psvr_signal_window_info_t *info)
	{
		return failing("signal_window_add") ? 3 : window_add(host, host_bytes, host_off, n_host, restart, info);
	}
};

// the window consumers' reader: stdout gets the text of the pairs that were handed over
struct PrintingReader : SignalWindowTaker {
	HostBackend &be;
	long long piece_pairs = 1 << 20, offers = 0, pieces = 0;
	explicit PrintingReader(HostBackend &b) : be(b) { if (const char *e = getenv("PSVR_CHECK_PIECE_PAIRS")) piece_pairs = atoll(e); }
	long long offer(const psvr_signal_window_info_t &info, std::string *why) override
	{
		long long taken = 0;
		uint64_t at = 0;
		++offers;
		if ((size_t)info.n_bytes != be.window.size()) { *why = "the offer is not the backend's window"; return 0; }
		while (taken < info.n_pairs) {
			if (be.failing("window_parse")) { *why = be.err; return taken; }
			FqHostResult r;
			fq_parse_host(be.window.data() + at, be.window.size() - at, 1, piece_pairs, (int64_t)1 << 60, &r);
			if (r.info.n_pairs < 1 || taken + r.info.n_pairs > info.n_pairs) { *why = "the window's text does not hold the pairs the route counted"; return taken; }
			fwrite(be.window.data() + at, 1, (size_t)r.info.used_bytes, stdout);
			at += (uint64_t)r.info.used_bytes, taken += r.info.n_pairs, ++pieces;
		}
		if (at != be.window.size()) { *why = "text behind the window's last pair"; return taken - 1; }
		return taken;
	}
};

// what a checker's route function returns: an error state of the route (3, 4, 5) ends the program with status 30 + state instead of
// SignalStep::run's abort() (the code is what the tests look at); `out` is where the handed-over text went
inline int route_status(int rc, long long pairs_done, FILE *out)
{
	if (rc <= 0) return rc;
	fflush(out);
	fprintf(stderr, "route returned state %d behind %lld pairs\n", rc, pairs_done);
	exit(30 + rc);
}
