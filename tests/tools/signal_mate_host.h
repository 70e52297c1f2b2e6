// signal_mate_host.h -- the one-lane host build of pansvr_amd/csrc/signal_mate_device.h, by psvr_signal_run_pos's steps: what the two checkers
// (signal_mate_check.cpp, signal_pos_route_check.cpp) share.  Every decision is the header's; this file only walks the lanes one by one.
#pragma once
#include <string>
#include <utility>
#include <vector>
#include "../../pansvr_amd/csrc/signal_mate_device.h"

namespace psvr {

struct SmHostBlock {
	int64_t n = 0, fails = 0, replayed = 0;
	bool complete = false;
	int bad = 0;                                             // sm_pos_bad of the block: the device declines it
	std::vector<int32_t> cand, mate, fail;
	std::vector<std::pair<int32_t, int32_t>> pairs;          // indices in the block
	std::vector<int32_t> left;
};

struct SmHostRec {
	const std::vector<const uint8_t *> &prim;
	const uint8_t *operator()(int32_t i) const { return prim[(size_t)i]; }
};

// the block at the front of prim (the primaries that are there), as the kernels decide it
inline SmHostBlock sm_host_block(const std::vector<const uint8_t *> &prim, int64_t limit, int64_t span, bool finish)
{
	SmHostBlock B;
	const int64_t avail = (int64_t)prim.size();
	int64_t end = avail;
	for (int64_t j = 1; j < avail && j < limit; ++j)
		if (sm_ends_block(bam_i32(prim[0] + 4), bam_i32(prim[0] + 8), bam_i32(prim[(size_t)j] + 4), bam_i32(prim[(size_t)j] + 8), span)) { end = j; break; }
	B.n = sm_block_size(avail, end, limit, finish, &B.complete);
	if (!B.complete || B.n < 2) return B;
	const int64_t n = B.n;
	std::vector<int32_t> pos((size_t)n), mpos((size_t)n), same((size_t)n), indeg((size_t)n, 0);
	std::vector<uint32_t> flag((size_t)n);
	const int32_t tid0 = bam_i32(prim[0] + 4);
	for (int64_t i = 0; i < n; ++i) {
		const uint8_t *r = prim[(size_t)i];
		pos[(size_t)i] = bam_i32(r + 8), mpos[(size_t)i] = bam_i32(r + 28), flag[(size_t)i] = bam_u16(r + 18), same[(size_t)i] = bam_i32(r + 4) == bam_i32(r + 24);
		const int bad = sm_pos_bad(n, i, tid0, bam_i32(prim[0] + 8), i > 0 ? bam_i32(prim[(size_t)i - 1] + 8) : 0, bam_i32(r + 4), pos[(size_t)i]);
		if (bad && (!B.bad || bad < B.bad)) B.bad = bad;
	}
	if (B.bad) return B;
	const FqGroup g;
	const SmHostRec R{prim};
	B.cand.assign((size_t)n, kSmSilent), B.mate.assign((size_t)n, kSmFree), B.fail.assign((size_t)n, 0);
	for (int64_t i = 0; i < n; ++i) {
		const int32_t c = sm_cand(g, (int32_t)n, tid0, pos.data(), mpos.data(), same.data(), R, (int32_t)i);
		B.cand[(size_t)i] = c;
		if (c >= 0) indeg[(size_t)c]++;
	}
	for (int64_t i = 0; i < n; ++i) if (sm_clean(B.cand.data(), indeg.data(), (int32_t)i)) B.mate[(size_t)i] = B.cand[(size_t)i], B.mate[(size_t)B.cand[(size_t)i]] = (int32_t)i;
	std::vector<int32_t> dlist;
	{
		const std::vector<int32_t> settled = B.mate;         // (the device's k_sm_class reads what k_sm_settle left)
		for (int64_t i = 0; i < n; ++i) if (sm_dirty(B.cand.data(), indeg.data(), settled.data(), (int32_t)i, &B.fail[(size_t)i])) dlist.push_back((int32_t)i);
	}
	B.replayed = (int64_t)dlist.size();
	if (!dlist.empty()) sm_replay(dlist.data(), (int64_t)dlist.size(), B.cand.data(), B.mate.data(), B.fail.data());
	for (int64_t i = 0; i < n; ++i) {
		if (sm_is_pair(n, B.mate.data(), flag.data(), i)) B.pairs.push_back({(int32_t)i, B.mate[(size_t)i]});
		if (B.mate[(size_t)i] == kSmFree) B.left.push_back((int32_t)i);
		B.fails += B.fail[(size_t)i];
	}
	return B;
}

// the record as the store holds it (block_size first), out of the host reader's fields (the bin is not kept there: 0)
template <class Record> std::vector<uint8_t> sm_record_bytes(const Record &r)
{
	std::vector<uint8_t> b(kBamRecHead + r.data.size());
	auto p32 = [&](size_t at, uint32_t v) { b[at] = (uint8_t)v, b[at + 1] = (uint8_t)(v >> 8), b[at + 2] = (uint8_t)(v >> 16), b[at + 3] = (uint8_t)(v >> 24); };
	p32(0, (uint32_t)(b.size() - 4)), p32(4, (uint32_t)r.tid), p32(8, (uint32_t)r.pos);
	b[12] = r.l_qname, b[13] = r.mapq, b[14] = b[15] = 0, b[16] = (uint8_t)r.n_cigar, b[17] = (uint8_t)(r.n_cigar >> 8), b[18] = (uint8_t)r.flag, b[19] = (uint8_t)(r.flag >> 8);
	p32(20, (uint32_t)r.l_qseq), p32(24, (uint32_t)r.mtid), p32(28, (uint32_t)r.mpos), p32(32, (uint32_t)r.isize);
	if (!r.data.empty()) memcpy(b.data() + kBamRecHead, r.data.data(), r.data.size());
	return b;
}

// Phase 2 over `n_left` ranks of the by-name order, by sm_left_is_pair / sm_left_is_error as k_sl_flags walks them.
// events: (rank, 1 pair of ranks (rank, rank + 1) / 0 pairing-error step), in rank order
template <class SameName> std::vector<std::pair<size_t, int>> sm_phase2_events(size_t n_left, SameName same)
{
	std::vector<std::pair<size_t, int>> ev;
	size_t start = 0;
	for (size_t j = 0; j < n_left; ++j) {
		if (j > 0 && !same(j - 1, j)) start = j;
		const bool partner = j + 1 < n_left && same(j, j + 1);
		if (sm_left_is_pair((int64_t)(j - start), partner)) ev.push_back({j, 1});
		else if (sm_left_is_error((int64_t)(j - start), partner, j + 1 == n_left)) ev.push_back({j, 0});
	}
	return ev;
}

} // namespace psvr
