// signal_mate_device.h -- which two records are a pair when the input is sorted by position: the mate rules of `panSVR signal`'s default mode
// (signal_step.h: SignalStep::run_pos_sorted, parts 1 to 4 of a block) in the form the device runs them: the bodies of the k_sm_* kernels
// of signal.hip and, compiled for the host with one "lane", of the checker that holds them to the host loop
// (tests/tools/signal_mate_check.cpp).  No HIP calls.  run_pos_sorted is the specification.
//
// A block is n primary records in file order, seen through pos[] / mpos[] / flag[] / same[] (tid == mtid) and a record accessor.
//   block end   the record whose tid differs from the first one's, or whose pos - pos[0] exceeds the span, is the block's last; so is
//               record number `limit`.  Without such a record the block is complete only when the input has ended.
//   served?     positions must not decrease (the last record excepted when it lies on another chromosome), and no position may reach
//               the end of the host's 64 bp index: the host loop aborts there, and that stays the host loop's to do.
//   cand(i)     a pure function of the block.  Unmapped block (tid -1): the next record, else the one before, when it has i's name.
//               Otherwise: with non-decreasing positions the host's 64 bp index selects exactly the records with pos == mpos[i], so
//               the first k != i behind a lower bound with pos[k] == mpos[i], mpos[k] == pos[i] and i's name.  kSmSilent: i takes no
//               turn (the last record, tid != mtid, the first record of an unmapped block, a mate position outside (pos[0], pos[n-2])).
//               kSmNone: i takes its turn and finds nobody.
//   mate[]      the sequential loop's outcome, exactly.  A turn links i and cand(i) when both are free.  Conflicts need equal names, so
//               the components of the graph i -> cand(i) are tiny: a component {i, m} with cand(i) == m, cand(m) in {i, none} and no
//               third record pointing into it (in-degrees) is settled by its own lane whatever the order; a record nobody points to
//               and that points to nobody is settled too; everything else is compacted in index order and replayed by one lane.
//   Mate failed a turn of a free record whose candidate is missing or taken.  In a clean component that is the target m when it is
//               active, finds nobody and lies in front of i; a lone active record without candidate; the replay says it for the rest.
//               The counter runs across blocks: turn number `base + rank + 1` prints a line when it is a multiple of 1000.
//   pairs       ascending i < n - 1 with a mate and without flag 0x80: (i, mate[i]).  left-overs: mate[i] none, in block order.
//   phase 2     the left-overs by name (strcmp), records with 0x40 first (sm_left_tie), append order.  Runs of equal names give
//               floor(L / 2) pairs each and one pairing-error step per odd run that is not the last (sm_left_is_pair / sm_left_is_error).
#pragma once
#include <stdint.h>
#include "signal_device.h"

namespace psvr {

static const int32_t kSmNone = -1, kSmSilent = -2, kSmFree = -1;
static const int32_t kSmIndex = 1000000, kSmStep = 64;       // SEARCH_POS_INDEX_SIZE, SEARCH_STEP
static const int64_t kSmSpan = 60000000, kSmRecords = 1000000;   // SEARCH_REGION_MAX, SAM_LOAD_BUFF_SIZE

// does the record (tid, pos) end the block that (tid0, pos0) began?
PSVR_FQ bool sm_ends_block(int32_t tid0, int32_t pos0, int32_t tid, int32_t pos, int64_t span) { return tid != tid0 || (int64_t)pos - pos0 > span; }
// the block's size: `avail` primaries lie behind its first record, `end` is the first that ends it (avail: none), at most `limit` go in
PSVR_FQ int64_t sm_block_size(int64_t avail, int64_t end, int64_t limit, bool finish, bool *complete)
{
	int64_t n = end < avail ? end + 1 : avail;
	if (n > limit) n = limit;
	*complete = finish || end < avail || avail >= limit;
	return n;
}
// 0: the rules serve record i's position, 1: it lies in front of its predecessor, 2: it overflows the host's index
// (pos_prev: of record i - 1, unused for i == 0; tid_i: record i's)
PSVR_FQ int sm_pos_bad(int64_t n, int64_t i, int32_t tid0, int32_t pos0, int32_t pos_prev, int32_t tid_i, int32_t pos_i)
{
	if (((int64_t)pos_i - pos0) / kSmStep >= kSmIndex - 2) return 2;
	if (i > 0 && pos_i < pos_prev && !(i == n - 1 && tid_i != tid0)) return 1;
	return 0;
}

template <class Rec>
PSVR_FQ int32_t sm_cand(const FqGroup &g, int32_t n, int32_t tid0, const int32_t *pos, const int32_t *mpos, const int32_t *same, const Rec &rec, int32_t i)
{
	if (i >= n - 1 || !same[i]) return kSmSilent;
	if (tid0 == -1) {
		if (i == 0) return kSmSilent;
		if (sg_same_name(g, rec(i + 1), rec(i))) return i + 1;
		if (sg_same_name(g, rec(i - 1), rec(i))) return i - 1;
		return kSmNone;
	}
	const int32_t mp = mpos[i];
	if (mp <= pos[0] || mp >= pos[n - 2]) return kSmSilent;
	int32_t lo = 0, hi = n - 1;                              // the lower bound of mp in pos[0, n - 1): every lane walks the same way
	while (lo < hi) {
		const int32_t mid = lo + (hi - lo) / 2;
		if (pos[mid] < mp) lo = mid + 1; else hi = mid;
	}
	for (int32_t base = lo; base < n - 1; base += (int32_t)FqGroup::width) {
		const int32_t k = base + (int32_t)g.lane;
		const bool in = k < n - 1 && pos[k] == mp;
		uint32_t hit = g.ballot(in && mpos[k] == pos[i] && k != i);
		while (hit) {
			const int32_t b = base + (int32_t)fq_ctz(hit);
			hit &= hit - 1;
			if (sg_same_name(g, rec(b), rec(i))) return b;
		}
		if (g.ballot(!in)) break;                            // the records at mp have ended
	}
	return kSmNone;
}

// is i -> cand[i] a component of its own, settled whatever the order of the turns?
PSVR_FQ bool sm_clean(const int32_t *cand, const int32_t *indeg, int32_t i)
{
	const int32_t m = cand[i];
	if (m < 0 || indeg[m] != 1) return false;
	const int32_t cm = cand[m];
	if (cm == i) return indeg[i] == 1;
	return cm < 0 && indeg[i] == 0;
}
// behind the clean components' links: is record i for the replay?  Otherwise *fail says whether its turn is a "Mate failed"
PSVR_FQ bool sm_dirty(const int32_t *cand, const int32_t *indeg, const int32_t *mate, int32_t i, int32_t *fail)
{
	*fail = 0;
	if (mate[i] != kSmFree) { *fail = cand[i] == kSmNone && mate[i] > i; return false; }
	if (cand[i] < 0 && indeg[i] == 0) { *fail = cand[i] == kSmNone; return false; }
	return true;
}
// the host loop over the replay list (ascending indices), by one lane
PSVR_FQ void sm_replay(const int32_t *list, int64_t n_list, const int32_t *cand, int32_t *mate, int32_t *fail)
{
	for (int64_t j = 0; j < n_list; ++j) {
		const int32_t i = list[j], m = cand[i];
		if (mate[i] != kSmFree || m == kSmSilent) continue;
		if (m < 0 || mate[m] != kSmFree) { fail[i] = 1; continue; }
		mate[i] = m, mate[m] = i;
	}
}
PSVR_FQ bool sm_is_pair(int64_t n, const int32_t *mate, const uint32_t *flag, int64_t i) { return i < n - 1 && mate[i] != kSmFree && !(flag[i] & 0x80); }
// turn number `turn` (counted across blocks from 1) prints a line when this is not -1: the line's slot among the block's notes
PSVR_FQ int64_t sm_note_slot(int64_t base, int64_t turn) { return turn % 1000 == 0 ? turn / 1000 - base / 1000 - 1 : -1; }
PSVR_FQ int64_t sm_note_count(int64_t base, int64_t fails) { return (base + fails) / 1000 - base / 1000; }
// phase 2: the tie key of the by-name order behind the name (records with flag 0x40 first; NOT name_tie_key's flag & 0xc0: 0x00 and 0xc0
// order the other way round there)
PSVR_FQ uint32_t sm_left_tie(uint32_t flag) { return flag & 0x40u ? 0u : 1u; }
// phase 2 at rank j of that order, `off` places behind its run's first: a pair begins at an even place with a partner of its name behind
// it; an even last place of a run that is not the last run is a pairing-error step
PSVR_FQ bool sm_left_is_pair(int64_t off, bool partner) { return !(off & 1) && partner; }
PSVR_FQ bool sm_left_is_error(int64_t off, bool partner, bool last_rank) { return !(off & 1) && !partner && !last_rank; }
PSVR_FQ bool sm_too_many_unmated(int64_t unmated, int64_t n) { return unmated * 20 > n; }

} // namespace psvr
