// bam_chain_device.h -- where the records of an inflated BAM stream begin, found side by side.  The record boundaries form one serial chain
// (every block_size says where the next one stands), records straddle BGZF members, and a single lane that follows the chain pays one memory
// round trip per record.  Here the stream is cut into segments of seg_bytes; every segment GUESSES its entry -- the first record start at or
// behind its first byte -- from what a record looks like, and walks from there to its end; one pass then SETTLES the guesses against the one
// thing that is known, the start of the first record, and walks again only the segments whose guess was wrong.  Compiled for the device (the
// bodies of k_chain_guess and k_chain_settle, bam_store.hip: a wavefront per segment, then one wavefront) and, with one "lane", for the host
// (tests/tools/bam_chain_check.cpp: the very same code under AddressSanitizer), as inflate_device.h is.
//   chain_record   the verdict on the record that starts at `at` when `end` bytes of the stream are there.  The rules are bam_record.h's:
//                  the reader's (block_size >= 32, l_seq >= 0, name + CIGAR + bases + qualities inside the record, a name of at least its
//                  NUL) and the store's cap on block_size (kBamRecStoreMaxBlock), in the reader's order: a record whose end is not there
//                  is cut off, whatever its head says
//   chain_guess    the lowest offset of the segment that chain_record calls good, that passes the hints (reference ids in [-1, n_ref),
//                  positions >= -1, a head that holds its own fields) and whose successor is good too or lies beyond the bytes; where the
//                  segment has none, the lowest whose head passes and whose end the bytes cut off (a record's last two bytes and the next
//                  record's first two read as a block_size of gigabytes in front of small fields: whole records are preferred, or every
//                  third segment of a real file guesses wrong); then the walk to the segment's end: exit = the first chain position at or
//                  behind the next segment
//   chain_settle   segment s is settled when guess[s] == entry[s], and then entry[s + 1] = exit[s]; the links guess[s + 1] == exit[s] are
//                  tested 64 at a time, and only a link that fails makes one lane walk that segment from its true entry
// Exact by construction: an accepted link starts where the one before ended, and the first starts at a known place; hints and guesses cost
// time, never a record.  The worst stream (every guess wrong) is the serial walk.  A malformed record counts only on the true chain.
// No load leaves bytes[0, end); every loop advances by at least 36 bytes or by one segment.
#pragma once
#include <stdint.h>
#include <string.h>
#include "bam_record.h"

#if defined(__HIPCC__)
#define PSVR_CF __host__ __device__ inline
#else
#define PSVR_CF inline
#endif

namespace psvr {

enum { kChainGood = 0, kChainBad = 1, kChainCutHead = 2, kChainCutEnd = 3 };   // chain_record's verdicts
enum { kChainSegOk = 0, kChainSegBad = 1, kChainSegCut = 2 };                 // how a segment's walk ended
static const long long kChainMinSeg = 64;

struct ChainSeg {                        // what a segment found out on its own
	long long guess;                     // -1: none
	long long exit;                      // where the walk from the guess stood when it ended
	int32_t count, how;                  // records walked; kChainSeg*
};
struct ChainResult {                     // chain_settle's word on one range
	long long total, tail;               // whole records on the chain; bytes behind the last one
	long long no_guess, wrong_guess, rewalked;
	long long bad_seg;                   // -1, or the segment in which the chain meets a malformed record
	long long bad_at;                    // ... and where that record stands
};

#if defined(__HIP_DEVICE_COMPILE__)
PSVR_CF uint64_t chain_ballot(bool p) { return __ballot(p); }
PSVR_CF long long chain_first(long long v)   // the first lane's value in every lane
{
	const uint32_t lo = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)(uint64_t)v), hi = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)((uint64_t)v >> 32));
	return (long long)((uint64_t)hi << 32 | lo);
}
PSVR_CF long long chain_sum(long long v)     // over the wavefront, in every lane
{
	for (int d = 32; d; d >>= 1) v += __shfl_xor(v, d, 64);
	return v;
}
#else
PSVR_CF uint64_t chain_ballot(bool p) { return p ? 1u : 0u; }
PSVR_CF long long chain_first(long long v) { return v; }
PSVR_CF long long chain_sum(long long v) { return v; }
#endif

PSVR_CF int chain_ctz(uint64_t m) { return __builtin_ctzll(m); }

// bam_rec_frame's three tests in the order that tells a record the bytes cut off from a malformed one, then the reader's rule
PSVR_CF int chain_record(const uint8_t *bytes, long long at, long long end, long long *len)
{
	*len = 0;
	if (end - at < 4) return kChainCutHead;
	const uint8_t *r = bytes + at;
	const uint32_t bs = bam_u32(r);
	if (bs < kBamRecMinBlock || bs > kBamRecStoreMaxBlock) return kChainBad;
	if (end - at < kBamRecHead) return kChainCutHead;
	*len = 4 + (long long)bs;
	if (*len > end - at) return kChainCutEnd;
	if (!bam_rec_reader_fits(r, bs) || !bam_rec_name_ends(r)) return kChainBad;
	return kChainGood;
}

// the hints: what the head of a record looks like whose block_size chain_record has passed.  For guessing only (n_ref < 0: the reference ids
// are not looked at)
PSVR_CF bool chain_hint(const uint8_t *r, uint32_t bs, int32_t n_ref)
{
	const int32_t tid = bam_i32(r + 4), pos = bam_i32(r + 8), mtid = bam_i32(r + 24), mpos = bam_i32(r + 28);
	if (pos < -1 || mpos < -1 || tid < -1 || mtid < -1) return false;
	if (n_ref >= 0 && (tid >= n_ref || mtid >= n_ref)) return false;
	return bam_rec_reader_fits(r, bs);
}

// could a record of the chain start at o?  0: no; 1: a whole record that looks like one, and so does what stands behind it (or nothing does:
// the bytes end there); 2: a head that looks like one, of a record that the bytes cut off
PSVR_CF int chain_plausible(const uint8_t *bytes, long long o, long long end, int32_t n_ref)
{
	long long len = 0, len2 = 0;
	const int v = chain_record(bytes, o, end, &len);
	if (v != kChainGood && v != kChainCutEnd) return 0;
	if (!chain_hint(bytes + o, (uint32_t)(len - 4), n_ref)) return 0;
	if (v == kChainCutEnd) return 2;
	const int v2 = chain_record(bytes, o + len, end, &len2);
	return v2 == kChainGood || v2 == kChainCutHead || (v2 == kChainCutEnd && chain_hint(bytes + o + len, (uint32_t)(len2 - 4), n_ref)) ? 1 : 0;
}

// record after record from `from` until one starts at or behind seg_end (one lane)
PSVR_CF void chain_walk(const uint8_t *bytes, long long from, long long seg_end, long long end, long long *exit, int32_t *count, int32_t *how)
{
	long long at = from;
	int32_t c = 0, h = kChainSegOk;
	while (at < seg_end) {
		long long len = 0;
		const int v = chain_record(bytes, at, end, &len);
		if (v == kChainBad) { h = kChainSegBad; break; }
		if (v != kChainGood) { h = kChainSegCut; break; }
		at += len, ++c;
	}
	*exit = at, *count = c, *how = h;
}

PSVR_CF long long chain_segments(long long end, long long seg) { return (end + seg - 1) / seg; }

// Segment s of bytes[0, end) by NL lanes: the lanes try NL neighbouring offsets a turn, the lowest that is plausible is the guess, the first
// lane walks.  Segment 0 does not guess: its entry is `start`.
template <int NL>
PSVR_CF void chain_guess(const uint8_t *bytes, long long end, long long seg, long long start, int32_t n_ref, long long s, ChainSeg *out, int lane)
{
	const long long lo = s * seg, hi = lo + seg < end ? lo + seg : end;
	long long g = -1, cut = -1;
	if (s == 0) g = start;
	else {
		for (long long o0 = lo; o0 < hi && g < 0; o0 += NL) {
			const long long o = o0 + lane;
			const int p = o < hi ? chain_plausible(bytes, o, end, n_ref) : 0;
			const uint64_t whole = chain_ballot(p == 1), head = chain_ballot(p == 2);
			if (whole) g = o0 + chain_ctz(whole);
			if (head && cut < 0) cut = o0 + chain_ctz(head);
		}
		if (g < 0) g = cut;
	}
	if (lane != 0) return;
	ChainSeg r = {g, g, 0, kChainSegOk};
	if (g >= 0) chain_walk(bytes, g, hi, end, &r.exit, &r.count, &r.how);
	out[s] = r;
}

// The guesses of all n_seg segments settled by NL lanes: entry[0 .. n_seg] and the segments' final counts cnt[0 .. n_seg) (both written by
// whichever lane holds the segment), the result in every lane.  seg[] is only read.
template <int NL>
PSVR_CF ChainResult chain_settle(const uint8_t *bytes, long long end, long long seg, long long start, long long n_seg, const ChainSeg *sg, long long *entry, int32_t *cnt, int lane)
{
	ChainResult R = {0, 0, 0, 0, 0, -1, -1};
	long long none = 0;
	for (long long i = lane; i < n_seg; i += NL) none += sg[i].guess < 0;
	R.no_guess = chain_sum(none);
	long long s = 0, e = start, total = 0;     // entry[s] = e is known; all of it the same in every lane
	bool stop = false;
	while (s < n_seg && !stop) {
		// the links of segments s .. s + NL - 1, each tested on its own: a segment holds if its guess is where the segment before left off
		const long long i = s + lane;
		bool holds = false;
		long long mine = 0;
		ChainSeg g = {-1, -1, 0, kChainSegOk};
		if (i < n_seg) {
			g = sg[i];
			mine = i == s ? e : sg[i - 1].exit;
			holds = g.guess >= 0 && g.guess == mine && g.how == kChainSegOk;
		}
		const uint64_t m = chain_ballot(holds);
		const int k = ~m ? chain_ctz(~m) : 64;           // the leading segments that hold
		if (lane < k) entry[i] = mine, cnt[i] = g.count;
		total += chain_sum(lane < k ? (long long)g.count : 0);
		if (k) {
			e = chain_first(chain_sum(lane == k - 1 ? g.exit : 0));
			s += k;
			if (k == NL) continue;
		}
		if (s >= n_seg) break;
		// segment s does not hold: a right guess whose walk met the stream's end or a malformed record, or a wrong guess or none
		ChainSeg w = {-1, e, 0, kChainSegOk};
		long long walked = 0, wrong = 0;
		if (lane == 0) {
			const ChainSeg t = sg[s];
			const long long hi = (s + 1) * seg < end ? (s + 1) * seg : end;
			if (t.guess == e) w = t;
			else {
				wrong = t.guess >= 0;
				if (e < hi) chain_walk(bytes, e, hi, end, &w.exit, &w.count, &w.how), walked = 1;   // (else a record covers the segment: no record starts in it)
			}
			entry[s] = e, cnt[s] = w.count;
		}
		R.wrong_guess += chain_first(wrong), R.rewalked += chain_first(walked);
		total += chain_first(w.count);
		const long long how = chain_first(w.how);
		e = chain_first(w.exit);
		if (how == kChainSegBad) R.bad_seg = s, R.bad_at = e;
		stop = how != kChainSegOk;
		++s;
	}
	// behind the stream's last whole record (or the malformed one) no record starts
	for (long long i = s + lane; i <= n_seg; i += NL) {
		entry[i] = e;
		if (i < n_seg) cnt[i] = 0;
	}
	R.total = total, R.tail = end - e;
	return R;
}

} // namespace psvr
