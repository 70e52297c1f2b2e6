// deflate_wave_device.h -- one BGZF member (a gzip member with the BC field around one RFC 1951 stream, SAMv1 4.1) compressed by ONE
// WAVEFRONT: the body of k_bgzf_deflate_wave (deflate_wave.hip: a wavefront per member of up to 0xff00 input bytes, the members of a call
// side by side) and, compiled for the host with one "lane", of the checker that zlib judges (tests/tools/deflate_wave_check.cpp).  The
// counterpart of inflate_device.h on the output side; deflate_device.h's encoder gives a member to one LANE, and a call of it lasts as
// long as one lane needs for its block.  htslib deflates a member with zlib on a host thread (bgzf.c: bgzf_compress).
//
// The member's bytes are a function of the input bytes and of nothing else: not of NL, not of timing.  Wherever lanes meet in one word the
// outcome is an associative, commutative operation on LDS (add, or, max), never "the last store wins", and every cross-lane step
// (ballot, pick, scan) has a host form with the same integer result.  The phases, each `for (i = lane; i < n; i += NL)` with inf_sync()
// between them:
//   1 LZ77, greedy, the window is the member itself.  Positions are taken 64 at a time.  A lane per position hashes its three bytes and reads
//     the candidate from an LDS table of positions that holds the state after all EARLIER groups; it also tries the fixed distances
//     1..kDfwNear, which a group-parallel matcher would otherwise not see (BAM qualities are runs).  Each candidate is extended by dword
//     compares against the member's own input.  Longest wins, then nearest.  The group's matches are resolved by a wave-uniform walk over
//     the ballot of "has a match": a match is taken and jumped over, a run of literals is skipped with one count-trailing-zeros.  Each
//     token start then finds its index by a population count and writes its token to the member's scratch slice, counts its symbols by LDS
//     atomics and enters its position into the table by an LDS max: the greatest position wins.
//     Efforts 1, 2, 3 (dfw_member_effort; 0 is the rule above, unchanged) add zlib's two means to it, hash chains and lazy evaluation:
//     * links: every position p with p + 4 <= n, covered by an earlier match or not, stores link[p] = the table entry it read (position + 1,
//       0 = none): the state after all earlier groups, so positions of one group do not link to one another.  After the distances 1 and 2
//       the candidates are c = head[h], link[c - 1], ... : 4, 8, 16 entries at most, until 0 or a distance above 32768; positions strictly
//       decrease; an entry at distance 1 or 2 (tried already) is passed over and counts as one of the 4, 8, 16.  Longest wins, then nearest
//       (the walk goes nearest first, the comparison is strict).  A link is read only for a position that entered the table, and such a
//       position has written its own link: scratch that was never written is never read.
//     * lazy: in the wave-uniform walk a match at `cur` whose successor in the same group has a strictly longer one goes out as a literal
//       and the walk continues at cur + 1, where the same test applies; a group's last position has no look-ahead.  The demotions are a
//       wave-uniform mask beside the token starts.
//   2 code lengths: the symbols are ranked by (frequency, symbol) with the lanes, each counting the symbols in front of its own; Moffat's
//     in-place algorithm and the 15-bit limit are deflate_device.h's (df_lengths_sorted: one lane, O(symbols)); canonical codes likewise.
//   3 the sizes of the three block types follow from the frequencies alone, so the smallest is chosen BEFORE anything is emitted and BSIZE
//     is known when the header is written: dynamic Huffman (code lengths sent with the fixed 4-bit code-length code of deflate_device.h),
//     fixed Huffman, or stored -- always stored when nothing else is smaller, which keeps every member within n + 31 bytes.
//   4 emission: the member is one LSB-first bit string from its first header byte on.  64 tokens at a time: each lane builds its token's bits
//     (at most 48), the lengths are prefix-summed across the wavefront, each lane ORs its bits into a zeroed LDS window at its offset, and
//     the window's complete words leave as one coalesced dword store.  CRC32 (inflate_device.h's 64 slices) and ISIZE end the string.
// Bounds: every load of input is inside in[0, n), every store inside slot[0, dfw_slot_bytes(n)) or tok[0, n + 1); every loop consumes input
// positions or tokens or is bounded by a table size; nothing waits for another workgroup.  link (efforts 1-3: n half-words per member): every
// index is a position < n, so every store and every chain load lies inside link[0, n); a link is written by one lane and read by another
// in a later group, so the group ends with the fence tok gets before phase 4 (inf_fence, then inf_sync).
#pragma once
#include <stdint.h>
#include "deflate_device.h"
#include "inflate_device.h"

namespace psvr {

static const int kDfwHashBits = 12;
static const uint32_t kDfwNear = 2;                  // the fixed distances tried besides the table's candidate
static const uint32_t kDfwWindow = 128;              // words of the emission window: 64 tokens of 48 bits are 96, plus the carried word
static const uint32_t kDfwTooFar = 4096;             // a 3-byte match farther back costs more than its literals (zlib's TOO_FAR)
static const int kDfwMaxEffort = 3;
// table candidates tried per position: one at effort 0, a chain of 4, 8, 16 at efforts 1, 2, 3
PSVR_IF constexpr uint32_t dfw_depth(int effort) { return effort > 0 ? 2u << effort : 1u; }

struct DfwLds {
	union {
		struct {                                     // phase 1
			uint32_t head[1 << kDfwHashBits];        // position + 1 of the last entry per hash, 0 = none
			uint16_t glen[64], gdist[64], ghash[64]; // per position of the group: match length (0 = none), distance - 1, hash (0xffff = none)
			uint8_t gbyte[64];
		} z;
		struct {                                     // phases 2-4
			uint32_t code[kDfLit + kDfDist];         // code | length << 16, bit-reversed (df_codes)
			uint16_t S[kDfLit], A[kDfLit];
			uint32_t win[kDfwWindow];
			uint64_t tbits[64];
			uint32_t tlen[64];
			uint32_t crc_tab[256];
			uint32_t red[64];
			uint32_t work[33 + 32];                  // df_lengths_sorted's and df_codes' counters
		} e;
	};
	uint32_t freq[kDfLit + kDfDist];
	uint8_t len[kDfLit + kDfDist + 4];
	uint32_t acc[4];
};

// bytes of a member's slot (its size rounded up to whole dwords: the bit string leaves in dwords) and of the largest member
PSVR_IF uint32_t dfw_member_max(uint32_t n) { return n + 31u; }                                  // 18 + stored block (5 + n) + 8
PSVR_IF uint32_t dfw_slot_bytes(uint32_t n) { return (dfw_member_max(n) + 3u + 63u) & ~63u; }

// ---- the cross-lane steps: wavefront on the device, a loop on the host ---------------------------------------------------------------------
#if defined(__HIP_DEVICE_COMPILE__)
PSVR_IF void dfw_add(uint32_t *p, uint32_t v) { __hip_atomic_fetch_add(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP); }
PSVR_IF void dfw_or(uint32_t *p, uint32_t v) { __hip_atomic_fetch_or(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP); }
PSVR_IF void dfw_max(uint32_t *p, uint32_t v) { __hip_atomic_fetch_max(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP); }
PSVR_IF uint32_t dfw_popc64(uint64_t x) { return (uint32_t)__popcll((unsigned long long)x); }
// bit k = (a[k] >= 3), k < cnt
PSVR_IF uint64_t dfw_ballot_match(const uint16_t *a, uint32_t cnt, int lane) { return (uint64_t)__ballot((uint32_t)lane < cnt && a[lane] >= 3); }
// a[i] for a wave-uniform i: the lane's own entry handed round
PSVR_IF uint32_t dfw_own(const uint16_t *a, int lane) { return a[lane]; }
PSVR_IF uint32_t dfw_pick(const uint16_t *, uint32_t own, uint32_t i) { return (uint32_t)__builtin_amdgcn_readlane((int)own, (int)INF_UNI(i)); }
// a[0..64) becomes its exclusive prefix sum; returns the total
PSVR_IF uint32_t dfw_scan64(uint32_t *a, int lane)
{
	const uint32_t v = a[lane];
	uint32_t s = v;
	for (int d = 1; d < 64; d <<= 1) { const uint32_t t = (uint32_t)__shfl_up((int)s, d, 64); if (lane >= d) s += t; }
	a[lane] = s - v;
	return (uint32_t)__builtin_amdgcn_readlane((int)s, 63);
}
#else
PSVR_IF void dfw_add(uint32_t *p, uint32_t v) { *p += v; }
PSVR_IF void dfw_or(uint32_t *p, uint32_t v) { *p |= v; }
PSVR_IF void dfw_max(uint32_t *p, uint32_t v) { if (v > *p) *p = v; }
PSVR_IF uint32_t dfw_popc64(uint64_t x) { return (uint32_t)__builtin_popcountll(x); }
PSVR_IF uint64_t dfw_ballot_match(const uint16_t *a, uint32_t cnt, int) { uint64_t m = 0; for (uint32_t k = 0; k < cnt; ++k) m |= (uint64_t)(a[k] >= 3) << k; return m; }
PSVR_IF uint32_t dfw_own(const uint16_t *, int) { return 0; }
PSVR_IF uint32_t dfw_pick(const uint16_t *a, uint32_t, uint32_t i) { return a[i]; }
PSVR_IF uint32_t dfw_scan64(uint32_t *a, int) { uint32_t s = 0; for (int k = 0; k < 64; ++k) { const uint32_t v = a[k]; a[k] = s, s += v; } return s; }
#endif

// extra bits of a literal/length symbol and of a distance symbol; the fixed code's lengths (RFC 1951 3.2.5, 3.2.6)
PSVR_IF uint32_t dfw_lit_extra(uint32_t s) { return s < 265u || s == 285u ? 0u : (s - 261u) >> 2; }
PSVR_IF uint32_t dfw_dist_extra(uint32_t d) { return d < 4u ? 0u : (d >> 1) - 1u; }
PSVR_IF uint32_t dfw_fixed_len(uint32_t i) { return i < 144u ? 8u : i < 256u ? 9u : i < 280u ? 7u : i < (uint32_t)kDfLit ? 8u : 5u; }   // i >= kDfLit: a distance

// the emission window: a bit string whose word `wbase` of the slot is win[0]
struct DfwOut {
	uint32_t *slot, *win;
	uint32_t wbase, bp;                              // first word not yet stored; the next free bit of the member
	// `v` (at most 48 bits) at bit `at` of the member: into three words at most, zero words are not touched
	PSVR_IF void put(uint32_t at, uint64_t v) const
	{
		const uint32_t w = (at >> 5) - wbase, sh = at & 31u;
		const uint64_t rest = (v >> 1) >> (31u - sh);
		const uint32_t a = (uint32_t)(v << sh), b = (uint32_t)rest, c = (uint32_t)(rest >> 32);
		if (a) dfw_or(win + w, a);
		if (b) dfw_or(win + w + 1, b);
		if (c) dfw_or(win + w + 2, c);
	}
	// the complete words leave (every word that holds a bit, when `all`), the begun one becomes win[0]
	template <int NL>
	PSVR_IF void flush(bool all, int lane)
	{
		inf_sync();
		const uint32_t nw = ((all ? bp + 31u : bp) >> 5) - wbase;
		for (uint32_t i = (uint32_t)lane; i < nw; i += NL) slot[wbase + i] = win[i];
		const uint32_t part = all ? 0u : INF_UNI(win[nw]);
		inf_sync();
		for (uint32_t i = (uint32_t)lane; i <= nw && i < kDfwWindow; i += NL) win[i] = i ? 0u : part;
		wbase += nw;
		inf_sync();
	}
};

// code lengths and codes of the n symbols with the frequencies f[] (phase 2)
template <int NL>
PSVR_IF void dfw_build_code(const uint32_t *f, int n, uint8_t *len, uint32_t *code, DfwLds *t, int lane)
{
	uint16_t *S = t->e.S, *A = t->e.A;
	inf_sync();
	if (lane == 0) t->acc[0] = 0;
	inf_sync();
	{
		uint32_t used = 0;
		for (int i = lane; i < n; i += NL) used += f[i] != 0;
		if (used) dfw_add(&t->acc[0], used);
	}
	inf_sync();
	int m = (int)INF_UNI(t->acc[0]);
	// at least two symbols get a code (deflate_device.h): the first unused ones count as seen once
	int f0 = -1, f1 = -1;
	for (int i = 0; m < 2 && i < n; ++i) if (!INF_UNI(f[i])) { if (f0 < 0) f0 = i; else f1 = i; ++m; }
	auto key = [&](int i) { const uint32_t v = f[i]; return v ? v : (i == f0 || i == f1) ? 1u : 0u; };
	for (int i = lane; i < n; i += NL) {
		len[i] = 0;
		const uint32_t fi = key(i);
		if (!fi) continue;
		uint32_t r = 0;
		for (int j = 0; j < n; ++j) { const uint32_t fj = key(j); r += fj && (fj < fi || (fj == fi && j < i)); }
		S[r] = (uint16_t)i, A[r] = (uint16_t)fi;                               // (a member's symbols number at most 65281: the sums fit)
	}
	inf_sync();
	if (lane == 0) {
		df_lengths_sorted(m, 15, len, A, S, (int *)t->e.work);
		df_codes(len, n, code, t->e.work + 33, t->e.work + 49);
	}
	inf_sync();
}

// One member: in[0, n), 1 <= n <= 0xff00, into slot[0, dfw_slot_bytes(n)) (dword aligned); tok: n + 1 words of scratch; link: n half-words of
// scratch when EFFORT > 0, not touched (and may be null) at effort 0.  Returns the member's size; every lane returns the same.
template <int NL, int EFFORT>
PSVR_IF uint32_t dfw_member_effort(const uint8_t *in, uint32_t n, uint8_t *slot, uint32_t *tok, uint16_t *link, DfwLds *t, int lane)
{
#if defined(__HIP_DEVICE_COMPILE__)
	static_assert(NL == 64, "a wavefront");
#endif
	static_assert(EFFORT >= 0 && EFFORT <= kDfwMaxEffort, "effort 0..3");
	constexpr uint32_t depth = dfw_depth(EFFORT);
	constexpr bool lazy = EFFORT > 0;
	const uint32_t hmask = (1u << kDfwHashBits) - 1u;
	auto ld32 = [&](uint32_t p) { uint32_t v; __builtin_memcpy(&v, in + p, 4); return v; };                   // p + 4 <= n
	for (uint32_t i = (uint32_t)lane; i <= hmask; i += NL) t->z.head[i] = 0;
	for (uint32_t i = (uint32_t)lane; i < (uint32_t)(kDfLit + kDfDist); i += NL) t->freq[i] = 0;
	inf_sync();
	// ---- 1: LZ77 ---------------------------------------------------------------------------------------------------------------------------
	uint32_t nt = 0, carry = 0;                                                // tokens so far; positions of the group a match from before covers
	for (uint32_t g = 0; g < n; g += 64) {
		const uint32_t cnt = n - g < 64u ? n - g : 64u;
		for (uint32_t k = (uint32_t)lane; k < cnt; k += NL) {
			const uint32_t p = g + k;
			uint32_t best = 0, bdist = 0, h = 0xffffu, byte;
			if (p + 4 <= n) {
				const uint32_t cur = ld32(p);
				byte = cur & 0xffu;
				h = ((cur & 0xffffffu) * 0x9E3779B1u >> (32 - kDfwHashBits)) & hmask;
				uint32_t c = 0;
				if (lazy) c = t->z.head[h], link[p] = (uint16_t)c;                 // the chain behind p: covered positions enter the table too
				if (k >= carry) {
					const uint32_t lim = n - p < 258u ? n - p : 258u;
					if (!lazy) c = t->z.head[h];
					// the fixed distances, then the chain, nearest first: c > link[c - 1] > ..., `depth` entries at most
					for (uint32_t j = 0; j < kDfwNear + depth; ++j) {
						uint32_t d;
						if (j < kDfwNear) { d = j + 1; if (d > p) continue; }
						else if (!lazy) { if (!c) continue; d = p + 1 - c; if (d > 32768u || d <= kDfwNear) continue; }   // (effort 0 keeps the form its code was measured in)
						else {
							if (!c) break;
							d = p + 1 - c;
							if (d > 32768u) break;
							c = j + 1 < kDfwNear + depth ? link[c - 1] : 0u;       // (entered the table, so it wrote its link: c - 1 < p)
							if (d <= kDfwNear) continue;
						}
						const uint32_t cp = p - d;
						if ((ld32(cp) ^ cur) & 0xffffffu) continue;
						uint32_t l = 3;
						while (l + 4 <= lim) {
							const uint32_t x = ld32(cp + l) ^ ld32(p + l);
							if (x) { l += df_ctz64(x) >> 3; break; }
							l += 4;
						}
						if (l + 4 > lim) while (l < lim && in[cp + l] == in[p + l]) ++l;
						if (l > best && !(l == 3 && d > kDfwTooFar)) best = l, bdist = d;
					}
				}
			} else byte = in[p];                                               // (the last three bytes of a member go out as literals)
			t->z.glen[k] = (uint16_t)best, t->z.gdist[k] = (uint16_t)(bdist - 1u), t->z.ghash[k] = (uint16_t)h, t->z.gbyte[k] = (uint8_t)byte;
		}
		inf_sync();
		// the token starts of the group: wave-uniform, a step per match and per run of literals
		uint64_t start = 0, demoted = 0;                                       // (demoted: a match that goes out as a literal, the next position's is longer)
		uint32_t cur = carry;
		if (cur < cnt) {
			const uint64_t mask = dfw_ballot_match(t->z.glen, cnt, lane);
			const uint32_t own = dfw_own(t->z.glen, lane);
			while (cur < cnt) {
				const uint64_t rest = mask >> cur;
				if (rest & 1u) {
					const uint32_t l = dfw_pick(t->z.glen, own, cur);
					start |= 1ull << cur;
					if (lazy && (rest & 2u) && dfw_pick(t->z.glen, own, cur + 1) > l) demoted |= 1ull << cur, cur += 1;
					else cur += l;
				}
				else {
					const uint32_t run = rest ? df_ctz64(rest) : cnt - cur;
					start |= (run >= 64u ? ~0ull : (1ull << run) - 1ull) << cur;
					cur += run;
				}
			}
		}
		carry = cur - cnt;
		for (uint32_t k = (uint32_t)lane; k < cnt; k += NL) {
			const uint32_t h = t->z.ghash[k];
			if (h != 0xffffu) dfw_max(&t->z.head[h], g + k + 1u);
			if (!(start >> k & 1u)) continue;
			const uint32_t at = nt + dfw_popc64(start & ((1ull << k) - 1ull));
			const uint32_t l = t->z.glen[k];
			if (l >= 3 && !(lazy && (demoted >> k & 1u))) {
				const uint32_t d1 = t->z.gdist[k];
				uint32_t s, d, eb, ev;
				df_len_code(l, s, eb, ev);
				df_dist_code(d1 + 1u, d, eb, ev);
				tok[at] = 0x80000000u | (l - 3u) << 16 | d1;
				dfw_add(&t->freq[s], 1), dfw_add(&t->freq[kDfLit + d], 1);
			} else {
				const uint32_t b = t->z.gbyte[k];
				tok[at] = b;
				dfw_add(&t->freq[b], 1);
			}
		}
		nt += dfw_popc64(start);
		if (lazy) inf_fence();                                                 // the links are read by other lanes, in later groups
		inf_sync();
	}
	if (lane == 0) tok[nt] = 0x40000100u, t->freq[256] = 1;                    // end of block, a token like the others
	++nt;
	inf_fence();                                                               // the tokens are read back by other lanes
	inf_sync();
	// ---- 2: code lengths and codes -------------------------------------------------------------------------------------------------------------
	uint32_t *lc = t->e.code, *dc = lc + kDfLit;
	uint8_t *ll = t->len, *dl = ll + kDfLit;
	dfw_build_code<NL>(t->freq, kDfLit, ll, lc, t, lane);
	dfw_build_code<NL>(t->freq + kDfLit, kDfDist, dl, dc, t, lane);
	inf_crc_table<NL>(t->e.crc_tab, lane);
	const uint32_t crc = inf_crc32<NL>(in, n, t->e.crc_tab, t->e.red, lane);
	// ---- 3: the three sizes, in bits ---------------------------------------------------------------------------------------------------------------
	if (lane == 0) t->acc[0] = 0, t->acc[1] = 0, t->acc[2] = 257, t->acc[3] = 1;
	inf_sync();
	{
		uint32_t dyn = 0, fix = 0, nl = 0, nd = 0;
		for (uint32_t i = (uint32_t)lane; i < (uint32_t)(kDfLit + kDfDist); i += NL) {
			const uint32_t f = t->freq[i], x = i < (uint32_t)kDfLit ? dfw_lit_extra(i) : dfw_dist_extra(i - kDfLit);
			dyn += f * (t->len[i] + x), fix += f * (dfw_fixed_len(i) + x);
			if (t->len[i]) { if (i < (uint32_t)kDfLit) nl = i + 1; else nd = i - kDfLit + 1; }
		}
		dfw_add(&t->acc[0], dyn), dfw_add(&t->acc[1], fix), dfw_max(&t->acc[2], nl), dfw_max(&t->acc[3], nd);
	}
	inf_sync();
	const uint32_t nl = INF_UNI(t->acc[2]), nd = INF_UNI(t->acc[3]);
	const uint32_t hdr_bits = 3 + 14 + 19 * 3 + 4 * (nl + nd);
	const uint32_t dyn_bytes = (hdr_bits + INF_UNI(t->acc[0]) + 7u) >> 3, fix_bytes = (3u + INF_UNI(t->acc[1]) + 7u) >> 3, sto_bytes = n + 5u;
	const int mode = dyn_bytes <= fix_bytes && dyn_bytes < sto_bytes ? 2 : fix_bytes < sto_bytes ? 1 : 0;
	const uint32_t payload = mode == 2 ? dyn_bytes : mode == 1 ? fix_bytes : sto_bytes;
	const uint32_t size = 18u + payload + 8u, bsize = size - 1u;
	auto hdr_byte = [&](uint32_t i) -> uint32_t {                              // gzip header with the BC extra field (BSIZE = member size - 1)
		return i == 0 ? 0x1fu : i == 1 ? 0x8bu : i == 2 ? 8u : i == 3 ? 4u : i == 9 ? 0xffu : i == 10 ? 6u : i == 12 ? 'B' : i == 13 ? 'C' : i == 14 ? 2u
		     : i == 16 ? (bsize & 0xffu) : i == 17 ? bsize >> 8 : 0u;
	};
	if (mode == 0) {                                                           // stored: BFINAL = 1, BTYPE = 00, LEN, ~LEN, the bytes
		for (uint32_t i = (uint32_t)lane; i < 18; i += NL) slot[i] = (uint8_t)hdr_byte(i);
		for (uint32_t i = (uint32_t)lane; i < 5; i += NL) slot[18 + i] = (uint8_t)(i == 0 ? 1u : i == 1 ? n : i == 2 ? n >> 8 : i == 3 ? ~n : ~n >> 8);
		for (uint32_t i = (uint32_t)lane; i < n; i += NL) slot[23 + i] = in[i];
		for (uint32_t i = (uint32_t)lane; i < 8; i += NL) slot[23 + n + i] = (uint8_t)((i < 4 ? crc : n) >> (8 * (i & 3u)));
		return size;
	}
	// ---- 4: emission ----------------------------------------------------------------------------------------------------------------------------
	if (mode == 1) {                                                           // the fixed code (RFC 1951 3.2.6) in the same table
		inf_sync();
		for (uint32_t i = (uint32_t)lane; i < (uint32_t)(kDfLit + kDfDist); i += NL) {
			const uint32_t l = dfw_fixed_len(i);
			const uint32_t v = i < 144u ? 0x30u + i : i < 256u ? 0x190u + (i - 144u) : i < 280u ? i - 256u : i < (uint32_t)kDfLit ? 0xc0u + (i - 280u) : i - kDfLit;
			uint32_t r = 0;
			for (uint32_t b = 0; b < l; ++b) r |= ((v >> b) & 1u) << (l - 1u - b);
			lc[i] = r | l << 16;
		}
	}
	DfwOut o;
	o.slot = (uint32_t *)slot, o.win = t->e.win, o.wbase = 0, o.bp = 0;
	inf_sync();
	for (uint32_t i = (uint32_t)lane; i < kDfwWindow; i += NL) o.win[i] = 0;
	inf_sync();
	for (uint32_t i = (uint32_t)lane; i < 18; i += NL) o.put(8 * i, hdr_byte(i));
	o.bp = 144;
	if (mode == 2) {
		// BFINAL, BTYPE = dynamic; HLIT, HDIST, HCLEN = 15: all 19 code-length codes in their order 16 17 18 0 8 7 ...: 16..18 unused, 0..15 four bits
		// each, whose canonical codes are the values themselves (sent bit-reversed)
		const uint32_t at = o.bp;
		if (lane == 0) o.put(at, 1u | 2u << 1 | (uint64_t)(nl - 257u) << 3 | (uint64_t)(nd - 1u) << 8 | 15ull << 13);
		for (uint32_t i = (uint32_t)lane; i < 19; i += NL) if (i >= 3) o.put(at + 17 + 3 * i, 4);
		for (uint32_t i = (uint32_t)lane; i < nl + nd; i += NL) {
			const uint32_t v = i < nl ? ll[i] : dl[i - nl];
			o.put(at + 74 + 4 * i, ((v & 1) << 3) | ((v & 2) << 1) | ((v & 4) >> 1) | ((v & 8) >> 3));
		}
		o.bp = at + hdr_bits;
	} else {
		if (lane == 0) o.put(o.bp, 1u | 1u << 1);
		o.bp += 3;
	}
	o.template flush<NL>(false, lane);
	for (uint32_t t0 = 0; t0 < nt; t0 += 64) {
		for (uint32_t k = (uint32_t)lane; k < 64; k += NL) {
			uint64_t v = 0;
			uint32_t nb = 0;
			if (t0 + k < nt) {
				const uint32_t x = tok[t0 + k];
				if (!(x & 0x80000000u)) { const uint32_t c = lc[x & 0x1ffu]; v = c & 0xffffu, nb = c >> 16; }
				else {
					uint32_t s, eb, ev;
					df_len_code(((x >> 16) & 0xff) + 3, s, eb, ev);
					uint32_t c = lc[s];
					v = c & 0xffffu, nb = c >> 16;
					v |= (uint64_t)ev << nb, nb += eb;
					df_dist_code((x & 0xffff) + 1, s, eb, ev);
					c = dc[s];
					v |= (uint64_t)(c & 0xffffu) << nb, nb += c >> 16;
					v |= (uint64_t)ev << nb, nb += eb;
				}
			}
			t->e.tbits[k] = v, t->e.tlen[k] = nb;
		}
		inf_sync();
		const uint32_t total = dfw_scan64(t->e.tlen, lane);
		inf_sync();
		for (uint32_t k = (uint32_t)lane; k < 64; k += NL) if (t->e.tbits[k]) o.put(o.bp + t->e.tlen[k], t->e.tbits[k]);
		o.bp += total;
		o.template flush<NL>(false, lane);
	}
	o.bp = (o.bp + 7u) & ~7u;
	for (uint32_t i = (uint32_t)lane; i < 2; i += NL) o.put(o.bp + 32 * i, i ? n : crc);
	o.bp += 64;
	o.template flush<NL>(true, lane);
	return o.bp >> 3;                                                          // (= size: the sizes of phase 3 are exact)
}

// effort 0: one table candidate, no chain, no look-ahead, no link scratch
template <int NL>
PSVR_IF uint32_t dfw_member(const uint8_t *in, uint32_t n, uint8_t *slot, uint32_t *tok, DfwLds *t, int lane)
{
	return dfw_member_effort<NL, 0>(in, n, slot, tok, nullptr, t, lane);
}

} // namespace psvr
