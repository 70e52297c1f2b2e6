// inflate_device.h -- one BGZF member (RFC 1951 inside RFC 1952, SAMv1 4.1) decoded by ONE WAVEFRONT: the body of k_bgzf_inflate
// (inflate.hip: a wavefront per member, the thousands of members of a batch side by side) and, compiled for the host with one "lane", of
// the checker that runs zlib-made and deliberately broken streams through the very same code under AddressSanitizer
// (tests/tools/inflate_check.cpp).  The counterpart of deflate_device.h; htslib inflates a member with zlib on the calling thread
// (bgzf.c: bgzf_read_block -> inflate_block), and so does bam_reader.h's serial route.
//   * the phases are written for NL lanes (`for (i = lane; i < n; i += NL)`), NL = 64 on the device and 1 on the host, with inf_sync()
//     between phases (empty on the host);
//   * the bit reader, the block headers and the symbol chain are wave-uniform: every lane carries the same state (the values go through
//     a read-first-lane, so the compiler keeps them in scalar registers and branches on them without masks);
//   * decoding tables, in the wavefront's InfLds (5.3 KB of LDS): per code the counts per length and the symbols in canonical order
//     (puff's decoder: the fallback for long codes), and a direct table over the next 10 (literal/length), 8 (distance) or 7 (code
//     lengths) bits that the lanes fill together, each entry by decoding its own index canonically;
//   * output: literals wait in a register of "their" lane (the k-th pending literal in lane k) and go out 64 at a time as one coalesced
//     store; a match is copied by the lanes together (distance < length: byte i = source byte i mod distance) straight from the
//     member's own output slice in global memory.  A match whose source was stored since the last wait first waits for those stores
//     (inf_fence: the window is the output itself, no ring in LDS);
//   * CRC32: a slice per lane from a table in LDS, the slices combined with x^(8 * bytes behind the slice) mod P (zlib's crc32_combine);
//   * malformed input is a status.  No load leaves [member, member + bsize), no store leaves out[0, isize); every loop consumes input
//     bits or is bounded by a table size.  The verdict is zlib's: accepted exactly when raw inflate of the payload reaches the end of the
//     stream having produced ISIZE bytes whose CRC32 is the trailer's (bytes between the end of the stream and the trailer are tolerated).
//     Which status a refused member gets is the first rule it breaks in stream order, and the trailer is looked at last.  Where one token
//     breaks two rules the order is: the input before the output (a stored block longer than what is left is kInfTruncated even when
//     ISIZE is too small for it as well); a code that cannot be told apart from one the payload's end cut off -- no code matches, fewer
//     than 15 bits are left and none follow -- is kInfTruncated, not kInfLitCode / kInfDistCode / kInfCodeLengths; a match is held to
//     the bytes in front of it before it is held to the room behind it (kInfFarBack before kInfTooLong).  tests/inflate_cases.py
//     holds every rule to its status.
#pragma once
#include <stdint.h>
#include <string.h>

#if defined(__HIPCC__)
#define PSVR_IF __host__ __device__ inline
#else
#define PSVR_IF inline
#endif

namespace psvr {

enum {                                   // a member's status
	kInfOk = 0,
	kInfHeader = 1,                      // the gzip header is not a BGZF one (bgzf_member_header)
	kInfBlockType = 2,                   // BTYPE 3
	kInfStored = 3,                      // LEN != ~NLEN
	kInfTruncated = 4,                   // the payload ends inside the stream (also: a stored block longer than what is left)
	kInfCounts = 5,                      // HLIT > 286 or HDIST > 30
	kInfCodeLengths = 6,                 // the code-length code, a repeat without a previous length or past the end
	kInfNoEob = 7,                       // no code for the end-of-block symbol
	kInfLitTable = 8,                    // over-subscribed or incomplete literal/length code
	kInfDistTable = 9,                   // the same for the distance code (a single 1-bit code is accepted, as zlib does)
	kInfLitCode = 10,                    // an unassigned code, symbol 286 or 287
	kInfDistCode = 11,                   // an unassigned code, symbol 30 or 31
	kInfFarBack = 12,                    // a distance that reaches in front of the member's first byte
	kInfTooLong = 13,                    // more output than ISIZE
	kInfTooShort = 14,                   // less
	kInfCrc = 15,
};

static const int kInfLitBits = 10, kInfDistBits = 8, kInfClBits = 7;

struct InfLds {                          // one wavefront's tables
	uint16_t lut_l[1 << kInfLitBits];    // symbol | length << 9; 0 = a longer code, or none
	uint16_t lut_d[1 << kInfDistBits];
	uint16_t lut_c[1 << kInfClBits];
	uint16_t sym_l[288], sym_d[32], sym_c[20];
	uint16_t cnt_l[16], cnt_d[16], cnt_c[16];
	uint8_t lens[320];                   // literal/length lengths, then the distance lengths (a run may cross from one into the other)
	uint32_t crc_tab[256];
	uint32_t red[64];
};

#if defined(__HIP_DEVICE_COMPILE__)
#define INF_UNI(x) ((uint32_t)__builtin_amdgcn_readfirstlane((int)(x)))
PSVR_IF void inf_sync() { __syncthreads(); }                                                   // (a workgroup is one wavefront)
// the stores of this wavefront so far are visible to the loads that follow, whichever lane issues them: a workgroup-scope release/acquire
// and the wait for the outstanding stores spelled out (with 64 threads per workgroup the compiler may treat the scope as one wavefront's)
PSVR_IF void inf_fence()
{
	__builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
	asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
	__builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
}
#else
#define INF_UNI(x) ((uint32_t)(x))
PSVR_IF void inf_sync() {}
PSVR_IF void inf_fence() {}
#endif

// The header rules of bam_reader.h's next_block(): magic, CM = 8, FEXTRA, a BC subfield of length 2 anywhere in the extra field (the last
// one counts), BSIZE large enough for header and trailer.  0: *bsize (the member's size) and *xlen are set; 1: `avail` bytes are not enough
// to tell (fewer than 18, or the extra field is cut off); 2: not a BGZF member.
PSVR_IF int bgzf_member_header(const uint8_t *p, uint64_t avail, uint32_t *bsize, uint32_t *xlen)
{
	if (avail < 18) return 1;
	if (p[0] != 0x1f || p[1] != 0x8b || p[2] != 8 || !(p[3] & 4)) return 2;
	const uint32_t xl = p[10] | (uint32_t)p[11] << 8;
	if (avail < 12 + (uint64_t)xl) return 1;
	uint32_t bs = 0;
	for (uint32_t o = 0; o + 4 <= xl;) {
		const uint8_t *e = p + 12 + o;
		const uint32_t slen = e[2] | (uint32_t)e[3] << 8;
		if (e[0] == 'B' && e[1] == 'C' && slen == 2 && o + 6 <= xl) bs = (e[4] | (uint32_t)e[5] << 8) + 1;
		o += 4 + slen;
	}
	if (bs < 12 + xl + 8) return 2;
	*bsize = bs, *xlen = xl;
	return 0;
}

// ---- CRC32 arithmetic (reflected, P = 0xEDB88320): a(x) * b(x) mod P, and x^(8 n) mod P -------------------------------------------------
PSVR_IF uint32_t inf_mulmod(uint32_t a, uint32_t b)
{
	uint32_t p = 0;
	for (int i = 0; i < 32; ++i) {                                                              // (no early exit: the lanes stay together)
		p ^= (a & (0x80000000u >> i)) ? b : 0u;
		b = (b & 1u) ? (b >> 1) ^ 0xEDB88320u : b >> 1;
	}
	return p;
}
PSVR_IF uint32_t inf_xpow8(uint32_t n)
{
	uint32_t p = 0x80000000u, b = 0x00800000u;                                                  // x^0, x^8
	for (; n; n >>= 1) {
		if (n & 1u) p = inf_mulmod(p, b);
		b = inf_mulmod(b, b);
	}
	return p;
}

// the byte table of the reflected CRC32 (a sync of the caller's comes before its first reader)
template <int NL>
PSVR_IF void inf_crc_table(uint32_t *crc_tab, int lane)
{
	for (int i = lane; i < 256; i += NL) {
		uint32_t c = (uint32_t)i;
		for (int k = 0; k < 8; ++k) c = (c & 1u) ? 0xEDB88320u ^ (c >> 1) : c >> 1;
		crc_tab[i] = c;
	}
}
// CRC32 of p[0, n) by the wavefront (shared with deflate_wave_device.h): lane k takes p[k * slice, (k + 1) * slice), the slices' CRCs are
// moved to the end and added.  crc_tab: inf_crc_table's; red: 64 words.  Every lane returns the same value.  Always inlined: with several
// kernels of one file calling it (deflate_wave.hip has one per effort) the compiler otherwise keeps it out of line, a call and two registers
// per kernel.
template <int NL>
__attribute__((always_inline)) PSVR_IF uint32_t inf_crc32(const uint8_t *p, uint32_t n, const uint32_t *crc_tab, uint32_t *red, int lane)
{
	inf_sync();
	const uint32_t slice = (n + 63u) / 64u;
	for (int k = lane; k < 64; k += NL) {                                                       // (64 slices on the host too: the same arithmetic)
		const uint32_t lo = (uint32_t)k * slice < n ? (uint32_t)k * slice : n;
		const uint32_t hi = lo + slice < n ? lo + slice : n;
		uint32_t c = 0xffffffffu;
		for (uint32_t i = lo; i < hi; ++i) c = crc_tab[(c ^ p[i]) & 0xffu] ^ (c >> 8);
		red[k] = hi > lo ? inf_mulmod(inf_xpow8(n - hi), ~c) : 0u;
	}
	inf_sync();
	uint32_t crc = 0;
	for (int i = 0; i < 64; ++i) crc ^= red[i];
	return INF_UNI(crc);
}

// ---- canonical codes ---------------------------------------------------------------------------------------------------------------------
// the symbol whose code starts the bit string v (first bit = bit 0), among the codes of at most `maxlen` bits (puff.c's decode())
PSVR_IF bool inf_canon(const uint16_t *cnt, const uint16_t *sym, uint32_t v, int maxlen, uint32_t &s, uint32_t &l)
{
	int32_t code = 0, first = 0, index = 0;
	for (int len = 1; len <= maxlen; ++len) {
		code |= (int32_t)(v & 1u), v >>= 1;
		const int32_t c = cnt[len];
		if (code - c < first) { s = sym[index + (code - first)], l = (uint32_t)len; return true; }
		index += c, first += c, first <<= 1, code <<= 1;
	}
	return false;
}
// cnt / sym / lut of the n code lengths in len[]; 0: complete, 1: over-subscribed, 2: incomplete (*maxlen: the longest code, 0 = none)
template <int NL>
PSVR_IF int inf_build(const uint8_t *len, int n, uint16_t *cnt, uint16_t *sym, uint16_t *lut, int lutbits, int lane, int *maxlen)
{
	inf_sync();                                                                                 // len[] is written, the tables' last readers are through
	for (int l = lane; l < 16; l += NL) {
		uint32_t c = 0;
		for (int i = 0; i < n; ++i) c += len[i] == l;
		cnt[l] = (uint16_t)c;
	}
	inf_sync();
	int left = 1, mx = 0;
	bool over = false;
	for (int l = 1; l < 16; ++l) {
		const int c = (int)INF_UNI(cnt[l]);
		left = (left << 1) - c;
		over |= left < 0;
		if (over) left = 0;
		if (c) mx = l;
	}
	*maxlen = mx;
	if (over) return 1;
	for (int l = lane + 1; l < 16; l += NL) {
		uint32_t k = 0;
		for (int j = 1; j < l; ++j) k += cnt[j];
		for (int i = 0; i < n; ++i) if (len[i] == l) sym[k++] = (uint16_t)i;
	}
	inf_sync();
	for (int k = lane; k < (1 << lutbits); k += NL) {
		uint32_t s = 0, l = 0;
		lut[k] = inf_canon(cnt, sym, (uint32_t)k, lutbits, s, l) ? (uint16_t)(s | l << 9) : (uint16_t)0;
	}
	inf_sync();
	return left > 0 ? 2 : 0;
}

// ---- bits --------------------------------------------------------------------------------------------------------------------------------
struct InfBits {                          // LSB-first reader over base[pos, end): aligned dwords, bytes at the two ends
	const uint8_t *base;
	uint32_t pos, end;
	uint64_t acc;
	uint32_t n;
	PSVR_IF void refill()                 // at least 33 bits afterwards unless the input ends
	{
		while (n <= 32) {
			if (pos + 4 <= end && (((uintptr_t)(base + pos)) & 3u) == 0) {
				uint32_t w;
				__builtin_memcpy(&w, base + pos, 4);
				acc |= (uint64_t)INF_UNI(w) << n, n += 32, pos += 4;
			} else if (pos < end) {
				acc |= (uint64_t)INF_UNI(base[pos]) << n, n += 8, pos += 1;
			} else break;
		}
	}
	PSVR_IF uint32_t peek(uint32_t k) const { return (uint32_t)acc & ((1u << k) - 1u); }       // k <= 16 (absent bits read as 0)
	PSVR_IF void drop(uint32_t k) { acc >>= k, n -= k; }
};

// a code of the table (lut, cnt, sym): false = unassigned, or the input ends inside it
PSVR_IF bool inf_symbol(InfBits &b, const uint16_t *lut, int lutbits, const uint16_t *cnt, const uint16_t *sym, uint32_t &s)
{
	const uint32_t e = INF_UNI(lut[b.peek((uint32_t)lutbits)]);
	uint32_t l = e >> 9;
	s = e & 511u;
	if (!e) {
		uint32_t s2 = 0, l2 = 0;
		const bool ok = inf_canon(cnt, sym, b.peek(15), 15, s2, l2);
		s = INF_UNI(s2), l = INF_UNI(l2);
		if (!INF_UNI(ok)) return false;
	}
	if (l > b.n) return false;
	b.drop(l);
	return true;
}

// ---- output ------------------------------------------------------------------------------------------------------------------------------
template <int NL>
struct InfOut {
	uint8_t *out;
	uint32_t o, isize;                    // bytes produced (the pending literals included), the slice's size
	uint32_t npend, clean;                // literals waiting in the lanes; out[0, clean) has been waited for
	uint32_t mine;
	int lane;
	PSVR_IF void flush()
	{
		if ((uint32_t)lane < npend) out[o - npend + (uint32_t)lane] = (uint8_t)mine;
		npend = 0;
	}
	PSVR_IF void literal(uint32_t v)      // o < isize is the caller's check
	{
		if ((uint32_t)lane == npend) mine = v;
		++npend, ++o;
		if (npend == (uint32_t)NL) flush();
	}
	PSVR_IF void match(uint32_t len, uint32_t dist)   // dist <= o, o + len <= isize
	{
		flush();
		const uint32_t span = len < dist ? len : dist;
		if (o - dist + span > clean) { inf_fence(); clean = o; }
		const uint8_t *src = out + (o - dist);
		uint8_t *dst = out + o;
		if (dist >= len) { for (uint32_t i = (uint32_t)lane; i < len; i += NL) dst[i] = src[i]; }
		else if (dist == 1) { const uint8_t v = src[0]; for (uint32_t i = (uint32_t)lane; i < len; i += NL) dst[i] = v; }
		else { for (uint32_t i = (uint32_t)lane; i < len; i += NL) dst[i] = src[i % dist]; }
		o += len;
	}
};

// an ISIZE no payload of `clen` bytes can reach (a match of 258 bytes costs two bits at least): refused before anything is laid out for it
PSVR_IF bool inf_isize_possible(uint32_t isize, uint32_t clen) { return (uint64_t)isize <= 1032ull * clen; }

// One member: member[0, bsize) with the payload behind its first `hdr` (= 12 + XLEN) bytes, inflated into out[0, isize) -- isize is the
// slice the caller laid out for it from the trailer's ISIZE, which is compared again here.  Every lane returns the same status.
template <int NL>
PSVR_IF int inf_member(const uint8_t *member, uint32_t bsize, uint32_t hdr, uint8_t *out, uint32_t isize, InfLds *t, int lane)
{
	if (bsize < hdr + 8u || hdr < 12u) return kInfHeader;
	const uint8_t *tr = member + bsize - 8;
	const uint32_t want_crc = tr[0] | (uint32_t)tr[1] << 8 | (uint32_t)tr[2] << 16 | (uint32_t)tr[3] << 24;
	const uint32_t want_n = tr[4] | (uint32_t)tr[5] << 8 | (uint32_t)tr[6] << 16 | (uint32_t)tr[7] << 24;
	inf_crc_table<NL>(t->crc_tab, lane);
	InfBits b;
	b.base = member, b.pos = hdr, b.end = bsize - 8, b.acc = 0, b.n = 0;
	InfOut<NL> w;
	w.out = out, w.o = 0, w.isize = isize, w.npend = 0, w.clean = 0, w.mine = 0, w.lane = lane;
	for (bool last = false; !last;) {
		b.refill();
		if (b.n < 3) return kInfTruncated;
		last = b.peek(1) != 0;
		const uint32_t type = b.peek(3) >> 1;
		b.drop(3);
		if (type == 3) return kInfBlockType;
		if (type == 0) {                                                                        // stored: to the next byte boundary, LEN, ~LEN, the bytes
			b.drop(b.n & 7u);
			b.refill();
			if (b.n < 32) return kInfTruncated;
			const uint32_t len = b.peek(16);
			b.drop(16);
			const uint32_t nlen = b.peek(16);
			b.drop(16);
			if ((len ^ 0xffffu) != nlen) return kInfStored;
			const uint32_t at = b.pos - b.n / 8;                                                // the next byte the reader has not handed out
			if (len > b.end - at) return kInfTruncated;
			if (len > isize - w.o) return kInfTooLong;
			w.flush();
			for (uint32_t i = (uint32_t)lane; i < len; i += NL) out[w.o + i] = member[at + i];
			w.o += len;
			b.pos = at + len, b.acc = 0, b.n = 0;
			continue;
		}
		int nl, nd;
		if (type == 1) {                                                                        // the fixed code (RFC 1951 3.2.6), through the same builder
			nl = 288, nd = 32;
			inf_sync();
			for (int i = lane; i < 320; i += NL) t->lens[i] = (uint8_t)(i < 144 ? 8 : i < 256 ? 9 : i < 280 ? 7 : i < 288 ? 8 : 5);
		} else {
			b.refill();
			if (b.n < 14) return kInfTruncated;
			nl = (int)b.peek(5) + 257, b.drop(5);
			nd = (int)b.peek(5) + 1, b.drop(5);
			const int nc = (int)b.peek(4) + 4;
			b.drop(4);
			if (nl > 286 || nd > 30) return kInfCounts;
			inf_sync();
			for (int i = 0; i < 19; ++i) {
				// the code-length alphabet's order 16 17 18 0 8 7 9 6 10 5 11 4 12 3 13 2 14 1 15, as arithmetic
				const uint32_t ord = i < 3 ? 16u + (uint32_t)i : i == 3 ? 0u : (i & 1) ? (uint32_t)(19 - i) / 2u : 8u + (uint32_t)(i - 4) / 2u;
				uint32_t v = 0;
				if (i < nc) {
					b.refill();
					if (b.n < 3) return kInfTruncated;
					v = b.peek(3), b.drop(3);
				}
				if (lane == 0) t->lens[ord] = (uint8_t)v;
			}
			int mx;
			const int rc = inf_build<NL>(t->lens, 19, t->cnt_c, t->sym_c, t->lut_c, kInfClBits, lane, &mx);
			// zlib: an incomplete code-length code is refused; one without any code reads every length as 0 and fails at the missing
			// end-of-block code, which is the same verdict
			if (rc != 0) return kInfCodeLengths;
			uint32_t prev = 0;
			for (int i = 0; i < nl + nd;) {
				b.refill();
				uint32_t s;
				if (!inf_symbol(b, t->lut_c, kInfClBits, t->cnt_c, t->sym_c, s)) return b.n < 7 && b.pos >= b.end ? kInfTruncated : kInfCodeLengths;
				if (s < 16) { if (lane == 0) t->lens[i] = (uint8_t)s; prev = s, ++i; continue; }
				const uint32_t eb = s == 16 ? 2u : s == 17 ? 3u : 7u;
				if (b.n < eb) return kInfTruncated;
				const uint32_t rep = (s == 16 ? 3u : s == 17 ? 3u : 11u) + b.peek(eb);
				b.drop(eb);
				if (s == 16 && i == 0) return kInfCodeLengths;
				if ((uint32_t)i + rep > (uint32_t)(nl + nd)) return kInfCodeLengths;
				const uint32_t v = s == 16 ? prev : 0u;
				if (lane == 0) for (uint32_t k = 0; k < rep; ++k) t->lens[(uint32_t)i + k] = (uint8_t)v;
				prev = v, i += (int)rep;
			}
			inf_sync();
			if (INF_UNI(t->lens[256]) == 0) return kInfNoEob;
		}
		{
			int mx;
			int rc = inf_build<NL>(t->lens, nl, t->cnt_l, t->sym_l, t->lut_l, kInfLitBits, lane, &mx);
			if (rc == 1 || (rc == 2 && mx != 1)) return kInfLitTable;
			rc = inf_build<NL>(t->lens + nl, nd, t->cnt_d, t->sym_d, t->lut_d, kInfDistBits, lane, &mx);
			if (rc == 1 || (rc == 2 && mx > 1)) return kInfDistTable;
		}
		for (;;) {
			b.refill();
			uint32_t s;
			if (!inf_symbol(b, t->lut_l, kInfLitBits, t->cnt_l, t->sym_l, s)) return b.n < 15 && b.pos >= b.end ? kInfTruncated : kInfLitCode;
			if (s < 256) {
				if (w.o >= isize) return kInfTooLong;
				w.literal(s);
				continue;
			}
			if (s == 256) break;
			if (s >= 286) return kInfLitCode;
			const uint32_t li = s - 257;
			const uint32_t leb = li < 8 || li == 28 ? 0u : (li >> 2) - 1u;
			uint32_t len = li < 8 ? 3u + li : li == 28 ? 258u : 3u + ((4u + (li & 3u)) << leb);
			if (b.n < leb) return kInfTruncated;
			len += b.peek(leb), b.drop(leb);
			b.refill();
			uint32_t d;
			if (!inf_symbol(b, t->lut_d, kInfDistBits, t->cnt_d, t->sym_d, d)) return b.n < 15 && b.pos >= b.end ? kInfTruncated : kInfDistCode;
			if (d >= 30) return kInfDistCode;
			const uint32_t deb = d < 4 ? 0u : (d >> 1) - 1u;
			uint32_t dist = d < 4 ? 1u + d : 1u + ((2u + (d & 1u)) << deb);
			if (b.n < deb) return kInfTruncated;
			dist += b.peek(deb), b.drop(deb);
			if (dist > w.o) return kInfFarBack;
			if (len > isize - w.o) return kInfTooLong;
			w.match(len, dist);
		}
	}
	w.flush();
	if (w.o != isize) return kInfTooShort;
	if (want_n != isize) return kInfTooShort;
	inf_fence();
	const uint32_t crc = inf_crc32<NL>(out, isize, t->crc_tab, t->red, lane);
	return crc == want_crc ? kInfOk : kInfCrc;
}

} // namespace psvr
