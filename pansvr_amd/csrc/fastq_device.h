// fastq_device.h -- the rules of step 0 (fastq_batch.h: FastqReader::read, FastqBatch::line, parse_ori_span, atoi_span) in the form the
// device runs them: the bodies of the kernels of fastq.hip and, compiled for the host with one "lane", of the checker that holds them to
// fastq_batch.h byte for byte (tests/fastq_check.cpp).  The counterpart of inflate_device.h / deflate_wave_device.h on the text side.
// fastq_batch.h's parser is the specification and the fallback; nothing here validates anything it does not.
//
// A window text[0, n) (n < 2^32), a flag at_end and the limits max_pairs / max_bases become
//   line_start[0 .. 8 P]  uint64, relative to the window          name_end[2 P]  uint16          base_off[2 P + 1]  int64
//   ori[2 P]              psvr_ori_t, every byte written          bases[base_off[2 P] + 1], a NUL behind the last base
// and one psvr_fastq_info_t.  The passes, each a kernel (or, on the host, a loop) of its own:
//   1 newlines     tiles of kFqTileBytes: a lane takes an aligned 16-byte piece, compares it with '\n' (fq_newline_mask) and counts; a piece
//                  that reaches over the window's end is read byte by byte, nothing behind text[n - 1] is touched.  The tiles' counts are
//                  scanned, the same masks then place the line starts in order (fq_emit_piece).  Only starts up to `cap` are stored.
//   2 the window   fq_lines_meta: the unterminated tail (a line only with at_end), the lines that count, the pairs they hold
//   3 lengths      fq_trimmed_len of every candidate read's sequence line; their scan is base_off
//   4 the cut      load_reads' rule (stop BEFORE a pair once the bases so far reach the limit): base_off is monotone, so exactly one pair
//                  p sees base_off[2p] < max_bases <= base_off[2(p + 1)] (or is the last): fq_cut_here; it writes the record (fq_fill_info)
//   5 extract      a group of lanes per read (kFqGroup on the device): the bases are copied lane by consecutive byte (fq_copy_bases), the
//                  header is read in pieces of one byte per lane, ' ' / '\t' / '_' are found by compares and the group's ballot, the
//                  tokens by a walk over the two bit masks that every lane makes alike (fq_parse_header); only the five atoi's and the
//                  flag token's two bytes are left to the group's first lane.  The walk ends with the tenth token.
#pragma once
#include <stdint.h>
#include <string.h>
#include "../../include/psvr_engine.h"

#if defined(__HIPCC__)
#define PSVR_FQ __host__ __device__ inline
#else
#define PSVR_FQ inline
#endif

namespace psvr {

static const int kFqTileLanes = 256, kFqPiece = 16;
static const int kFqTileBytes = kFqTileLanes * kFqPiece;     // 4096 bytes of text per workgroup of the newline passes
static const int kFqGroup = 16;                              // lanes per read in the extract pass

struct FqMeta { int64_t n_lines, avail; };                   // complete lines that count (<= 8 max_pairs), pairs they hold

PSVR_FQ uint32_t fq_ctz(uint32_t x) { return (uint32_t)__builtin_ctz(x); }
PSVR_FQ uint32_t fq_popc(uint32_t x) { return (uint32_t)__builtin_popcount(x); }

// bit i = (byte i of w == c); exact for every byte (no carry leaves a byte: the high bits are masked off before the add)
PSVR_FQ uint32_t fq_eq_mask8(uint64_t w, uint8_t c)
{
	const uint64_t x = w ^ (0x0101010101010101ull * c);
	const uint64_t t = ((x & 0x7f7f7f7f7f7f7f7full) + 0x7f7f7f7f7f7f7f7full) | x;      // high bit of a byte: the byte is not zero
	const uint64_t z = ~t & 0x8080808080808080ull;
	return (uint32_t)(((z >> 7) * 0x0102040810204080ull) >> 56);
}

// bit j = (pos + j < n and text[pos + j] == '\n'), j < 16.  pos is a multiple of 16; on the device text is 16-byte aligned.
PSVR_FQ uint32_t fq_newline_mask(const char *text, uint64_t pos, uint64_t n)
{
	if (pos >= n) return 0;
	if (pos + kFqPiece <= n) {
		uint64_t w[2];
#if defined(__HIP_DEVICE_COMPILE__)
		const ulonglong2 v = *(const ulonglong2 *)(text + pos);
		w[0] = v.x, w[1] = v.y;
#else
		memcpy(w, text + pos, 16);
#endif
		return fq_eq_mask8(w[0], '\n') | fq_eq_mask8(w[1], '\n') << 8;
	}
	uint32_t m = 0;
	for (uint64_t j = 0; pos + j < n; ++j) m |= (uint32_t)(text[pos + j] == '\n') << j;
	return m;
}

// the line starts behind the newlines of one piece; `rank` newlines lie in front of the piece.  Line k + 1 starts behind newline k.
PSVR_FQ void fq_emit_piece(uint32_t mask, uint64_t pos, uint64_t rank, uint64_t cap, uint64_t *line_start)
{
	while (mask) {
		const uint32_t j = fq_ctz(mask);
		mask &= mask - 1;
		++rank;
		if (rank <= cap) line_start[rank] = pos + j + 1;
	}
}

// entries of line_start a call may write: [0, fq_line_cap + 1)
PSVR_FQ uint64_t fq_line_cap(uint64_t n, int64_t max_pairs)
{
	const uint64_t by_text = n + 1;                          // (a line has at least its newline, or is the tail)
	return (uint64_t)max_pairs < by_text / 8 + 1 ? (uint64_t)max_pairs * 8 : by_text;
}
PSVR_FQ int64_t fq_pair_cap(uint64_t n, int64_t max_pairs) { const int64_t by_text = (int64_t)((n + 1) / 8); return max_pairs < by_text ? max_pairs : by_text; }

// after the newline passes: nl newlines in the window
PSVR_FQ FqMeta fq_lines_meta(const char *text, uint64_t n, int at_end, uint64_t nl, int64_t max_pairs, uint64_t cap, uint64_t *line_start)
{
	line_start[0] = 0;
	const bool tail = at_end && n > 0 && text[n - 1] != '\n';
	if (tail && nl + 1 <= cap) line_start[nl + 1] = n;
	const uint64_t lines = nl + (tail ? 1 : 0);
	FqMeta m;
	m.n_lines = (int64_t)(lines / 8 < (uint64_t)max_pairs ? lines : (uint64_t)max_pairs * 8);
	m.avail = m.n_lines / 8;
	return m;
}

// FastqBatch::line: the line [a, b) without its trailing '\n' and '\r'
PSVR_FQ uint32_t fq_trimmed_len(const char *text, uint64_t a, uint64_t b)
{
	uint64_t m = b - a;
	while (m > 0 && (text[a + m - 1] == '\n' || text[a + m - 1] == '\r')) --m;
	return (uint32_t)m;
}

// pair p (< avail) is the last one kept
PSVR_FQ bool fq_cut_here(int64_t p, int64_t avail, const int64_t *base_off, int64_t max_bases)
{
	return base_off[2 * p] < max_bases && (p + 1 == avail || base_off[2 * (p + 1)] >= max_bases);
}
PSVR_FQ void fq_fill_info(int64_t kept, FqMeta m, int64_t max_pairs, int64_t max_bases, const int64_t *base_off, const uint64_t *line_start, psvr_fastq_info_t *info)
{
	info->n_pairs = kept, info->used_bytes = (int64_t)line_start[8 * kept], info->total_bases = base_off[2 * kept], info->n_lines = m.n_lines;
	info->stop = kept < m.avail ? 1 : m.avail == max_pairs ? 0 : info->total_bases >= max_bases ? 1 : 2;
	info->reserved = 0;
}

// atoi_span
PSVR_FQ int fq_atoi(const char *p, const char *e)
{
	while (p < e && (*p == ' ' || (*p >= '\t' && *p <= '\r'))) ++p;
	bool neg = false;
	if (p < e && (*p == '-' || *p == '+')) neg = *p == '-', ++p;
	unsigned v = 0;
	while (p < e && *p >= '0' && *p <= '9') v = v * 10u + (unsigned)(*p - '0'), ++p;
	return neg ? (int)(0u - v) : (int)v;
}

// ---- the group of lanes that shares a read: kFqGroup lanes of a wavefront on the device, one lane on the host ---------------------------
#if defined(__HIP_DEVICE_COMPILE__)
struct FqGroup {
	static const uint32_t width = kFqGroup;
	uint32_t lane, shift;                                    // lane inside the group; the group's first lane inside the wavefront
	// bit k = the predicate of the group's lane k.  Control flow is uniform inside a group, so all of its lanes are here together; lanes of
	// other groups that are elsewhere leave zeros in bits nobody looks at.
	__device__ uint32_t ballot(bool p) const { return (uint32_t)(__ballot(p) >> shift) & ((1u << kFqGroup) - 1u); }
};
#else
struct FqGroup {
	static const uint32_t width = 1;
	uint32_t lane = 0, shift = 0;
	uint32_t ballot(bool p) const { return p ? 1u : 0u; }
};
#endif

PSVR_FQ void fq_copy_bases(const FqGroup &g, const char *src, uint32_t len, char *dst)
{
	for (uint32_t i = g.lane; i < len; i += FqGroup::width) dst[i] = src[i];
}

// slots of the six tokens that are looked at: 0-4 and 9
PSVR_FQ void fq_set_slot(uint32_t a[6], int nt, uint32_t v)
{
	const int slot = nt < 5 ? nt : nt == 9 ? 5 : 6;
	for (int k = 0; k < 6; ++k) if (k == slot) a[k] = v;
}

// the header line h[0, n) (trimmed): name_end and the original alignment (FastqReader::read's per-read loop, parse_ori_span)
PSVR_FQ void fq_parse_header(const FqGroup &g, const char *h, uint32_t n, uint16_t *name_end, psvr_ori_t *ori)
{
	const uint32_t kNone = 0xffffffffu;
	uint32_t sp = n ? kNone : 0;                             // first ' ' or '\t' at an index >= 1
	uint32_t ts[6], te[6];
	for (int k = 0; k < 6; ++k) ts[k] = te[k] = n;
	int nt = 0;                                              // tokens closed so far
	bool in_tok = false, done = n == 0;
	for (uint32_t base = 0; base < n && !done; base += FqGroup::width) {
		const uint32_t i = base + g.lane;
		const bool v = i < n;
		const char ch = v ? h[i] : 0;
		uint32_t C = g.ballot(v);                            // the piece's bytes that belong to the comment
		if (sp == kNone) {
			const uint32_t S = g.ballot(v && i >= 1 && (ch == ' ' || ch == '\t'));
			if (!S) continue;
			sp = base + fq_ctz(S);
		}
		const uint32_t U = g.ballot(v && ch == '_');
		const uint32_t first = sp + 1;
		if (first >= base + FqGroup::width) continue;
		if (first > base) C &= ~((1u << (first - base)) - 1u);
		uint32_t tok = C & ~U, und = C & U;
		// strtok_r(..., "_"): a token starts at the next byte that is no '_' and ends in front of the next '_'
		for (;;) {
			if (!in_tok) {
				if (!tok) break;
				const uint32_t b = fq_ctz(tok);
				fq_set_slot(ts, nt, base + b), in_tok = true;
				und &= ~((2u << b) - 1u);
			} else {
				if (!und) break;
				const uint32_t b = fq_ctz(und);
				fq_set_slot(te, nt, base + b), in_tok = false;
				if (++nt == 10) { done = true; break; }
				tok &= ~((2u << b) - 1u);
			}
		}
	}
	if (sp == kNone) sp = n;
	if (in_tok) fq_set_slot(te, nt, n), ++nt;
	if (g.lane != 0) return;
	*name_end = (uint16_t)(sp > 65535u ? 65535u : sp);
	psvr_ori_t o;
	o.chr_id = nt > 0 ? fq_atoi(h + ts[0], h + te[0]) : 0;
	o.ref_bg = nt > 1 ? (uint32_t)fq_atoi(h + ts[1], h + te[1]) : 0;
	o.read_bg = nt > 2 ? (uint32_t)fq_atoi(h + ts[2], h + te[2]) : 0;
	o.align_score = nt > 3 ? (uint32_t)fq_atoi(h + ts[3], h + te[3]) : 0;
	o.mapq = nt > 4 ? (uint8_t)fq_atoi(h + ts[4], h + te[4]) : 0;
	o.direction = nt > 9 && te[5] - ts[5] >= 1 && h[ts[5]] == 'F' ? 1 : 0;
	o.unmapped = nt > 9 && te[5] - ts[5] >= 2 && h[ts[5] + 1] == 'Y' ? 1 : 0;
	o.reserved = 0;
	*ori = o;
}

// read r of the kept pairs: its bases and its header
PSVR_FQ void fq_extract_read(const FqGroup &g, const char *text, const uint64_t *line_start, const int64_t *base_off, int64_t r, char *bases, uint16_t *name_end, psvr_ori_t *ori)
{
	fq_copy_bases(g, text + line_start[4 * r + 1], (uint32_t)(base_off[r + 1] - base_off[r]), bases + base_off[r]);
	fq_parse_header(g, text + line_start[4 * r], fq_trimmed_len(text, line_start[4 * r], line_start[4 * r + 1]), &name_end[r], &ori[r]);
}

} // namespace psvr

#if !defined(__HIPCC__)
// ---- the host build: the same passes in the same order, one lane --------------------------------------------------------------------------
#include <vector>
namespace psvr {

struct FqHostResult {
	psvr_fastq_info_t info;
	std::vector<uint64_t> line_start;
	std::vector<uint16_t> name_end;
	std::vector<int64_t> base_off;
	std::vector<psvr_ori_t> ori;
	std::vector<char> bases;                                 // total_bases + 1
};

inline void fq_parse_host(const char *text, uint64_t n, int at_end, int64_t max_pairs, int64_t max_bases, FqHostResult *out)
{
	const uint64_t cap = fq_line_cap(n, max_pairs), ntile = (n + kFqTileBytes - 1) / kFqTileBytes;
	const int64_t pcap = fq_pair_cap(n, max_pairs);
	std::vector<uint64_t> ls(cap + 1, 0);
	std::vector<uint64_t> tile_off(ntile + 1, 0);
	for (uint64_t t = 0; t < ntile; ++t) {
		uint32_t c = 0;
		for (int l = 0; l < kFqTileLanes; ++l) c += fq_popc(fq_newline_mask(text, t * kFqTileBytes + (uint64_t)l * kFqPiece, n));
		tile_off[t + 1] = tile_off[t] + c;
	}
	for (uint64_t t = 0; t < ntile; ++t) {
		uint64_t rank = tile_off[t];
		for (int l = 0; l < kFqTileLanes; ++l) {
			const uint64_t pos = t * kFqTileBytes + (uint64_t)l * kFqPiece;
			const uint32_t m = fq_newline_mask(text, pos, n);
			fq_emit_piece(m, pos, rank, cap, ls.data());
			rank += fq_popc(m);
		}
	}
	const FqMeta meta = fq_lines_meta(text, n, at_end, tile_off[ntile], max_pairs, cap, ls.data());
	std::vector<int64_t> off((size_t)(2 * pcap + 2), 0);
	for (int64_t r = 0; r <= 2 * pcap; ++r) off[(size_t)r + 1] = off[(size_t)r] + (r < 2 * meta.avail ? fq_trimmed_len(text, ls[(size_t)(4 * r + 1)], ls[(size_t)(4 * r + 2)]) : 0);
	int64_t kept = 0;
	for (int64_t p = 0; p < meta.avail; ++p) if (fq_cut_here(p, meta.avail, off.data(), max_bases)) kept = p + 1;
	fq_fill_info(kept, meta, max_pairs, max_bases, off.data(), ls.data(), &out->info);
	const int64_t R = 2 * kept;
	out->line_start.assign(ls.begin(), ls.begin() + (size_t)(8 * kept + 1));
	out->base_off.assign(off.begin(), off.begin() + (size_t)(R + 1));
	out->name_end.assign((size_t)R, 0), out->ori.resize((size_t)R), out->bases.assign((size_t)out->info.total_bases + 1, 0);
	FqGroup g;
	for (int64_t r = 0; r < R; ++r) fq_extract_read(g, text, ls.data(), off.data(), r, out->bases.data(), out->name_end.data(), out->ori.data());
}

} // namespace psvr
#endif
