// bam_emit_device.h -- the rules of the main BAM file's records (sam_emit.h: the direct BAM branch of SamEmitter::main_pair) in the form the
// device runs them: the bodies of the kernels of bam_emit.hip and, compiled for the host with one "lane", of the checker that holds them
// to sam_emit.h byte for byte (tests/tools/bam_emit_device_check.cpp).  The counterpart of fastq_device.h on the output side; it uses that
// header's group of lanes (FqGroup).  SamEmitter::main_pair is the specification and the fallback: a pair it would not take through its
// direct path is declined here, never formatted another way.
//
// For pair p of a run of results (psvr_read_hdr_t[2 P], psvr_pair_result_t[P], psvr_cand_t[], uint32 cigar[]) over a parsed window (text, line
// index, name ends, psvr_ori_t) a pair is in one of three states:
//   0  nothing to write: !gain, or every read is skipped (primary == -1; primary == -2 under not_ori; chr_id == 0xffffffff or outside
//      [0, n_header); (int)ref_bg - 1 < 0 -- the host drops the last two silently as well)
//   1  written here: the records of its reads that are not skipped, mate 0 first
//   2  declined, zero bytes, the host formats the pair: a read that would be written has a name of length 0 or over 254, a quality line
//      whose trimmed length differs from the sequence line's, a '\t' or NUL in its comment, an SV / MV / XA anchor whose string holds a
//      '\t', a primary candidate with n_cigar == 0, n_cigar > 0xffff or an operator nibble over 8 -- or a result index that leaves the
//      arrays it was given: cand_off outside [0, n_cands], cand_off + primary / secondary outside [0, n_cands), cigar_off + n_cigar
//      outside [0, n_cigar_words], an anchor id outside [-1, n_anchor).  (Also a pair whose records would not fit 2^31 - 1 bytes.)
// The index rule is the bounds guarantee: whatever the results hold, nothing outside the given arrays, the window's text and the tables is
// read.  A record's bytes are walked by ONE function, be_record, templated on its sink: BeCount adds up (the size pass), BeWrite stores
// (the write pass), so the two cannot disagree.  Every lane of a group walks the same control flow and keeps the same position; a byte is
// stored by exactly one lane: scalar fields and decimal text by the group's first lane, name / CIGAR / SEQ / QUAL / strings / comment by
// lane (i mod width) for output byte (or word) i.  A SEQ byte is made from its two bases by the lane that owns it.
#pragma once
#include <stdint.h>
#include <string.h>
#include "../../include/psvr_engine.h"
#include "fastq_device.h"
#include "bam_record.h"

namespace psvr {

// per index: the anchors' strings.  print_string of anchor i = text[off[i], off[i + 1]), vcf_id = text[off[n_anchor + i], off[n_anchor + i + 1]);
// tab[i]: bit 0 = the print string holds a '\t', bit 1 = the vcf id does
struct BeTables {
	const char *text;
	const uint32_t *off;
	const uint8_t *tab;
	int32_t n_anchor, n_header;
};

// what a pass reads: the window's arrays are indexed by the window's reads, the results by the run's (run pair p = window pair first_pair + p)
struct BeInput {
	const char *text; const uint64_t *line_start; const uint16_t *name_end; const psvr_ori_t *ori;
	int64_t first_pair;
	const psvr_read_hdr_t *hdr; const psvr_pair_result_t *pairs;
	const psvr_cand_t *cands; int64_t n_cands;
	const uint32_t *cig; int64_t n_cig;
	int32_t not_ori;
	BeTables T;
};

// ---- sinks: put(i, b) stores byte b at the current position + i (the caller is the lane that owns it) --------------------------------------
struct BeCount {
	static constexpr bool writes = false;
	uint64_t pos = 0;
	PSVR_FQ void put(uint64_t, uint8_t) {}
};
struct BeWrite {
	static constexpr bool writes = true;
	uint8_t *out;
	uint64_t pos;
	PSVR_FQ void put(uint64_t i, uint8_t b) { out[pos + i] = b; }
};

// the group's sum of v (every lane of the group is here: control flow is uniform inside a group)
PSVR_FQ int64_t be_group_sum(const FqGroup &g, int64_t v)
{
#if defined(__HIP_DEVICE_COMPILE__)
	for (int d = 1; d < kFqGroup; d <<= 1) v += (int64_t)__shfl_xor((long long)v, d, kFqGroup);
#endif
	(void)g;
	return v;
}

template <class S> PSVR_FQ void be_u8(const FqGroup &g, S &o, unsigned x) { if (S::writes && g.lane == 0) o.put(0, (uint8_t)x); o.pos += 1; }
template <class S> PSVR_FQ void be_u16(const FqGroup &g, S &o, unsigned x) { if (S::writes && g.lane == 0) o.put(0, (uint8_t)x), o.put(1, (uint8_t)(x >> 8)); o.pos += 2; }
template <class S> PSVR_FQ void be_u32(const FqGroup &g, S &o, uint32_t x)
{
	if (S::writes && g.lane == 0) o.put(0, (uint8_t)x), o.put(1, (uint8_t)(x >> 8)), o.put(2, (uint8_t)(x >> 16)), o.put(3, (uint8_t)(x >> 24));
	o.pos += 4;
}
template <class S> PSVR_FQ void be_lit(const FqGroup &g, S &o, const char *s, uint32_t n) { if (S::writes && g.lane == 0) for (uint32_t i = 0; i < n; ++i) o.put(i, (uint8_t)s[i]); o.pos += n; }
// n bytes of src, lane by consecutive byte
template <class S> PSVR_FQ void be_copy(const FqGroup &g, S &o, const char *src, uint32_t n)
{
	if (S::writes) for (uint32_t i = g.lane; i < n; i += FqGroup::width) o.put(i, (uint8_t)src[i]);
	o.pos += n;
}
// RawOut::num for the 32-bit values the records hold (%d)
template <class S> PSVR_FQ void be_num(const FqGroup &g, S &o, int32_t x)
{
	const uint32_t neg = x < 0 ? 1u : 0u;
	uint32_t u = neg ? 0u - (uint32_t)x : (uint32_t)x, nd = 1;
	for (uint32_t t = u; t >= 10; t /= 10) ++nd;
	if (S::writes && g.lane == 0) {
		if (neg) o.put(0, '-');
		for (uint32_t i = nd; i-- > 0;) o.put(neg + i, (uint8_t)('0' + u % 10)), u /= 10;
	}
	o.pos += neg + nd;
}
// RawOut::bam_int: an integer tag in the smallest type
template <class S> PSVR_FQ void be_tag_int(const FqGroup &g, S &o, char t0, char t1, int32_t x)
{
	be_u8(g, o, (uint8_t)t0), be_u8(g, o, (uint8_t)t1);
	if (x < 0) {
		if (x >= -128) be_u8(g, o, 'c'), be_u8(g, o, (uint8_t)(int8_t)x);
		else if (x >= -32768) be_u8(g, o, 's'), be_u16(g, o, (uint16_t)(int16_t)x);
		else be_u8(g, o, 'i'), be_u32(g, o, (uint32_t)x);
	} else {
		if (x <= 255) be_u8(g, o, 'C'), be_u8(g, o, (unsigned)x);
		else if (x <= 65535) be_u8(g, o, 'S'), be_u16(g, o, (unsigned)x);
		else be_u8(g, o, 'I'), be_u32(g, o, (uint32_t)x);
	}
}
template <class S> PSVR_FQ void be_tag_z(const FqGroup &g, S &o, char t0, char t1) { be_u8(g, o, (uint8_t)t0), be_u8(g, o, (uint8_t)t1), be_u8(g, o, 'Z'); }

// nt16_code (bam_writer.h) of a base, and of its reverse-strand character (getReverseChar: A C G T in either case, anything else N)
PSVR_FQ uint32_t be_code(uint8_t c)
{
	if (c >= '0' && c <= '3') return 1u << (c - '0');
	if (c >= 'a' && c <= 'z') c = (uint8_t)(c - 32);
	switch (c) {
	case '=': return 0; case 'A': return 1; case 'C': return 2; case 'M': return 3; case 'G': return 4; case 'R': return 5; case 'S': return 6; case 'V': return 7;
	case 'T': return 8; case 'W': return 9; case 'Y': return 10; case 'H': return 11; case 'K': return 12; case 'D': return 13; case 'B': return 14;
	}
	return 15;
}
PSVR_FQ uint32_t be_rc_code(uint8_t c)
{
	switch (c) {
	case 'A': case 'a': return 8;
	case 'C': case 'c': return 4;
	case 'G': case 'g': return 2;
	case 'T': case 't': return 1;
	}
	return 15;
}
// the CIGAR word after the host's round trip of its length through "%d" of an int16 (negative lengths keep their sign bits), and the reference
// bases that word covers (bam_record.h, as the bin's bam_reg2bin)
PSVR_FQ uint32_t be_cigar_word(uint32_t len16, uint32_t op) { return (uint32_t)(int32_t)(int16_t)(uint16_t)len16 << 4 | op; }
PSVR_FQ int64_t be_cigar_span(uint32_t len16, uint32_t op) { return bam_cigar_ref_len(be_cigar_word(len16, op)); }

// base + k stays inside [0, n): *at = base + k
PSVR_FQ bool be_index(int64_t base, int32_t k, int64_t n, int64_t *at)
{
	if (base < 0 || base > n) return false;
	const int64_t i = base + k;
	if (i < 0 || i >= n) return false;
	*at = i;
	return true;
}
// an anchor id a record names: -1 (none) or one of the table's; `bit` of its flags says that its string holds a tab
PSVR_FQ bool be_anchor_ok(const BeTables &T, int32_t id, unsigned bit) { return id == -1 || (id >= 0 && id < T.n_anchor && !(T.tab[id] & bit)); }

// one read of a pair as both passes see it
struct BeRead {
	bool is_ori;
	int32_t chr_id, direction, mapq, pos;
	uint32_t align_score, chain_score, n_cigar;
	int64_t rlen;                                            // the CIGAR's reference span
	const uint32_t *cig;                                     // the primary candidate's words (not for the original alignment)
	int64_t sc;                                              // the secondary candidate's index, -1: none
	const char *nt, *ct, *st, *qt;                           // name, comment, sequence line, quality line
	uint32_t nn, cn, read_l;
};

// the state of read k of run pair p (0 skipped, 1 written, 2 declined) and, for 1, what be_record needs
PSVR_FQ int be_plan_read(const FqGroup &g, const BeInput &in, int64_t p, int k, BeRead *R)
{
	const psvr_read_hdr_t &rr = in.hdr[2 * p + k];
	const int64_t wr = 2 * (in.first_pair + p) + k;
	const psvr_ori_t &ori = in.ori[wr];
	if (rr.primary == -1) return 0;
	R->is_ori = rr.primary == -2;
	if (in.not_ori && R->is_ori) return 0;
	const uint64_t *ls = in.line_start + 4 * wr;
	const uint32_t hl = fq_trimmed_len(in.text, ls[0], ls[1]), ne = in.name_end[wr];
	const char *h = in.text + ls[0];
	R->nt = h + (hl ? 1 : 0), R->nn = hl && ne ? ne - 1 : 0;
	if (ne < hl) R->ct = h + ne + 1, R->cn = hl - ne - 1; else R->ct = h + hl, R->cn = 0;
	R->st = in.text + ls[1], R->read_l = fq_trimmed_len(in.text, ls[1], ls[2]);
	R->qt = in.text + ls[3];
	const uint32_t qn = fq_trimmed_len(in.text, ls[3], ls[4]);
	uint32_t ref_bg;
	int64_t ci = -1;
	R->cig = nullptr, R->sc = -1, R->chain_score = 0, R->rlen = 0;
	if (R->is_ori) {
		R->chr_id = ori.chr_id, R->direction = ori.direction, R->mapq = ori.mapq, ref_bg = ori.ref_bg >= 0x7fffffffu ? 1u : ori.ref_bg, R->align_score = ori.align_score;
	} else {
		if (!be_index(rr.cand_off, rr.primary, in.n_cands, &ci)) return 2;
		const psvr_cand_t &cd = in.cands[ci];
		R->chr_id = cd.chr_id, R->direction = cd.direction, R->mapq = cd.mapq, ref_bg = cd.ref_bg, R->align_score = cd.align_score, R->chain_score = cd.chain_score;
	}
	if ((uint32_t)R->chr_id == 0xffffffffu || R->chr_id < 0 || R->chr_id >= in.T.n_header) return 0;
	R->pos = (int32_t)ref_bg;
	if (R->pos <= 0) return 0;                               // pos - 1 < 0
	// ---- the read would be written: what the direct path does not take
	if (R->nn == 0 || R->nn > 254 || qn != R->read_l) return 2;
	for (uint32_t base = 0; base < R->cn; base += FqGroup::width) {
		const uint32_t i = base + g.lane;
		const char ch = i < R->cn ? R->ct[i] : 'x';
		if (g.ballot(ch == '\t' || ch == 0)) return 2;
	}
	if (!be_anchor_ok(in.T, rr.prim_sv_id, 1) || (rr.has_mate && !be_anchor_ok(in.T, rr.mate_sv_id, 1))) return 2;
	if (rr.secondary >= 0) {
		if (!be_index(rr.cand_off, rr.secondary, in.n_cands, &R->sc)) return 2;
		if (!be_anchor_ok(in.T, in.cands[R->sc].sv_id, 2)) return 2;
	}
	if (R->is_ori) {
		R->n_cigar = ori.read_bg > 0 ? 2u : 1u;
		if (ori.read_bg > 0) R->rlen += be_cigar_span(ori.read_bg, 4);
		R->rlen += be_cigar_span(R->read_l - ori.read_bg, 0);
		return 1;
	}
	const psvr_cand_t &cd = in.cands[ci];
	R->n_cigar = cd.n_cigar;
	if (cd.n_cigar == 0 || cd.n_cigar > 0xffffu || cd.cigar_off < 0 || cd.cigar_off > in.n_cig || (int64_t)cd.n_cigar > in.n_cig - cd.cigar_off) return 2;
	R->cig = in.cig + cd.cigar_off;
	int64_t span = 0;
	for (uint32_t base = 0; base < cd.n_cigar; base += FqGroup::width) {
		const uint32_t i = base + g.lane;
		const uint32_t w = i < cd.n_cigar ? R->cig[i] : 0u;
		if (g.ballot((w & 0xf) > 8)) return 2;
		if (i < cd.n_cigar) span += be_cigar_span(w >> 4, w & 0xf);
	}
	R->rlen = be_group_sum(g, span);
	return 1;
}

// RC:Z: the comment with the separators strtok_r cut behind its first ten tokens turned into ',' (ori_cuts); one at the very last byte ends
// the string there.  (No NUL inside: such a comment was declined.)
template <class S> PSVR_FQ void be_comment(const FqGroup &g, S &o, const char *ct, uint32_t cn)
{
	int nt = 0;
	bool in_tok = false;
	uint32_t len = cn;
	for (uint32_t base = 0; base < cn; base += FqGroup::width) {
		const uint32_t i = base + g.lane;
		const bool v = i < cn;
		const char ch = v ? ct[i] : 0;
		const uint32_t C = g.ballot(v), U = g.ballot(v && ch == '_');
		uint32_t tok = C & ~U, und = U, cuts = 0;
		while (nt < 10) {
			if (!in_tok) {
				if (!tok) break;
				const uint32_t b = fq_ctz(tok);
				in_tok = true;
				und &= ~((2u << b) - 1u);
			} else {
				if (!und) break;
				const uint32_t b = fq_ctz(und);
				cuts |= 1u << b, in_tok = false, ++nt;
				tok &= ~((2u << b) - 1u);
			}
		}
		if (cn - 1 - base < FqGroup::width && (cuts >> (cn - 1 - base) & 1u)) len = cn - 1;
		if (S::writes && v && i < len) o.put(i, (uint8_t)((cuts >> g.lane & 1u) ? ',' : ch));
	}
	o.pos += len;
}

// one anchor string of the table
template <class S> PSVR_FQ void be_anchor(const FqGroup &g, S &o, const BeTables &T, int64_t slot)
{
	be_copy(g, o, T.text + T.off[slot], T.off[slot + 1] - T.off[slot]);
}

// SEQ: two 4-bit codes per byte, the odd tail's low nibble 0; QUAL: phred values (no_qual: 0xff, a quality line that is "*"); the reverse
// strand through getReverseStr_char / getReverseStr_qual_char (whose loop bound swaps the middle pair of an even-length read back).  Shared
// with the second file's records (bam_ori_device.h).
template <class S> PSVR_FQ void be_seq_qual(const FqGroup &g, S &body, const char *st, const char *qt, uint32_t n, bool rev, bool no_qual)
{
	const uint32_t nb = (n + 1) / 2;
	if (S::writes) {
		for (uint32_t j = g.lane; j < nb; j += FqGroup::width) {
			const uint32_t i = 2 * j;
			const uint32_t hi = rev ? be_rc_code((uint8_t)st[n - 1 - i]) : be_code((uint8_t)st[i]);
			const uint32_t lo = i + 1 < n ? (rev ? be_rc_code((uint8_t)st[n - 2 - i]) : be_code((uint8_t)st[i + 1])) : 0u;
			body.put(j, (uint8_t)(hi << 4 | lo));
		}
		const bool even = !(n & 1) && n >= 2;
		for (uint32_t j = g.lane; j < n; j += FqGroup::width) {
			const bool keep = !rev || (even && (j == n / 2 - 1 || j == n / 2));
			body.put((uint64_t)nb + j, no_qual ? (uint8_t)0xff : (uint8_t)(qt[keep ? j : n - 1 - j] - 33));
		}
	}
	body.pos += (uint64_t)nb + n;
}

// the record of a read whose state is 1: SamEmitter::main_pair's direct BAM branch, field for field
template <class S> PSVR_FQ void be_record(const FqGroup &g, const BeInput &in, int64_t p, int k, const BeRead &R, S &o)
{
	const psvr_read_hdr_t &rr = in.hdr[2 * p + k];
	const psvr_pair_result_t &pr = in.pairs[p];
	const psvr_ori_t &ori = in.ori[2 * (in.first_pair + p) + k];
	S body = o;                                              // behind block_size, which is known when the record's end is
	body.pos += 4;
	const uint32_t flag = (uint8_t)((k == 0 ? 0x40 : 0) + (R.direction == 0 ? 0x10 : 0) + (rr.has_mate ? 0 : 0x8));
	const uint32_t isize = R.direction == 1 ? (uint32_t)pr.cur_isize : 0u - (uint32_t)pr.cur_isize;
	const int64_t p0 = (int64_t)R.pos - 1;
	be_u32(g, body, (uint32_t)R.chr_id), be_u32(g, body, (uint32_t)p0);
	be_u8(g, body, R.nn + 1), be_u8(g, body, (unsigned)R.mapq);
	be_u16(g, body, (unsigned)bam_reg2bin(p0, p0 + R.rlen));
	be_u16(g, body, R.n_cigar), be_u16(g, body, flag), be_u32(g, body, R.read_l);
	int32_t mtid = -1;
	int64_t pnext = 0;
	if (rr.has_mate) {
		const int32_t mp = (int32_t)rr.mate_ref_bg, mc = rr.mate_chr_id;
		if (mc >= 0 && mc < in.T.n_header && mp > 0) mtid = mc;
		pnext = mp;
	}
	be_u32(g, body, (uint32_t)mtid), be_u32(g, body, (uint32_t)(pnext - 1)), be_u32(g, body, isize);
	be_copy(g, body, R.nt, R.nn), be_u8(g, body, 0);
	// CIGAR: a word per lane, stored byte by byte (a record starts at any byte)
	if (R.is_ori) {
		if (ori.read_bg > 0) be_u32(g, body, be_cigar_word(ori.read_bg, 4));
		be_u32(g, body, be_cigar_word(R.read_l - ori.read_bg, 0));
	} else {
		if (S::writes) for (uint32_t i = g.lane; i < R.n_cigar; i += FqGroup::width) {
			const uint32_t w = R.cig[i], x = be_cigar_word(w >> 4, w & 0xf);
			body.put(4 * (uint64_t)i, (uint8_t)x), body.put(4 * (uint64_t)i + 1, (uint8_t)(x >> 8)), body.put(4 * (uint64_t)i + 2, (uint8_t)(x >> 16)), body.put(4 * (uint64_t)i + 3, (uint8_t)(x >> 24));
		}
		body.pos += 4 * (uint64_t)R.n_cigar;
	}
	be_seq_qual(g, body, R.st, R.qt, R.read_l, R.direction == 0, false);
	// the tags
	be_tag_int(g, body, 'A', 'S', (int32_t)R.align_score), be_tag_int(g, body, 'O', 'S', (int32_t)ori.align_score);
	be_tag_z(g, body, 'O', 'A'), be_num(g, body, ori.chr_id), be_u8(g, body, ','), be_num(g, body, (int32_t)(ori.ref_bg >= 0x7fffffffu ? 1u : ori.ref_bg)), be_u8(g, body, ',');
	be_num(g, body, (int32_t)ori.read_bg), be_u8(g, body, ','), be_num(g, body, (int32_t)ori.mapq), be_lit(g, body, rr.unmapped ? ",U;" : ",M;", 3), be_u8(g, body, 0);
	if (!R.is_ori) be_tag_int(g, body, 'C', 'S', (int32_t)R.chain_score);
	if (rr.prim_sv_id >= 0) be_tag_z(g, body, 'S', 'V'), be_anchor(g, body, in.T, rr.prim_sv_id), be_u8(g, body, 0);
	if (rr.has_mate && rr.mate_sv_id >= 0) be_tag_z(g, body, 'M', 'V'), be_anchor(g, body, in.T, rr.mate_sv_id), be_u8(g, body, 0);
	if (R.sc >= 0) {
		const psvr_cand_t &sc = in.cands[R.sc];
		be_tag_z(g, body, 'X', 'A'), be_num(g, body, sc.chr_id), be_u8(g, body, ','), be_num(g, body, (int32_t)sc.ref_bg), be_u8(g, body, ','), be_num(g, body, (int32_t)sc.read_bg);
		be_u8(g, body, ','), be_num(g, body, (int32_t)sc.align_score), be_lit(g, body, sc.direction == 1 ? ",F," : ",R,", 3);
		if (sc.sv_id >= 0) be_anchor(g, body, in.T, (int64_t)in.T.n_anchor + sc.sv_id); else be_u8(g, body, '*');
		be_u8(g, body, ';'), be_u8(g, body, 0);
	}
	be_tag_z(g, body, 'R', 'C'), be_comment(g, body, R.ct, R.cn), be_u8(g, body, 0);
	be_u32(g, o, (uint32_t)(body.pos - o.pos - 4));          // block_size
	o.pos = body.pos;
}

// pair p: its state; for state 1 the sink has walked its records (*records of them)
template <class S> PSVR_FQ int be_pair(const FqGroup &g, const BeInput &in, int64_t p, S &o, int32_t *records)
{
	*records = 0;
	if (!in.pairs[p].gain) return 0;
	BeRead R0, R1;                                           // (two named records, not an array: they stay in registers)
	const int s0 = be_plan_read(g, in, p, 0, &R0), s1 = be_plan_read(g, in, p, 1, &R1);
	if (s0 == 2 || s1 == 2) return 2;
	if (s0 == 0 && s1 == 0) return 0;
	if (s0 == 1) be_record(g, in, p, 0, R0, o), ++*records;
	if (s1 == 1) be_record(g, in, p, 1, R1, o), ++*records;
	return 1;
}

// the size pass for one pair: state, bytes, records
PSVR_FQ int be_pair_size(const FqGroup &g, const BeInput &in, int64_t p, int32_t *bytes, int32_t *records)
{
	BeCount c;
	int st = be_pair(g, in, p, c, records);
	if (st == 1 && c.pos > 0x7fffffffull) st = 2;
	if (st != 1) *records = 0;
	*bytes = st == 1 ? (int32_t)c.pos : 0;
	return st;
}

} // namespace psvr

// ---- host side: the table of an index's anchor strings, and the same passes with one lane ------------------------------------------------
#include <string>
#include <vector>
namespace psvr {

struct BeTableHost {
	std::vector<char> text;
	std::vector<uint32_t> off;                               // 2 n + 1
	std::vector<uint8_t> tab;                                // n (+ 1: never empty)
	// print(i) / vid(i): the C strings of anchor i
	template <class F1, class F2> void build(int n, F1 &&print, F2 &&vid)
	{
		text.clear(), off.assign(1, 0), tab.assign((size_t)n + 1, 0);
		for (int pass = 0; pass < 2; ++pass)
			for (int i = 0; i < n; ++i) {
				const char *s = pass ? vid(i) : print(i);
				if (!s) s = "";
				const size_t len = strlen(s);
				if (memchr(s, '\t', len)) tab[(size_t)i] |= (uint8_t)(1 << pass);
				text.insert(text.end(), s, s + len);
				off.push_back((uint32_t)text.size());
			}
		text.push_back(0);
	}
	BeTables view(int n_header) const { BeTables T; T.text = text.data(), T.off = off.data(), T.tab = tab.data(), T.n_anchor = (int32_t)(off.size() / 2), T.n_header = n_header; return T; }
};

#if !defined(__HIPCC__)
struct BeHostResult {
	std::vector<uint8_t> bytes, state;
	std::vector<int64_t> pair_off;                           // P + 1
	int64_t n_records = 0, n_written = 0, n_declined = 0;
};
inline void be_emit_host(const BeInput &in, int64_t P, BeHostResult *out)
{
	FqGroup g;
	out->state.assign((size_t)P, 0), out->pair_off.assign((size_t)P + 1, 0);
	out->n_records = out->n_written = out->n_declined = 0;
	for (int64_t p = 0; p < P; ++p) {
		int32_t nb, nr;
		const int st = be_pair_size(g, in, p, &nb, &nr);
		out->state[(size_t)p] = (uint8_t)st, out->pair_off[(size_t)p + 1] = out->pair_off[(size_t)p] + nb;
		out->n_records += nr, out->n_written += st == 1, out->n_declined += st == 2;
	}
	out->bytes.assign((size_t)out->pair_off[(size_t)P], 0xEE);
	for (int64_t p = 0; p < P; ++p) {
		if (out->state[(size_t)p] != 1) continue;
		BeWrite w;
		w.out = out->bytes.data(), w.pos = (uint64_t)out->pair_off[(size_t)p];
		int32_t nr;
		be_pair(g, in, p, w, &nr);
	}
}
#endif

} // namespace psvr
