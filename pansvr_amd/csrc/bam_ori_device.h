// bam_ori_device.h -- the rules of the second BAM file's records (sam_emit.h: the BAM branch of SamEmitter::ori_pair, through emit() and
// BamWriter::encode / put_tags) in the form the device runs them: the bodies of the ori kernels of bam_emit.hip and, compiled for the host
// with one "lane", of the checker that holds them to sam_emit.h byte for byte (tests/tools/bam_ori_device_check.cpp).  The counterpart of
// bam_emit_device.h for the second file; it uses that header's sinks, primitives, SEQ/QUAL block and index rule.  SamEmitter::ori_pair is
// the specification and the fallback: a pair it would not encode through the plain path is declined here, never formatted another way.
//
// For pair p of a run of results over a parsed window, in this order:
//   0  the gate fails: !(max_score <= min_filter_score) or one of the two ori[].chr_id is -1 -- before any text is touched
//   2  a '\t' or NUL in either read's comment
//   per read, mate 0 first, in parse_ori_record's own order (the first verdict counts):
//      0  no "FLAG_"                         2  the flag or the mapq behind it is not a plain number ("_" between them)
//      0  no "CIGAR_" behind it, no '_' closing the CIGAR, fewer than 6 bytes from that '_' on
//      2  one of the three MATE_ numbers is not a plain number ('-' allowed, "_" between them)
//      0  no "TAG_" behind them
//      (a plain number: 1-9 digits; anything else is what the host hands to its sscanf path)
//   the `proper` rule, read 0 then read 1, stopping at the first read that clears it:
//      max == -1 clears it; max == -2 clears it when ori_has_clip(CIGAR text, 25); otherwise the candidate cand_off + max clears it with
//      n_cigar == 0 or a sum of its 'I' lengths >= 25.  2: cand_off outside [0, n_cands], cand_off + max outside [0, n_cands),
//      cigar_off + n_cigar outside [0, n_cigar_words]
//   0  the pair is still proper
//   per read of the kept pair:
//      skipped (the read, not the pair): chr_id outside [0, n_header) or (int)(ref_bg + 1) - 1 < 0
//      2  a name of length 0 or over 254; a quality line not as long as the sequence line; an empty or "*" sequence line; a CIGAR text
//         acceptable_cigar refuses (an operator without digits, a letter outside MIDNSHP=XB, trailing digits), one with a '-', one of more
//         than 65535 operators; an aux field shorter than 5 bytes or without its two colons; an aux type other than i A Z H (f and B ARE
//         DECLINED: strtof and the array items stay with the host); an i value that is not a '-'-optional run of 1-9 digits
//   0  both reads skipped       1  written: the records of the reads that are not skipped, mate 0 first
//   2  the pair's records exceed 2^31 - 1 bytes
// Whatever the results and the text hold, nothing outside the given arrays and the window's lines is read: every text position looked at
// lies inside the comment [ct, ct + cn), every index is checked (be_index) before it is followed.  The record's bytes are walked by ONE
// function, bo_read, templated on its sink (BeCount / BeWrite).  The text is parsed by every lane of the group alike (the same loads, the
// same verdicts: control flow is uniform); a byte is stored by exactly one lane: scalar fields by the group's first lane, name / CIGAR
// words / SEQ / QUAL / strings by lane (i mod width) for output byte (or word) i.
#pragma once
#include "bam_emit_device.h"

namespace psvr {

struct BoInput {
	const char *text; const uint64_t *line_start; const uint16_t *name_end; const psvr_ori_t *ori;
	int64_t first_pair;
	const psvr_read_hdr_t *hdr; const psvr_pair_result_t *pairs;
	const psvr_cand_t *cands; int64_t n_cands;
	const uint32_t *cig; int64_t n_cig;
	int32_t min_filter_score, n_header;
};

// what parse_ori_record makes of a comment: positions are relative to the comment
struct BoText {
	const char *ct; uint32_t cn;
	int32_t flag, mapq, mate_chr, mate_b, isize;             // mate_b: the MATE_ position as written (mate_pos - 1)
	uint32_t cg, cgn;                                        // the CIGAR text
	uint32_t tg, tl;                                         // what follows "TAG_", to the comment's end
};

static const uint32_t kBoNone = 0xffffffffu;

// memmem(ct + from, e - from, lit, n)
PSVR_FQ uint32_t bo_find(const char *ct, uint32_t from, uint32_t e, const char *lit, uint32_t n)
{
	for (uint32_t i = from; i + n <= e; ++i) {
		uint32_t j = 0;
		while (j < n && ct[i + j] == lit[j]) ++j;
		if (j == n) return i;
	}
	return kBoNone;
}
// parse_ori_record's `number`: 1-9 digits, a '-' in front where `sign`; *p moves behind it
PSVR_FQ bool bo_number(const char *ct, uint32_t *p, uint32_t e, bool sign, int32_t *v)
{
	uint32_t q = *p;
	bool neg = false;
	if (sign && q < e && ct[q] == '-') neg = true, ++q;
	const uint32_t d0 = q;
	int32_t x = 0;
	while (q < e && ct[q] >= '0' && ct[q] <= '9' && q - d0 < 10) { if (q - d0 < 9) x = x * 10 + (ct[q] - '0'); ++q; }
	if (q == d0 || q - d0 > 9) return false;
	*v = neg ? -x : x, *p = q;
	return true;
}
// 0 a section is missing, 1 parsed, 2 the host's sscanf path
PSVR_FQ int bo_parse(const char *ct, uint32_t cn, BoText *T)
{
	const uint32_t e = cn;
	T->ct = ct, T->cn = cn;
	const uint32_t f = bo_find(ct, 0, e, "FLAG_", 5);
	if (f == kBoNone) return 0;
	uint32_t p = f + 5;
	if (!bo_number(ct, &p, e, false, &T->flag) || p >= e || ct[p] != '_') return 2;
	++p;
	if (!bo_number(ct, &p, e, false, &T->mapq)) return 2;
	uint32_t cg = bo_find(ct, f + 5, e, "CIGAR_", 6);
	if (cg == kBoNone) return 0;
	cg += 6;
	uint32_t ce = cg;
	while (ce < e && ct[ce] != '_') ++ce;
	if (ce >= e) return 0;
	T->cg = cg, T->cgn = ce - cg;
	if (e - ce < 6) return 0;
	p = ce + 6;                                              // skips "_MATE_"
	if (!bo_number(ct, &p, e, true, &T->mate_chr) || p >= e || ct[p] != '_') return 2;
	++p;
	if (!bo_number(ct, &p, e, true, &T->mate_b) || p >= e || ct[p] != '_') return 2;
	++p;
	if (!bo_number(ct, &p, e, true, &T->isize)) return 2;
	const uint32_t tg = bo_find(ct, ce + 6, e, "TAG_", 4);
	if (tg == kBoNone) return 0;
	T->tg = tg + 4, T->tl = e - (tg + 4);
	return 1;
}
PSVR_FQ bool bo_no_cigar(const BoText &T) { return T.cgn == 0 || (T.cgn == 1 && T.ct[T.cg] == '*'); }
// ori_has_clip on the CIGAR text
PSVR_FQ bool bo_has_clip(const BoText &T, int32_t min_clip)
{
	if (bo_no_cigar(T)) return true;
	uint32_t first_len = 0, last_len = 0, n = 0, ops = 0;
	char first_op = 0, last_op = 0;
	for (uint32_t i = 0; i < T.cgn; ++i) {
		const char ch = T.ct[T.cg + i];
		if (ch >= '0' && ch <= '9') { n = n * 10u + (uint32_t)(ch - '0'); continue; }
		if (ops++ == 0) first_op = ch, first_len = n;
		last_op = ch, last_len = n, n = 0;
	}
	if (!ops) return true;
	uint32_t tot = 0;
	if (first_op == 'S' || first_op == 'H') tot += first_len;
	if (last_op == 'S' || last_op == 'H') tot += last_len;
	return (int32_t)tot >= min_clip;
}
PSVR_FQ uint32_t bo_cigar_op(char ch)
{
	switch (ch) {
	case 'M': return 0; case 'I': return 1; case 'D': return 2; case 'N': return 3; case 'S': return 4;
	case 'H': return 5; case 'P': return 6; case '=': return 7; case 'X': return 8; case 'B': return 9;
	}
	return 16;
}
// the CIGAR text as acceptable_cigar takes it and BamWriter::encode reads it (no '-'): word i goes to lane (i mod width).  false: refused
template <class S> PSVR_FQ bool bo_cigar(const FqGroup &g, S &o, const BoText &T, uint32_t *n_ops, int64_t *rlen)
{
	uint32_t len = 0, k = 0;
	bool digit = false;
	int64_t span = 0;
	for (uint32_t i = 0; i < T.cgn; ++i) {
		const char ch = T.ct[T.cg + i];
		if (ch >= '0' && ch <= '9') { len = len * 10u + (uint32_t)(ch - '0'), digit = true; continue; }
		const uint32_t op = bo_cigar_op(ch);
		if (!digit || op > 9) return false;
		const uint32_t w = len << 4 | op;
		span += bam_cigar_ref_len(w);
		if (S::writes && k % FqGroup::width == g.lane) o.put(4 * (uint64_t)k, (uint8_t)w), o.put(4 * (uint64_t)k + 1, (uint8_t)(w >> 8)), o.put(4 * (uint64_t)k + 2, (uint8_t)(w >> 16)), o.put(4 * (uint64_t)k + 3, (uint8_t)(w >> 24));
		++k, len = 0, digit = false;
	}
	if (digit) return false;
	o.pos += 4 * (uint64_t)k;
	*n_ops = k, *rlen = span;
	return true;
}
// the aux fields of the TAG_ text: the '_' in front of "XX:t:" is a field's end (parse_ori_record), the text's last byte is dropped;
// put_tags' rules field by field.  false: declined
template <class S> PSVR_FQ bool bo_tags(const FqGroup &g, S &o, const BoText &T)
{
	const char *t = T.ct + T.tg;
	const uint32_t tl = T.tl, tn = tl ? tl - 1 : 0;
	uint32_t a = 0;
	while (a < tn) {
		uint32_t b = a;
		while (b < tn && !(b + 5 < tl && t[b] == '_' && t[b + 3] == ':' && t[b + 5] == ':')) ++b;
		const uint32_t len = b - a;
		if (len) {
			if (len < 5 || t[a + 2] != ':' || t[a + 4] != ':') return false;
			const char ty = t[a + 3];
			const uint32_t v = a + 5, vn = b - v;
			if (ty == 'i') {
				uint32_t q = v;
				int32_t x;
				if (!bo_number(t, &q, b, true, &x) || q != b) return false;
				be_tag_int(g, o, t[a], t[a + 1], x);
			} else if (ty == 'A') {
				be_u8(g, o, (uint8_t)t[a]), be_u8(g, o, (uint8_t)t[a + 1]), be_u8(g, o, 'A'), be_u8(g, o, vn ? (uint8_t)t[v] : ' ');
			} else if (ty == 'Z' || ty == 'H') {
				be_u8(g, o, (uint8_t)t[a]), be_u8(g, o, (uint8_t)t[a + 1]), be_u8(g, o, (uint8_t)ty), be_copy(g, o, t + v, vn), be_u8(g, o, 0);
			} else return false;
		}
		a = b + 1;
	}
	return true;
}

// read k of a kept pair: 0 skipped, 1 the sink has walked its record, 2 declined (the sink's position is then of no use)
template <class S> PSVR_FQ int bo_read(const FqGroup &g, const BoInput &in, int64_t p, int k, const BoText &T, S &o)
{
	const int64_t wr = 2 * (in.first_pair + p) + k;
	const psvr_ori_t &ori = in.ori[wr];
	const uint32_t ref_bg = ori.ref_bg >= 0x7fffffffu ? 1u : ori.ref_bg;
	if (ori.chr_id < 0 || ori.chr_id >= in.n_header) return 0;
	if ((int64_t)(int32_t)(ref_bg + 1u) - 1 < 0) return 0;
	const uint64_t *ls = in.line_start + 4 * wr;
	const uint32_t hl = fq_trimmed_len(in.text, ls[0], ls[1]), ne = in.name_end[wr];
	const char *nt = in.text + ls[0] + (hl ? 1 : 0), *st = in.text + ls[1], *qt = in.text + ls[3];
	const uint32_t nn = hl && ne ? ne - 1 : 0, n = fq_trimmed_len(in.text, ls[1], ls[2]), qn = fq_trimmed_len(in.text, ls[3], ls[4]);
	if (nn == 0 || nn > 254 || qn != n || n == 0 || (n == 1 && st[0] == '*')) return 2;
	const bool has_cigar = !bo_no_cigar(T);
	uint32_t n_ops = 0;
	int64_t rlen = 0;
	if (has_cigar) {
		BeCount c;
		if (!bo_cigar(g, c, T, &n_ops, &rlen) || n_ops > 0xffffu) return 2;
	}
	const uint32_t flag = (uint32_t)T.flag | (has_cigar ? 0u : 4u);
	S body = o;                                              // behind block_size, which is known when the record's end is
	body.pos += 4;
	const int64_t p0 = (int64_t)(int32_t)(ref_bg + 1u) - 1;
	be_u32(g, body, (uint32_t)ori.chr_id), be_u32(g, body, (uint32_t)(int32_t)p0);
	be_u8(g, body, nn + 1), be_u8(g, body, (uint8_t)T.mapq);
	be_u16(g, body, (unsigned)bam_reg2bin(p0, p0 + (has_cigar && !(flag & 4u) ? rlen : 1)));
	be_u16(g, body, n_ops), be_u16(g, body, flag & 0xffffu), be_u32(g, body, n);
	const int32_t mp = T.mate_b + 1;
	const int32_t mtid = T.mate_chr >= 0 && T.mate_chr < in.n_header && !(mp - 1 < 0) ? T.mate_chr : -1;
	be_u32(g, body, (uint32_t)mtid), be_u32(g, body, (uint32_t)T.mate_b), be_u32(g, body, (uint32_t)T.isize);
	be_copy(g, body, nt, nn), be_u8(g, body, 0);
	if (has_cigar) bo_cigar(g, body, T, &n_ops, &rlen);
	be_seq_qual(g, body, st, qt, n, (T.flag & 0x10) != 0, n == 1 && qt[0] == '*');
	if (!bo_tags(g, body, T)) return 2;
	be_tag_int(g, body, 'M', 'S', in.pairs[p].max_score);
	be_u32(g, o, (uint32_t)(body.pos - o.pos - 4));          // block_size
	o.pos = body.pos;
	return 1;
}

// a '\t' or NUL in the comment of window read wr; its span
PSVR_FQ bool bo_comment(const FqGroup &g, const BoInput &in, int64_t wr, const char **ct, uint32_t *cn)
{
	const uint64_t *ls = in.line_start + 4 * wr;
	const uint32_t hl = fq_trimmed_len(in.text, ls[0], ls[1]), ne = in.name_end[wr];
	const char *h = in.text + ls[0];
	if (ne < hl) *ct = h + ne + 1, *cn = hl - ne - 1; else *ct = h + hl, *cn = 0;
	for (uint32_t base = 0; base < *cn; base += FqGroup::width) {
		const uint32_t i = base + g.lane;
		const char ch = i < *cn ? (*ct)[i] : 'x';
		if (g.ballot(ch == '\t' || ch == 0)) return false;
	}
	return true;
}

// pair p: its state; for state 1 the sink has walked its records (*records of them)
template <class S> PSVR_FQ int bo_pair(const FqGroup &g, const BoInput &in, int64_t p, S &o, int32_t *records)
{
	*records = 0;
	const psvr_pair_result_t &pr = in.pairs[p];
	const int64_t w0 = 2 * (in.first_pair + p);
	if (!(pr.max_score <= in.min_filter_score && in.ori[w0].chr_id != -1 && in.ori[w0 + 1].chr_id != -1)) return 0;
	const char *c0, *c1;
	uint32_t n0, n1;
	const bool ok0 = bo_comment(g, in, w0, &c0, &n0), ok1 = bo_comment(g, in, w0 + 1, &c1, &n1);
	if (!ok0 || !ok1) return 2;
	BoText T0, T1;                                           // (two named records, not an array: they stay in registers)
	int s = bo_parse(c0, n0, &T0);
	if (s != 1) return s;
	s = bo_parse(c1, n1, &T1);
	if (s != 1) return s;
	bool proper = pr.proper != 0;
	for (int k = 0; proper && k < 2; ++k) {
		const int32_t mx = k == 0 ? pr.max1 : pr.max2;
		if (mx == -1) proper = false;
		else if (mx == -2) { if (bo_has_clip(k == 0 ? T0 : T1, 25)) proper = false; }
		else {
			int64_t ci;
			if (!be_index(in.hdr[2 * p + k].cand_off, mx, in.n_cands, &ci)) return 2;
			const psvr_cand_t &cd = in.cands[ci];
			if (cd.cigar_off < 0 || cd.cigar_off > in.n_cig || (int64_t)cd.n_cigar > in.n_cig - cd.cigar_off) return 2;
			int64_t tot = 0;
			for (uint32_t j = g.lane; j < cd.n_cigar; j += FqGroup::width) {
				const uint32_t w = in.cig[cd.cigar_off + j];
				if ((w & 0xf) == 1) tot += (int32_t)(int16_t)(uint16_t)(w >> 4);
			}
			tot = be_group_sum(g, tot);
			if (cd.n_cigar == 0 || tot >= 25) proper = false;
		}
	}
	if (proper) return 0;
	const int s0 = bo_read(g, in, p, 0, T0, o);
	if (s0 == 2) return 2;
	const int s1 = bo_read(g, in, p, 1, T1, o);
	if (s1 == 2) return 2;
	*records = (s0 == 1) + (s1 == 1);
	return *records ? 1 : 0;
}

// the size pass for one pair: state, bytes, records
PSVR_FQ int bo_pair_size(const FqGroup &g, const BoInput &in, int64_t p, int32_t *bytes, int32_t *records)
{
	BeCount c;
	int st = bo_pair(g, in, p, c, records);
	if (st == 1 && c.pos > 0x7fffffffull) st = 2;
	if (st != 1) *records = 0;
	*bytes = st == 1 ? (int32_t)c.pos : 0;
	return st;
}

#if !defined(__HIPCC__)
// the same passes with one lane
inline void bo_emit_host(const BoInput &in, int64_t P, BeHostResult *out)
{
	FqGroup g;
	out->state.assign((size_t)P, 0), out->pair_off.assign((size_t)P + 1, 0);
	out->n_records = out->n_written = out->n_declined = 0;
	for (int64_t p = 0; p < P; ++p) {
		int32_t nb, nr;
		const int st = bo_pair_size(g, in, p, &nb, &nr);
		out->state[(size_t)p] = (uint8_t)st, out->pair_off[(size_t)p + 1] = out->pair_off[(size_t)p] + nb;
		out->n_records += nr, out->n_written += st == 1, out->n_declined += st == 2;
	}
	out->bytes.assign((size_t)out->pair_off[(size_t)P], 0xEE);
	for (int64_t p = 0; p < P; ++p) {
		if (out->state[(size_t)p] != 1) continue;
		BeWrite w;
		w.out = out->bytes.data(), w.pos = (uint64_t)out->pair_off[(size_t)p];
		int32_t nr;
		bo_pair(g, in, p, w, &nr);
	}
}
#endif

} // namespace psvr
