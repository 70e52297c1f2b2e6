// signal_device.h -- the per-pair rules of `panSVR signal -N` (signal_step.h: SignalStep::pair and write_fastq) over record bytes, in the form
// the device runs them: the bodies of the kernels of signal.hip and, compiled for the host with one "lane", of the checker that holds them to
// SignalStep byte for byte (tests/tools/signal_device_check.cpp).  No HIP calls.  SignalStep::pair is the specification; the decision (is
// the pair written?) never needs the host, only the formatting of a pair is ever declined.
//
// A record is `rec`, a pointer to its block_size (bam_record.h), and must pass bam_rec_reader_fits and bam_rec_name_ends: name, CIGAR,
// bases and qualities lie inside it, the optional fields are what is left.  A pair (r1, r2) of consecutive primary records is in one state:
//   0  not written: it passes the filter (and -D is not given), or -U discards it
//   1  written here: the eight lines of its two reads
//   2  to be written, zero bytes here, the host formats it: a read holds a base code outside {1, 2, 4, 8, 15} (write_fastq prints
//      "Wrong base!" and a short sequence there: that behaviour stays in one place) -- or a quality of 223, whose character is the NUL that
//      ends the host's "%s", or a text that would not fit 2^31 - 1 bytes
//   3  the names of the two records differ (strcmp)
//   4  not first / second in template: !(flag1 & 0x40) || !(flag2 & 0x80)
//   5  would be written, but l_qseq of read 1 >= 2048
// and kSgNoteIsize of its note says "wrong ISIZE" where the host route prints that line (behind the -U return).
// The text is walked by ONE function, sg_pair, templated on its sink (bam_emit_device.h: BeCount adds up, BeWrite stores), so the size pass
// and the write pass cannot disagree.  Every lane of a group (fastq_device.h: FqGroup) walks the same control flow and keeps the same
// position; decimal text and literals are stored by the group's first lane, name / bases / qualities / tag strings by lane (i mod width).
// STAT_ (the create options' four numbers) goes behind the flag quartets of read 1 when stat_here: the caller gives it to the first pair
// that is written at all (states 1 and 2), once.
#pragma once
#include <stdint.h>
#include "../../include/psvr_engine.h"
#include "bam_emit_device.h"
#include "bam_record.h"

namespace psvr {

static const uint32_t kSgNoteIsize = 1;
static const int kSgMaxIsize = 100000, kSgMaxLen = 1000;     // BamStat's histograms

// the length of the C string at p, which has a NUL inside [p, p + n)
PSVR_FQ uint32_t sg_cstr_len(const FqGroup &g, const uint8_t *p, uint32_t n)
{
	for (uint32_t base = 0; base < n; base += FqGroup::width) {
		const uint32_t i = base + g.lane;
		const uint32_t z = g.ballot(i < n && p[i] == 0);
		if (z) return base + fq_ctz(z);
	}
	return n;
}
PSVR_FQ bool sg_primary(const uint8_t *rec) { return !(bam_u16(rec + 18) & 0x900); }
// strcmp(qname1, qname2) == 0
PSVR_FQ bool sg_same_name(const FqGroup &g, const uint8_t *r1, const uint8_t *r2)
{
	const uint32_t n1 = sg_cstr_len(g, r1 + kBamRecHead, r1[12]), n2 = sg_cstr_len(g, r2 + kBamRecHead, r2[12]);
	if (n1 != n2) return false;
	for (uint32_t base = 0; base < n1; base += FqGroup::width) {
		const uint32_t i = base + g.lane;
		if (g.ballot(i < n1 && r1[kBamRecHead + i] != r2[kBamRecHead + i])) return false;
	}
	return true;
}
// BamStat::collect: the bins of one record, -1: none
PSVR_FQ void sg_collect_bins(const uint8_t *rec, int32_t *isize_bin, int32_t *len_bin)
{
	const int32_t is = bam_i32(rec + 32), l = bam_i32(rec + 20);
	const uint32_t a = is < 0 ? 0u - (uint32_t)is : (uint32_t)is;
	*isize_bin = a > 0 && a < (uint32_t)kSgMaxIsize ? (int32_t)a : -1;
	*len_bin = l >= 0 && l < kSgMaxLen ? l : -1;
}

// one read of a pair as SignalStep::pair sees it
struct SgRead {
	const uint8_t *rec, *cig, *seq, *qual, *aux, *end;
	uint32_t flag, n_cigar, name_n;
	int32_t tid, pos, mtid, mpos, isize, l_qseq, mapq;
	int32_t lowq, soft_l, soft_r, indel_nm, score, xa, nm;
	bool has_nm, bad_base;
};

// the Z string of tag t0 t1 (string_tag: 'Z' only) and its length, or null
PSVR_FQ const uint8_t *sg_string_tag(const SgRead &R, char t0, char t1, uint32_t *len)
{
	const uint8_t *v = bam_aux_find(R.aux, R.end, t0, t1);
	if (!v || v[0] != 'Z') return nullptr;
	uint32_t n = 0;
	while (v[1 + n]) ++n;                                    // (bam_aux_find has seen its NUL inside the record)
	*len = n;
	return v + 1;
}

PSVR_FQ void sg_read(const FqGroup &g, const psvr_signal_opt_t &o, const uint8_t *rec, SgRead *R)
{
	R->rec = rec, R->tid = bam_i32(rec + 4), R->pos = bam_i32(rec + 8), R->mapq = rec[13], R->n_cigar = bam_u16(rec + 16), R->flag = bam_u16(rec + 18);
	R->l_qseq = bam_i32(rec + 20), R->mtid = bam_i32(rec + 24), R->mpos = bam_i32(rec + 28), R->isize = bam_i32(rec + 32);
	R->cig = rec + kBamRecHead + rec[12], R->seq = R->cig + 4 * (uint64_t)R->n_cigar, R->qual = R->seq + ((uint64_t)R->l_qseq + 1) / 2, R->aux = R->qual + R->l_qseq;
	R->end = rec + 4 + (uint64_t)bam_u32(rec);
	R->name_n = sg_cstr_len(g, rec + kBamRecHead, rec[12]);
	// get_bam_low_quality_num(0, 100000, '/'), and the base codes write_fastq has no letter for
	const uint32_t n = (uint32_t)R->l_qseq;
	int64_t lowq = 0, bad = 0;
	for (uint32_t k = g.lane; k < n; k += FqGroup::width) {
		if (k < 100000u) lowq += R->qual[k] < (uint8_t)'/';
		const uint32_t c = (R->seq[k >> 1] >> ((~k & 1u) << 2)) & 0xfu;
		bad += !(c == 1 || c == 2 || c == 4 || c == 8 || c == 15) || R->qual[k] == 223;   // (quality 223 prints as a NUL, which ends the host's "%s")
	}
	R->lowq = (int32_t)be_group_sum(g, lowq), R->bad_base = be_group_sum(g, bad) != 0;
	// bam_has_SH_cigar, bam_has_INDEL_NM, getScoreByCigar
	R->soft_l = R->soft_r = 0;
	if (R->n_cigar) {
		const uint32_t f = bam_u32(R->cig), l = bam_u32(R->cig + 4 * (uint64_t)(R->n_cigar - 1u));
		if ((f & 0xf) == 4 || (f & 0xf) == 5) R->soft_l = (int32_t)(f >> 4);
		if ((l & 0xf) == 4 || (l & 0xf) == 5) R->soft_r = (int32_t)(l >> 4);
	}
	int64_t indel = 0, score = 0;
	for (uint32_t k = g.lane; k < R->n_cigar; k += FqGroup::width) {
		const uint32_t w = bam_u32(R->cig + 4 * (uint64_t)k);
		const int32_t op = (int32_t)(w & 0xf), len = (int32_t)(w >> 4);
		if (op == 0 || op == 7) score += (int64_t)len * o.match;
		else if (op == 1 || op == 2 || op == 4 || op == 5) {
			if (op == 1 || op == 2) indel += len;
			const int64_t p1 = o.gap_open + (int64_t)len * o.gap_ex, p2 = o.gap_open2 + (int64_t)len * o.gap_ex2;
			score -= p1 < p2 ? p1 : p2;
		}
	}
	indel = be_group_sum(g, indel), score = be_group_sum(g, score);
	R->nm = 0;
	R->has_nm = bam_aux_int(bam_aux_find(R->aux, R->end, 'N', 'M'), &R->nm);
	R->indel_nm = (int32_t)(indel + R->nm);
	score -= (int64_t)(o.mismatch + o.match) * ((int64_t)R->nm - indel);
	R->score = score > 0 ? (int32_t)score : 0;
	// get_XA_number
	R->xa = 0;
	if (R->mapq <= 0) {
		uint32_t xn = 0;
		const uint8_t *xa = sg_string_tag(*R, 'X', 'A', &xn);
		if (!xa) R->xa = 6;
		else {
			int64_t c = 0;
			for (uint32_t k = g.lane; k < xn; k += FqGroup::width) c += xa[k] == ';';
			R->xa = (int32_t)be_group_sum(g, c);
		}
	}
}

PSVR_FQ char sg_base_char(uint32_t code, bool rc)
{
	switch (code) {
	case 1: return rc ? 'T' : 'A';
	case 2: return rc ? 'G' : 'C';
	case 4: return rc ? 'C' : 'G';
	case 8: return rc ? 'A' : 'T';
	}
	return 'N';
}

template <class S> PSVR_FQ void sg_num_(const FqGroup &g, S &o, int32_t x) { be_num(g, o, x), be_u8(g, o, '_'); }
template <class S> PSVR_FQ void sg_stat(const FqGroup &g, const psvr_signal_opt_t &opt, S &o)
{
	be_lit(g, o, "STAT_", 5);
	for (int k = 0; k < 4; ++k) sg_num_(g, o, opt.stat[k]);
}

template <class S> PSVR_FQ void sg_tag_z(const FqGroup &g, S &o, const SgRead &R, char t0, char t1)
{
	uint32_t n = 0;
	const uint8_t *v = sg_string_tag(R, t0, t1, &n);
	if (v) be_u8(g, o, (uint8_t)t0), be_u8(g, o, (uint8_t)t1), be_lit(g, o, ":Z:", 3), be_copy(g, o, (const char *)v, n), be_u8(g, o, '_');
}
// the flag quartet of a read (strand, unmapped, indel + NM > 8, clip > 10) as its four characters, first in the low byte
PSVR_FQ uint32_t sg_quartet(bool fwd, bool unmapped, bool indel, bool clip)
{
	return (uint32_t)(fwd ? 'F' : 'R') | (uint32_t)(unmapped ? 'Y' : 'N') << 8 | (uint32_t)(indel ? 'Y' : 'N') << 16 | (uint32_t)(clip ? 'Y' : 'N') << 24;
}

// one read's four lines: write_fastq with the comment SignalStep::pair builds for it
template <class S>
PSVR_FQ void sg_fastq(const FqGroup &g, const psvr_signal_opt_t &opt, const SgRead &R, const SgRead &M, int32_t isize, uint32_t fl, uint32_t ml, bool stat_here, S &o)
{
	be_u8(g, o, '@'), be_copy(g, o, (const char *)R.rec + kBamRecHead, R.name_n), be_u8(g, o, ' ');
	sg_num_(g, o, R.tid), sg_num_(g, o, R.pos), sg_num_(g, o, R.soft_l), sg_num_(g, o, R.score), sg_num_(g, o, R.mapq), sg_num_(g, o, M.mapq);
	sg_num_(g, o, R.xa), sg_num_(g, o, M.xa), sg_num_(g, o, isize);
	be_u32(g, o, fl), be_u8(g, o, '_'), be_u32(g, o, ml), be_u8(g, o, '_');
	if (stat_here) sg_stat(g, opt, o);
	be_lit(g, o, "FLAG_", 5), sg_num_(g, o, (int32_t)R.flag), sg_num_(g, o, R.mapq), be_lit(g, o, "CIGAR_", 6);
	for (uint32_t k = 0; k < R.n_cigar; ++k) {
		const uint32_t w = bam_u32(R.cig + 4 * (uint64_t)k), op = w & 0xf;
		be_num(g, o, (int32_t)(w >> 4));
		if (op < 10) be_u8(g, o, (uint8_t)"MIDNSHP=XB"[op]);     // (op 10 is the string's NUL on the host: nothing is printed)
	}
	be_u8(g, o, '_');
	be_lit(g, o, "MATE_", 5), sg_num_(g, o, R.mtid), sg_num_(g, o, R.mpos), sg_num_(g, o, R.isize), be_lit(g, o, "TAG_", 4);
	sg_tag_z(g, o, R, 'X', 'A'), sg_tag_z(g, o, R, 'M', 'C'), sg_tag_z(g, o, R, 'S', 'A');
	if (R.has_nm) be_lit(g, o, "NM:i:", 5), sg_num_(g, o, R.nm);
	be_u8(g, o, '\n');
	// bases and qualities; mapped and reverse: getReverseStr_char, and getReverseStr_qual with its len/2 + 1 bound (the two middle entries
	// of an even length are swapped twice)
	const uint32_t n = (uint32_t)R.l_qseq;
	const bool rev = !(R.flag & 0x4) && (R.flag & 0x10);
	if (S::writes) {
		for (uint32_t j = g.lane; j < n; j += FqGroup::width) {
			const uint32_t k = rev ? n - 1 - j : j;
			o.put(j, (uint8_t)sg_base_char((R.seq[k >> 1] >> ((~k & 1u) << 2)) & 0xfu, rev));
		}
		const bool even = !(n & 1) && n >= 2;
		for (uint32_t j = g.lane; j < n; j += FqGroup::width) {
			const bool keep = !rev || (even && (j == n / 2 - 1 || j == n / 2));
			o.put((uint64_t)n + 3 + j, (uint8_t)(R.qual[keep ? j : n - 1 - j] + 33));
		}
	}
	o.pos += n;
	be_lit(g, o, "\n+\n", 3);
	o.pos += n;
	be_u8(g, o, '\n');
}

// the pair's state; for state 1 the sink has walked its text.  Names and template flags (states 3 and 4) are the caller's run loop's tests,
// in front of everything else, as in SignalStep::run.
template <class S> PSVR_FQ int sg_pair(const FqGroup &g, const psvr_signal_opt_t &opt, const uint8_t *r1, const uint8_t *r2, bool stat_here, S &o, uint32_t *note)
{
	*note = 0;
	if (!sg_same_name(g, r1, r2)) return 3;
	if (!(bam_u16(r1 + 18) & 0x40) || !(bam_u16(r2 + 18) & 0x80)) return 4;
	SgRead A, B;                                             // (two named reads, not an array: they stay in registers)
	sg_read(g, opt, r1, &A), sg_read(g, opt, r2, &B);
	const int32_t isize = (int32_t)(A.isize < 0 ? 0u - (uint32_t)A.isize : (uint32_t)A.isize);
	if (opt.discard_full_match) {
		const int64_t min_score = ((int64_t)A.l_qseq + B.l_qseq) * opt.match - 4 * (int64_t)(opt.match + opt.mismatch);
		const bool near_full = (int64_t)A.score + B.score >= min_score, isize_ok = isize != 0 && isize > opt.isize_min && isize < opt.isize_max;
		if (near_full && isize_ok && A.tid == B.tid && A.tid <= opt.max_tid && B.tid <= opt.max_tid) return 0;
	}
	if ((int64_t)A.isize + B.isize != 0 && A.isize != B.isize) *note |= kSgNoteIsize;
	bool dirA = !(A.flag & 0x10), dirB = !(B.flag & 0x10);
	if (A.pos > B.pos) { const bool t = dirA; dirA = dirB, dirB = t; }
	if (isize == A.l_qseq && isize == B.l_qseq && !dirA && dirB) dirA = true, dirB = false;
	const bool unA = (A.flag & 0x4) != 0, unB = (B.flag & 0x4) != 0;
	int32_t clipA = A.soft_l + A.soft_r, clipB = B.soft_l + B.soft_r, inA = A.indel_nm, inB = B.indel_nm, lqA = A.lowq, lqB = B.lowq;
	const uint32_t fa = sg_quartet(!(A.flag & 0x10), unA, inA > 8, clipA > 10), fb = sg_quartet(!(B.flag & 0x10), unB, inB > 8, clipB > 10);
	// 1 NM or INDEL in 2 low-quality bases
	clipA -= lqA; if (clipA < 0) lqA = -clipA, clipA = 0;
	lqA >>= 1, inA -= lqA; if (inA < 0) inA = 0;
	clipB -= lqB; if (clipB < 0) lqB = -clipB, clipB = 0;
	lqB >>= 1, inB -= lqB; if (inB < 0) inB = 0;
	bool pass = true;
	if (A.mapq < 10 && B.mapq < 10) pass = false;            // reason bit 1
	if (unA || unB) pass = false;                            // 2
	if (isize > 1000) pass = false;                          // 4
	if (!dirA || dirB) pass = false;                         // 8
	if (inA + inB > 15) pass = false;                        // 16
	if (clipA + clipB > 10) pass = false;                    // 32
	if (A.tid != B.tid || A.tid > opt.max_tid || B.tid > opt.max_tid) pass = false;   // 64
	if (pass && !opt.not_use_filter) return 0;
	if (!(A.l_qseq < 2048)) return 5;
	if (A.bad_base || B.bad_base) return 2;
	sg_fastq(g, opt, A, B, isize, fa, fb, stat_here, o);
	sg_fastq(g, opt, B, A, isize, fb, fa, false, o);
	return 1;
}

// the size pass for one pair (without STAT_: sg_stat_bytes on top for the pair that carries it)
PSVR_FQ int sg_pair_size(const FqGroup &g, const psvr_signal_opt_t &opt, const uint8_t *r1, const uint8_t *r2, int32_t *bytes, uint32_t *note)
{
	BeCount c;
	int st = sg_pair(g, opt, r1, r2, false, c, note);
	if (st == 1 && c.pos > 0x7fffff00ull) st = 2;
	*bytes = st == 1 ? (int32_t)c.pos : 0;
	return st;
}
PSVR_FQ int32_t sg_stat_bytes(const FqGroup &g, const psvr_signal_opt_t &opt)
{
	BeCount c;
	sg_stat(g, opt, c);
	return (int32_t)c.pos;
}

} // namespace psvr
