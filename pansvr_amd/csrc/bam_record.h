// bam_record.h -- what a BAM alignment record is (SAMv1 sections 4.2 and 5.3), once, for everything that looks into one: the host's
// sorter and reader (sorted_bam.h, bam_reader.h), the encoders (bam_writer.h, sam_emit.h, bam_emit_device.h), the record store's kernels and
// its host pre-walk (bam_store.hip) and the record-chain finder (bam_chain_device.h).  Compiled for the host and for the device, as
// bam_chain_device.h is; no STL, no allocation; tests/tools/bam_record_check.cpp holds it to a Python restatement under AddressSanitizer.
// A record is handed over as `rec`, a pointer to its block_size field:
//   rec + 0 block_size | 4 refID | 8 pos | 12 l_read_name | 13 mapq | 14 bin | 16 n_cigar_op | 18 flag | 20 l_seq | 24 next_refID | 28 next_pos |
//   32 tlen | 36 read_name, cigar, seq, qual, aux                                                  (block_size counts everything behind itself)
//   loads          bam_u16 / bam_u32 / bam_i32: little-endian, from any address
//   the span       bam_cigar_ref_len(word): the reference bases one CIGAR word covers (M D N = X), all 28 bits of its length;
//                  bam_rec_ref_span(rec): their sum over the record's CIGAR
//   the bin        bam_reg2bin(beg, end)
//   the sort key   bam_sort_key(tid, pos, flag): samtools' coordinate order (bam_sort.c bam1_lt) as one unsigned number, exact while
//                  bam_key_exact(pos)
//   the fields     bam_rec_derived(rec, &m): tid, pos, end, len, bin and flag as the sorter, the store's table and the .bai builder use them
//   the validity   bam_rec_frame -> bam_rec_cigar_inside (the formatter's rule) or bam_rec_reader_fits -> bam_rec_name_ends (the reader's);
//                  every layer reads only what the layers before it have vouched for
//   the tags       bam_aux_find(aux begin, aux end, t0, t1): the reader's bam_aux_get walk with its size rules; bam_aux_int: the integer codes
#pragma once
#include <stdint.h>
#include <string.h>

#if defined(__HIPCC__)
#define PSVR_BR __host__ __device__ inline
#else
#define PSVR_BR inline
#endif

namespace psvr {

static const uint32_t kBamRecHead = 36;                      // block_size and the fixed part
static const uint32_t kBamRecMinBlock = 32;                  // the fixed part alone
// The largest block_size the record store takes (bam_store.hip, and the chain finder that feeds it): its lengths go through an int32 scan.
// No rule of the format: the host routes have no such bound, and no function below applies it.
static const uint32_t kBamRecStoreMaxBlock = 0x7ffffff0u;

PSVR_BR uint16_t bam_u16(const uint8_t *p) { uint16_t v; memcpy(&v, p, 2); return v; }
PSVR_BR uint32_t bam_u32(const uint8_t *p) { uint32_t v; memcpy(&v, p, 4); return v; }
PSVR_BR int32_t bam_i32(const uint8_t *p) { return (int32_t)bam_u32(p); }

// Reference bases one CIGAR word covers: its length when the op is M, D, N, = or X.  The length is the word's upper 28 bits: an encoder that
// has written (uint32)len << 4 | op covers (uint32)len & 0xfffffff bases, whatever sign bits len had.
PSVR_BR int64_t bam_cigar_ref_len(uint32_t word)
{
	const uint32_t op = word & 0xf;
	return op == 0 || op == 2 || op == 3 || op == 7 || op == 8 ? (int64_t)(word >> 4) : 0;
}
// ... and the whole CIGAR's (of a record whose CIGAR lies inside it: bam_rec_cigar_inside)
PSVR_BR int64_t bam_rec_ref_span(const uint8_t *rec)
{
	const uint8_t *cig = rec + kBamRecHead + rec[12];
	const uint32_t n_cig = bam_u16(rec + 16);
	int64_t span = 0;
	for (uint32_t k = 0; k < n_cig; ++k) span += bam_cigar_ref_len(bam_u32(cig + 4 * k));
	return span;
}

PSVR_BR int bam_reg2bin(int64_t beg, int64_t end)            // SAMv1 section 5.3
{
	--end;
	if (beg >> 14 == end >> 14) return (int)(((1 << 15) - 1) / 7 + (beg >> 14));
	if (beg >> 17 == end >> 17) return (int)(((1 << 12) - 1) / 7 + (beg >> 17));
	if (beg >> 20 == end >> 20) return (int)(((1 << 9) - 1) / 7 + (beg >> 20));
	if (beg >> 23 == end >> 23) return (int)(((1 << 6) - 1) / 7 + (beg >> 23));
	if (beg >> 26 == end >> 26) return (int)(((1 << 3) - 1) / 7 + (beg >> 26));
	return 0;
}

// samtools' coordinate order as a key: reference id as unsigned (unplaced records last), position, forward strand before reverse.  The
// position's field is 32 bits of pos + 1: it orders as the comparator for every pos in [-1, 2^31 - 2]
PSVR_BR uint64_t bam_sort_key(int32_t tid, int32_t pos, uint32_t flag)
{
	return (uint64_t)(uint32_t)tid << 32 | (uint64_t)(((uint32_t)pos + 1u) << 1) | ((flag >> 4) & 1);
}
PSVR_BR bool bam_key_exact(int32_t pos) { return pos >= -1 && pos <= 0x7ffffffe; }

// What a sorter and an index need of a record (bam_rec_cigar_inside holds), into the members of *m that carry these names (the members of
// psvr_bam_rec_meta_t that do not depend on where the record is stored): the record covers [max(pos, 0), end) on its reference, a CIGAR
// without reference bases counts as one base; len = the record with its block_size; bin = the 16 bits the record's own field holds
template <class M> PSVR_BR void bam_rec_derived(const uint8_t *rec, M *m)
{
	const int32_t pos = bam_i32(rec + 8);
	const int64_t span = bam_rec_ref_span(rec), beg = pos < 0 ? 0 : pos, end = beg + (span > 0 ? span : 1);
	m->tid = bam_i32(rec + 4), m->pos = pos, m->end = end, m->len = 4 + bam_u32(rec);
	m->bin = (uint16_t)bam_reg2bin(beg, end), m->flag = bam_u16(rec + 18);
}

// ---- is this a whole, well-formed record?  `avail` bytes are there from rec on
// The frame, everybody's rule: the head is there, block_size holds at least the fixed part, and the record ends inside the bytes given.
// (The chain finder decides the same three in an order of its own, for its four verdicts: chain_record, bam_chain_device.h.)
PSVR_BR bool bam_rec_frame(const uint8_t *rec, uint64_t avail)
{
	if (avail < kBamRecHead) return false;
	const uint32_t bs = bam_u32(rec);
	return bs >= kBamRecMinBlock && bs <= avail - 4;
}
// The formatter's rule (SortRecords::add_stream and the store's appends, which take what the project's own encoders wrote): inside a frame,
// name + CIGAR lie inside the record -- all that bam_rec_derived reads
PSVR_BR bool bam_rec_cigar_inside(const uint8_t *rec)
{
	return (uint64_t)rec[12] + 4 * (uint64_t)bam_u16(rec + 16) <= (uint64_t)bam_u32(rec) - kBamRecMinBlock;
}
// The reader's rule (BamReader::next and the chain finder, which take files from anywhere): given the head and bs, a block_size of at least
// the fixed part, l_seq >= 0, a name of at least min_name bytes, and name + CIGAR + bases + qualities lie inside the record.  (k_chain_guess
// runs this for every byte offset of a BAM file; the order of the tests and n_cigar_op's two byte loads are the form it was measured in.)
PSVR_BR bool bam_rec_fields_fit(const uint8_t *rec, uint32_t bs, uint32_t min_name)
{
	const uint64_t l_name = rec[12], n_cig = rec[16] | (uint32_t)rec[17] << 8;
	const int32_t l_seq = bam_i32(rec + 20);
	if (l_seq < 0) return false;
	return l_name >= min_name && l_name + 4 * n_cig + ((uint64_t)l_seq + 1) / 2 + (uint64_t)l_seq <= (uint64_t)bs - kBamRecMinBlock;
}
// ... as BamReader::next asks it, which reports a missing name with the name's NUL
PSVR_BR bool bam_rec_fields_inside(const uint8_t *rec) { return bam_rec_fields_fit(rec, bam_u32(rec), 0); }
// ... and whole, with a name of at least one byte (bs: the record's block_size, for a caller that has loaded it)
PSVR_BR bool bam_rec_reader_fits(const uint8_t *rec, uint32_t bs) { return bam_rec_fields_fit(rec, bs, 1); }
PSVR_BR bool bam_rec_reader_fits(const uint8_t *rec) { return bam_rec_reader_fits(rec, bam_u32(rec)); }
// The name's NUL (the reader's again: the name is used as a C string), of a record that is there and passes bam_rec_reader_fits
PSVR_BR bool bam_rec_name_ends(const uint8_t *rec) { return rec[kBamRecHead + rec[12] - 1] == 0; }

// ---- the optional fields [p, e) behind the qualities (SAMv1 section 4.2.4)
// bam_aux_get: the type byte of tag t0 t1, or null.  The walk ends with "not found" at an unknown type and at a value that leaves [p, e)
// (Z / H: its NUL included), so whoever reads the value it returns stays inside the record.
PSVR_BR const uint8_t *bam_aux_find(const uint8_t *p, const uint8_t *e, char t0, char t1)
{
	while (e - p >= 3) {
		const bool hit = p[0] == (uint8_t)t0 && p[1] == (uint8_t)t1;
		const uint8_t *v = p + 2, *val = v + 1;
		uint64_t sz = 0;
		switch ((char)v[0]) {
		case 'A': case 'c': case 'C': sz = 1; break;
		case 's': case 'S': sz = 2; break;
		case 'i': case 'I': case 'f': sz = 4; break;
		case 'd': sz = 8; break;
		case 'Z': case 'H': {
			const uint8_t *q = val;
			while (q < e && *q) ++q;
			if (q >= e) return nullptr;                          // no terminator inside the record
			sz = (uint64_t)(q - val) + 1;
			break;
		}
		case 'B': {
			if (e - val < 5) return nullptr;
			const char st = (char)val[0];
			const uint32_t cnt = bam_u32(val + 1);
			sz = 5 + (uint64_t)((st == 'c' || st == 'C') ? 1 : (st == 's' || st == 'S') ? 2 : 4) * cnt;
			break;
		}
		default: return nullptr;
		}
		if (sz > (uint64_t)(e - val)) return nullptr;            // the value runs past the record
		if (hit) return v;
		p = val + sz;
	}
	return nullptr;
}
// bam_get_num_tag (clib/bam_file.c:456-468) of a type byte bam_aux_find returned: the six integer codes only
PSVR_BR bool bam_aux_int(const uint8_t *v, int32_t *num)
{
	if (!v) return false;
	switch ((char)v[0]) {
	case 'c': *num = (int8_t)v[1]; return true;
	case 'C': *num = v[1]; return true;
	case 's': *num = (int16_t)bam_u16(v + 1); return true;
	case 'S': *num = bam_u16(v + 1); return true;
	case 'i': case 'I': *num = bam_i32(v + 1); return true;
	}
	return false;
}

} // namespace psvr
