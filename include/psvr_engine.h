/*
 * psvr_engine.h -- C ABI of the MI355X (gfx950) re-alignment engine.
 *
 * This is the drop-in boundary for panSVR's `aln` / `fc_aln` hot path.  Every entry point
 * names the reference interface it replaces (paths relative to the panSVR tree).
 * Plain C types only; no exceptions cross the boundary; every call returns an int status
 * (0 = PSVR_OK) and psvr_last_error() describes the last failure on the calling thread.
 *
 * Seam B2 (kernel):  psvr_extd2_batch*  replaces  ksw_extd2_sse   (src/kswlib/ksw2.h:63-64)
 *                    psvr_extz2_batch   replaces  ksw_extz2_sse   (src/kswlib/ksw2.h:57-58)
 * Seam B3 (seeding): psvr_seed_search_kmer_batch, psvr_seed_mem_batch
 *                                       replace   deBGA_INDEX::search_kmer / UNITIG_MEM_search
 *                                                 (src/deBGA_index.hpp:205-208; built copy
 *                                                  src/PanSVgenerateVCF/deBGA_index.hpp:198-201)
 * Seam B1 (batch):   psvr_engine_*      replaces  kt_for(worker_for -> align_read_pair)
 *                                                 (src/jlra_aln.cpp:115,140-147;
 *                                                  src/PanSVgenerateVCF/read_realignment.cpp:114,154-161,745-803)
 */
#ifndef PSVR_ENGINE_H_
#define PSVR_ENGINE_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PSVR_OK                0
#define PSVR_ERR_ARG           1   /* bad argument (null pointer, negative size, ...) */
#define PSVR_ERR_UNSUPPORTED   2   /* shape/flag outside what the device kernels implement */
#define PSVR_ERR_DEVICE        3   /* HIP runtime error (message in psvr_last_error) */
#define PSVR_ERR_NOMEM         4
#define PSVR_ERR_IO            5   /* index files missing / malformed */
#define PSVR_ERR_OVERFLOW      6   /* a caller-provided output arena was too small */

const char *psvr_last_error(void);
/* number of visible HIP devices; <0 on error.  Never falls back to a CPU path. */
int psvr_device_count(void);
/* Page-locked host memory for the buffers handed to psvr_engine_upload / psvr_engine_download / psvr_engine_align_batch
 * (optional: any host memory works, page-locked memory moves at the link's rate instead of a third of it).  The reference
 * side keeps its read / record buffers alive across batches (Classify_buff_pool, read_realignment.hpp:324-345): allocate
 * them once with these.  NULL on failure (psvr_last_error says why). */
void *psvr_host_alloc(size_t bytes);
void psvr_host_free(void *p);
/* Optional: sets up the device's queues on a thread of its own and returns at once.  The first streams of a process cost 3 - 14 ms each
 * and an engine uses four; a caller that has something else to do first (the command: loading the index, src/jlra_aln.cpp:29-57 in the
 * reference's order of work) calls this before it and finds them ready when it creates its engines.  Nothing depends on it. */
int psvr_device_warmup(int device, int n_streams);

/* ------------------------------------------------------------------------------------------
 * Seam B2: batched banded DP.  Field-for-field ksw_extz_t (src/kswlib/ksw2.h:26-35); the
 * CIGAR is written to a caller arena at [cigar_off, cigar_off + n_cigar) instead of a
 * callee-realloc'ed pointer (the reference's kalloc/malloc mix-up is not reproduced).
 * ------------------------------------------------------------------------------------------ */
#define PSVR_KSW_NEG_INF (-0x40000000)
#define PSVR_EZ_SCORE_ONLY  0x01
#define PSVR_EZ_RIGHT       0x02
#define PSVR_EZ_GENERIC_SC  0x04
#define PSVR_EZ_APPROX_MAX  0x08
#define PSVR_EZ_APPROX_DROP 0x10
#define PSVR_EZ_EXTZ_ONLY   0x40
#define PSVR_EZ_REV_CIGAR   0x80

typedef struct psvr_extz {
	int32_t max, zdropped;
	int32_t max_q, max_t;
	int32_t mqe, mqe_t;
	int32_t mte, mte_q;
	int32_t score;
	int32_t n_cigar;
	int32_t reach_end;
	int32_t reserved;
	int64_t cigar_off;      /* first op of this alignment in the cigar arena (uint32 units) */
} psvr_extz_t;

/* the scalar arguments of ksw_extd2_sse, in its order (m, mat, q, e, q2, e2, w, zdrop, end_bonus, flag) */
typedef struct psvr_ksw_params {
	int8_t  m;              /* alphabet size (5) */
	int8_t  mat[25];        /* m*m scoring matrix (KSW_ALN_handler::ksw_gen_mat_D, read_realignment.cpp:829-843) */
	int8_t  q, e, q2, e2;   /* gap open/extend pairs; extz2 uses q,e only */
	int32_t w;              /* band width (<0 disables) */
	int32_t zdrop;
	int32_t end_bonus;
	int32_t flag;           /* PSVR_EZ_* */
} psvr_ksw_params_t;

/* Upper bound of CIGAR ops alignment (qlen,tlen) can emit; the arena needs the sum over the batch. */
static inline int64_t psvr_cigar_bound(int32_t qlen, int32_t tlen) { return (int64_t)qlen + tlen + 2; }

/*
 * Host-buffer form: n independent problems; problem i has query  qseq[q_off[i] .. +qlen[i])  and
 * target tseq[t_off[i] .. +tlen[i]) with codes 0..m-1.  Results in ez[i]; CIGAR ops (BAM encoding
 * len<<4|op) in cigar_arena (capacity cigar_cap uint32).  Runs on HIP device `device`.
 * Accepted domain: any 0 <= qlen, tlen < 2^28 (longer sequences: PSVR_ERR_UNSUPPORTED), bounded by device memory.
 * A problem's workspace is its direction bytes, ((qlen + tlen - 1) * n_col + 1) * 16 bytes with
 * n_col = (min(qlen, tlen, w + 1) + 15) / 16 + 1 (none under PSVR_EZ_SCORE_ONLY for sequences over 8000 bases),
 * plus about 12 * tlen bytes when a sequence is longer than 8000 bases.  The batch runs in groups of
 * consecutive problems whose workspace stays under min(4 GiB, half the free device memory); a problem
 * larger than that runs alone, and if its workspace exceeds the free device memory the call returns
 * PSVR_ERR_NOMEM with the byte count in psvr_last_error().
 */
int psvr_extd2_batch(int device, int64_t n,
                     const uint8_t *qseq, const int64_t *q_off, const int32_t *qlen,
                     const uint8_t *tseq, const int64_t *t_off, const int32_t *tlen,
                     const psvr_ksw_params_t *par,
                     psvr_extz_t *ez, uint32_t *cigar_arena, int64_t cigar_cap);

int psvr_extz2_batch(int device, int64_t n,
                     const uint8_t *qseq, const int64_t *q_off, const int32_t *qlen,
                     const uint8_t *tseq, const int64_t *t_off, const int32_t *tlen,
                     const psvr_ksw_params_t *par,
                     psvr_extz_t *ez, uint32_t *cigar_arena, int64_t cigar_cap);

/*
 * Device-pointer form (same domain; all pointers are HIP device memory, `stream` is a hipStream_t or NULL):
 * nothing is copied and nothing synchronises; `work` is a device workspace of at least
 * psvr_dp_plan_workspace_bytes(plan) bytes.  ez[i].cigar_off must be pre-set by the caller
 * (e.g. an exclusive scan of psvr_cigar_bound).  tools/dp_bench.py times this form; bench.py times
 * psvr_engine_run (the whole path).
 */
typedef struct psvr_dp_plan psvr_dp_plan_t;   /* opaque: size classes + index lists for one batch shape */
int psvr_dp_plan_create(int device, int64_t n, const int32_t *qlen_host, const int32_t *tlen_host,
                        const psvr_ksw_params_t *par, int variant /*0 extd2, 1 extz2*/, psvr_dp_plan_t **plan);
int64_t psvr_dp_plan_workspace_bytes(const psvr_dp_plan_t *plan);
int psvr_dp_plan_launch(psvr_dp_plan_t *plan,
                        const uint8_t *d_qseq, const int64_t *d_q_off,
                        const uint8_t *d_tseq, const int64_t *d_t_off,
                        psvr_extz_t *d_ez, uint32_t *d_cigar_arena, void *d_work, void *stream);
/* fills n_kernels/name/launch geometry of the plan for profiling reports */
int psvr_dp_plan_describe(const psvr_dp_plan_t *plan, char *buf, size_t buflen);
void psvr_dp_plan_destroy(psvr_dp_plan_t *plan);

/*
 * What the planners derive from a parameter set before they look at a shape (no device is touched): the predicates that decide
 * which kernel families a problem may go to.  The tests hold them against the reference library's behaviour.
 */
typedef struct psvr_dp_regime {
	int32_t skip;           /* the reference returns right after ksw_reset_extz for these parameters */
	int32_t swapped;        /* extd2: the gap pairs arrived with q+e > q2+e2 and were exchanged */
	int32_t nowrap_ok;      /* in-band values provably fit int8 (the bound holds and the boundary costs are the recurrences'): the team / tiny kernels may run */
	int32_t zdrop_inert;    /* extd2: the z-drop rule cannot fire whatever the sequences: the engine's lean team variant may run */
	int32_t long_thres;
	int32_t qe_shift;       /* pre-swap q+e minus post-swap q+e (0 for pairs in plain order) */
} psvr_dp_regime_t;
int psvr_dp_regime(const psvr_ksw_params_t *par, int variant /*0 extd2, 1 extz2*/, psvr_dp_regime_t *out);


/* ------------------------------------------------------------------------------------------
 * The deBGA unipath k-mer index, resident in HBM.
 * Replaces deBGA_INDEX::load_index_file + building_chr_index + building_bam_header
 * (src/deBGA_index.cpp:40-86,363-439 / src/PanSVgenerateVCF/deBGA_index.cpp:33-80,354-431).
 * The nine files are uploaded once; the 2 GiB first-level table `unipath_g.hash` stays a dense
 * uint64[4^14+1] prefix-sum array so that one 16-byte gather returns hash[h], hash[h+1].
 * ------------------------------------------------------------------------------------------ */
typedef struct psvr_index psvr_index_t;

typedef struct psvr_index_view {           /* host pointers, element counts (not bytes) */
	const uint64_t *ref_seq;  uint64_t n_ref_seq;   /* ref.seq          2-bit MSB-first, 32 bases/word */
	const uint64_t *seq;      uint64_t n_seq;       /* unipath.seqb     same packing */
	const uint64_t *seqf;     uint64_t n_seqf;      /* unipath.seqfb    unipath start offsets (U+1) */
	const uint64_t *pos;      uint64_t n_pos;       /* unipath.pos      1-based reference positions */
	const uint64_t *posp;     uint64_t n_posp;      /* unipath.posp     (U+1) */
	const uint64_t *hash;     uint64_t n_hash;      /* unipath_g.hash   4^14+1 prefix sums */
	const uint32_t *kmer;     uint64_t n_kmer;      /* unipath_g.kmer   low 16 bits of each 22-mer */
	const uint64_t *off;      uint64_t n_off;       /* unipath_g.offset */
	const char *chr_text;                           /* contents of unipath.chr (name, cumulative end+1 alternating) */
	const char *const *header_names; int32_t n_header; /* @SQ names of the ORIGINAL genome header (bam_name2id lookups) */
} psvr_index_view_t;

int psvr_index_create(const psvr_index_view_t *view, int device, psvr_index_t **out);
/* The same with the eight arrays of `view` already in the memory of `device` (device pointers; chr_text / header_names stay host
 * pointers): one process per GPU receives them through a collective -- rank 0 uploads, an RCCL broadcast over xGMI brings them to
 * the other ranks (SURVEY 8(e) "broadcast index"; bench.py --gpus N) -- and builds its index from them, device to device. */
int psvr_index_create_from_device(const psvr_index_view_t *view, int device, psvr_index_t **out);
/* reads the nine files from `index_dir` and the @SQ lines of `header_sam` */
int psvr_index_load(const char *index_dir, const char *header_sam, int device, psvr_index_t **out);
/* Multi-GPU: a second copy of an index that is already resident on another device, moved device to device (xGMI peer
 * copies instead of N host uploads; SURVEY 8(e) "broadcast index").  `src` stays valid. */
int psvr_index_clone(const psvr_index_t *src, int device, psvr_index_t **out);
/* The index straight from the anchor FASTA (what `deBGA index -k 22` + load_index_file do through nine files: the builder of
 * `panSVR index` runs on the host, the 2 GiB first-level table is expanded in HBM and never exists on the host or on disk) */
int psvr_index_build(const char *anchors_fa, const char *header_sam, int device, psvr_index_t **out);
void psvr_index_destroy(psvr_index_t *idx);
int64_t psvr_index_device_bytes(const psvr_index_t *idx);
int32_t psvr_index_n_anchor(const psvr_index_t *idx);
/* SV_chr_info::vcf_print_string / vcf_id of anchor `sv_id` (deBGA_index.hpp:116-119); NULL if out of range */
const char *psvr_index_sv_print_string(const psvr_index_t *idx, int32_t sv_id);
const char *psvr_index_sv_vcf_id(const psvr_index_t *idx, int32_t sv_id);

/* ------------------------------------------------------------------------------------------
 * Seam B3: the two index look-ups of the seed loop, batched (src/PanSVgenerateVCF/deBGA_index.hpp:198-201; north-star copy
 * src/deBGA_index.hpp:205-208).  The engine runs the same device functions inside its seeding kernel; these entry points
 * expose them on their own (host buffers in, host buffers out) so the seeding stage can be bound or tested separately.
 * ------------------------------------------------------------------------------------------ */
/* bool deBGA_INDEX::search_kmer(20, kmer, range, 2) for n 20-mers (40 significant bits each): found[i], and when found the
 * inclusive index range range[2i] .. range[2i+1] of the 22-mers of unipath_g.kmer / unipath_g.offset that start with it */
int psvr_seed_search_kmer_batch(const psvr_index_t *idx, int64_t n, const uint64_t *kmers, int64_t *range, uint8_t *found);
typedef struct psvr_vertex_mem {            /* vertex_MEM, deBGA_index.hpp:24-58 (+ the right_i the reference returns through max_right_i) */
	uint64_t uid;
	uint32_t seed_id;                       /* position in the caller's vector in the reference: always 0 here */
	uint32_t read_pos, uni_pos_off, length, pos_n;
	uint32_t right_i;
} psvr_vertex_mem_t;
/* int deBGA_INDEX::UNITIG_MEM_search(kmer_index, ..., read_bit, read_off, read_length, 20, max_right_i) for n items: item i extends
 * index entry kmer_index[i] inside its unipath against the 2-bit packed read (32 bases per word, MSB first) that starts at
 * read_bits[word_off[i]]; every read needs ceil(len / 32) + 1 words (the reference's read_bit arrays are padded the same way) */
int psvr_seed_mem_batch(const psvr_index_t *idx, int64_t n, const uint64_t *kmer_index, const uint64_t *read_bits, int64_t n_words,
                        const int64_t *word_off, const uint32_t *read_off, const uint32_t *read_len, psvr_vertex_mem_t *out);
/* test seam: the Bloom filter over the index's 20-mers as built on the device (aln_device.h bloom_slot), copied to the host;
 * n_words = 0 only reports its size (64-bit words) and the shift of its word hash */
int psvr_index_bloom_read(const psvr_index_t *idx, uint64_t *words, int64_t n_words, int64_t *n_words_out, uint32_t *shift_out);

/* ------------------------------------------------------------------------------------------
 * Seam B1: one batch of read pairs through seeding -> chaining -> extension DP -> pairing.
 * Replaces kt_for(worker_for -> align_read_pair) minus the SAM text formatting
 * (src/PanSVgenerateVCF/read_realignment.cpp:114,154-161,745-775; legacy src/jlra_aln.cpp:115,140-147).
 * Results are those of the reference at `-t 1`: the engine consumes the same rand()/random_r
 * draw sequence in input order (see DESIGN.md "rand() order").
 * ------------------------------------------------------------------------------------------ */
typedef struct psvr_engine psvr_engine_t;

typedef struct psvr_aln_params {           /* MAP_PARA, read_realignment.hpp:46-129 */
	int32_t match, mismatch, gap_open, gap_ex, gap_open2, gap_ex2, zdrop;
	int32_t normal_read_length, isize_min, isize_max;   /* STAT_ of the first read or 150/100/900 */
	int32_t min_filter_score;
} psvr_aln_params_t;
void psvr_aln_params_default(psvr_aln_params_t *p);

/* the original alignment parsed from the FASTQ comment (single_end_handler::parse_ori_mapping_rst,
 * read_realignment.hpp:392-429): tokens 0-4 and the signal-flag token */
typedef struct psvr_ori {
	int32_t  chr_id;
	uint32_t ref_bg, read_bg, align_score;
	uint8_t  mapq, direction /* 1 = FORWARD */, unmapped, reserved;
} psvr_ori_t;

#define PSVR_MAX_RESULT 12                  /* MAX_OUTPUT_NUMBER * 2, read_realignment.hpp:323,328 */
typedef struct psvr_cand {                  /* MAX_IDX_OUTPUT, read_realignment.hpp:243-319 */
	uint32_t align_score, chain_score, ref_bg, read_bg;
	int32_t  chr_id, sv_id;
	uint32_t max_index;
	uint32_t n_cigar;
	int64_t  cigar_off;                     /* into the engine's cigar arena (uint32 len<<4|op) */
	uint8_t  direction, mapq, reserved[6];
} psvr_cand_t;

typedef struct psvr_read_result {
	int32_t n_result;
	uint8_t unmapped, early_out, is_str, reserved;
	int32_t primary, secondary;             /* -1 none, -2 the original alignment, k>=0 = cand[k] */
	int32_t has_mate, mate_chr_id;
	uint32_t mate_ref_bg;
	int32_t prim_sv_id, mate_sv_id;         /* SV:Z / MV:Z anchors of the primary record */
	uint32_t n_seed[2];                     /* trace: UNI_SEEDs per strand */
	uint32_t reserved1;                     /* 0 (the alignment hole in front of the 64-bit fields, named so that every byte of a record is written) */
	uint64_t seed_hash[2], chain_hash[2];   /* trace: FNV-1a of the sorted seeds / chaining DP per strand */
	psvr_cand_t cand[PSVR_MAX_RESULT];
} psvr_read_result_t;

/* The same results in the form the engine keeps them in HBM: one 48-byte header per read and a dense list of only the
 * candidates that exist (the fixed 12-slot psvr_read_result_t is materialised from these on request).  A pipeline that
 * formats SAM records needs nothing else; a 1 M-pair batch comes back as ~0.2 GB instead of 1.35 GB. */
typedef struct psvr_read_hdr {
	int32_t n_result;
	uint8_t unmapped, early_out, is_str, reserved;
	int32_t primary, secondary;             /* -1 none, -2 the original alignment, k>=0 = cands[cand_off + k] */
	int32_t has_mate, mate_chr_id;
	uint32_t mate_ref_bg;
	int32_t prim_sv_id, mate_sv_id;
	int32_t reserved2;
	int64_t cand_off;                       /* first of this read's n_result candidates in the candidate list */
} psvr_read_hdr_t;

typedef struct psvr_pair_result {           /* PE_score, read_realignment.hpp:434-628 */
	int32_t max_score, cur_isize;
	int32_t proper, gain;
	int32_t max1, max2;                     /* -1 none, -2 original, k */
} psvr_pair_result_t;

int psvr_engine_create(const psvr_index_t *idx, const psvr_aln_params_t *par, psvr_engine_t **out);
void psvr_engine_destroy(psvr_engine_t *eng);
/*
 * n_pairs read pairs; read r = 2*pair + mate has bases[base_off[r] .. base_off[r+1]) (ASCII) and ori[r].
 * reads[2*n_pairs] / pairs[n_pairs] receive the results; CIGARs of all candidates are appended to
 * cigar[] (capacity cigar_cap uint32; PSVR_ERR_OVERFLOW if too small).  `trace` != 0 also fills the
 * per-strand trace hashes.  Host-buffer form: copies in, runs, copies out.
 */
int psvr_engine_align_batch(psvr_engine_t *eng, int64_t n_pairs, const char *bases, const int64_t *base_off,
                            const psvr_ori_t *ori, psvr_read_result_t *reads, psvr_pair_result_t *pairs,
                            uint32_t *cigar, int64_t cigar_cap, int trace);
/* Device-resident form used by bench.py: upload once, run the hot path any number of times with the
 * rand() state rewound, download once.  No host<->device traffic inside psvr_engine_run. */
int psvr_engine_upload(psvr_engine_t *eng, int64_t n_pairs, const char *bases, const int64_t *base_off, const psvr_ori_t *ori);
int psvr_engine_run(psvr_engine_t *eng, int trace, void *stream);
int psvr_engine_download(psvr_engine_t *eng, psvr_read_result_t *reads, psvr_pair_result_t *pairs,
                         uint32_t *cigar, int64_t cigar_cap, int64_t *cigar_used);
/* Compact form of the same results: hdr[2*n_pairs], pairs[n_pairs], then only the candidates and CIGAR words that exist,
 * densely packed in read order (cands[k].cigar_off indexes `cigar`).  Call with cands == NULL (or cigar == NULL) to learn
 * cand_used / cigar_used first; PSVR_ERR_OVERFLOW if a capacity is too small (the counts are still returned).
 * The four destinations may be host memory (page-locked: psvr_host_alloc) or memory of the engine's device: the ordered
 * gather of a one-process-per-GPU host (reference: output_results, read_realignment.cpp:165-176, which walks the batch in
 * input order) sends a block on to its peer straight from HBM. */
int psvr_engine_download_compact(psvr_engine_t *eng, psvr_read_hdr_t *hdr, psvr_pair_result_t *pairs,
                                 psvr_cand_t *cands, int64_t cand_cap, int64_t *cand_used,
                                 uint32_t *cigar, int64_t cigar_cap, int64_t *cigar_used);
/*
 * Multi-GPU: read pairs are independent given the index, except that the reference consumes ONE rand()/random_r draw
 * sequence in input order.  When consecutive shards of a batch run on different GPUs, shard r starts at the stream
 * position where shard r-1 ended.  pos/end = {rand() draws, handler-0 random_r draws, handler-1 random_r draws}.
 *   psvr_engine_set_stream_pos : where the NEXT run starts (default: where the previous batch ended)
 *   psvr_engine_stream_end     : where the last run ended
 *   psvr_engine_rebase         : the last run should have started at `pos`: move it there, re-running only the pairs whose
 *                                draws moved (results afterwards == a run started at `pos`)
 * The exchange of the three integers between ranks is the caller's (one all-gather; see pansvr_amd/dist.py).
 */
int psvr_engine_set_stream_pos(psvr_engine_t *eng, const int64_t pos[3]);
int psvr_engine_stream_end(psvr_engine_t *eng, int64_t end[3]);
int psvr_engine_rebase(psvr_engine_t *eng, const int64_t pos[3], void *stream);
/* work counters of the last run (probes, hits, dp problems, cells, speculative re-runs ...) as JSON */
int psvr_engine_stats(const psvr_engine_t *eng, char *buf, size_t buflen);

/* ---- FASTQ text parsed on the device (step 0 of the batch seam) ---------------------------------------------------------------------------
 * Replaces, for a caller of seam B1 that holds FASTQ text, load_reads' kseq_read loop + parse_ori_mapping_rst
 * (src/PanSVgenerateVCF/read_realignment.cpp:121-152, read_realignment.hpp:392-429): the interleaved FASTQ of the `signal` step, four lines
 * per read and two reads per pair, becomes the three arrays psvr_engine_upload takes -- in device memory, where the engine wants them.
 * psvr_fastq_parse looks at the window text[0, n_bytes) (host memory, page-locked or pageable, free again when the call returns;
 * n_bytes >= 2^32: PSVR_ERR_UNSUPPORTED).  A line ends with its '\n'; with at_end != 0 the window's end closes an unterminated last
 * line, otherwise such a tail is no line.  Only the first 8 * max_pairs lines count; eight lines are a pair.  Leading pairs are kept
 * while the bases of the pairs in front of them stay below max_bases (load_reads' rule: the first pair is always taken when
 * max_bases > 0).  For the kept pairs, with every line stripped of its trailing '\n' and '\r' bytes:
 *   line_start[0 .. 8 n_pairs]   where every line starts in the window; info->used_bytes = line_start[8 n_pairs]
 *   base_off[0 .. 2 n_pairs]     exclusive prefix sum of the sequence lines' lengths; bases[]: their bytes, unchanged, then a NUL
 *   name_end[r]                  min(65535, index of the first ' ' or '\t' at or behind byte 1 of the header line, or its length)
 *   ori[r]                       parse_ori_mapping_rst on what follows that byte: strtok_r(.., "_") tokens 0-4 through atoi (a wrapping
 *                                32-bit accumulator), direction / unmapped from token 9's first two bytes ('F', 'Y'); every byte is written
 * Nothing is validated: a malformed text gives what the reference's loop would make of it.  The arrays stay on the device until the next
 * psvr_fastq_parse; psvr_fastq_download copies them out (any pointer may be NULL; bases has room for total_bases + 1),
 * psvr_engine_upload_fastq hands pairs [first_pair, first_pair + n_pairs) to an engine of the same device (another device: PSVR_ERR_ARG)
 * with exactly the effect of psvr_engine_upload on the downloaded arrays, device to device; it returns when `fq` may be parsed into again.
 * A psvr_fastq_t has a stream of its own and one owner at a time; several run beside each other and beside engines. */
typedef struct psvr_fastq psvr_fastq_t;          /* device buffers of one parsed window, kept across calls while the next fits */
typedef struct psvr_fastq_info {
	int64_t n_pairs, used_bytes, total_bases, n_lines;   /* n_lines: complete lines seen (<= 8*max_pairs) */
	int32_t stop;                                         /* 0 max_pairs, 1 max_bases, 2 the window ran out of lines */
	int32_t reserved;
} psvr_fastq_info_t;
int  psvr_fastq_create(int device, psvr_fastq_t **out);
int  psvr_fastq_parse(psvr_fastq_t *fq, const char *text, int64_t n_bytes, int at_end,
                      int64_t max_pairs, int64_t max_bases, psvr_fastq_info_t *info);
int  psvr_fastq_download(const psvr_fastq_t *fq, uint64_t *line_start, uint16_t *name_end,
                         int64_t *base_off, psvr_ori_t *ori, char *bases);   /* any pointer may be NULL */
int  psvr_engine_upload_fastq(psvr_engine_t *eng, const psvr_fastq_t *fq, int64_t first_pair, int64_t n_pairs);
void psvr_fastq_destroy(psvr_fastq_t *fq);

/* ---- The main BAM file's records encoded on the device (step 2 of the batch seam, between the engine and the BGZF writer) -----------------
 * Replaces, for a caller that parsed its FASTQ text with psvr_fastq_parse, the record formatting of output_BAM for the main output file
 * (single_end_handler::output_BAM, src/PanSVgenerateVCF/read_realignment.cpp:479-536, reached from output_results :165-176): the BAM
 * records of a run of pairs are made in device memory from the window a psvr_fastq_t holds (names, comments, bases, qualities, original
 * alignments) and a set of results.  Per pair p of the run, one of three states:
 *   0  nothing to write (gain == 0, or every read is skipped: primary == -1, primary == -2 under PSVR_EMIT_NOT_ORI, a chr_id that is
 *      0xffffffff or outside the header, a position below 1)
 *   1  bytes[pair_off[p], pair_off[p + 1]) hold the records of its reads (block_size first, as in a BAM stream; mate 0 first) -- exactly
 *      what the command's host formatter writes for the pair
 *   2  declined, no bytes: the caller formats the pair on the host.  A read that would be written has a name of length 0 or over 254, a
 *      quality line that is not as long as the sequence line, a tab or NUL in its comment, an anchor string with a tab, a CIGAR of 0 or
 *      more than 65535 operations or with an operator beyond 'X' -- or a result index that leaves the arrays it was given (cand_off +
 *      primary / secondary, cigar_off + n_cigar, an anchor id outside [-1, n_anchor)).  Whatever the results hold, nothing outside the
 *      given arrays is read.
 * psvr_bam_emit_results takes the results from the caller (host arrays in the compact form of psvr_engine_download_compact: hdr[2 n_pairs],
 * pairs[n_pairs], hdr.cand_off indexes cands[0, n_cands), cand.cigar_off indexes cigar[0, n_cigar); uploaded by the call, free again when it
 * returns) for window pairs [first_pair, first_pair + n_pairs).  psvr_bam_emit_engine takes the results of eng's last run where they lie in
 * HBM: eng's last upload must have been psvr_engine_upload_fastq(eng, fq, ...), run since, and fq not parsed into since (otherwise
 * PSVR_ERR_ARG, and psvr_last_error() says which; a psvr_fastq_t remembers how often it was parsed into).  Both run the same kernels.
 * fq, the engine and the emitter's index must be on one device (PSVR_ERR_ARG otherwise); no device: PSVR_ERR_DEVICE.  *info, if not NULL,
 * receives the run's totals.  The records stay on the device until the emitter's next run; psvr_bam_emit_download copies out
 * bytes[0, n_bytes) (cap < n_bytes: PSVR_ERR_OVERFLOW), pair_off[n_pairs + 1] and pair_state[n_pairs]; any pointer may be NULL; a
 * destination is host memory (page-locked or not) or memory of the emitter's device.  The index must outlive the emitter (its table of the
 * anchors' strings is made on the device once per index, by the first psvr_bam_emit_create).  A psvr_bam_emit_t has a stream of its own and
 * one owner at a time; several run beside each other and beside engines. */
typedef struct psvr_bam_emit psvr_bam_emit_t;      /* device buffers of one emitted run of pairs + a stream; one owner at a time */
typedef struct psvr_bam_emit_info { int64_t n_bytes, n_records, n_written_pairs, n_declined_pairs; } psvr_bam_emit_info_t;
#define PSVR_EMIT_NOT_ORI 1                         /* -Q: reads whose primary is the original alignment are not written */
int  psvr_bam_emit_create(const psvr_index_t *idx, psvr_bam_emit_t **out);
int  psvr_bam_emit_results(psvr_bam_emit_t *em, const psvr_fastq_t *fq, int64_t first_pair, int64_t n_pairs,
                           const psvr_read_hdr_t *hdr, const psvr_pair_result_t *pairs, const psvr_cand_t *cands, int64_t n_cands,
                           const uint32_t *cigar, int64_t n_cigar, int32_t flags, psvr_bam_emit_info_t *info);
int  psvr_bam_emit_engine(psvr_bam_emit_t *em, psvr_engine_t *eng, const psvr_fastq_t *fq, int32_t flags, psvr_bam_emit_info_t *info);
int  psvr_bam_emit_download(const psvr_bam_emit_t *em, void *bytes, int64_t cap, int64_t *pair_off, uint8_t *pair_state);
void psvr_bam_emit_destroy(psvr_bam_emit_t *em);

/* ---- The second BAM file's records encoded on the device (the -p file: pairs neither aligner placed well) -----------------------------------
 * Replaces, for the same caller, the record formatting of single_end_handler::output_ori_bam (src/PanSVgenerateVCF/read_realignment.cpp:
 * 656-717, reached from :776-797): the ORIGINAL alignment of both reads of a pair, rebuilt from the FLAG_ / CIGAR_ / MATE_ / TAG_ sections of
 * their FASTQ comments.  The calls run on a psvr_bam_emit_t and leave their records in it as psvr_bam_emit_results / _engine do: an emitter
 * holds the records of its last run, whichever file they are for, and psvr_bam_emit_download, psvr_bgzf_stream_append_emit and
 * psvr_bam_store_append_emit work on it unchanged.  Per pair p of the run, one of three states:
 *   0  nothing to write: max_score > min_filter_score or an original chr_id of -1 (decided before any text is read); a comment without
 *      one of its sections (FLAG_, CIGAR_ and its closing '_', six bytes behind that, TAG_); a pair that is `proper` and whose reads show
 *      neither a clip nor an insertion of 25 bases (max1 / max2 == -1; == -2 with the CIGAR text's end clips; else the candidate's I
 *      operators or an empty CIGAR); every read skipped (an original chr_id outside the header)
 *   1  bytes[pair_off[p], pair_off[p + 1]) hold the records of its reads that are not skipped, mate 0 first -- exactly what the command's
 *      host formatter writes for the pair: flag and mapq from FLAG_ (flag | 4 without a CIGAR), the CIGAR words parsed from the text
 *      (operators up to 'B'), mate fields from MATE_, SEQ / QUAL reversed under flag 0x10, the aux fields of the TAG_ text (i in the
 *      smallest type; A, Z, H copied), MS:i:max_score last
 *   2  declined, no bytes: the caller formats the pair on the host.  A name of length 0 or over 254, a quality line that is not as long as
 *      the sequence line, an empty or "*" sequence line, a tab or NUL in a comment, a FLAG_ / MATE_ number that is not 1-9 plain digits, a
 *      CIGAR text with an operator without digits, an unknown letter, a '-', trailing digits or more than 65535 operators, an aux field
 *      shorter than 5 bytes or without its two colons, an aux type other than i A Z H (f and B are declined), an i value that is not a
 *      '-'-optional run of 1-9 digits, records of more than 2^31 - 1 bytes -- or a result index that leaves the arrays it was given
 *      (cand_off + max1 / max2, cigar_off + n_cigar).  Whatever the results and the text hold, nothing outside the given arrays and the
 *      window is read.
 * Arguments, preconditions, error codes and the one-device rule are those of psvr_bam_emit_results / psvr_bam_emit_engine; the gate's
 * min_filter_score comes from the caller, or from the parameters eng was created with.  Both run the same kernels. */
int  psvr_bam_emit_ori_results(psvr_bam_emit_t *em, const psvr_fastq_t *fq, int64_t first_pair, int64_t n_pairs,
                               const psvr_read_hdr_t *hdr, const psvr_pair_result_t *pairs, const psvr_cand_t *cands, int64_t n_cands,
                               const uint32_t *cigar, int64_t n_cigar, int32_t min_filter_score, psvr_bam_emit_info_t *info);
int  psvr_bam_emit_ori_engine(psvr_bam_emit_t *em, psvr_engine_t *eng, const psvr_fastq_t *fq, psvr_bam_emit_info_t *info);  /* min_filter_score: eng's parameters */

/* ---- BGZF members on the device (the BAM output's compression) --------------------------------------------------------------
 * Replaces, for the drop-in command's BAM output, htslib's bgzf_compress (htslib bgzf.c: zlib deflate of 0xff00-byte blocks on the host,
 * reached from the reference's sam_write1 calls, read_realignment.cpp:166-176 -> bam_file.c).  `in` (host memory, n_bytes) is cut into
 * blocks of 16 KB (BGZF allows any size up to 64 KB; htslib uses 0xff00); every block becomes one BGZF member (gzip header with the BC field, raw DEFLATE, CRC32, ISIZE), the members are
 * written next to each other into `out` (host memory, out_cap bytes; psvr_bgzf_bound(n_bytes) always suffices) and *out_bytes is their
 * total size.  The EOF marker block is the caller's.  Any BGZF / gzip reader decodes the result; the bytes differ from zlib's. */
int64_t psvr_bgzf_bound(int64_t n_bytes);
int psvr_bgzf_compress(int device, const void *in, int64_t n_bytes, void *out, int64_t out_cap, int64_t *out_bytes);

/* ---- BGZF members on the device, a wavefront per member (the BAM output's compression, sorted or not) ---------------------------------
 * The same service as psvr_bgzf_compress with the member's bytes shared by the 64 lanes of a wavefront instead of given to one lane, and
 * with the member offsets returned (a sorted BAM's index needs them for its virtual offsets).  `in` (host memory, n_bytes) is cut into
 * members of member_bytes input bytes (256..0xff00; 0 = 0xff00, htslib's size); member i becomes one BGZF member (gzip header with the BC
 * field, one DEFLATE block -- dynamic Huffman, fixed Huffman or stored, whichever is smallest --, CRC32, ISIZE).  The members are written
 * next to each other into out[0, *out_bytes) (host memory; psvr_bgzf_members_bound(n_bytes, member_bytes) always suffices, and every
 * member is at most 31 bytes larger than its input, so it fits BGZF's 64 KB).  member_off, if not NULL, has room for member_cap + 1
 * entries: member_off[i] = where member i starts in `out`, member_off[*n_members] = *out_bytes.  The EOF marker block is the caller's.
 * A member's bytes depend on its input bytes alone: the same input gives the same member in every call, at every offset, on the device
 * and in the encoder's host build (tests/tools/deflate_wave_check.cpp).  Any BGZF / gzip reader decodes them; they differ from zlib's.
 * n_bytes == 0: no members, PSVR_OK.  out_cap or member_cap too small: PSVR_ERR_OVERFLOW (*out_bytes and *n_members are still set when the
 * device ran).  Bytes of `out` behind *out_bytes are unspecified.  Device buffers and the call's stream (of the lowest priority) are kept
 * across calls; calls are serialised.
 * psvr_bgzf_compress_members_effort is the same call with the encoder's effort, 0..3 (anything else: PSVR_ERR_ARG); psvr_bgzf_compress_members
 * is that call at effort 0.  Effort 0 tries one hash-table candidate per position besides the distances 1 and 2 and takes every match it
 * finds (greedy).  Efforts 1, 2 and 3 walk a hash chain of 4, 8 and 16 candidates and match lazily (a match gives way to a longer one at
 * the next position), zlib's two means: smaller members for more time in the member kernel.  The chains live in device scratch (2 bytes per
 * input byte) that only a call at effort > 0 allocates.  At every effort a member's bytes depend on its input bytes and the effort alone
 * (the host build: tests/tools/deflate_effort_check.cpp), and every effort's members hold the same data. */
int64_t psvr_bgzf_members_bound(int64_t n_bytes, int32_t member_bytes);
int psvr_bgzf_compress_members(int device, const void *in, int64_t n_bytes, int32_t member_bytes,
                               void *out, int64_t out_cap, int64_t *out_bytes,
                               int64_t *member_off, int64_t member_cap, int64_t *n_members);
int psvr_bgzf_compress_members_effort(int device, const void *in, int64_t n_bytes, int32_t member_bytes,
                                      void *out, int64_t out_cap, int64_t *out_bytes,
                                      int64_t *member_off, int64_t member_cap, int64_t *n_members, int32_t effort);

/* ---- A BGZF stream that lives on the device (the hand-over from psvr_bam_emit_* to the member compressor) ------------------------------
 * Joins the two sections above: a byte stream in HBM that is cut every member_bytes bytes (as in psvr_bgzf_compress_members: 256..0xff00,
 * 0 = 0xff00) and whose members the same encoder makes, on the same process-wide buffers and stream.  The contract: concatenate the members
 * every psvr_bgzf_stream_take of a stream returned, and the result is byte for byte what psvr_bgzf_compress_members returns for the
 * concatenation of everything appended, at the same member_bytes and effort -- however appends and takes were interleaved.
 *   set_effort    the encoder's effort (0..3, as in psvr_bgzf_compress_members_effort; anything else: PSVR_ERR_ARG) of every take from the
 *                 next one on; a new stream is at effort 0.  Members of takes at different efforts concatenate to a valid stream of the same data.
 *   append        n_bytes of host memory (the BAM header, records the host formatted) behind what is pending; the bytes are free again when
 *                 the call returns.
 *   append_emit   bytes[pair_off[first_pair], pair_off[first_pair + n_pairs]) of em's last run, device to device: one kernel launch that
 *                 reads the two offsets and the pending count where they lie in HBM, so the call queues and returns without a round trip.
 *                 `em` MUST NOT BE RUN AGAIN (psvr_bam_emit_results / _engine) or destroyed UNTIL A LATER take, pending or recover ON `s`
 *                 HAS RETURNED: until then the copy may still be reading its records.  A pair range outside the run, an emitter without a
 *                 valid run, an emitter on another device: PSVR_ERR_ARG.  A range of zero bytes appends nothing.
 *   pending       bytes appended and not yet taken (a wait for what is queued); < 0: minus a status.
 *   take          compresses every whole member that is pending, with finish != 0 also the tail as a last, shorter member (a stream that
 *                 ends on a member boundary gets no empty member; nothing pending: no members, PSVR_OK).  The members go to
 *                 out[0, *out_bytes) (host memory), member_off / member_cap / n_members as in psvr_bgzf_compress_members (any may be NULL),
 *                 *in_bytes = stream bytes consumed.  What stays pending is less than member_bytes and starts the next member.
 *                 out_cap < psvr_bgzf_members_bound(pending, member_bytes), or more members than member_cap: PSVR_ERR_OVERFLOW and nothing
 *                 is consumed.  One wait per call (a second, short one in front when an append_emit has been queued since the last call
 *                 that waited: the count it left is then read back first).
 *   recover       copies the pending bytes to bytes[0, *n_bytes) (host memory) and empties the stream: what a caller that gives the device
 *                 route up continues from.  cap too small: PSVR_ERR_OVERFLOW, *n_bytes is set, nothing is lost.
 * An append_emit that would leave the emitter's bytes or the stream's buffer is not made, and from the call that notices it on (the next one
 * that reads the count back) every call answers PSVR_ERR_DEVICE; so does every call after one that failed while it changed the pending bytes.
 * Device memory: the length of a pair range is known on the device only, so until the next call that waits every append_emit reserves room
 * for em's WHOLE run behind what may be pending (the buffer grows by half on top); many short ranges of a large run between two waits cost
 * ranges x run bytes of HBM -- ask `pending` in between, as the command does after every piece.
 * The EOF marker block is the caller's.  A stream has one owner at a time; its calls are serialised with psvr_bgzf_compress_members. */
typedef struct psvr_bgzf_stream psvr_bgzf_stream_t;
int     psvr_bgzf_stream_create(int device, int32_t member_bytes, psvr_bgzf_stream_t **out);
int     psvr_bgzf_stream_set_effort(psvr_bgzf_stream_t *s, int32_t effort);
int     psvr_bgzf_stream_append(psvr_bgzf_stream_t *s, const void *bytes, int64_t n_bytes);
int     psvr_bgzf_stream_append_emit(psvr_bgzf_stream_t *s, const psvr_bam_emit_t *em, int64_t first_pair, int64_t n_pairs);
int64_t psvr_bgzf_stream_pending(psvr_bgzf_stream_t *s);
int     psvr_bgzf_stream_take(psvr_bgzf_stream_t *s, int finish, void *out, int64_t out_cap, int64_t *out_bytes,
                              int64_t *member_off, int64_t member_cap, int64_t *n_members, int64_t *in_bytes);
int     psvr_bgzf_stream_recover(psvr_bgzf_stream_t *s, void *bytes, int64_t cap, int64_t *n_bytes);
void    psvr_bgzf_stream_destroy(psvr_bgzf_stream_t *s);

/* ---- BGZF members inflated on the device (the BAM input's decompression) --------------------------------------------------------------
 * Replaces, for the commands that read a BAM (`panSVR signal`, `panSVR sort`, `panSVR aln` with a *.bam read file), htslib's
 * bgzf_read_block -> inflate_block (htslib bgzf.c: zlib inflate of one member at a time on the calling thread).
 * `in` (host memory) holds BGZF members back to back.  Whole members are consumed: *in_used is the size of the longest prefix of n_bytes
 * made of whole members (a cut-off member at the end is the caller's to complete), *out_bytes the sum of their ISIZE fields.
 * out == NULL: only the sizes are computed (no device needed for that).  Otherwise the members are inflated on HIP device `device`, one
 * wavefront per member, into out[0, *out_bytes), in order (out_cap too small: PSVR_ERR_OVERFLOW, the sizes still returned).
 * member_off, if not NULL, has room for member_cap + 1 entries: member_off[i] = where member i starts in `out`, member_off[*n_members] =
 * *out_bytes (more members than member_cap: PSVR_ERR_OVERFLOW); n_members and bad_member may be NULL.
 * Every member's CRC32 and ISIZE are checked on the device.  A member zlib would refuse (its header is judged by the rules of the
 * command's serial reader: magic, CM, FEXTRA, a BC subfield of length 2 anywhere in the extra field, BSIZE large enough for header and
 * trailer) -> PSVR_ERR_IO; *bad_member is its index and psvr_last_error() names index and byte offset; the bytes of the members in front
 * of it are valid, nothing is promised from its start on.  A member with a bad header ends the chain: *in_used and *out_bytes cover the
 * members in front of it.  Device buffers and the call's stream are kept across calls; calls are serialised. */
int psvr_bgzf_decompress(int device, const void *in, int64_t n_bytes, int64_t *in_used,
                         void *out, int64_t out_cap, int64_t *out_bytes,
                         int64_t *member_off, int64_t member_cap, int64_t *n_members, int64_t *bad_member);

/* ---- Stable order of 64-bit keys on the device (the coordinate sort of the BAM output) -------------------------------------------------
 * Replaces, for `panSVR aln --sort` and `panSVR sort`, the ordering step of `samtools sort` that panSVR_run.sh:53 runs between `aln` and
 * `fc_sv` (samtools bam_sort.c: the key (uint64)tid << 32 | (uint32)(pos + 1) << 1 | reverse, ties in input order).
 * order[i] = index of the i-th smallest key; equal keys keep ascending index (stable).
 * Host pointers; 0 <= n < 2^32 (else PSVR_ERR_UNSUPPORTED); runs on HIP device `device`.  An LSD radix sort with 8-bit digits in tiles of
 * 2048 keys; passes whose digit is the same for every key are skipped.  Device memory: about 24 bytes per key, allocated per call
 * (PSVR_ERR_NOMEM with the byte count in psvr_last_error() when it does not fit).  The arguments are looked at before the device: n == 0
 * answers PSVR_OK without one (psvr_sort_order_names below asks for the device first, and answers PSVR_ERR_DEVICE even then). */
int psvr_sort_order_u64(int device, int64_t n, const uint64_t *keys, uint32_t *order);

/* ---- Name order on the device (`panSVR sort -n`) --------------------------------------------------------------------------------------------
 * order[i] = index of the i-th name.  Name i is the NUL-terminated string at names + name_off[i] (names[0, n_bytes), host pointers); the order
 * is strcmp's (unsigned bytes up to the first NUL), equal names by tie[i] ascending (tie == NULL: all equal; `panSVR sort -n` passes
 * flag & 0xc0, first read before second), then by ascending index (stable).  This project's name order, not samtools' natural one.
 * The names are cut into big-endian 8-byte chunks, NUL-padded, and ordered by runs of psvr_sort_order_u64's radix sort: the tie key, then the
 * chunks from the last to the first, each run stable over the order of the run before; a chunk that is the same for every name costs one
 * histogram.  n >= 2^32 or a name longer than 254 bytes: PSVR_ERR_UNSUPPORTED; an offset outside the blob or a name without a NUL before the
 * blob's end: PSVR_ERR_ARG; no device: PSVR_ERR_DEVICE (asked first); n == 0 is fine.  Device memory: n_bytes + about 41 bytes per name,
 * allocated per call (PSVR_ERR_NOMEM with the byte count in psvr_last_error() when it does not fit). */
int psvr_sort_order_names(int device, int64_t n, const void *names, int64_t n_bytes, const int64_t *name_off, const uint8_t *tie, uint32_t *order);

/* ---- The main BAM file's records kept and ordered in HBM (the coordinate sort of the BAM output without a host trip) -------------------------
 * Joins psvr_bam_emit_*, psvr_sort_order_u64 and psvr_bgzf_stream_*: what `samtools sort` + `samtools index` do between the `aln` and `fc_sv`
 * steps (panSVR_run.sh:53-54), for records that the device encoded and that the device compresses.  A store keeps BAM records (block_size
 * first, as in a BAM stream) in device memory, in chunks that are allocated once and never moved, with a table of one entry per record that
 * is built on the device: where the record lies, its length, samtools' key (uint64)tid << 32 | (uint32)(pos + 1) << 1 | reverse, the
 * reference span of its CIGAR (1 without one) and the bin recomputed from position and span (reg2bin(max(pos, 0), max(pos, 0) + span), as
 * `panSVR sort` recomputes it).
 *   append        records back to back from host memory (what the host formatter wrote for a chunk); free again when the call returns (a
 *                 wait).  The bytes are checked on the host first: a record cut off by the end, a block_size below 32 or a CIGAR that leaves
 *                 its record: PSVR_ERR_ARG, and nothing is appended (a record of 2 GiB or more: PSVR_ERR_UNSUPPORTED, likewise).
 *   append_emit   bytes[pair_off[first_pair], pair_off[first_pair + n_pairs]) of em's last run, device to device, queued without a round trip.
 *                 `em` MUST NOT BE RUN AGAIN or destroyed UNTIL A LATER info, append, order or download ON `st` HAS RETURNED (the rule of
 *                 psvr_bgzf_stream_append_emit).  A pair range outside the run, an emitter without a valid run or on another device:
 *                 PSVR_ERR_ARG.  The records are found by walking the block_size chain inside each state-1 pair, bounded by the pair's bytes.
 *   append_bgzf   a BAM file's own bytes: in[0, n_bytes) holds whole BGZF members back to back (host memory; *in_used: the longest prefix made of
 *                 whole members, what is behind it is the caller's to complete).  The members are inflated on the device, a wavefront each,
 *                 straight into the store, and the records are found there: the block_size chain of an inflated stream is serial, so the
 *                 stream is cut into segments (16 KiB; PSVR_BAM_STORE_SEG_BYTES, at least 64) that each guess their first record start
 *                 and walk from it, and one pass settles the guesses against the known start and walks again where a guess was wrong --
 *                 exact for every stream, fast for real ones.  `skip`: inflated bytes at the front of this call that are no records (the BAM
 *                 header's remainder; 0, or less than the first member's ISIZE on a call that continues no record); n_ref >= 0: the
 *                 file's reference count, a hint for the guesses only.  Every whole record is appended; the bytes behind the last one
 *                 (the tail) stay in the store for the next call to complete.  While the tail is not empty append and append_emit are
 *                 refused (PSVR_ERR_ARG), and so is order ("truncated BAM stream").  The header rules and the ISIZE check are
 *                 psvr_bgzf_decompress's; a header that is none, or a member that does not inflate to its ISIZE and CRC32: PSVR_ERR_IO,
 *                 *bad_member its index, nothing of the call is appended and the store stays usable.  A record on the chain that
 *                 BamReader's rules refuse (block_size < 32 or > 0x7ffffff0, l_seq < 0, fields that leave the record, a name without NUL):
 *                 PSVR_ERR_DEVICE, from then on for every call.  The call waits.
 *   chain_info    waits; the chain finder's counters summed over all append_bgzf calls (segments, segments without a guess, guesses
 *                 that were wrong, segments walked again) and the tail's length.
 *   info          waits for what is queued; key_exact == 0: some position lies outside [-1, 2^31 - 2].
 *   order         sorts the keys where they lie (the sort of psvr_sort_order_u64: stable, equal keys keep append order) and computes where
 *                 every record goes in the sorted stream.  Afterwards appends are refused (PSVR_ERR_ARG).  key_exact == 0 or 2^32 and more
 *                 records: PSVR_ERR_UNSUPPORTED, and nothing changes.  An empty store is ordered too.
 *   order_names   order, by name instead of by coordinate (psvr_sort_order_names' order: the name with strcmp, flag & 0xc0, append order); the
 *                 names are read where the records lie, through the table's addresses.  A record's name ends at its first NUL, and at
 *                 l_read_name bytes at the latest: a name field without a NUL (append from the host takes one; append_bgzf and
 *                 `panSVR sort`'s reader refuse it) is compared as its l_read_name bytes, never beyond.  It needs no key: key_exact == 0 is no obstacle.  Refused
 *                 like order while a tail is pending, and once the store has been ordered the other way (PSVR_ERR_ARG).  Afterwards
 *                 info.ordered == 2 (1 after order), and appends, meta, stream and download behave as after order.  A failure before
 *                 the first key has moved leaves the store unchanged.
 *   meta          for sorted ranks [first_rank, first_rank + n), what the .bai needs: tid, pos, end = max(pos, 0) + span, len = 4 + block_size,
 *                 the recomputed bin, flag, and index = the record's number in append order.  Only after order (else PSVR_ERR_ARG).
 *   stream        appends the records of those ranks, with the recomputed bin in bytes 14-15, behind the pending bytes of a
 *                 psvr_bgzf_stream_t on the same device, device to device (one gather kernel; returns when the bytes are pending).  The host
 *                 knows every length after order: the stream's count stays exact and no room is reserved beyond the bytes themselves.
 *   download      every record in append order, with the recomputed bin, to bytes[0, *n_bytes) (host memory; cap too small:
 *                 PSVR_ERR_OVERFLOW, *n_bytes is set).  Works before and after order: what a caller that gives the device route up continues from.
 * An append from an emitter that would leave the emitter's bytes, a chain that leaves its pair, a block_size below 32 or a CIGAR that leaves
 * its record is noticed on the device: nothing further is copied, and from the next call that waits on every call answers PSVR_ERR_DEVICE.
 * No device: PSVR_ERR_DEVICE.  A failed device allocation: PSVR_ERR_NOMEM with the byte count in psvr_last_error(), and nothing stored is lost.
 * Device memory: the records, about 48 bytes per record of table, about 70 more per record from order on; until the next call that waits
 * every append_emit reserves room for em's WHOLE run in the current chunk (256 MiB, or the run's size) and in the table.
 * A store has one owner at a time; its calls are serialised with psvr_bgzf_compress_members and the streams'. */
typedef struct psvr_bam_store psvr_bam_store_t;
typedef struct psvr_bam_store_info { int64_t n_records, n_bytes; int32_t key_exact, ordered; } psvr_bam_store_info_t;
typedef struct psvr_bam_chain_info { int64_t segments, no_guess, wrong_guess, rewalked, tail_bytes; } psvr_bam_chain_info_t;
typedef struct psvr_bam_rec_meta { int64_t end; int32_t tid, pos; uint32_t len, index; uint16_t bin, flag; uint32_t pad; } psvr_bam_rec_meta_t; /* 32 bytes */
int  psvr_bam_store_create(int device, psvr_bam_store_t **out);
int  psvr_bam_store_append(psvr_bam_store_t *st, const void *bytes, int64_t n_bytes);
int  psvr_bam_store_append_emit(psvr_bam_store_t *st, const psvr_bam_emit_t *em, int64_t first_pair, int64_t n_pairs);
int  psvr_bam_store_append_bgzf(psvr_bam_store_t *st, const void *in, int64_t n_bytes, int64_t skip, int32_t n_ref, int64_t *in_used, int64_t *bad_member);
int  psvr_bam_store_chain_info(psvr_bam_store_t *st, psvr_bam_chain_info_t *info);   /* waits; counters summed over all appends */
int  psvr_bam_store_info(psvr_bam_store_t *st, psvr_bam_store_info_t *info);       /* waits for what is queued */
int  psvr_bam_store_order(psvr_bam_store_t *st);
int  psvr_bam_store_order_names(psvr_bam_store_t *st);
int  psvr_bam_store_meta(psvr_bam_store_t *st, int64_t first_rank, int64_t n, psvr_bam_rec_meta_t *meta);
int  psvr_bam_store_stream(psvr_bam_store_t *st, psvr_bgzf_stream_t *s, int64_t first_rank, int64_t n);
int  psvr_bam_store_download(psvr_bam_store_t *st, void *bytes, int64_t cap, int64_t *n_bytes);
void psvr_bam_store_destroy(psvr_bam_store_t *st);
/*   drop          the first n_front records (append order) cease to exist: n_records and n_bytes fall, the table's entries of the rest slide to
 *                 the front and meta.index counts from the first record kept.  A pending tail stays pending (the next append_bgzf completes
 *                 it).  Every chunk that holds none of the remaining records and is not the one being filled is released; one released
 *                 chunk of the standard size is kept as a spare for the next chunk the store needs.  After order / order_names, or with
 *                 n_front outside [0, n_records]: PSVR_ERR_ARG.  The call waits.  What a caller that works through a long file piece by
 *                 piece (psvr_signal_run below) bounds its device memory with: a piece's inflated bytes plus a chunk.
 *   footprint     what the store holds in device memory for records: the live chunks and the spare one, and their bytes. */
int  psvr_bam_store_drop(psvr_bam_store_t *st, int64_t n_front);
int  psvr_bam_store_footprint(psvr_bam_store_t *st, int64_t *chunks, int64_t *bytes);

/* ---- `panSVR signal -N` over a record store: pair, judge and format FASTQ text in HBM ---------------------------------------------------------
 * The per-pair rules of the name-sorted `signal` step (SignalStep::pair and write_fastq, pansvr_amd/csrc/signal_step.h) over the records of a
 * psvr_bam_store_t, read where they lie through the store's address table (pansvr_amd/csrc/signal_device.h holds the rules for host and
 * device).  Only FASTQ text and a small per-pair table come back.
 *   create        the options of the step: the six scores, max_tid, -D (not_use_filter), -U (discard_full_match) with its insert-size window,
 *                 and the four numbers of the STAT_ field, which the first pair that is written at all carries, once per object.
 *   run           over the store's records [first_record, n_records) in append order: the primary records (!(flag & 0x900)) are compacted and
 *                 paired (2j, 2j + 1); with an odd count the last primary is not consumed and info->consumed is its record index, otherwise
 *                 n_records (`finish` changes nothing: the host loop drops a lone last record too).  Every pair gets a state:
 *                   0 not written   1 written into the text buffer   2 to be written, but formatted by the host (a base code outside
 *                   {1, 2, 4, 8, 15}, a quality of 223, or a text of 2 GiB)   3 the names differ   4 not first / second in template
 *                   5 would be written but l_qseq of read 1 >= 2048
 *                 and a note (bit 0: "wrong ISIZE").  The text holds the state-1 pairs in front of the first pair of state >= 3, back to
 *                 back in pair order.  Both records of every pair in front of that pair are added to the two histograms of BamStat::collect,
 *                 which accumulate over all runs.  A record that BamReader's rules refuse: PSVR_ERR_IO, nothing is counted.  The store must
 *                 not be ordered and must be on the object's device (PSVR_ERR_ARG).  The call waits.
 *   text          the text of the last run to text[0, info.text_bytes) (cap too small: PSVR_ERR_OVERFLOW).
 *   pairs         the table of the last run, pairs[0, info.pairs) (40 bytes per pair): rec1 / rec2 are record indices of the store as it was at the run.
 *   side          the records the host needs, gathered by the run and downloaded in one piece, side[0, info.side_bytes): of every pair in
 *                 front of the first error pair that is declined or carries a note, and of the error pair, the two records back to
 *                 back (block_size first) at the pair's side_off (-1: the pair has none).  One download per run, however many pairs
 *                 the host formats.
 *   pair_records  the bytes of the two records of pair p of the last run, back to back (block_size first), for the host formatter; the store
 *                 must hold the records still (no drop in between).
 *   stats         isize_n[100000] and len_n[1000], accumulated over all runs.
 *   window        the text SignalStep's host loop would have written for the pairs in front of the last run's first error pair, complete and
 *                 in pair order, in device memory (pansvr_amd/csrc/signal_window_device.h): the state-1 ranges come from the run's text buffer,
 *                 the state-2 pairs from host_text, whose bytes [host_off[i], host_off[i + 1]) are the host formatter's text of the i-th
 *                 state-2 pair in front of the first error pair (uploaded by the call), each at its place; state-0 pairs contribute nothing.
 *                 n_host is not the number of such pairs, host_off is not monotone from 0 or does not end at host_bytes: PSVR_ERR_ARG;
 *                 a window of 2^32 bytes or more: PSVR_ERR_UNSUPPORTED.  info: n_bytes of the window, n_pairs whose text it holds (states 1
 *                 and 2), n_host_pairs of them from the host.  The call waits; the window stays until the next run or window call.
 *   window_add    the same for the last run (run, run_pos or run_left), written behind the bytes the object's kept window already holds: a kept
 *                 window grows run by run and survives later runs, until an add with restart != 0 (which empties it first), a window call
 *                 or destroy.  info carries the kept window's totals.  Refused as window is (a total of 2^32 bytes or more:
 *                 PSVR_ERR_UNSUPPORTED; no memory: PSVR_ERR_NOMEM), and a refused or failed add leaves the kept window's bytes and counts
 *                 as they were.  window_text and psvr_fastq_parse_signal read a kept window as they read the other.
 *   window_text   bytes [first, first + n) of the window to dst, which is host memory or memory of the object's device (outside the
 *                 window: PSVR_ERR_ARG).
 *   psvr_fastq_parse_signal   exactly the effect of psvr_fastq_parse on the bytes [first_byte, n_bytes) of sg's window with at_end = 1, the
 *                 bytes copied device to device into fq's own text buffer: sg may be run again once the call returns, and the emitter
 *                 finds names, comments and qualities in fq as it does behind psvr_fastq_parse.  fq and sg on two devices, no window, or
 *                 first_byte outside [0, n_bytes]: PSVR_ERR_ARG.  info->used_bytes lets the caller come back with first_byte + used_bytes
 *                 when max_pairs / max_bases wanted fewer pairs than the window holds.
 *   psvr_fastq_text   bytes [first, first + n) of the text fq was last parsed from (either way) to dst in host memory, for a caller that
 *                 never held the text (outside that text: PSVR_ERR_ARG).
 * No device: PSVR_ERR_DEVICE.  Calls run under the store's mutex on its stream, serialised with the store's. */
typedef struct psvr_signal psvr_signal_t;
typedef struct psvr_signal_opt {
	int32_t gap_open, gap_ex, gap_open2, gap_ex2, match, mismatch, max_tid, not_use_filter, discard_full_match, isize_min, isize_max;
	int32_t stat[4];                                    /* read_len, min_i, mid_i, max_i of STAT_ */
} psvr_signal_opt_t;
typedef struct psvr_signal_info { int64_t pairs, written, declined, first_error, text_bytes, consumed, side_bytes; } psvr_signal_info_t;
typedef struct psvr_signal_pair { int64_t text_off, rec1, rec2, side_off; int32_t bytes; uint8_t state, note; uint16_t pad; } psvr_signal_pair_t; /* 40 bytes */
int  psvr_signal_create(int device, const psvr_signal_opt_t *opt, psvr_signal_t **out);
int  psvr_signal_run(psvr_signal_t *sg, psvr_bam_store_t *st, int64_t first_record, int32_t finish, psvr_signal_info_t *info);
int  psvr_signal_text(psvr_signal_t *sg, void *text, int64_t cap);
int  psvr_signal_pairs(psvr_signal_t *sg, psvr_signal_pair_t *pairs, int64_t cap);
int  psvr_signal_side(psvr_signal_t *sg, void *bytes, int64_t cap);
int  psvr_signal_pair_records(psvr_signal_t *sg, psvr_bam_store_t *st, int64_t pair, void *bytes, int64_t cap, int64_t *n_bytes);
int  psvr_signal_stats(psvr_signal_t *sg, uint64_t *isize_n, uint64_t *len_n);
typedef struct psvr_signal_window_info { int64_t n_bytes, n_pairs, n_host_pairs; } psvr_signal_window_info_t;
int  psvr_signal_window(psvr_signal_t *sg, const void *host_text, int64_t host_bytes, const int64_t *host_off, int64_t n_host, psvr_signal_window_info_t *info);
int  psvr_signal_window_add(psvr_signal_t *sg, const void *host_text, int64_t host_bytes, const int64_t *host_off, int64_t n_host, int32_t restart,
                            psvr_signal_window_info_t *info);
int  psvr_signal_window_text(psvr_signal_t *sg, void *dst, int64_t first, int64_t n);   /* dst: host memory or memory of sg's device */
int  psvr_fastq_parse_signal(psvr_fastq_t *fq, const psvr_signal_t *sg, int64_t first_byte, int64_t max_pairs, int64_t max_bases, psvr_fastq_info_t *info);
int  psvr_fastq_text(const psvr_fastq_t *fq, void *dst, int64_t first, int64_t n);
void psvr_signal_destroy(psvr_signal_t *sg);

/* ---- `panSVR signal --mate-device`: the blocks of the position-sorted mode, mated where the records lie ------------------------------------
 * SignalStep::run_pos_sorted's block rules (pansvr_amd/csrc/signal_mate_device.h holds them for host and device) over the primary records of
 * the store behind first_record, in append order.
 *   run_pos   A block: up to opt->block_records primaries (0: 1 000 000); the first one on another chromosome than the block's first, or more
 *             than opt->block_span (0: 60 000 000) behind it, is its last.  A block that is not complete, with finish == 0: pos_info->complete
 *             = 0, nothing is consumed, nothing else is filled (a mark and a scan).  Otherwise the mates are found exactly as the host loop
 *             finds them, the pairs (the record without flag 0x80 first, in that record's order) go through psvr_signal_run's size, fix,
 *             side, write and hist passes -- info, text, pairs, side and stats answer as behind psvr_signal_run, state 3 cannot occur --
 *             and the records without mate are gathered in block order for psvr_signal_left.  pos_info: the block's primaries, the record
 *             index the caller drops the store to (consumed), the unmated records and their bytes, the "Mate failed" turns of all blocks
 *             so far, the notes that wait, the records the one-lane replay walked.  A finished input of fewer than two primaries is
 *             consumed and gives nothing (the host loop drops a single record).
 *             Declined with PSVR_ERR_UNSUPPORTED and the reason in psvr_last_error(), nothing consumed: positions that decrease inside the
 *             block (its last record on another chromosome excepted), a position that overflows the host loop's 1 M-entry index.
 *   mate_notes  for every 1000th "Mate failed" turn of the last block what the host loop's line says: number, index in block, block size,
 *             tid, pos, name.
 *             Every block's unmated records are also copied, device to device, into a second record store that the object owns.
 *   left      the last block's unmated records back to back (block_size first), left[0, pos_info.left_bytes) (what went into that store).
 *   run_left  The by-name pass over that store.  The first call orders it by the host comparator (name by strcmp, records with flag 0x40
 *             first, append order) and builds the pair list: a run of L equal names gives floor(L / 2) pairs and, when L is odd and the run
 *             is not the last, one pairing-error step.  Every call runs pairs [first_pair, first_pair + max_pairs) of that list through
 *             psvr_signal_run's passes; a slice whose text would reach 2 GiB is halved until it does not, so left_info.n_pairs may be
 *             smaller than max_pairs and the caller goes on from first_pair + n_pairs: info, text, pairs (rec1 / rec2 are
 *             indices into the left store, in append order), side and stats answer as behind a run.  left_info: the store's records, the
 *             pairs and error steps of the whole pass, the slice, and whether pairs remain.  An odd number of records: PSVR_ERR_UNSUPPORTED.
 *   left_errors  per pair of the last slice, the pairing-error steps of the whole pass in front of it (left_info.errors - the last pair's
 *             figure lie behind the last pair).
 * No device: PSVR_ERR_DEVICE. */
typedef struct psvr_signal_pos_opt { int64_t block_records, block_span; } psvr_signal_pos_opt_t;
typedef struct psvr_signal_pos_info { int64_t complete, primaries, consumed, unmated, left_bytes, mate_failed, notes, replayed; } psvr_signal_pos_info_t;   /* 64 bytes */
typedef struct psvr_signal_mate_note { int64_t number; int32_t index, block, tid, pos; char name[256]; } psvr_signal_mate_note_t;                         /* 280 bytes */
int  psvr_signal_run_pos(psvr_signal_t *sg, psvr_bam_store_t *st, int64_t first_record, int32_t finish, const psvr_signal_pos_opt_t *opt, psvr_signal_info_t *info,
                         psvr_signal_pos_info_t *pos_info);
int  psvr_signal_mate_notes(psvr_signal_t *sg, psvr_signal_mate_note_t *notes, int64_t cap);
int  psvr_signal_left(psvr_signal_t *sg, void *bytes, int64_t cap);
typedef struct psvr_signal_left_info { int64_t records, pairs, errors, first_pair, n_pairs, more; } psvr_signal_left_info_t;                               /* 48 bytes */
int  psvr_signal_run_left(psvr_signal_t *sg, int64_t first_pair, int64_t max_pairs, psvr_signal_info_t *info, psvr_signal_left_info_t *left_info);
int  psvr_signal_left_errors(psvr_signal_t *sg, int64_t *errors, int64_t cap);

#ifdef __cplusplus
}
#endif
#endif /* PSVR_ENGINE_H_ */
