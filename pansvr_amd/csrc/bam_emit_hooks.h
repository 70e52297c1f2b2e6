// bam_emit_hooks.h -- what bam_emit.hip asks of engine.hip, which alone knows what a psvr_index_t and a psvr_engine_t are: the index's
// table of anchor strings on the device (built once per index, on first use) and the view of an engine's last results in HBM together
// with where its batch came from.
#pragma once
#include "bam_emit_device.h"

struct psvr_fastq;
struct psvr_index;
struct psvr_engine;

namespace psvr {

// the device table of ix->host.svh (BeTableHost's layout) and n_header; *device = where it lives.  A status of psvr_engine.h.
int index_emit_tables(const psvr_index *ix, BeTables *T, int *device);

struct EngineEmitView {
	int device;
	bool ran;                                                // psvr_engine_run has succeeded since the last upload
	const psvr_fastq *fq;                                    // the last upload was psvr_engine_upload_fastq(eng, fq, first_pair, n_pairs); nullptr: it was not
	int64_t first_pair, n_pairs;
	uint64_t generation;                                     // fq's at that upload
	const psvr_read_hdr_t *hdr; const psvr_pair_result_t *pairs;   // device pointers: hdr.cand_off indexes cands, cand.cigar_off indexes cig
	const psvr_cand_t *cands; int64_t n_cands;
	const uint32_t *cig; int64_t n_cig;
	int32_t min_filter_score;                                // of the engine's parameters (the second file's gate)
};
void engine_emit_view(const psvr_engine *e, EngineEmitView *v);

} // namespace psvr
