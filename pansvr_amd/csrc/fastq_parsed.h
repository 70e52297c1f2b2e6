// fastq_parsed.h -- what a psvr_fastq_t is: the device buffers of one parsed window (fastq.hip fills them, engine.hip's
// psvr_engine_upload_fastq reads them device to device).
#pragma once
#include "common.h"

struct psvr_fastq {
	int device = 0;
	hipStream_t stream = nullptr;
	psvr::DevBuf text, cnt, tile_off, tmp, line_start, slen, base_off, name_end, ori, bases, meta, info;
	psvr_fastq_info_t *h_info = nullptr;                     // page-locked: the one record a call reads back
	psvr_fastq_info_t last = {0, 0, 0, 0, 0, 0};             // of the window the buffers hold
	bool valid = false;
	int64_t n_text = 0;                                      // bytes of text[] the window was parsed from (psvr_fastq_text)
	uint64_t generation = 0;                                 // of the window the buffers hold: drawn from one process-wide counter at create and by every parse, so no
	                                                         // two windows of a process share one, whatever address their parser has: who remembers a window can tell that it is gone
};
