// signal_run.h -- what a psvr_signal_t is: the device buffers of the last run and of its window (signal.hip fills them, fastq.hip's
// psvr_fastq_parse_signal reads the window device to device).
#pragma once
#include "common.h"

struct psvr_bam_store;

struct psvr_signal {
	int device = 0;
	psvr_signal_opt_t opt;
	bool spent = false;                                      // STAT_ has been given to a pair
	psvr::DevBuf mark, poff, prim, state, note, bytes, toff, tmp, text, ctl, isize_n, len_n, sbytes, soff, side;
	long long *h_ctl = nullptr;                              // page-locked read-back of ctl
	// the last run
	bool valid = false;
	const psvr_bam_store *store = nullptr;
	long long store_generation = 0, first_record = 0, pairs = 0, text_bytes = 0, side_bytes = 0;
	long long n_front = 0, written = 0, declined = 0;        // pairs in front of the first error pair; of those in state 1, in state 2
	// the last run's window (psvr_signal_window): gone with the next run
	psvr::DevBuf wflag, wrank, wcut, wseg, whost, whoff, window;
	bool win_valid = false;
	long long win_bytes = 0;
};
