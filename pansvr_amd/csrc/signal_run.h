// signal_run.h -- what a psvr_signal_t is: the device buffers of the last run and of its window (signal.hip fills them, fastq.hip's
// psvr_fastq_parse_signal reads the window device to device).
#pragma once
#include <memory>
#include <vector>
#include "common.h"
#include "sort_device.h"

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
	// the window: the last run's (psvr_signal_window), gone with the next run, or a kept one (psvr_signal_window_add), which grows run by run
	// and stays until a restart or a psvr_signal_window call
	psvr::DevBuf wflag, wrank, wcut, wseg, whost, whoff, window;
	bool win_valid = false, win_kept = false;
	long long win_bytes = 0, win_pairs = 0, win_host_pairs = 0;
	void run_begins() { valid = false; if (!win_kept) win_valid = false; }
	// psvr_signal_run_pos: the block's structure of arrays, the mate tables, the lists, the unmated records side by side, the notes
	psvr::DevBuf bprim, spos, smpos, sflag, ssame, cand, indeg, mate, dirty, fail, doff, dlist, pflag, lflag, pfoff, lfoff, ffoff, lbytes, lboff, left, notes, mctl;
	long long *h_mctl = nullptr;                             // page-locked read-back of mctl
	long long mate_failed = 0;                               // "Mate failed" turns of all blocks so far
	bool pos_valid = false;                                  // the last run was a run_pos that consumed a block
	long long left_bytes = 0, n_notes = 0;
	// the left store: the unmated records of all blocks, a chunk per block, copied device to device; laddr[i] is record i's address
	std::vector<std::unique_ptr<psvr::DevBuf>> left_chunks;
	psvr::DevBuf laddr, lkeys, lprim, lerr, lctl;
	long long left_n = 0, laddr_cap = 0;
	// psvr_signal_run_left: the order (psvr::sort_order_names_device with the host comparator's tie key), the pair list from the runs
	psvr::NameScratch lN;
	psvr::SortScratch lS;
	std::vector<uint32_t> lhist;
	bool left_ordered = false, left_valid = false;
	long long left_pairs = 0, left_errors = 0, slice_first = 0, slice_pairs = 0;
};
