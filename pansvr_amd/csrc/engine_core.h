// engine_core.h -- batch orchestration of seam B1, independent of where the stages execute.
//
// `BE` (backend) owns memory and runs the stages: the product backend (engine.hip) launches HIP
// kernels on the MI355X; tests/emu provides a host backend that loops over the same
// __host__ __device__ stage functions so this logic can be checked against the oracle without a GPU.
//
// rand() order: the reference consumes one process-wide rand() stream in input order
// (N-base substitution, tied chains, tied pair scores) plus one random_r stream per handler
// (expand_seed sampling).  The streams are precomputed tables in HBM.  A pair is the atomic unit: its
// mate 0 runs prep..select first, mate 1 starts where mate 0 stopped, the pairing stage where mate 1
// stopped, so the draws D_p of pair p are a pure function of its stream offset O_p, and
// O_{p+1} = O_p + D_p(O_p).  D_p is almost always independent of O_p, so the batch runs speculatively:
//   1. run every pair at a guessed offset, scan the counts into offsets, re-run the pairs that drew from
//      a stale offset (most of them only need the pairing stage again);
//   2. the pairs whose count does depend on the drawn values form a serial chain that would cost one round
//      per flip.  Almost all of them contain N bases: D_p then depends on the substituted residues, not on
//      the offset, so every pair with 1..3 N draws is ALSO evaluated once per residue combination in
//      round 1 ("variant" shadow slots with forced draws, ~6 % extra work) and the chain
//      O_{s+1} = O_s + D_s(stream content at O_s) is walked exactly on the host through those tables;
//   3. any other pair whose count changes between two evaluations (tied chains in repeats) is evaluated at
//      a window of offsets around its estimate in the next round and joins the same host walk;
//   4. repeat until no pair is dirty (3-4 rounds in practice).
#pragma once
#include <stdint.h>
#include <stdio.h>
#include <string.h>
#include <algorithm>
#include <atomic>
#include <cstdlib>
#include <initializer_list>
#include <mutex>
#include <string>
#include <thread>
#include <chrono>
#include <type_traits>
#include <vector>
#include "aln_device.h"
#include "dp_plan.h"

namespace psvr {

// glibc TYPE_3 additive feedback generator: rand() (seed 1) and initstate_r(seed, 128-byte state)
struct HostRand3 {
	int32_t ring[31];
	int f, b;
	void seed(unsigned s)
	{
		int32_t word = s ? (int32_t)s : 1;
		ring[0] = word;
		for (int i = 1; i < 31; ++i) {
			long hi = word / 127773, lo = word % 127773;
			word = (int32_t)(16807 * lo - 2836 * hi);
			if (word < 0) word += 2147483647;
			ring[i] = word;
		}
		f = 3, b = 0;
		for (int i = 0; i < 310; ++i) next();
	}
	int32_t next()
	{
		uint32_t val = (uint32_t)ring[f] + (uint32_t)ring[b];
		ring[f] = (int32_t)val;
		int32_t r = (int32_t)(val >> 1);
		if (++f >= 31) { f = 0; ++b; }
		else if (++b >= 31) b = 0;
		return r;
	}
};

struct RandStream {           // lazily extended table of one generator + device mirror
	HostRand3 gen;
	std::vector<int32_t> host;   // host[k] = draw number k (absolute)
	void ensure(long long n) { while ((long long)host.size() < n) host.push_back(gen.next()); }
};

// The process-wide rand() stream (the reference never seeds it: seed 1), generated once for every engine of the process in blocks that never
// move.  Each engine used to keep a table of its own and extend it when its position left the device window: a pipeline's job slots -- or
// the devices of one command -- each generated the same millions of draws again, 17 ms at a time in the middle of a run (the overlapped
// rate through the ABI lost a third to it, the CLI's engine stage ~2 ms per batch).
struct SharedRand {
	static constexpr int kLog = 22;                      // 4 M draws per block
	static constexpr long long kMask = (1ll << kLog) - 1;
	std::mutex mu;
	HostRand3 gen;
	int32_t *blk[1 << 12] = {};                          // 16 G draws
	std::atomic<long long> n{0};
	SharedRand() { gen.seed(1); }
	~SharedRand() { for (int32_t *b : blk) delete[] b; }
	void ensure(long long want)
	{
		if (want <= n.load(std::memory_order_acquire)) return;
		std::lock_guard<std::mutex> lk(mu);
		long long k = n.load(std::memory_order_relaxed);
		want = (want + 0xfffff) & ~0xfffffll;            // a million at a time
		for (; k < want; ++k) {
			int32_t *&b = blk[k >> kLog];
			if (!b) b = new int32_t[(size_t)1 << kLog];
			b[k & kMask] = gen.next();
		}
		n.store(k, std::memory_order_release);
	}
	int32_t at(long long k) const { return blk[k >> kLog][k & kMask]; }          // k below what the caller has ensure()d
	void prefetch(long long k) const { if (k >= 0 && k < n.load(std::memory_order_relaxed)) __builtin_prefetch(blk[k >> kLog] + (k & kMask)); }
	// the draws [from, from + cnt) handed to `put(dst offset, source, entries)` block by block
	template <class F> void pieces(long long from, long long cnt, F &&put) const
	{
		for (long long o = 0; o < cnt;) {
			const long long k = from + o, room = (kMask + 1) - (k & kMask), m = cnt - o < room ? cnt - o : room;
			put(o, blk[k >> kLog] + (k & kMask), m);
			o += m;
		}
	}
};
inline SharedRand &shared_grand() { static SharedRand s; return s; }

struct DpIO {                 // what the DP stage needs beyond Ctx
	long long begin, end;     // descriptor range of this round
	int32_t *qlen, *tlen;
	long long *q_off, *t_off;
	uint8_t *qbuf, *tbuf;
	psvr_extz_t *ez;
	uint32_t *cig;
	long long qbytes, tbytes, cig_words;
};

// a backend that plans the DP stage on the device says so (kDevicePlan): its st_dp_plan brings the queue tops and flags with the plan
template <class B, class = void> struct plans_on_device : std::false_type {};
template <class B> struct plans_on_device<B, std::void_t<decltype(B::kDevicePlan)>> : std::true_type {};

// one device -> host copy: the backends' d2h takes a list of them and synchronises once
struct Readback { void *h; const void *d; size_t n; };
typedef std::initializer_list<Readback> Readbacks;

// The memory side of a backend whose "device" is host memory (tests/emu): zero-filled buffers, readbacks that are plain copies.
// EngineCore's default: such a backend only runs the stages.  (GpuBE is its own memory: DevBuf buffers, readbacks staged through
// page-locked memory.)
struct HostMem {
	struct Buf {                                 // the host twin of DevBuf
		void *p = nullptr;
		size_t bytes = 0;
		Buf() = default;
		Buf(const Buf &) = delete;
		Buf &operator=(const Buf &) = delete;
		~Buf() { release(); }
		void release() { free(p); p = nullptr; bytes = 0; }
		bool alloc(size_t n)
		{
			release();
			p = calloc(n ? n : 1, 1);
			bytes = p ? n : 0;
			return p != nullptr;
		}
	};
	bool note(bool ok) { return ok; }
	void d2h(Readbacks rb) { for (const Readback &x : rb) if (x.n) memcpy(x.h, x.d, x.n); }
	void d2h(void *h, const void *d, size_t n) { d2h({{h, d, n}}); }
	// (GPU: the small readbacks now, the long one queued behind them; here everything is there at once)
	std::vector<int32_t> late_buf;
	int32_t *d2h_early_late(Readbacks early, const void *dl, size_t nl)
	{
		d2h(early);
		late_buf.resize(nl / 4 + 1);
		memcpy(late_buf.data(), dl, nl);
		return late_buf.data();
	}
	void d2h_late_done() {}
	std::vector<int32_t> listed_idx;
	void gather_listed(const long long *a, const long long *b, const int32_t *cc, const int32_t *idx, long long n, long long *oa, long long *ob, int32_t *oc)
	{
		if (!n) return;                          // (the indices of the gather before stay: scatter_listed_i32 is not called then)
		listed_idx.assign(idx, idx + n);
		for (long long i = 0; i < n; ++i) oa[i] = a[idx[i]], ob[i] = b[idx[i]], oc[i] = cc[idx[i]];
	}
	void scatter_listed_i32(int32_t *a, const int32_t *val, long long n) { for (long long i = 0; i < n; ++i) a[listed_idx[i]] = val[i]; }
};

struct RunStats {
	long long rounds = 0, pairs_run = 0, pair_only = 0, shadow_runs = 0, sensitive = 0, window_miss = 0, dp_problems = 0, cands = 0, adopted = 0, stale_open = 0, dp_seq_bytes = 0, from_walk = 0;
	long long walk_pairs = 0, walk_us = 0, n_special = 0, special_const = 0, special_nomove = 0;     // the host walk over the N / tie-sensitive pairs: entries, microseconds (all rounds of the batch)
	unsigned long long counters[16] = {0};
};

// BE runs the stages; Mem owns the buffers and reads results back (d2h, d2h_early_late / d2h_late_done, gather_listed /
// scatter_listed_i32): GpuBE is both, a host backend keeps the default
template <class BE, class Mem = HostMem> struct EngineCore {
	BE &be;
	HostMem host;                                   // (Mem = HostMem)
	Mem &mem;
	// Device memory: every buffer is a member of Mem's owning type (GpuBE: DevBuf), freed when the core goes; Ctx and DpIO, the stages'
	// arguments, hold plain pointers into them.  get() (re)allocates one; a failure is noted by Mem (an ABI caller gets PSVR_ERR_DEVICE)
	// and clears alloc_ok.
	typedef typename Mem::Buf Buf;
	template <class T> struct Dev : Buf { operator T *() const { return (T *)this->p; } };
	bool alloc_ok = true;
	template <class T> T *get(Dev<T> &b, unsigned long long n) { alloc_ok &= mem.note(b.alloc((n ? n : 1) * sizeof(T))); return b; }
	Ctx c;
	long long P = 0, R = 0;                 // pairs / reads of the uploaded batch
	long long total_bases = 0;
	SharedRand &grand = shared_grand();             // rand(): one stream per process, as in the reference
	RandStream hrand[2];                            // random_r: one per handler
	long long grand_pos = 0, hrand_pos[2] = {0, 0};     // draws consumed by earlier batches
	long long grand_dev_n = 0, hrand_dev_n = 0;
	// the device tables hold a WINDOW of the host streams: entries [base, base + n).  A run, a rebase or a new batch whose needs lie inside the
	// window keeps it (a shard that moves behind its predecessors' draws, the next batch of a pipeline: no 28 MB upload, no hipFree)
	long long grand_dev_base = 0, hrand_dev_base[2] = {0, 0}, grand_dev_cap = 0, hrand_dev_cap = 0;
	Dev<int32_t> d_grand, d_hrand[2];
	// the per-batch buffers behind Ctx's arrays of the same names, and the scratch arenas
	struct {
		Dev<long long> poff, hoff;
		Dev<int32_t> rcnt, hcnt, str_list, read_l, n_ccand;
		Dev<unsigned int> str_cnt;
		Dev<uint8_t> active, unmapped, is_str, has_n4, has_mem, bin, seed_list;
		Dev<uint64_t> rb;
		Dev<Strand> strand;
		Dev<ChainCand> ccand;
		Dev<psvr_read_hdr_t> rh;
		Dev<psvr_pair_result_t> pres;
		Dev<unsigned long long> stats;
		Dev<VMem> mem;
		Dev<USeed> us;
		Dev<PathN> path;
		Dev<Seg> seg;
		Dev<DpDesc> dp;
		Dev<CandWork> cw;
		Dev<uint32_t> cig;
		Dev<psvr_cand_t> cand;
	} cb;
	// the core's own per-batch buffers
	Dev<long long> d_noff, d_nhoff;
	Dev<int32_t> d_work, d_workp;                    // full re-run list (real pairs then shadow slots) and the pairing-only list
	Dev<int32_t> d_ctot, d_src;                      // per slot: total draws of the last evaluation; slot -> input pair
	Dev<int32_t> d_hprev;                            // per slot x mate: random_r draws of the last evaluation (to see whether a round changed anything)
	Dev<uint8_t> d_sens;                             // per pair: known count-sensitive
	Dev<int32_t> d_slist;                            // newly detected sensitive pairs
	long long cap_S = 0, cap_P = 0; int cap_lm = 0;  // what the per-batch buffers were sized for (cap_S = 0: they are not usable)
	Dev<uint8_t> d_force, d_mask;                    // forced draws per read; per pair: resolved on the host (special or sensitive)
	// the special pairs on the device: the list, which of them draw the same number under every residue assignment (resolved there, not in the
	// host walk), the variant slot each of those carries and the offset it was adopted at
	Dev<SpecialPair> d_special;
	Dev<int32_t> d_vsrc, d_spidx;                    // variant slot -> pair, the special pairs' numbers: constant for the batch, copied / scattered device to device at every run
	Dev<uint8_t> d_sp_class;
	Dev<int32_t> d_sp_adopted;
	Dev<long long> d_sp_adopted_at;
	std::vector<uint8_t> h_sp_class;
	Dev<uint8_t> d_hasn;                             // per pair: a read of it draws for N bases (its draws are not just chain-selection ties)
	Dev<int32_t> d_resel, d_resel4;                  // pairs whose chain selection runs again on its own (reselect_pair); of those, the ones that go on from the walk
	std::vector<int32_t> h_n_idx;                    // pairs with N draws (built by upload())
	static const long long kReselCap = 1 << 16;      // tie-only pairs a round can resolve on the spot; beyond that they run in full
	Dev<int32_t> d_cmask;                            // totals with the host-resolved pairs masked out
	typedef SpecialPair Special;                     // (aln_device.h: the device looks at them too)
	std::vector<Special> special;                    // pairs with 1..3 N draws, ascending
	long long V = 0;                                 // variant slots [P, P+V)
	long long S = 0;                                 // slots = P real pairs + V variants + window-shadow capacity
	static const int kWin = 32;                      // offsets evaluated per sensitive pair and round
	Dev<unsigned long long> d_tops;           // the rounds' counters (aln_device.h TopWord)
	// the six arena tops, each in a cache line of its own (kTopStride words apart): a wavefront's atomic on a line costs ~12 ns however many
	// lanes take part, and atomics on one line are served one after the other (tools/atomic_rate_bench.hip) -- three counters that the
	// walk bumps per read shared one line
	static constexpr int kTopStride = kArenaTopStride * kArenaMaxShards;   // words between two arenas' first counters
	Dev<unsigned long long> d_atops;
	Dev<int32_t> d_flags;                     // the arenas' overflow flags and the stages' sticky words (aln_device.h FlagWord)
	unsigned long long cap[kArenaFlags] = {};        // the arenas' capacities, by their flag's name
	DpIO dp;
	struct { Dev<int32_t> qlen, tlen; Dev<long long> q_off, t_off; Dev<uint8_t> qbuf, tbuf; Dev<psvr_extz_t> ez; Dev<uint32_t> cig; } dpb;   // behind dp
	long long dp_cap_q = 0, dp_cap_t = 0, dp_cap_c = 0, dp_cap_n = 0;
	RunStats stats;
	std::string err;

	explicit EngineCore(BE &b) : be(b), mem(memory(b)) { memset(&c, 0, sizeof c); memset(&dp, 0, sizeof dp); }
	Mem &memory(BE &b)
	{
		if constexpr (std::is_same<Mem, BE>::value) return b;
		else return host;
	}

	void init(const DevIndex &ix, const psvr_aln_params_t &par)
	{
		c.idx = ix;
		c.par = par;
		int k = 0;                                 // ksw_gen_mat_D, rr.cpp:829-843
		for (int l = 0; l < 4; ++l) { for (int m = 0; m < 4; ++m) c.mat[k++] = (int8_t)(l == m ? par.match : -par.mismatch); c.mat[k++] = 0; }
		for (int m = 0; m < 5; ++m) c.mat[k++] = 0;
		// rr.cpp:62-67 at -t 1: the two handlers seed their random_r state with rand() draws #0 and #1
		grand.ensure(2);
		hrand[0].gen.seed((unsigned)grand.at(0));
		hrand[1].gen.seed((unsigned)grand.at(1));
		grand_pos = 2;
	}

	// PSVR_RAND_SHRINK=<n>: a window sized for a run holds 1/n of its entries, so that a small input walks through the "draw window
	// exhausted -> extend -> run the batch again" path (tests); the extension itself is not shrunk
	static long long shrunk_window(long long n, bool extension)
	{
		const char *e = extension ? nullptr : getenv("PSVR_RAND_SHRINK");
		const long long f = e ? atoll(e) : 0;
		return f > 1 ? n / f + 64 : n;
	}
	bool upload_rand(long long need_g, long long need_h, bool extension = false)
	{
		// entries beyond what this run needs: room for the position to move before the window is uploaded again (a batch of 1 M pairs needs a
		// window of 4.7 M and draws ~0.4 M times: forty batches; small inputs stay small)
		const long long margin_h = 1 << 20, margin = std::max<long long>(margin_h, 4 * need_g);
		if (!(d_grand && grand_pos >= grand_dev_base && grand_pos + need_g <= grand_dev_base + grand_dev_n)) {
			const long long n = shrunk_window(need_g + need_g / 2 + 4096 + margin, extension);
			grand.ensure(grand_pos + n);
			if (n > grand_dev_cap || !d_grand) {
				if (!get(d_grand, n)) return false;
				grand_dev_cap = n;
			}
			grand.pieces(grand_pos, n, [&](long long o, const int32_t *src, long long m) { be.h2d(d_grand + o, src, (size_t)m * 4); });
			grand_dev_base = grand_pos, grand_dev_n = n;
		}
		bool hok = d_hrand[0] && d_hrand[1];
		for (int k = 0; k < 2 && hok; ++k) hok = hrand_pos[k] >= hrand_dev_base[k] && hrand_pos[k] + need_h <= hrand_dev_base[k] + hrand_dev_n;
		if (!hok) {
			const long long n = shrunk_window(need_h + need_h / 2 + 4096 + margin_h, extension);
			for (int k = 0; k < 2; ++k) {
				hrand[k].ensure(hrand_pos[k] + n);
				if ((n > hrand_dev_cap || !d_hrand[k]) && !get(d_hrand[k], n)) return false;
				be.h2d(d_hrand[k], hrand[k].host.data() + hrand_pos[k], n * 4);
				hrand_dev_base[k] = hrand_pos[k];
			}
			if (n > hrand_dev_cap) hrand_dev_cap = n;
			hrand_dev_n = n;
		}
		c.grand = d_grand, c.grand_n = grand_dev_n, c.grand_base = grand_dev_base;
		for (int k = 0; k < 2; ++k) c.hrand[k] = d_hrand[k], c.hrand_base[k] = hrand_dev_base[k];
		c.hrand_n = hrand_dev_n;
		return true;
	}

	// ---- batch upload: allocate everything sized by the batch
	// the batch's three arrays on the device, in buffers of their own (kept while the next batch fits), and the list the device's pass
	// over the batch leaves: (pair, n0 | n1 << 8) for every pair a read of which will draw for N bases
	long long in_cap_bases = 0, in_cap_R = 0;
	Dev<char> d_bases;
	Dev<long long> d_off;
	Dev<psvr_ori_t> d_ori;
	Dev<int32_t> d_nlist;
	int upload(long long n_pairs, const char *bases, const int64_t *base_off, const psvr_ori_t *ori)
	{
		const int rc = place_batch(n_pairs, bases, base_off, ori);
		// a failure, too, returns only when the batch's copies are through: the caller's arrays are free once upload returns (psvr_engine.h)
		if (rc) be.h2d_wait();
		return rc;
	}
	int place_batch(long long n_pairs, const char *bases, const int64_t *base_off, const psvr_ori_t *ori)
	{
		// a block of a larger batch may be handed over as a window of the batch's arrays: offsets then start at base_off[0] > 0
		const long long b0 = n_pairs ? base_off[0] : 0;
		return place_batch_from(n_pairs, b0, n_pairs ? base_off[2 * n_pairs] - b0 : 0, [&]() {
			be.h2d_start(d_bases, bases + b0, total_bases);
			be.h2d_start(d_off, base_off, (R + 1) * 8);
			be.h2d_start(d_ori, ori, R * sizeof(psvr_ori_t));
		});
	}
	// The same batch from arrays that are already in this device's memory (psvr_engine_upload_fastq: what psvr_fastq_parse left there).
	// The host cannot read base_off there: the caller says where the window's bases start (b0) and how many there are.
	int upload_device(long long n_pairs, const char *src_bases, const int64_t *src_off, const psvr_ori_t *src_ori, long long b0, long long n_bases)
	{
		const int rc = place_batch_from(n_pairs, b0, n_bases, [&]() {
			be.d2d_start(d_bases, src_bases + b0, total_bases);
			be.d2d_start(d_off, src_off, (R + 1) * 8);
			be.d2d_start(d_ori, src_ori, R * sizeof(psvr_ori_t));
		});
		if (rc) be.h2d_wait();
		return rc;
	}
	// start_copies() puts the three arrays' copies into d_bases / d_off / d_ori on the backend's queue
	template <class Copies> int place_batch_from(long long n_pairs, long long b0, long long n_bases, Copies &&start_copies)
	{
		P = n_pairs, R = 2 * n_pairs;
		total_bases = R ? n_bases : 0;
		// The three arrays go to the device first, and the DEVICE looks at them (scan_batch: the longest read, the pairs whose reads will
		// draw for N bases; early-out reads draw nothing, rr.cpp:414 returns first).  Until round 4 the host made those passes over every
		// base before the transfer started -- 5 of an upload's 12 ms for 1 M pairs on eight threads, which a pipeline's three job slots
		// took from the thread that drives the runs: the overlapped rate through the ABI was bound by it.
		if (!d_bases || total_bases > in_cap_bases || R > in_cap_R) {
			in_cap_bases = total_bases + total_bases / 8 + 64, in_cap_R = R + R / 8 + 2;
			alloc_ok = true;
			get(d_bases, in_cap_bases + 64);     // slack: the prep kernel loads whole 32-base groups
			get(d_off, in_cap_R + 1), get(d_ori, in_cap_R), get(d_nlist, 2 * (in_cap_R / 2 + 2));
			if (!alloc_ok) { d_bases.release(); err = "device allocation failed (batch)"; return PSVR_ERR_NOMEM; }
		}
		special.clear(), h_n_idx.clear();
		V = 0;
		int lmax = 0;
		if (R > 0) {
			start_copies();
			std::vector<int32_t> nl;                                     // (pair, counts) pairs as the device appended them
			if (!be.scan_batch(d_bases - b0, d_off, d_ori, P, c.par.match, d_nlist, &lmax, nl)) { err = "device pass over the batch failed"; return PSVR_ERR_DEVICE; }
			// (scan_batch has synchronised: the caller's arrays are free again)
			if (lmax > kMaxReadLen) { err = "read longer than MAX_READ_LEN 1600"; return PSVR_ERR_UNSUPPORTED; }
			std::vector<std::pair<int32_t, int32_t>> srt(nl.size() / 2);
			for (size_t i = 0; i < srt.size(); ++i) srt[i] = {nl[2 * i], nl[2 * i + 1]};
			std::sort(srt.begin(), srt.end());
			for (const auto &e : srt) {
				const int n0 = e.second & 0xff, n1 = (e.second >> 8) & 0xff;   // (counts saturate at 255: anything beyond 3 is "many")
				h_n_idx.push_back(e.first);
				if (n0 + n1 <= 3) { special.push_back(Special{e.first, (uint8_t)n0, (uint8_t)n1, (int32_t)(P + V), 1 << (2 * (n0 + n1))}); V += 1ll << (2 * (n0 + n1)); }
			}
		}
		c.n_pairs = P;
		int lm = (lmax + 31) & ~31;
		if (lm < 32) lm = 32;
		const long long shadow_cap = P / 16 + 8192;
		S = P + V + shadow_cap;
		c.n_slots = S;
		// keep every per-batch buffer (and the arenas) while the new batch fits
		const bool fits = S <= cap_S && lm <= cap_lm && P <= cap_P;
		c.bases = d_bases - b0, c.base_off = d_off, c.ori = d_ori;
		if (fits) {
			upload_variants();
			return PSVR_OK;
		}
		cap_S = S, cap_lm = lm, cap_P = P;
		c.lmax = lm;
		c.wmax = c.lmax / 32 + 2;
		const long long RS = 2 * S;                                 // reads incl. shadow slots
		alloc_ok = true;
		c.poff = get(cb.poff, S), c.rcnt = get(cb.rcnt, 3 * S), get(d_noff, S);
		c.hoff = get(cb.hoff, RS), c.hcnt = get(cb.hcnt, RS), get(d_nhoff, RS);
		c.active = get(cb.active, RS), c.unmapped = get(cb.unmapped, RS), c.is_str = get(cb.is_str, RS), c.has_n4 = get(cb.has_n4, RS);
		c.has_mem = get(cb.has_mem, RS);
		c.str_list = get(cb.str_list, RS), c.str_cnt = get(cb.str_cnt, 4);
		c.read_l = get(cb.read_l, RS);
		c.bin = get(cb.bin, (unsigned long long)RS * 2 * c.lmax);
		c.rb = get(cb.rb, (unsigned long long)RS * 2 * c.wmax);
		c.seed_list = get(cb.seed_list, (unsigned long long)RS * c.lmax);
		c.strand = get(cb.strand, 2 * RS);
		c.ccand = get(cb.ccand, 12 * RS), c.n_ccand = get(cb.n_ccand, RS);
		c.rh = get(cb.rh, RS), c.pres = get(cb.pres, S);
		get(d_work, S), get(d_workp, P);
		get(d_ctot, S), get(d_src, S), get(d_sens, P), get(d_slist, P);
		get(d_hprev, 2 * S);
		get(d_force, 8 * S), get(d_mask, P), get(d_cmask, P);
		get(d_hasn, P), get(d_resel, P), get(d_resel4, P < kReselCap ? P : kReselCap);
		{
			const long long nsp = S / 4 + 1;                 // (a special pair has >= 4 variant slots: whatever batch fits these buffers later has no more)
			get(d_vsrc, S), get(d_spidx, nsp);
			get(d_special, nsp), get(d_sp_class, nsp), get(d_sp_adopted, nsp), get(d_sp_adopted_at, nsp);
		}
		get(d_tops, kTopWords), get(d_atops, kArenaFlags * kTopStride), get(d_flags, kFlagWords);
		const long long R2 = RS;
		cap[kFlagMem] = (unsigned long long)2 * R2 * kMemSlot + (unsigned long long)R2 * 16 + 4096;
		cap[kFlagUs] = (unsigned long long)R2 * 48 + 65536;
		cap[kFlagCw] = (unsigned long long)R2 * 3 + 1024;
		cap[kFlagSeg] = cap[kFlagCw] * 16;
		cap[kFlagDp] = (unsigned long long)R2 * 4 + 1024;
		cap[kFlagCig] = (unsigned long long)R2 * 48 + 4096;
		// PSVR_ARENA_SHRINK=<n>: start with 1/n of the scratch arenas, so that a small input walks through the overflow -> grow -> re-run
		// path of every arena (tests)
		if (const char *e = getenv("PSVR_ARENA_SHRINK")) {
			const unsigned long long n = (unsigned long long)atoll(e);
			if (n > 1) {
				for (int a : {kFlagUs, kFlagCw, kFlagSeg, kFlagDp, kFlagCig}) cap[a] = cap[a] / n + 64;
				const unsigned long long slots = (unsigned long long)2 * R2 * kMemSlot;    // fixed per-strand slots: only the bump region behind them shrinks
				cap[kFlagMem] = slots + (cap[kFlagMem] - slots) / n + 64;
			}
		}
		c.stats = get(cb.stats, 16);
		if (!alloc_ok || !alloc_arenas()) { cap_S = 0; err = "device allocation failed"; return PSVR_ERR_NOMEM; }
		c.err = d_flags + kFlagErr, c.stale_open = d_flags + kFlagStaleOpen, c.any_h = d_flags + kFlagAnyH;
		upload_variants();
		return PSVR_OK;
	}

	// variant slots: pair s at every combination of its N-substitution residues.  Only those slots force draws, so the
	// table is zeroed on the device and just their rows are uploaded, once per batch.
	void upload_variants()
	{
		{
			std::vector<uint8_t> force((size_t)8 * V, 0);
			h_vsrc.assign(V, 0), h_sp_idx.assign(special.size(), 0);
			for (size_t i = 0; i < special.size(); ++i) {
				const Special &sp = special[i];
				h_sp_idx[i] = sp.pair;
				for (int v = 0; v < sp.nvar; ++v) {
					long long slot = sp.vslot + v;
					h_vsrc[slot - P] = sp.pair;
					int code = v;
					for (int k = 0; k < 2; ++k) {
						int n = k == 0 ? sp.n1 : sp.n2;
						uint8_t *f = &force[4 * (2 * (slot - P) + k)];
						f[0] = (uint8_t)n;
						for (int j = 0; j < n; ++j) f[1 + j] = (uint8_t)(code & 3), code >>= 2;
					}
				}
			}
			be.dzero(d_force, (size_t)8 * S);
			if (V) be.h2d(d_force + (size_t)8 * P, force.data(), force.size());
			be.dzero(d_hasn, (size_t)P);
			if (!special.empty()) {                                   // (constant for the batch, like d_force)
				be.h2d(d_special, special.data(), special.size() * sizeof(Special));
				be.h2d(d_spidx, h_sp_idx.data(), h_sp_idx.size() * 4);
			}
			if (V) be.h2d(d_vsrc, h_vsrc.data(), V * 4);
			if (!h_n_idx.empty()) be.scatter_u8(d_hasn, h_n_idx.data(), (long long)h_n_idx.size(), 1);
		}
	}

	bool alloc_arenas()
	{
		alloc_ok = true;
		// an arena's storage, and its counter, capacity and overflow flag at its place (FlagWord) in d_atops, cap[] and d_flags
		// nshard 1: mem has fixed slots in front; dp, cw: their ids are ranges the host plans on; cig: downloaded as one piece
		auto place = [&](auto &a, auto &buf, int w, unsigned int nshard) {
			a.base = get(buf, cap[w]), a.top = d_atops + w * kTopStride, a.cap = cap[w], a.overflow = d_flags + w, a.nshard = nshard;
		};
		place(c.mem, cb.mem, kFlagMem, 1), place(c.us, cb.us, kFlagUs, BE::kArenaShards), c.path = get(cb.path, cap[kFlagUs]);
		place(c.seg, cb.seg, kFlagSeg, BE::kArenaShards), place(c.dp, cb.dp, kFlagDp, 1), place(c.cw, cb.cw, kFlagCw, 1), place(c.cig, cb.cig, kFlagCig, 1);
		c.cand = get(cb.cand, cap[kFlagCw]);       // candidate records share the CandWork arena's indices
		return alloc_ok;
	}
	// which arenas filled up in a round, by their flag's name: what run_slots and the round end report and grow_arenas takes
	struct ArenaFull {
		int32_t flag[kArenaFlags] = {};
		bool any() const { int a = 0; for (int32_t f : flag) a |= f; return a != 0; }
	};
	// a scratch arena overflowed (repeat-rich reads expand to many seeds): grow it 4x; the caller runs the batch again
	int grow_arenas(const ArenaFull &full)
	{
		for (int a = 0; a < kArenaFlags; ++a) if (full.flag[a]) cap[a] *= 4;
		if (full.flag[kFlagMem]) cap[kFlagMem] += (unsigned long long)4 * S * kMemSlot;
		fprintf(stderr, "[psvr] scratch arena overflow (mem %d us %d seg %d dp %d cand %d cigar %d): growing 4x and re-running the batch\n", full.flag[kFlagMem], full.flag[kFlagUs],
		        full.flag[kFlagSeg], full.flag[kFlagDp], full.flag[kFlagCw], full.flag[kFlagCig]);
		if (!alloc_arenas()) { cap_S = 0; err = "device allocation failed while growing arenas"; return PSVR_ERR_NOMEM; }
		return PSVR_OK;
	}
	// a stage asked for a draw beyond the device's window of a stream: a window four times as long; the caller runs the batch again
	int extend_rand_window(int stage_err)
	{
		fprintf(stderr, "[psvr] draw window exhausted (%s, %lld rand() and %lld random_r entries): extending and re-running the batch\n", stage_err == kErrRandWindow ? "rand()" : "random_r",
		        c.grand_n, c.hrand_n);
		be.dzero(d_flags, kFlagWords * sizeof(int32_t));
		grand_dev_n = hrand_dev_n = 0;
		if (!upload_rand(c.grand_n * 4, c.hrand_n * 4, true)) { err = "rand table allocation failed"; return PSVR_ERR_NOMEM; }
		return PSVR_OK;
	}

	// the DP stage's buffers for n problems and qb / tb / cw bytes and CIGAR words: grown to need + need / 4 + 1024 when a round needs more
	bool ensure_dp(long long n, long long qb, long long tb, long long cw)
	{
		auto room = [](long long need) { return need + need / 4 + 1024; };
		alloc_ok = true;
		if (n + 2 > dp_cap_n) {
			dp_cap_n = room(n + 2);
			dp.qlen = get(dpb.qlen, dp_cap_n), dp.tlen = get(dpb.tlen, dp_cap_n), dp.q_off = get(dpb.q_off, dp_cap_n), dp.t_off = get(dpb.t_off, dp_cap_n);
			dp.ez = get(dpb.ez, dp_cap_n);
		}
		if (qb + 64 > dp_cap_q) dp.qbuf = get(dpb.qbuf, dp_cap_q = room(qb + 64));
		if (tb + 64 > dp_cap_t) dp.tbuf = get(dpb.tbuf, dp_cap_t = room(tb + 64));
		if (cw + 64 > dp_cap_c) dp.cig = get(dpb.cig, dp_cap_c = room(cw + 64));
		if (!alloc_ok) dp_cap_n = dp_cap_q = dp_cap_t = dp_cap_c = 0;     // (every one of them again next time)
		return alloc_ok;
	}

	// the stages of one round over a list of slots: mate 0, then mate 1 (continues mate 0's draws), then the
	// candidate / DP / pairing stages
	// `nwalk`: entries behind the first nwork of `work` that go on from the walk (their chain selection has been repeated already, k_reselect)
	// `full`: the arenas that filled up; the round has ended behind the walk then (PSVR_OK all the same) and the batch must run again
	int run_slots(const int32_t *work, long long nwork, long long &dp_done, long long &cw_done, long long nwalk, ArenaFull &full)
	{
		if (nwork + nwalk <= 0) return PSVR_OK;
		for (int mate = 0; mate < 2; ++mate) {
			be.st_prep(c, work, nwork, mate);
			be.st_str(c, work, nwork, mate);
			be.st_seed(c, work, nwork, mate);
			be.st_chain(c, work, nwork, mate);
		}
		be.st_walk(c, work, nwork + nwalk);
		int32_t fl[kFlagWords];
		long long dp_end, cw_end;
		if constexpr (plans_on_device<BE>::value) {
			// the DP stage is planned and placed on the device behind the walk: the queue tops and the flags come back with the plan, the
			// round's one readback before the DP launches (nothing is placed when an arena has overflowed)
			int rc = be.st_dp_plan(*this, dp_done, dp_end, cw_end, fl);
			if (rc) return rc;
		} else {
			constexpr int first = kFlagDp * kTopStride, dp_at = 0, cw_at = kFlagCw * kTopStride - first;   // one readback from the dp counter to the cw counter
			unsigned long long tops[cw_at + 1];
			mem.d2h({{tops, d_atops + first, sizeof tops}, {fl, d_flags, sizeof fl}});
			dp_end = (long long)tops[dp_at], cw_end = (long long)tops[cw_at];
		}
		note_sticky_flags(fl);
		// An arena that filled up in the stages so far ends the round here: what follows (assembly, the reads' tails) would walk records
		// that were never written.  (The CIGAR arena is filled by the assembly: the round end sees that one.)
		for (int a : {kFlagMem, kFlagUs, kFlagSeg, kFlagDp, kFlagCw}) full.flag[a] = fl[a] != 0;
		if (dp_end > (long long)cap[kFlagDp]) full.flag[kFlagDp] = 1;
		if (cw_end > (long long)cap[kFlagCw]) full.flag[kFlagCw] = 1;
		if (full.any()) return PSVR_OK;
		if (dp_end > dp_done) {
			dp.begin = dp_done, dp.end = dp_end;
			int rc = be.st_dp(*this);
			if (rc) return rc;
		}
		c.dp_ez = dp.ez ? dp.ez - dp_done : nullptr, c.dp_cig = dp.cig;   // DP ids are absolute, the result buffers are per round
		if (cw_end > cw_done) be.st_assemble(c, cw_done, cw_end);
		stats.dp_problems += dp_end - dp_done, stats.cands += cw_end - cw_done;
		dp_done = dp_end, cw_done = cw_end;
		be.st_finalize_pair(c, work, nwork + nwalk);       // both reads' tails, then the pairing, by the same worker: the records stay close
		return PSVR_OK;
	}
	// the words of a flag readback that only ever go up during a run
	void note_sticky_flags(const int32_t *fl)
	{
		if (fl[kFlagAnyH]) any_h = true;
		if (fl[kFlagStaleOpen]) stats.stale_open = 1;
	}

	// ---- one full run of the uploaded batch (rand state is NOT advanced: call commit() for that)
	struct Win { int32_t pair; long long eval_off; int32_t eval_tot; std::vector<long long> off; std::vector<int32_t> tot; };   // window-resolved pair
	// state of the current batch's resolution, kept so that rebase() can continue from it
	std::vector<int32_t> w_listed, w_cur_tot, w_res;    // scratch of the host offset walk, kept across iterations
	std::vector<long long> w_pre, w_cur_off;
	std::vector<int32_t> h_vsrc, h_sp_idx;            // variant slot -> pair; pairs with variant slots (built by upload())
	// per variant slot: c1, c2, c3 -- read back once per batch (1 MB on the bench batch); a plain buffer: a vector's resize() would zero what the
	// readback overwrites
	struct HostTable {
		int32_t *p = nullptr;
		size_t n = 0, cap = 0;
		bool empty() const { return n == 0; }
		void clear() { n = 0; }
		int32_t *data() { return p; }
		const int32_t &operator[](size_t i) const { return p[i]; }
		bool resize(size_t want)
		{
			if (want > cap) {
				free(p);
				cap = want + want / 4 + 1024;
				p = (int32_t *)malloc(cap * sizeof(int32_t));
				if (!p) { cap = n = 0; return false; }
			}
			n = want;
			return true;
		}
		~HostTable() { free(p); }
		HostTable() = default;
		HostTable(const HostTable &) = delete;
		HostTable &operator=(const HostTable &) = delete;
	} vcnt;
	// The host walk's view of the variant table: per host-resolved special pair the rows of its variant slots, (c1, 2 D + adoptable), copied
	// out of the 1 MB table once per batch in walk order.  The walk visits a few thousand pairs once per step with cold caches: through
	// special[] by search, the table by row and three more per-pair arrays it paid ~170 ns of cache misses per pair (0.5 ms for 2.9 k
	// pairs); over arrays laid out in the order it walks them the prefetchers keep up.
	struct HwRow { int32_t c1, d_ok; };
	std::vector<HwRow> hw_rows;
	std::vector<int32_t> sp_row0;                     // per special pair: its first row in hw_rows (-1: none)
	std::vector<int32_t> l_si;                        // per entry of the walk's list: its index in special[] (-1: a window-resolved pair)
	void build_rows()
	{
		if (vcnt.empty()) return;
		const size_t nl = l_si.size();
		for (size_t k = 0; k < nl; ++k) {
			if (k + 12 < nl && l_si[k + 12] >= 0) __builtin_prefetch(&vcnt[3 * (size_t)(special[(size_t)l_si[k + 12]].vslot - P)]);
			const int32_t si = l_si[k];
			if (si < 0 || sp_row0[(size_t)si] >= 0) continue;
			const Special &sp = special[(size_t)si];
			sp_row0[(size_t)si] = (int32_t)hw_rows.size();
			const int32_t *vc = &vcnt[3 * (size_t)(sp.vslot - P)];
			for (int v = 0; v < sp.nvar; ++v, vc += 3) {
				// adoptable: the two reads of that variant slot drew at least the forced residues (see the walk)
				HwRow r; r.c1 = vc[0], r.d_ok = 2 * (vc[0] + vc[1] + vc[2]) + ((vc[0] >= sp.n1 && vc[1] >= sp.n2) ? 1 : 0);
				hw_rows.push_back(r);
			}
		}
	}
	std::vector<Win> wins;                            // window-resolved (tie-sensitive) pairs, ascending
	std::vector<char> is_special;                     // a special pair whose prediction failed falls back to the window method
	std::vector<int32_t> adopted, adopt_pair, adopt_slot;   // per special pair: the variant slot whose records it carries (-1 none); this walk's new adoptions
	std::vector<long long> adopted_at;                      // ... and the stream offset it was adopted at (a slot whose pairing draws is adopted again when the pair moves)
	long long dp_done = 0, cw_done = 0;
	bool have_run = false;
	bool any_h = false;                               // a read of this batch has drawn from random_r

	// The device statistics pointer is null during a run without statistics (the stages then count nothing); back in place when the run is
	// over, however it ends.
	struct StatsOff {
		Ctx &c;
		unsigned long long *keep;
		StatsOff(Ctx &ctx, bool want_stats) : c(ctx), keep(ctx.stats) { if (!want_stats) c.stats = nullptr; }
		~StatsOff() { c.stats = keep; }
		StatsOff(const StatsOff &) = delete;
		StatsOff &operator=(const StatsOff &) = delete;
	};

	// What one pass of iterate() hands to the next, and what the phases of a pass hand to each other.
	struct Round {
		// the next evaluation: d_work holds nfull dirty real pairs, then nshadow shadow slots, then nwalk pairs that go on from the walk;
		// d_workp the npair_only pairs that only repeat their pairing stage
		const int32_t *work = nullptr;                    // nullptr = identity: round 1 runs every real pair and every variant slot
		long long nfull = 0, npair_only = 0, nshadow = 0, nwalk = 0;
		bool pair_done = false;                           // the pairing-only list has run (behind the round end that made it, its length still on the device)
		bool pre_tot = false;                             // ... and its totals were taken right behind it (they sit in the words kTopNewSens, kTopChanged and in d_slist)
		std::vector<int32_t> sh_src;                      // the shadow slots of that evaluation: pair ...
		std::vector<long long> sh_off;                    // ... and offset
		bool resume = false;                              // a rebase: the first pass evaluates nothing and starts at the offsets; the random_r scans run in every pass
		// the pass in hand
		bool gathered = false;                            // the walk's list has been built and gathered behind the totals (first round)
		bool h_scans = false;                             // the random_r offsets were scanned (d_nhoff is valid)
		unsigned long long nnew = 0, changed = 0;         // read_totals: newly count-sensitive pairs; did any evaluated slot draw a different number than last time?
		unsigned long long tops[kTopReadEnd - kTopReadFirst];   // end_round's readback of the counters ...
		int32_t flags[kFlagWords];                               // ... and of the flag block
		unsigned long long top(int word) const { return tops[word - kTopReadFirst]; }
		ArenaFull full;                                   // verdict kGrowArenas: which
		int rc = PSVR_OK;                                 // verdict kFailed: why (with `err`)
	};
	enum Verdict { kNextRound, kDone, kGrowArenas, kExtendWindow, kFailed };

	// A run and its restarts: set up, iterate, and when an arena or a draw window was too small enlarge it and run the batch again.
	// `restarts`: how many a caller has used up already (rebase).
	int run(int trace, bool want_stats, int restarts = 0)
	{
		for (;; ++restarts) {
			stats = RunStats();
			c.trace = trace;
			if (P == 0) return PSVR_OK;
			Round r;
			Verdict v;
			{
				StatsOff quiet(c, want_stats);
				if (!upload_rand(total_bases / 64 + 4096, 4096)) { err = "rand table allocation failed"; return PSVR_ERR_NOMEM; }
				begin_run();
				r.nfull = P + V;
				v = iterate(r, want_stats);
			}
			if (v != kGrowArenas && v != kExtendWindow) return r.rc;
			const int rc = prepare_restart(v, r, restarts);
			if (rc) return rc;
		}
	}
	// what a grow or an extend verdict asks for before the batch runs again
	int prepare_restart(Verdict v, const Round &r, int restarts)
	{
		if (restarts > 8) {
			err = v == kGrowArenas ? "scratch arena overflow persists after 8 growth steps" : "draw window exhausted again after 8 restarts of the batch";
			return PSVR_ERR_OVERFLOW;
		}
		return v == kGrowArenas ? grow_arenas(r.full) : extend_rand_window(r.flags[kFlagErr]);
	}
	void begin_run()
	{
		// initial guess: nobody draws.  One pass over the slots: poff = grand_pos, hoff = the two random_r positions, rcnt = hcnt = ctot = hprev =
		// sens = mask = 0, src = identity (the variant slots: their pair); the special pairs' classes and adoptions; the counters, flags and
		// statistics; the bump region's start behind the per-strand MEM slots -- a dozen fills, copies and memsets of their own were 0.1 ms per run.
		{
			RunInit ri;
			ri.poff = c.poff, ri.hoff = c.hoff, ri.rcnt = c.rcnt, ri.hcnt = c.hcnt, ri.ctot = d_ctot, ri.hprev = d_hprev, ri.src = d_src, ri.sens = d_sens, ri.mask = d_mask;
			ri.S = S, ri.P = P, ri.V = V, ri.g = grand_pos, ri.h0 = hrand_pos[0], ri.h1 = hrand_pos[1];
			ri.vsrc = d_vsrc, ri.spidx = d_spidx, ri.nsp = (long long)special.size();
			ri.sp_class = d_sp_class, ri.sp_adopted = d_sp_adopted, ri.sp_adopted_at = d_sp_adopted_at;
			ri.tops = d_tops, ri.n_tops = kTopRunInit, ri.atops = d_atops, ri.n_atops = kArenaFlags * kTopStride, ri.flags = d_flags, ri.stats = cb.stats;   // (the statistics are cleared whether or not this run counts)
			ri.mem_top = c.mem.top, ri.mem0 = (unsigned long long)4 * S * kMemSlot;   // bump region starts behind the per-strand slots
			be.run_init(ri);
		}
		c.src = d_src, c.force = d_force;
		// (the special pairs are masked after the pass above has cleared every pair's bit)
		if (!h_sp_idx.empty()) be.scatter_u8_dev(d_mask, d_spidx, (long long)h_sp_idx.size(), 1);
		h_sp_class.assign(special.size(), 0);
		dp_done = 0, cw_done = 0, any_h = false;
		vcnt.clear(), wins.clear(), is_special.assign(special.size(), 1);
		hw_rows.clear(), sp_row0.assign(special.size(), -1);
		adopted.assign(special.size(), -1), adopted_at.assign(special.size(), -1), adopt_pair.clear(), adopt_slot.clear();
		have_run = true;
	}

	// The streams of this batch start somewhere else than assumed (another rank's shard precedes it): move every offset
	// and re-run only what drew from a stale position.  Results and draw counts afterwards are those of a run() that had
	// started at the new position.
	int rebase(long long g, long long h0, long long h1, int trace, bool want_stats)
	{
		if (!have_run || P == 0) { grand_pos = g, hrand_pos[0] = h0, hrand_pos[1] = h1; return PSVR_OK; }
		if (g == grand_pos && h0 == hrand_pos[0] && h1 == hrand_pos[1]) return PSVR_OK;
		grand_pos = g, hrand_pos[0] = h0, hrand_pos[1] = h1;
		Round r;
		Verdict v;
		{
			StatsOff quiet(c, want_stats);
			if (!upload_rand(total_bases / 64 + 4096, 4096)) { err = "rand table allocation failed"; return PSVR_ERR_NOMEM; }
			for (Win &w : wins) w.off.clear(), w.tot.clear(), w.eval_off = -1;
			r.resume = true;
			v = iterate(r, want_stats);
		}
		if (v != kGrowArenas && v != kExtendWindow) return r.rc;
		// too small an arena or window: a full run from the new position
		const int rc = prepare_restart(v, r, 0);
		return rc ? rc : run(trace, want_stats, 1);
	}

	// The rounds: evaluate the slots of the round, read their totals, walk the offsets on the host, mark what is dirty, plan the next round.
	Verdict iterate(Round &r, bool want_stats)
	{
		Verdict v = kNextRound;
		for (bool evaluate = !r.resume; v == kNextRound; evaluate = true) {
			r.gathered = r.h_scans = false;
			if (evaluate) {
				if ((v = evaluate_round(r)) != kNextRound) break;
				if ((v = read_totals(r)) != kNextRound) break;
				// A re-run round in which every slot drew exactly as often as at its previous evaluation leaves every offset where it is: the
				// streams are consistent, the bookkeeping below would find nothing dirty.
				if (r.work != nullptr && r.nnew == 0 && r.changed == 0 && r.nshadow == 0 && wins.empty()) { v = kDone; break; }
				take_in_windows_and_sensitive(r);
			}
			resolve_offsets(r, want_stats);
			end_round(r, want_stats);
			if ((v = verdict(r)) == kNextRound) plan_offset_windows(r);
		}
		if (v == kDone && want_stats) mem.d2h(stats.counters, c.stats, sizeof stats.counters);
		return v;
	}

	// ---- the phases of a pass
	// Evaluate a round: the listed slots through the stages, the pairing-only list, and the totals passes over both.
	Verdict evaluate_round(Round &r)
	{
		stats.rounds++;
		if (r.work == nullptr) stats.pairs_run += P, stats.shadow_runs += V; else stats.pairs_run += r.nfull, stats.shadow_runs += r.nshadow;
		stats.pair_only += r.npair_only;
		// the pairs that only repeat their pairing stage are not among the slots that run in full: a backend with a second queue does
		// them beside the stage chain
		const bool beside = r.npair_only > 0 && !r.pair_done && be.side_begin();
		if (beside) { be.st_pair(c, d_workp, r.npair_only); be.side_end(); }
		stats.from_walk += r.nwalk;
		r.full = ArenaFull();
		r.rc = run_slots(r.work, r.nfull + r.nshadow, dp_done, cw_done, r.nwalk, r.full);
		if (beside) be.side_wait();
		if (r.rc) return kFailed;
		if (r.full.any()) return kGrowArenas;
		if (r.npair_only && !beside && !r.pair_done) be.st_pair(c, d_workp, r.npair_only);
		r.pair_done = false;
		// totals of the evaluated slots; a real pair whose total differs from what the offsets assumed is sensitive
		unsigned long long *const cnt = d_tops + kTopNewSens;                        // (and kTopChanged behind it)
		if (!r.pre_tot) be.dzero(cnt, (kTopChanged + 1 - kTopNewSens) * sizeof *cnt);
		be.st_totals(c, r.work, r.nfull + r.nshadow + r.nwalk, d_ctot, d_hprev, d_sens, d_slist, cnt, r.work != nullptr);
		if (r.npair_only && !r.pre_tot) be.st_totals(c, d_workp, r.npair_only, d_ctot, d_hprev, d_sens, d_slist, cnt, true);
		r.pre_tot = false;
		return kNextRound;
	}

	// Read the round's totals counters: r.nnew, r.changed.  In the first round the offset scans and the walk's list ride on the same wait.
	Verdict read_totals(Round &r)
	{
		static_assert(kTopChanged == kTopNewSens + 1, "the two totals counters are read as one piece");
		unsigned long long nnew_chg[2] = {0, 0};
		const unsigned long long *const cnt = d_tops + kTopNewSens;
		const size_t table_bytes = (size_t)3 * V * 4;
		const bool want_vcnt = vcnt.empty() && V && r.work == nullptr;   // the variant slots' draw counts ride on the same synchronisation
		if (r.work == nullptr && r.nshadow == 0) {
			// first round: the offset scans go out behind the totals.  Two short readbacks instead of one long one: first the counters and
			// the special pairs' classes (the pairs every variant of which draws alike leave the host's hands here: unmasked, class 1 --
			// six of seven on the bench batch), with the variant slots' draw counts (1 MB) queued behind them; the host marks the classes
			// and builds its list of the pairs that are left while that copy runs, and the gather for just those pairs brings it in.
			// (One readback of everything had the host walk 20 k pairs, 17 k of them to find they were none of its business, behind a
			// 1.4 MB copy: 0.39 ms of idle GPU per step.)
			const bool classify = want_vcnt && !special.empty();
			if (classify) be.st_special_class(c, d_special, (long long)special.size(), d_mask, d_sp_class);
			enqueue_offset_scans(r);
			int32_t *late = want_vcnt ? mem.d2h_early_late({{nnew_chg, cnt, sizeof nnew_chg}, {h_sp_class.data(), d_sp_class, classify ? special.size() : 0}}, c.rcnt + 3 * P, table_bytes)
			                          : (mem.d2h(nnew_chg, cnt, sizeof nnew_chg), (int32_t *)nullptr);
			if (classify) for (size_t i = 0; i < special.size(); ++i) if (h_sp_class[i] && is_special[i] == 1) is_special[i] = 2;
			build_listed();
			gather_listed();
			if (want_vcnt) {
				mem.d2h_late_done();                      // (the gather's synchronisation has brought the late copy in as well; no list, no gather: waits here)
				// the table is read at random by the walk below: out of the page-locked region the DMA engine has just written every
				// row is a miss to memory (~170 ns per pair measured: 0.45 ms for 2.9 k pairs); one streaming copy (1 MB, ~35 us) puts it in
				// the CPU's caches
				if (!vcnt.resize((size_t)3 * V)) return no_variant_table(r);
				else if (late) memcpy(vcnt.data(), late, table_bytes);
				else mem.d2h(vcnt.data(), c.rcnt + 3 * P, table_bytes);
				build_rows();
			}
			r.gathered = true;
		} else if (want_vcnt) {
			if (!vcnt.resize((size_t)3 * V)) return no_variant_table(r);
			mem.d2h({{nnew_chg, cnt, sizeof nnew_chg}, {vcnt.data(), c.rcnt + 3 * P, table_bytes}});
		}
		else mem.d2h(nnew_chg, cnt, sizeof nnew_chg);
		r.nnew = nnew_chg[0], r.changed = nnew_chg[1];
		return kNextRound;
	}
	Verdict no_variant_table(Round &r) { err = "host allocation failed (variant table)"; r.rc = PSVR_ERR_NOMEM; return kFailed; }

	// Take in what the round found: the window tables of the pairs evaluated with offset shadows, and the newly sensitive pairs.
	void take_in_windows_and_sensitive(Round &r)
	{
		if (r.nshadow > 0) {
			std::vector<int32_t> tot(r.nshadow);
			mem.d2h(tot.data(), d_ctot + (P + V), r.nshadow * 4);
			size_t sh = 0;
			for (Win &w : wins) {
				w.off.clear(), w.tot.clear();
				while (sh < r.sh_src.size() && r.sh_src[sh] == w.pair) w.off.push_back(r.sh_off[sh]), w.tot.push_back(tot[sh]), ++sh;
			}
		}
		if (r.nnew) {
			std::vector<int32_t> add(r.nnew);
			mem.d2h(add.data(), d_slist, r.nnew * 4);
			for (int32_t s : add) {
				for (size_t i = 0; i < special.size(); ++i) if (special[i].pair == s) is_special[i] = 0;
				Win w; w.pair = s, w.eval_off = -1, w.eval_tot = 0;
				wins.push_back(w);
			}
			std::sort(wins.begin(), wins.end(), [](const Win &a, const Win &b) { return a.pair < b.pair; });
			be.scatter_u8(d_mask, add.data(), (long long)add.size(), 1);
			stats.sensitive = (long long)wins.size();
			r.gathered = false;                             // the mask and the lists have changed
		}
	}

	// The masked prefix of the totals in front of every pair, and the random_r offsets: only when a read has sampled at all (expand_seed beyond
	// POS_N_MAX positions) or the streams' start has moved -- otherwise every read stands at the stream's start, where run_init put it, and
	// six scan launches per pass are saved.  (The kernels go out first: the host builds its lists while they run.)
	void enqueue_offset_scans(Round &r)
	{
		r.h_scans = any_h || r.resume;
		be.st_mask_totals(d_ctot, d_mask, P, d_cmask);
		be.st_scan(d_cmask, P, 1, 0, 0, d_noff);
		if (r.h_scans) {
			be.st_scan(c.hcnt, P, 2, 0, hrand_pos[0], d_nhoff);          // (do not depend on the host walk: they run while the host works)
			be.st_scan(c.hcnt, P, 2, 1, hrand_pos[1], d_nhoff);
		}
	}
	// every host-resolved pair, ascending: the special pairs the device has not classified away and the window-resolved ones
	void build_listed()
	{
		w_listed.clear(), l_si.clear();
		size_t wi = 0;                                    // both parts are ascending: merged on the way
		for (size_t i = 0; i < special.size(); ++i) {
			if (is_special[i] != 1) continue;            // (2: resolved on the device; 0: window-resolved, among `wins`)
			for (; wi < wins.size() && wins[wi].pair < special[i].pair; ++wi) w_listed.push_back(wins[wi].pair), l_si.push_back(-1);
			w_listed.push_back(special[i].pair), l_si.push_back((int32_t)i);
		}
		for (; wi < wins.size(); ++wi) w_listed.push_back(wins[wi].pair), l_si.push_back(-1);
		w_pre.resize(w_listed.size()), w_cur_off.resize(w_listed.size()), w_cur_tot.resize(w_listed.size()), w_res.resize(w_listed.size());
		build_rows();                                    // (once the table is there; the first round calls it again when it has arrived)
	}
	// ... their last evaluation (offset, total) and the masked prefix in front of them
	void gather_listed()
	{
		mem.gather_listed(d_noff, c.poff, d_ctot, w_listed.data(), (long long)w_listed.size(), w_pre.data(), w_cur_off.data(), w_cur_tot.data());
	}

	// Resolve the offsets of the host-resolved pairs: the scans, the list, the gather (unless they rode on the totals), the host walk, and
	// its totals back into d_ctot.
	void resolve_offsets(Round &r, bool want_stats)
	{
		if (!r.gathered) {
			enqueue_offset_scans(r);
			build_listed();
			gather_listed();
		}
		if (want_stats && !vcnt.empty() && stats.n_special == 0) count_special_kinds();
		const auto walk_t0 = std::chrono::steady_clock::now();
		walk_offsets();
		stats.walk_pairs += (long long)w_listed.size();
		stats.walk_us += (long long)std::chrono::duration_cast<std::chrono::microseconds>(std::chrono::steady_clock::now() - walk_t0).count();
		if (!w_listed.empty()) mem.scatter_listed_i32(d_ctot, w_res.data(), (long long)w_listed.size());   // same indices as gather_listed
	}
	// (diagnostic) how many of the N pairs draw the same number whatever residues they get / draw nothing but those residues
	void count_special_kinds()
	{
		for (const Special &sp : special) {
			bool cst = true, nomove = true;
			const int32_t *v0 = &vcnt[3 * (sp.vslot - P)];
			for (int v = 0; v < sp.nvar; ++v) {
				const int32_t *vc = &vcnt[3 * (sp.vslot - P + v)];
				if (vc[0] != v0[0] || vc[0] + vc[1] + vc[2] != v0[0] + v0[1] + v0[2]) cst = false;
				if (vc[2] != 0 || vc[0] != sp.n1 || vc[1] != sp.n2) nomove = false;
			}
			stats.n_special++, stats.special_const += cst, stats.special_nomove += nomove;
		}
	}

	// The host walk: O_{s+1} = O_s + D_s(stream content at O_s) over the host-resolved pairs, in input order.  Host arrays only -- this is
	// the definition a walk anywhere else has to agree with.
	//   in:  w_listed[i] the pair, l_si[i] its index in special[] (-1: window-resolved); w_pre[i] the draws of every other pair in front of it
	//        (the masked prefix); w_cur_off[i], w_cur_tot[i] where it was last evaluated and what it drew there; is_special / sp_row0 /
	//        hw_rows the variant tables; wins the window tables; adopted / adopted_at what each special pair carries; the rand() stream
	//   out: w_res[i] the draws of the pair at its offset, w_cur_off[i] that offset (where it must be evaluated next); adopt_pair /
	//        adopt_slot gain the adoptions decided here (adopted / adopted_at follow); wins[].eval_off / eval_tot; stats.window_miss
	void walk_offsets()
	{
		const size_t n = w_listed.size();
		const int32_t *const listed = w_listed.data(), *const cur_tot = w_cur_tot.data();
		const long long *const pre = w_pre.data();
		long long *const cur_off = w_cur_off.data();
		int32_t *const res = w_res.data();
		long long acc = 0;
		size_t wi = 0;
		for (size_t i = 0; i < n; ++i) {
			const int32_t s = listed[i];
			const long long t = grand_pos + pre[i] + acc;
			// (the draws a pair further down will look at: its offset moves by a few entries at most until the walk is there -- each
			// pair's look-up is otherwise a miss to memory, the list being spread over the whole batch's draws)
			if (i + 8 < n) grand.prefetch(grand_pos + pre[i + 8] + acc);
			int32_t D = cur_tot[i];
			const int32_t sidx = l_si[i];
			if (sidx >= 0 && is_special[(size_t)sidx] == 2) {
				// classified while this list was on its way: its total stands whatever its offset (and is part of `pre` for the pairs behind it)
				res[i] = D;
				continue;
			}
			if (sidx >= 0 && is_special[(size_t)sidx] == 1 && sp_row0[(size_t)sidx] >= 0) {
				const size_t si = (size_t)sidx;
				const Special &sp = special[si];
				const HwRow *rows = &hw_rows[(size_t)sp_row0[si]];
				grand.ensure(t + 64);
				int code = 0, sh2 = 0;
				for (int j = 0; j < sp.n1; ++j) code |= (grand.at(t + j) & 3) << sh2, sh2 += 2;
				const int32_t c1 = rows[code].c1;                           // mate 0 does not depend on mate 1's residues
				for (int j = 0; j < sp.n2; ++j) code |= (grand.at(t + c1 + j) & 3) << sh2, sh2 += 2;
				const HwRow vr = rows[code];
				D = vr.d_ok >> 1;
				// The two reads of that variant slot drew nothing but the forced residues: their records ARE this pair's at any offset
				// (adopted below instead of running the pair again where its draws have moved to).  If the slot's pairing stage drew
				// too, the adoption runs the pairing again at the pair's offset (adopt_variant): again whenever the offset moves.
				// (a read of the slot that drew for tied chains as well -- vc > n -- is adopted if its selection, repeated at this offset,
				// leaves the candidates and the counts as they are; the device declines otherwise and the pair runs in full)
				// (the same slot at another offset is adopted again even if nothing of it depends on the offset: the adoption is also what
				// tells mark_dirty that the pair stands where it belongs -- left alone it ran in full, 3.7 k pairs per rebase of the bench batch)
				if ((vr.d_ok & 1) && (adopted[si] != sp.vslot + code || adopted_at[si] != t)) {
					adopted[si] = sp.vslot + code, adopted_at[si] = t;
					adopt_pair.push_back(s), adopt_slot.push_back(sp.vslot + code);
				}
			} else if (sidx < 0) {
				while (wi < wins.size() && wins[wi].pair < s) ++wi;
				if (wi < wins.size() && wins[wi].pair == s) {
					Win &w = wins[wi];
					w.eval_off = cur_off[i], w.eval_tot = cur_tot[i];
					long long best = std::llabs(t - w.eval_off);
					for (size_t k = 0; k < w.off.size(); ++k) {
						long long d = std::llabs(w.off[k] - t);
						if (d < best) best = d, D = w.tot[k];
					}
					if (best != 0) stats.window_miss++;
				}
			}
			res[i] = D, acc += D;
			cur_off[i] = t;                                  // where the pair must be evaluated next
		}
	}

	// End the round on the device: new offsets from the totals, the adoptions, which pairs drew from a stale offset (k_dirty / k_reselect), the
	// pairing-only repeats and their totals -- and the round's one readback: the counters and the flags, into r.
	void end_round(Round &r, bool want_stats)
	{
		be.st_scan(d_ctot, P, 1, 0, grand_pos, d_noff);
		// the totals counters of k_totals_dev below, the lists' counters (in cache lines of their own: kTopFull, kTopPairOnly), the
		// adoptions: one fill (to the buffer's end: a size the runtime does not split)
		be.dzero(d_tops + kTopNewSens, (kTopWords - kTopNewSens) * sizeof(unsigned long long));
		// adoptions: the special pairs the device resolves, and in the same launch the ones this walk decided
		if (!special.empty()) {
			be.st_adopt_auto(c, d_special, (long long)special.size(), d_sp_class, d_mask, d_noff, d_sp_adopted, d_sp_adopted_at, want_stats ? d_tops + kTopAdopted : nullptr,
			                 adopt_pair.data(), adopt_slot.data(), (long long)adopt_pair.size());
			stats.adopted += (long long)adopt_pair.size();
			adopt_pair.clear(), adopt_slot.clear();
		}
		be.st_dirty(c, d_noff, r.h_scans ? d_nhoff : c.hoff, d_work, d_tops + kTopFull, d_workp, d_tops + kTopPairOnly, d_hasn, d_resel, d_tops + kTopTieSeen, P < kReselCap ? P : kReselCap, d_resel4,
		            d_tops + kTopFromWalk);
		// the pairing-only repeats go out at once (the list's length is on the device; the host reads it below for the totals pass)
		be.st_pair_dev(c, d_workp, d_tops + kTopPairOnly);
		r.pair_done = true;
		// ... and their totals, which the next round would take first thing: when nothing else is left to run (the usual case) that round
		// is over with the readback below instead of costing a synchronisation of its own
		be.st_totals_dev(c, d_workp, d_tops + kTopPairOnly, P, d_ctot, d_hprev, d_sens, d_slist, d_tops + kTopNewSens);
		r.pre_tot = true;
		mem.d2h({{r.tops, d_tops + kTopReadFirst, sizeof r.tops}, {r.flags, d_flags, sizeof r.flags}});
		note_sticky_flags(r.flags);
		stats.adopted += (long long)r.top(kTopAdopted);
	}

	// What the round end's readback says: run the batch again with larger arenas or a longer draw window, an error, done, or the next
	// round -- whose list lengths it sets.
	Verdict verdict(Round &r)
	{
		for (int a = 0; a < kArenaFlags; ++a) r.full.flag[a] = r.flags[a];
		if (r.full.any()) return kGrowArenas;
		const int stage_err = r.flags[kFlagErr];
		if (stage_err_is_window(stage_err)) return kExtendWindow;
		if (stage_err) { char b[128]; snprintf(b, sizeof b, "device stage error %d (the reference would abort here)", stage_err); err = b; r.rc = PSVR_ERR_UNSUPPORTED; return kFailed; }
		r.nfull = (long long)r.top(kTopFull), r.npair_only = (long long)r.top(kTopPairOnly), r.nshadow = 0, r.nwalk = (long long)r.top(kTopFromWalk);
		if (r.nfull == 0 && r.npair_only == 0 && r.nwalk == 0) return kDone;
		if (r.nfull == 0 && r.nwalk == 0 && r.top(kTopNewSens) == 0 && r.top(kTopChanged) == 0 && wins.empty()) {
			// the round that only repeats pairing stages: they have run, drew as often as before, nothing is sensitive -- the streams are consistent
			stats.rounds++, stats.pair_only += r.npair_only;
			return kDone;
		}
		if (stats.rounds > 200) { err = "rand()-order resolution did not converge in 200 rounds"; r.rc = PSVR_ERR_UNSUPPORTED; return kFailed; }
		r.work = d_work;
		return kNextRound;
	}

	// Plan the offset windows of the next round: shadow slots around the new offset of every tie-sensitive pair that moves; then the work
	// list is complete: the dirty real pairs, the shadow slots, the pairs that go on from the walk.
	void plan_offset_windows(Round &r)
	{
		r.sh_src.clear(), r.sh_off.clear();
		const long long cap = S - P - V;
		size_t li = 0;
		for (Win &w : wins) {
			while (li < w_listed.size() && w_listed[li] < w.pair) ++li;
			const long long t = li < w_listed.size() && w_listed[li] == w.pair ? w_cur_off[li] : w.eval_off;
			if (t == w.eval_off && !w.off.empty()) continue;            // evaluated there already
			if ((long long)r.sh_src.size() + kWin > cap) break;
			for (int k = -kWin / 2; k < kWin / 2; ++k) {
				if (k == 0 || t + k < grand_pos) continue;
				r.sh_src.push_back(w.pair), r.sh_off.push_back(t + k);
			}
		}
		r.nshadow = (long long)r.sh_src.size();
		if (r.nshadow) {
			be.h2d(d_src + P + V, r.sh_src.data(), r.nshadow * 4);
			be.h2d(c.poff + P + V, r.sh_off.data(), r.nshadow * 8);
			be.copy_hoff_to_shadows(c, P + V, r.nshadow);
			be.append_iota(d_work, r.nfull, P + V, r.nshadow);      // work list: dirty real pairs, then the shadow slots
		}
		if (r.nwalk) be.append_list(d_work, r.nfull + r.nshadow, d_resel4, r.nwalk);   // ... then the pairs that go on from the walk
	}

	// where the three streams stand after this batch (valid after run()/rebase())
	void stream_end(long long out[3])
	{
		out[0] = grand_pos, out[1] = hrand_pos[0], out[2] = hrand_pos[1];
		if (P == 0) return;
		// the last pair's offset + draw count of each stream (one readback: poff[P-1], then hoff / hcnt of the pair are neighbours)
		long long lo, ho[2];
		int32_t lc, hc[2];
		mem.d2h({{&lo, c.poff + (P - 1), 8}, {&lc, d_ctot + (P - 1), 4}, {ho, c.hoff + 2 * (P - 1), 16}, {hc, c.hcnt + 2 * (P - 1), 8}});
		out[0] = lo + lc, out[1] = ho[0] + hc[0], out[2] = ho[1] + hc[1];
	}

	// advance the rand streams past this batch (the reference's generators keep running across batches)
	void commit()
	{
		if (P == 0) return;
		long long e[3];
		stream_end(e);
		grand_pos = e[0], hrand_pos[0] = e[1], hrand_pos[1] = e[2];
		have_run = false;
	}
};

} // namespace psvr
