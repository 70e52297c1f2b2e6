// signal.hip -- psvr_signal_* (include/psvr_engine.h): `panSVR signal -N --signal-device`, the per-pair rules of the name-sorted signal step
// (signal_device.h, held to SignalStep::pair by tests/tools/signal_device_check.cpp) over the records of a psvr_bam_store_t, read where they
// lie through the store's address table.  One run, all on DfwCtx's stream under its mutex (serialised with the store's calls):
//   k_sg_mark      a lane per record: BamReader's rules once more (a store also takes records from the host by the formatter's rule), primary?
//   scan, k_sg_compact   the primary records' indices side by side: pair p = primaries (2p, 2p + 1)
//   k_sg_size      kFqGroup lanes per pair walk sg_pair with the counting sink: state, note, bytes; the first error pair and the first
//                  written pair by atomicMin
//   k_sg_fix       a lane per pair: pairs from the first error pair on get no bytes, the first written pair gets STAT_'s (once per object),
//                  written and declined pairs are counted
//                  -- and how many bytes of records the host will want of the pair: both records of a declined or noted pair and of the error pair
//   scan, k_sg_sum where every pair's text and side records go; the totals for the host, which sizes the two buffers (the run's one wait in the middle)
//   k_sg_side      kFqGroup lanes per such pair copy its two records side by side: the host formats thousands of declined pairs from ONE download
//   k_sg_write     kFqGroup lanes per state-1 pair walk sg_pair again with the storing sink (byte stores: a pair's text starts anywhere)
//   k_sg_hist      a lane per pair in front of the first error pair: BamStat::collect of both records.  len_n is privatised per workgroup in
//                  LDS and flushed once (nearly all reads have one length: global atomics would serialise on one address); isize_n spreads over
//                  hundreds of bins and takes global atomics.
// psvr_signal_window, behind a run: the run's text and the host formatter's text of the state-2 pairs become one window in pair order
// (signal_window_device.h), on the same stream:
//   k_sg_wflag, scan, k_sg_wcut, k_sg_wseg   the segment table from the pair table     k_sg_window   an output tile per workgroup
// psvr_signal_window_add is the same body (sg_window_add) at a base: the run's window goes behind the bytes of a kept window, which grows run
// by run and survives the runs; a workgroup per tile of the whole window that meets the add's bytes, each writing the add's bytes only.
// Bounds: a record is read only after k_sg_mark has vouched for name, CIGAR, bases and qualities; the tag walk (bam_aux_find) stays inside
// the record by its own rules; a pair's text is written into exactly the bytes the size pass counted for it, and a write pass that ends
// anywhere else raises the refusal flag.
#include <hip/hip_runtime.h>
#include <limits.h>
#include <stdlib.h>
#include <algorithm>
#include <memory>
#include <vector>
#include "../../include/psvr_engine.h"
#include "common.h"
#include "scan.h"
#include "bgzf_members.h"
#include "bam_store_run.h"
#include "signal_device.h"
#include "signal_mate_device.h"
#include "copy_aligned_device.h"
#include "signal_run.h"
#include "signal_window_device.h"

namespace psvr {

// ctl[]: 0 primaries, 1 first error pair, 2 first written pair, 3 written (state 1), 4 declined (state 2), 5 refused, 6 text bytes,
// 7 the pair that carries STAT_ (-1: none), 8 the last primary's index behind first_record, 9 side bytes
enum { kSgPrim = 0, kSgFirstErr, kSgFirstWritten, kSgWritten, kSgDeclined, kSgRefused, kSgText, kSgStatPair, kSgLastPrim, kSgSide, kSgCtl = 16 };
static const long long kSgNone = LLONG_MAX;

__global__ __launch_bounds__(256) void k_sg_mark(const uint64_t *addr, long long first, long long m, int32_t *mark, long long *ctl)
{
	const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
	if (i > m) return;
	int32_t v = 0;
	if (i < m) {
		const uint8_t *rec = (const uint8_t *)(uintptr_t)addr[first + i];
		if (!bam_rec_reader_fits(rec) || !bam_rec_name_ends(rec)) ctl[kSgRefused] = 1;
		else v = sg_primary(rec) ? 1 : 0;
	}
	mark[i] = v;
}
__global__ __launch_bounds__(256) void k_sg_compact(const int32_t *mark, const long long *poff, long long m, uint32_t *prim)
{
	const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
	if (i < m && mark[i]) prim[poff[i]] = (uint32_t)i;
}

struct SgGroupIds { long long p; FqGroup g; };
__device__ inline SgGroupIds sg_group()
{
	SgGroupIds G;
	G.p = (long long)blockIdx.x * (256 / kFqGroup) + threadIdx.x / kFqGroup;
	G.g.lane = threadIdx.x % kFqGroup, G.g.shift = (threadIdx.x & 63u) / kFqGroup * kFqGroup;
	return G;
}

// pairs [0, p_max]: those from the run's pair count on (p_max among them) get zero bytes, so the scan runs over p_max + 1 entries
__global__ __launch_bounds__(256) void k_sg_size(psvr_signal_opt_t opt, const uint64_t *addr, long long first, const uint32_t *prim, const long long *poff, long long m, long long p_max,
                                                 uint8_t *state, uint8_t *note, int32_t *bytes, long long *ctl)
{
	const SgGroupIds G = sg_group();
	if (G.p > p_max) return;                                 // (the whole group)
	const long long P = poff[m] / 2;
	if (ctl[kSgRefused] != 0 || G.p >= P) {
		if (G.g.lane == 0) bytes[G.p] = 0, state[G.p] = 0, note[G.p] = 0;
		return;
	}
	const uint8_t *r1 = (const uint8_t *)(uintptr_t)addr[first + prim[2 * G.p]], *r2 = (const uint8_t *)(uintptr_t)addr[first + prim[2 * G.p + 1]];
	int32_t nb = 0;
	uint32_t nt = 0;
	const int st = sg_pair_size(G.g, opt, r1, r2, &nb, &nt);
	if (G.g.lane == 0) {
		state[G.p] = (uint8_t)st, note[G.p] = (uint8_t)nt, bytes[G.p] = nb;
		if (st >= 3) atomicMin((unsigned long long *)&ctl[kSgFirstErr], (unsigned long long)G.p);
		if (st == 1 || st == 2) atomicMin((unsigned long long *)&ctl[kSgFirstWritten], (unsigned long long)G.p);
	}
}

__global__ __launch_bounds__(256) void k_sg_fix(psvr_signal_opt_t opt, int spent, const uint64_t *addr, long long first, const uint32_t *prim, const long long *poff, long long m, long long p_max,
                                                const uint8_t *state, const uint8_t *note, int32_t *bytes, int32_t *sbytes, long long *ctl)
{
	const long long p = (long long)blockIdx.x * 256 + threadIdx.x, P = poff[m] / 2;
	const long long fe = ctl[kSgFirstErr], fw = ctl[kSgFirstWritten];
	const bool live = p < P && ctl[kSgRefused] == 0;
	const int st = live ? state[p] : 0;
	if (live && p >= fe) bytes[p] = 0;
	const bool front = live && p < fe;
	if (p <= p_max) {                                        // the records the host will want: both of a declined or noted pair, and of the error pair
		long long want = 0;
		if (live && (p == fe || (front && (st == 2 || note[p]))))
			for (int k = 0; k < 2; ++k) want += 4 + (long long)bam_u32((const uint8_t *)(uintptr_t)addr[first + prim[2 * p + k]]);
		sbytes[p] = (int32_t)want;                           // (a record the store holds has at most 0x7ffffff0 + 4 bytes; two that long the text's 2 GiB rule has refused)
	}
	if (front && p == fw && !spent) {
		FqGroup g;
		g.lane = 0, g.shift = 0;
		ctl[kSgStatPair] = p;
		if (st == 1) bytes[p] += sg_stat_bytes(g, opt);
	}
	const unsigned long long w = __ballot(front && st == 1), d = __ballot(front && st == 2);
	if ((threadIdx.x & 63u) == 0) {
		if (w) atomicAdd((unsigned long long *)&ctl[kSgWritten], (unsigned long long)__popcll(w));
		if (d) atomicAdd((unsigned long long *)&ctl[kSgDeclined], (unsigned long long)__popcll(d));
	}
}

__global__ void k_sg_sum(const long long *poff, long long m, const uint32_t *prim, const long long *toff, const long long *soff, long long p_max, long long *ctl)
{
	const long long np = poff[m];
	ctl[kSgPrim] = np, ctl[kSgText] = toff[p_max], ctl[kSgSide] = soff[p_max], ctl[kSgLastPrim] = np > 0 ? (long long)prim[np - 1] : -1;
}

__global__ __launch_bounds__(256) void k_sg_write(psvr_signal_opt_t opt, const uint64_t *addr, long long first, const uint32_t *prim, long long n_pairs, const uint8_t *state,
                                                  const int32_t *bytes, const long long *toff, uint8_t *text, long long text_bytes, long long *ctl)
{
	const SgGroupIds G = sg_group();
	if (G.p >= n_pairs || state[G.p] != 1) return;           // (the whole group)
	const long long at = toff[G.p];
	if (at < 0 || bytes[G.p] < 0 || at + bytes[G.p] > text_bytes) { if (G.g.lane == 0) ctl[kSgRefused] = 2; return; }
	const uint8_t *r1 = (const uint8_t *)(uintptr_t)addr[first + prim[2 * G.p]], *r2 = (const uint8_t *)(uintptr_t)addr[first + prim[2 * G.p + 1]];
	BeWrite w;
	w.out = text, w.pos = (uint64_t)at;
	uint32_t nt = 0;
	const int st = sg_pair(G.g, opt, r1, r2, G.p == ctl[kSgStatPair], w, &nt);
	if (G.g.lane == 0 && (st != 1 || w.pos != (uint64_t)(at + bytes[G.p]))) ctl[kSgRefused] = 2;
}

// the two records of every pair the host wants, side by side at soff[p]
__global__ __launch_bounds__(256) void k_sg_side(const uint64_t *addr, long long first, const uint32_t *prim, long long n_pairs, const int32_t *sbytes, const long long *soff, uint8_t *side,
                                                 long long side_bytes, long long *ctl)
{
	const SgGroupIds G = sg_group();
	if (G.p >= n_pairs || sbytes[G.p] == 0) return;          // (the whole group)
	long long at = soff[G.p];
	if (at < 0 || at + sbytes[G.p] > side_bytes) { if (G.g.lane == 0) ctl[kSgRefused] = 2; return; }
	for (int k = 0; k < 2; ++k) {
		const uint8_t *r = (const uint8_t *)(uintptr_t)addr[first + prim[2 * G.p + k]];
		const long long n = 4 + (long long)bam_u32(r);
		if (at + n > soff[G.p] + sbytes[G.p]) { if (G.g.lane == 0) ctl[kSgRefused] = 2; return; }
		for (long long i = G.g.lane; i < n; i += kFqGroup) side[at + i] = r[i];
		at += n;
	}
}

__global__ __launch_bounds__(256) void k_sg_hist(const uint64_t *addr, long long first, const uint32_t *prim, long long n_pairs, unsigned long long *isize_n, unsigned long long *len_n)
{
	__shared__ uint32_t len_l[kSgMaxLen];
	for (int k = threadIdx.x; k < kSgMaxLen; k += 256) len_l[k] = 0;
	__syncthreads();
	for (long long p = (long long)blockIdx.x * 256 + threadIdx.x; p < n_pairs; p += (long long)gridDim.x * 256)
		for (int k = 0; k < 2; ++k) {
			int32_t ib, lb;
			sg_collect_bins((const uint8_t *)(uintptr_t)addr[first + prim[2 * p + k]], &ib, &lb);
			if (ib >= 0) atomicAdd(&isize_n[ib], 1ull);
			if (lb >= 0) atomicAdd(&len_l[lb], 1u);
		}
	__syncthreads();
	for (int k = threadIdx.x; k < kSgMaxLen; k += 256) if (len_l[k]) atomicAdd(&len_n[k], (unsigned long long)len_l[k]);
}

// ---- the window (signal_window_device.h) ----
__global__ __launch_bounds__(256) void k_sg_wflag(const uint8_t *state, long long n_front, int32_t *flag)
{
	const long long p = (long long)blockIdx.x * 256 + threadIdx.x;
	if (p <= n_front) flag[p] = sw_flag(p, n_front, state);
}
__global__ __launch_bounds__(256) void k_sg_wcut(const int32_t *flag, const long long *rank, const long long *toff, long long n_front, long long n_host, long long *cut, long long *ctl)
{
	const long long p = (long long)blockIdx.x * 256 + threadIdx.x;
	if (p >= n_front || !flag[p]) return;
	if (rank[p] < 0 || rank[p] >= n_host) { ctl[kSgRefused] = 3; return; }
	cut[rank[p]] = toff[p];
}
__global__ __launch_bounds__(256) void k_sg_wseg(const long long *cut, const long long *host_off, long long n_host, long long text_bytes, long long host_bytes, long long base, SwSeg *seg, long long *ctl)
{
	const long long k = (long long)blockIdx.x * 256 + threadIdx.x;
	if (k > 2 * n_host) return;
	const SwSeg s = sw_segment_add(k, n_host, (const int64_t *)cut, (const int64_t *)host_off, text_bytes, base);
	// (inside its source and inside the add's bytes of the window, whatever the tables say: the tiles trust the table)
	if (s.len < 0 || s.off < 0 || s.off + s.len > (s.src ? host_bytes : text_bytes) || s.out < base || s.out + s.len > base + text_bytes + host_bytes) ctl[kSgRefused] = 3;
	seg[k] = s;
}
// a workgroup per tile of the whole window that meets the add's bytes [base, end): first_tile is the one base lies in
__global__ __launch_bounds__(256) void k_sg_window(const SwSeg *seg, long long n_seg, const uint8_t *text, const uint8_t *host, uint8_t *out, long long base, long long end, long long first_tile,
                                                   const long long *ctl)
{
	if (ctl[kSgRefused] != 0) return;                        // (the whole launch)
	sw_tile_add(first_tile + blockIdx.x, seg, n_seg, text, host, out, base, end, threadIdx.x, 256);
}

static int sg_no_device() { return set_error(PSVR_ERR_DEVICE, "no HIP device visible: the engine has no CPU path"); }
static int sg_run_pairs(psvr_signal *sg, const uint64_t *addr, const psvr_bam_store *st, DfwCtx &c, int64_t first_record, const long long *poff, long long p_max, const char *who, psvr_signal_info_t *info, long long text_limit = 0);

} // namespace psvr

using namespace psvr;

extern "C" int psvr_signal_create(int device, const psvr_signal_opt_t *opt, psvr_signal_t **out)
{
	if (!out || !opt) return set_error(PSVR_ERR_ARG, "psvr_signal_create: null argument");
	*out = nullptr;
	if (psvr_device_count() <= 0) return sg_no_device();
	DfwCtx &c = dfw_ctx();
	std::lock_guard<std::mutex> lk(c.mu);
	if (int rc = dfw_bind(c, device)) return rc;
	psvr_signal *sg = new psvr_signal;
	sg->device = device, sg->opt = *opt;
	hipError_t e = sg->ctl.alloc(kSgCtl * 8);
	if (e == hipSuccess) e = sg->isize_n.alloc((size_t)kSgMaxIsize * 8);
	if (e == hipSuccess) e = sg->len_n.alloc((size_t)kSgMaxLen * 8);
	if (e == hipSuccess) e = hipHostMalloc((void **)&sg->h_ctl, kSgCtl * 8, hipHostMallocDefault);
	if (e == hipSuccess) e = hipMemsetAsync(sg->isize_n.p, 0, (size_t)kSgMaxIsize * 8, c.stream);
	if (e == hipSuccess) e = hipMemsetAsync(sg->len_n.p, 0, (size_t)kSgMaxLen * 8, c.stream);
	if (e == hipSuccess) e = hipStreamSynchronize(c.stream);
	if (e != hipSuccess) {
		(void)hipGetLastError();
		if (sg->h_ctl) (void)hipHostFree(sg->h_ctl);
		delete sg;
		return set_error(PSVR_ERR_DEVICE, "psvr_signal_create: %s", hipGetErrorString(e));
	}
	*out = sg;
	return PSVR_OK;
}

extern "C" void psvr_signal_destroy(psvr_signal_t *sg)
{
	if (!sg) return;
	DfwCtx &c = dfw_ctx();
	std::lock_guard<std::mutex> lk(c.mu);
	(void)hipSetDevice(sg->device);
	if (c.stream) (void)hipStreamSynchronize(c.stream);
	if (sg->h_ctl) (void)hipHostFree(sg->h_ctl);
	if (sg->h_mctl) (void)hipHostFree(sg->h_mctl);
	delete sg;
}

extern "C" int psvr_signal_run(psvr_signal_t *sg, psvr_bam_store_t *st, int64_t first_record, int32_t finish, psvr_signal_info_t *info)
{
	(void)finish;                                            // (a lone last primary record is dropped by the host loop as well: the caller's to leave)
	if (psvr_device_count() <= 0) return sg_no_device();
	if (!sg || !st || !info) return set_error(PSVR_ERR_ARG, "psvr_signal_run: null argument");
	if (st->device != sg->device) return set_error(PSVR_ERR_ARG, "psvr_signal_run: the store is on device %d, the signal object on device %d", st->device, sg->device);
	DfwCtx &c = dfw_ctx();
	std::lock_guard<std::mutex> lk(c.mu);
	if (int rc = dfw_bind(c, sg->device)) return rc;
	if (int rc = store_refresh(st, c, true)) return rc;
	sg->run_begins();
	if (st->ordered) return set_error(PSVR_ERR_ARG, "psvr_signal_run: the store has been ordered: the pairs are those of its append order");
	if (first_record < 0 || first_record > st->n_rec) return set_error(PSVR_ERR_ARG, "psvr_signal_run: first record %lld of %lld", (long long)first_record, st->n_rec);
	const long long m = st->n_rec - first_record, p_max = m / 2;
	if (m >= (1ll << 31)) return set_error(PSVR_ERR_UNSUPPORTED, "psvr_signal_run: %lld records in one run (at most 2^31 - 1)", m);
	const long long n_scan = std::max(m, p_max) + 1;
	if (sg->mark.ensure((size_t)(m + 1) * 4) || sg->poff.ensure((size_t)(m + 1) * 8) || sg->prim.ensure((size_t)(m + 1) * 4) || sg->state.ensure((size_t)p_max + 1) ||
	    sg->note.ensure((size_t)p_max + 1) || sg->bytes.ensure((size_t)(p_max + 1) * 4) || sg->toff.ensure((size_t)(p_max + 1) * 8) || sg->sbytes.ensure((size_t)(p_max + 1) * 4) ||
	    sg->soff.ensure((size_t)(p_max + 1) * 8) || sg->tmp.ensure(scan_tmp_bytes(2, n_scan))) {
		(void)hipGetLastError();
		return set_error(PSVR_ERR_NOMEM, "psvr_signal_run: device allocation failed for the tables of %lld records (%zu bytes)", m, (size_t)m * 24);
	}
	long long *ctl = sg->ctl.as<long long>();
	long long *h = sg->h_ctl;
	for (int k = 0; k < kSgCtl; ++k) h[k] = 0;
	h[kSgFirstErr] = h[kSgFirstWritten] = kSgNone, h[kSgStatPair] = -1, h[kSgLastPrim] = -1;
	const uint64_t *addr = (const uint64_t *)st->addr.p;
	const long long *poff = (const long long *)sg->poff.p;
	const unsigned g_rec = (unsigned)((m + 256) / 256);
	StreamDrain drain{c.stream};
	PSVR_HIP(hipMemcpyAsync(ctl, h, kSgCtl * 8, hipMemcpyHostToDevice, c.stream));
	hipLaunchKernelGGL(k_sg_mark, dim3(g_rec), dim3(256), 0, c.stream, addr, (long long)first_record, m, sg->mark.as<int32_t>(), ctl);
	ScanSet X = {};
	X.cnt[0] = sg->mark.as<int32_t>(), X.out[0] = sg->poff.as<long long>(), X.stride[0] = 1;
	scan_launch(X, 1, m + 1, sg->tmp.as<long long>(), c.stream);
	hipLaunchKernelGGL(k_sg_compact, dim3(g_rec), dim3(256), 0, c.stream, (const int32_t *)sg->mark.p, poff, m, sg->prim.as<uint32_t>());
	drain.armed = false;
	if (int rc = sg_run_pairs(sg, addr, st, c, first_record, poff + m, p_max, "psvr_signal_run", info)) return rc;
	info->consumed = (sg->h_ctl[kSgPrim] & 1) ? first_record + sg->h_ctl[kSgLastPrim] : st->n_rec;
	return PSVR_OK;
}

namespace psvr {
// The pairs (prim[2p], prim[2p + 1]) of sg->prim, *n_listed / 2 of them (a device cell; p_max is the host's upper bound): size, fix, side,
// write and hist, behind whatever the caller has queued on the stream (the ctl upload among it).  Fills info but for `consumed`.
static int sg_run_pairs(psvr_signal *sg, const uint64_t *addr, const psvr_bam_store *st, DfwCtx &c, int64_t first_record, const long long *poff, long long p_max, const char *who, psvr_signal_info_t *info, long long text_limit)
{
	const long long m = 0;                                   // (the kernels read the count at poff[m])
	long long *ctl = sg->ctl.as<long long>();
	long long *h = sg->h_ctl;
	const uint32_t *prim = (const uint32_t *)sg->prim.p;
	const unsigned g_grp = (unsigned)((p_max + 1 + 256 / kFqGroup - 1) / (256 / kFqGroup)), g_pair = (unsigned)((p_max + 256) / 256);
	StreamDrain drain{c.stream};
	hipLaunchKernelGGL(k_sg_size, dim3(g_grp), dim3(256), 0, c.stream, sg->opt, addr, (long long)first_record, prim, poff, m, p_max, sg->state.as<uint8_t>(), sg->note.as<uint8_t>(),
	                   sg->bytes.as<int32_t>(), ctl);
	hipLaunchKernelGGL(k_sg_fix, dim3(g_pair), dim3(256), 0, c.stream, sg->opt, sg->spent ? 1 : 0, addr, (long long)first_record, prim, poff, m, p_max, (const uint8_t *)sg->state.p,
	                   (const uint8_t *)sg->note.p, sg->bytes.as<int32_t>(), sg->sbytes.as<int32_t>(), ctl);
	ScanSet Y = {};
	Y.cnt[0] = sg->bytes.as<int32_t>(), Y.out[0] = sg->toff.as<long long>(), Y.stride[0] = 1;
	Y.cnt[1] = sg->sbytes.as<int32_t>(), Y.out[1] = sg->soff.as<long long>(), Y.stride[1] = 1;
	scan_launch(Y, 2, p_max + 1, sg->tmp.as<long long>(), c.stream);
	hipLaunchKernelGGL(k_sg_sum, dim3(1), dim3(1), 0, c.stream, poff, m, prim, (const long long *)sg->toff.p, (const long long *)sg->soff.p, p_max, ctl);
	PSVR_HIP(hipGetLastError());
	PSVR_HIP(hipMemcpyAsync(h, ctl, kSgCtl * 8, hipMemcpyDeviceToHost, c.stream));
	PSVR_HIP(hipStreamSynchronize(c.stream));
	if (h[kSgRefused]) return set_error(PSVR_ERR_IO, "%s: malformed BAM record among the records behind record %lld of the store (BamReader's rules refuse it)", who, (long long)first_record);
	const long long n_prim = h[kSgPrim], P = n_prim / 2, first_err = h[kSgFirstErr] == kSgNone ? -1 : h[kSgFirstErr], text_bytes = h[kSgText];
	const long long n_front = first_err >= 0 ? first_err : P;
	const long long side_bytes = h[kSgSide];
	// (text_limit: the caller comes back with fewer pairs; nothing has been written, counted or spent)
	if (text_limit > 0 && text_bytes > text_limit) return set_error(PSVR_ERR_OVERFLOW, "%s: the text of %lld pairs has %lld bytes (at most %lld)", who, n_prim / 2, text_bytes, text_limit);
	if (n_prim < 0 || n_prim > 2 * p_max + 1 || text_bytes < 0 || side_bytes < 0) return set_error(PSVR_ERR_DEVICE, "%s: the run's counts are inconsistent (%lld listed records, room for %lld pairs, %lld text bytes)", who, n_prim, p_max, text_bytes);
	if (sg->text.ensure((size_t)text_bytes) || sg->side.ensure((size_t)side_bytes)) { (void)hipGetLastError(); return set_error(PSVR_ERR_NOMEM, "%s: device allocation failed for %lld bytes of text and %lld of records", who, text_bytes, side_bytes); }
	if (side_bytes > 0) {                                        // (the error pair is behind the front: P pairs are looked at)
		const unsigned gs = (unsigned)((P + 256 / kFqGroup - 1) / (256 / kFqGroup));
		hipLaunchKernelGGL(k_sg_side, dim3(gs), dim3(256), 0, c.stream, addr, (long long)first_record, prim, P, (const int32_t *)sg->sbytes.p, (const long long *)sg->soff.p, sg->side.as<uint8_t>(),
		                   side_bytes, ctl);
		PSVR_HIP(hipGetLastError());
		PSVR_HIP(hipMemcpyAsync(h + kSgRefused, ctl + kSgRefused, 8, hipMemcpyDeviceToHost, c.stream));
	}
	if (n_front > 0) {
		const unsigned gw = (unsigned)((n_front + 256 / kFqGroup - 1) / (256 / kFqGroup)), gh = (unsigned)std::min<long long>((n_front + 255) / 256, 1024);
		hipLaunchKernelGGL(k_sg_write, dim3(gw), dim3(256), 0, c.stream, sg->opt, addr, (long long)first_record, prim, n_front, (const uint8_t *)sg->state.p, (const int32_t *)sg->bytes.p,
		                   (const long long *)sg->toff.p, sg->text.as<uint8_t>(), text_bytes, ctl);
		hipLaunchKernelGGL(k_sg_hist, dim3(gh), dim3(256), 0, c.stream, addr, (long long)first_record, prim, n_front, sg->isize_n.as<unsigned long long>(), sg->len_n.as<unsigned long long>());
		PSVR_HIP(hipGetLastError());
		PSVR_HIP(hipMemcpyAsync(h + kSgRefused, ctl + kSgRefused, 8, hipMemcpyDeviceToHost, c.stream));
	}
	drain.armed = false;
	PSVR_HIP(hipStreamSynchronize(c.stream));
	if (h[kSgRefused]) return set_error(PSVR_ERR_DEVICE, "%s: the write pass did not end where the size pass said (the text is not used)", who);
	if (h[kSgStatPair] >= 0) sg->spent = true;
	sg->valid = true, sg->store = st, sg->store_generation = st ? st->generation : 0, sg->first_record = first_record, sg->pairs = P, sg->text_bytes = text_bytes, sg->side_bytes = side_bytes;
	sg->n_front = n_front, sg->written = h[kSgWritten], sg->declined = h[kSgDeclined];
	info->side_bytes = side_bytes;
	info->pairs = P, info->written = h[kSgWritten], info->declined = h[kSgDeclined], info->first_error = first_err, info->text_bytes = text_bytes;
	return PSVR_OK;
}
} // namespace psvr


extern "C" int psvr_signal_text(psvr_signal_t *sg, void *text, int64_t cap)
{
	if (psvr_device_count() <= 0) return sg_no_device();
	if (!sg || cap < 0 || (cap > 0 && !text)) return set_error(PSVR_ERR_ARG, "psvr_signal_text: bad argument");
	if (!sg->valid) return set_error(PSVR_ERR_ARG, "psvr_signal_text: no run");
	if (cap < sg->text_bytes) return set_error(PSVR_ERR_OVERFLOW, "psvr_signal_text: the run's text has %lld bytes, the buffer has %lld", sg->text_bytes, (long long)cap);
	if (sg->text_bytes == 0) return PSVR_OK;
	DfwCtx &c = dfw_ctx();
	std::lock_guard<std::mutex> lk(c.mu);
	if (int rc = dfw_bind(c, sg->device)) return rc;
	PSVR_HIP(hipMemcpyAsync(text, sg->text.p, (size_t)sg->text_bytes, hipMemcpyDeviceToHost, c.stream));
	PSVR_HIP(hipStreamSynchronize(c.stream));
	return PSVR_OK;
}

namespace psvr {
// The one body of psvr_signal_window and psvr_signal_window_add: the last run's window written at `base` of sg->window.  keep: the add -- base
// is what the kept window holds (0 behind a restart), and nothing of the object changes unless the call succeeds; otherwise base is 0 and the
// window is the run's, which dies with it.
static int sg_window_add(psvr_signal *sg, const void *host_text, int64_t host_bytes, const int64_t *host_off, int64_t n_host, bool keep, bool restart, const char *who, psvr_signal_window_info_t *info)
{
	if (psvr_device_count() <= 0) return sg_no_device();
	if (!sg || !info || (host_bytes > 0 && !host_text)) return set_error(PSVR_ERR_ARG, "%s: null argument", who);
	if (!sg->valid) return set_error(PSVR_ERR_ARG, "%s: no run", who);
	if (const char *bad = sw_args_bad(host_bytes, host_off, n_host, sg->declined))
		return set_error(PSVR_ERR_ARG, "%s: %s (%lld host pairs with %lld bytes, the run has %lld)", who, bad, (long long)n_host, (long long)host_bytes, sg->declined);
	const bool grows = keep && !restart && sg->win_kept && sg->win_valid;
	const long long base = grows ? sg->win_bytes : 0, base_pairs = grows ? sg->win_pairs : 0, base_host = grows ? sg->win_host_pairs : 0;
	const long long n_front = sg->n_front, text_bytes = sg->text_bytes, n_out = text_bytes + host_bytes, n_seg = 2 * n_host + 1, end = base + n_out;
	if (end >= (1ll << 32)) return set_error(PSVR_ERR_UNSUPPORTED, "%s: a window of %lld bytes (at most 2^32 - 1: the parser's offsets)", who, end);
	DfwCtx &c = dfw_ctx();
	std::lock_guard<std::mutex> lk(c.mu);
	if (int rc = dfw_bind(c, sg->device)) return rc;
	if (!keep) sg->win_valid = false, sg->win_kept = false;
	// (the window buffer grows geometrically into a new allocation; the old one is the window until the copy has succeeded)
	DevBuf grown;
	const size_t need = (size_t)end + 16;
	if (sg->wflag.ensure((size_t)(n_front + 1) * 4) || sg->wrank.ensure((size_t)(n_front + 1) * 8) || sg->wcut.ensure((size_t)(n_host + 1) * 8) || sg->wseg.ensure((size_t)n_seg * sizeof(SwSeg)) ||
	    sg->whost.ensure((size_t)host_bytes + 16) || sg->whoff.ensure((size_t)(n_host + 1) * 8) || sg->tmp.ensure(scan_tmp_bytes(1, n_front + 1)) ||
	    (!sg->text.p && sg->text.ensure(16)) ||                  // (a run without text: the kernel still gets a pointer; a run's text is never reallocated here)
	    (need > sg->window.bytes && grown.alloc(std::max(need + need / 4, keep ? std::min(2 * sg->window.bytes, ((size_t)1 << 32) + 16) : (size_t)0)))) {
		(void)hipGetLastError();
		return set_error(PSVR_ERR_NOMEM, "%s: device allocation failed for a window of %lld bytes and %lld segments", who, end, n_seg);
	}
	if (grown.p) {
		const long long held = keep && sg->win_kept && sg->win_valid ? sg->win_bytes : 0;   // (behind a restart too: a failed add leaves them readable)
		if (held > 0) {
			StreamDrain drain{c.stream};
			PSVR_HIP(hipMemcpyAsync(grown.p, sg->window.p, (size_t)held, hipMemcpyDeviceToDevice, c.stream));
			drain.armed = false;
			PSVR_HIP(hipStreamSynchronize(c.stream));
		}
		std::swap(grown.p, sg->window.p), std::swap(grown.bytes, sg->window.bytes);
	}
	long long *ctl = sg->ctl.as<long long>();
	long long *h = sg->h_ctl;
	h[kSgRefused] = 0;
	StreamDrain drain{c.stream};
	PSVR_HIP(hipMemcpyAsync(ctl + kSgRefused, h + kSgRefused, 8, hipMemcpyHostToDevice, c.stream));
	if (n_host) {
		if (host_bytes) PSVR_HIP(hipMemcpyAsync(sg->whost.p, host_text, (size_t)host_bytes, hipMemcpyHostToDevice, c.stream));
		PSVR_HIP(hipMemcpyAsync(sg->whoff.p, host_off, (size_t)(n_host + 1) * 8, hipMemcpyHostToDevice, c.stream));
		hipLaunchKernelGGL(k_sg_wflag, dim3((unsigned)((n_front + 256) / 256)), dim3(256), 0, c.stream, (const uint8_t *)sg->state.p, n_front, sg->wflag.as<int32_t>());
		ScanSet X = {};
		X.cnt[0] = sg->wflag.as<int32_t>(), X.out[0] = sg->wrank.as<long long>(), X.stride[0] = 1;
		scan_launch(X, 1, n_front + 1, sg->tmp.as<long long>(), c.stream);
		hipLaunchKernelGGL(k_sg_wcut, dim3((unsigned)((n_front + 255) / 256)), dim3(256), 0, c.stream, (const int32_t *)sg->wflag.p, (const long long *)sg->wrank.p, (const long long *)sg->toff.p, n_front,
		                   (long long)n_host, sg->wcut.as<long long>(), ctl);
	}
	hipLaunchKernelGGL(k_sg_wseg, dim3((unsigned)((n_seg + 255) / 256)), dim3(256), 0, c.stream, (const long long *)sg->wcut.p, (const long long *)sg->whoff.p, (long long)n_host, text_bytes,
	                   (long long)host_bytes, base, sg->wseg.as<SwSeg>(), ctl);
	if (n_out)
		hipLaunchKernelGGL(k_sg_window, dim3((unsigned)sw_add_tiles(base, n_out)), dim3(256), 0, c.stream, (const SwSeg *)sg->wseg.p, n_seg, (const uint8_t *)sg->text.p, (const uint8_t *)sg->whost.p,
		                   sg->window.as<uint8_t>(), base, end, (long long)sw_add_first_tile(base), (const long long *)ctl);
	PSVR_HIP(hipGetLastError());
	PSVR_HIP(hipMemcpyAsync(h + kSgRefused, ctl + kSgRefused, 8, hipMemcpyDeviceToHost, c.stream));
	drain.armed = false;
	PSVR_HIP(hipStreamSynchronize(c.stream));
	// (a refused table: no tile has written, so a kept window's bytes [0, base) and its counts stand)
	if (h[kSgRefused]) return set_error(PSVR_ERR_DEVICE, "%s: the segment table does not fit the run's text and the host text (the window is not used)", who);
	sg->win_valid = true, sg->win_kept = keep, sg->win_bytes = end, sg->win_pairs = base_pairs + sg->written + sg->declined, sg->win_host_pairs = base_host + n_host;
	info->n_bytes = sg->win_bytes, info->n_pairs = sg->win_pairs, info->n_host_pairs = sg->win_host_pairs;
	return PSVR_OK;
}
} // namespace psvr

extern "C" int psvr_signal_window(psvr_signal_t *sg, const void *host_text, int64_t host_bytes, const int64_t *host_off, int64_t n_host, psvr_signal_window_info_t *info)
{
	return sg_window_add(sg, host_text, host_bytes, host_off, n_host, false, true, "psvr_signal_window", info);
}

extern "C" int psvr_signal_window_add(psvr_signal_t *sg, const void *host_text, int64_t host_bytes, const int64_t *host_off, int64_t n_host, int32_t restart, psvr_signal_window_info_t *info)
{
	return sg_window_add(sg, host_text, host_bytes, host_off, n_host, true, restart != 0, "psvr_signal_window_add", info);
}

extern "C" int psvr_signal_window_text(psvr_signal_t *sg, void *dst, int64_t first, int64_t n)
{
	if (psvr_device_count() <= 0) return sg_no_device();
	if (!sg || first < 0 || n < 0 || (n > 0 && !dst)) return set_error(PSVR_ERR_ARG, "psvr_signal_window_text: bad argument");
	if (!sg->win_valid) return set_error(PSVR_ERR_ARG, "psvr_signal_window_text: no window");
	if (first > sg->win_bytes || n > sg->win_bytes - first) return set_error(PSVR_ERR_ARG, "psvr_signal_window_text: bytes [%lld, %lld) of a window of %lld", (long long)first, (long long)(first + n), sg->win_bytes);
	if (n == 0) return PSVR_OK;
	DfwCtx &c = dfw_ctx();
	std::lock_guard<std::mutex> lk(c.mu);
	if (int rc = dfw_bind(c, sg->device)) return rc;
	PSVR_HIP(hipMemcpyAsync(dst, sg->window.as<uint8_t>() + first, (size_t)n, hipMemcpyDefault, c.stream));
	PSVR_HIP(hipStreamSynchronize(c.stream));
	return PSVR_OK;
}

extern "C" int psvr_signal_pairs(psvr_signal_t *sg, psvr_signal_pair_t *pairs, int64_t cap)
{
	if (psvr_device_count() <= 0) return sg_no_device();
	if (!sg || cap < 0 || (cap > 0 && !pairs)) return set_error(PSVR_ERR_ARG, "psvr_signal_pairs: bad argument");
	if (!sg->valid) return set_error(PSVR_ERR_ARG, "psvr_signal_pairs: no run");
	const long long P = sg->pairs;
	if (cap < P) return set_error(PSVR_ERR_OVERFLOW, "psvr_signal_pairs: the run has %lld pairs, the table has room for %lld", P, (long long)cap);
	if (P == 0) return PSVR_OK;
	DfwCtx &c = dfw_ctx();
	std::lock_guard<std::mutex> lk(c.mu);
	if (int rc = dfw_bind(c, sg->device)) return rc;
	std::vector<uint8_t> state((size_t)P), note((size_t)P);
	std::vector<int32_t> bytes((size_t)P);
	std::vector<long long> toff((size_t)P), soff((size_t)P);
	std::vector<int32_t> sbytes((size_t)P);
	std::vector<uint32_t> prim((size_t)(2 * P));
	{
		StreamDrain drain{c.stream};                             // (it waits: the vectors are whole below, and never outlived by a copy)
		PSVR_HIP(hipMemcpyAsync(state.data(), sg->state.p, (size_t)P, hipMemcpyDeviceToHost, c.stream));
		PSVR_HIP(hipMemcpyAsync(note.data(), sg->note.p, (size_t)P, hipMemcpyDeviceToHost, c.stream));
		PSVR_HIP(hipMemcpyAsync(bytes.data(), sg->bytes.p, (size_t)P * 4, hipMemcpyDeviceToHost, c.stream));
		PSVR_HIP(hipMemcpyAsync(toff.data(), sg->toff.p, (size_t)P * 8, hipMemcpyDeviceToHost, c.stream));
		PSVR_HIP(hipMemcpyAsync(prim.data(), sg->prim.p, (size_t)P * 8, hipMemcpyDeviceToHost, c.stream));
		PSVR_HIP(hipMemcpyAsync(soff.data(), sg->soff.p, (size_t)P * 8, hipMemcpyDeviceToHost, c.stream));
		PSVR_HIP(hipMemcpyAsync(sbytes.data(), sg->sbytes.p, (size_t)P * 4, hipMemcpyDeviceToHost, c.stream));
	}
	for (long long p = 0; p < P; ++p) {
		psvr_signal_pair_t &o = pairs[p];
		o.text_off = toff[(size_t)p], o.rec1 = sg->first_record + prim[(size_t)(2 * p)], o.rec2 = sg->first_record + prim[(size_t)(2 * p + 1)];
		o.side_off = sbytes[(size_t)p] ? soff[(size_t)p] : -1;
		o.bytes = bytes[(size_t)p], o.state = state[(size_t)p], o.note = note[(size_t)p], o.pad = 0;
	}
	return PSVR_OK;
}

extern "C" int psvr_signal_side(psvr_signal_t *sg, void *bytes, int64_t cap)
{
	if (psvr_device_count() <= 0) return sg_no_device();
	if (!sg || cap < 0 || (cap > 0 && !bytes)) return set_error(PSVR_ERR_ARG, "psvr_signal_side: bad argument");
	if (!sg->valid) return set_error(PSVR_ERR_ARG, "psvr_signal_side: no run");
	if (cap < sg->side_bytes) return set_error(PSVR_ERR_OVERFLOW, "psvr_signal_side: the run's side records have %lld bytes, the buffer has %lld", sg->side_bytes, (long long)cap);
	if (sg->side_bytes == 0) return PSVR_OK;
	DfwCtx &c = dfw_ctx();
	std::lock_guard<std::mutex> lk(c.mu);
	if (int rc = dfw_bind(c, sg->device)) return rc;
	PSVR_HIP(hipMemcpyAsync(bytes, sg->side.p, (size_t)sg->side_bytes, hipMemcpyDeviceToHost, c.stream));
	PSVR_HIP(hipStreamSynchronize(c.stream));
	return PSVR_OK;
}

extern "C" int psvr_signal_pair_records(psvr_signal_t *sg, psvr_bam_store_t *st, int64_t pair, void *bytes, int64_t cap, int64_t *n_bytes)
{
	if (psvr_device_count() <= 0) return sg_no_device();
	if (!sg || !st || !n_bytes || cap < 0 || (cap > 0 && !bytes)) return set_error(PSVR_ERR_ARG, "psvr_signal_pair_records: bad argument");
	*n_bytes = 0;
	DfwCtx &c = dfw_ctx();
	std::lock_guard<std::mutex> lk(c.mu);
	if (int rc = dfw_bind(c, sg->device)) return rc;
	if (int rc = store_refresh(st, c, true)) return rc;
	if (!sg->valid || sg->store != st || sg->store_generation != st->generation) return set_error(PSVR_ERR_ARG, "psvr_signal_pair_records: the store is not the last run's, or records were dropped since");
	if (pair < 0 || pair >= sg->pairs) return set_error(PSVR_ERR_ARG, "psvr_signal_pair_records: pair %lld of %lld", (long long)pair, sg->pairs);
	uint32_t prim[2];
	uint64_t addr[2];
	psvr_bam_rec_meta_t meta[2];
	StreamDrain drain{c.stream};
	PSVR_HIP(hipMemcpyAsync(prim, sg->prim.as<uint32_t>() + 2 * pair, 8, hipMemcpyDeviceToHost, c.stream));
	PSVR_HIP(hipStreamSynchronize(c.stream));
	for (int k = 0; k < 2; ++k) {
		const long long r = sg->first_record + prim[k];
		if (r < 0 || r >= st->n_rec) return set_error(PSVR_ERR_DEVICE, "psvr_signal_pair_records: record %lld of %lld", r, st->n_rec);
		PSVR_HIP(hipMemcpyAsync(&addr[k], st->addr.as<uint64_t>() + r, 8, hipMemcpyDeviceToHost, c.stream));
		PSVR_HIP(hipMemcpyAsync(&meta[k], st->meta.as<psvr_bam_rec_meta_t>() + r, sizeof(psvr_bam_rec_meta_t), hipMemcpyDeviceToHost, c.stream));
	}
	PSVR_HIP(hipStreamSynchronize(c.stream));
	*n_bytes = (int64_t)meta[0].len + meta[1].len;
	if (cap < *n_bytes) return set_error(PSVR_ERR_OVERFLOW, "psvr_signal_pair_records: the pair's records have %lld bytes, the buffer has %lld", (long long)*n_bytes, (long long)cap);
	PSVR_HIP(hipMemcpyAsync(bytes, (const void *)(uintptr_t)addr[0], meta[0].len, hipMemcpyDeviceToHost, c.stream));
	PSVR_HIP(hipMemcpyAsync((uint8_t *)bytes + meta[0].len, (const void *)(uintptr_t)addr[1], meta[1].len, hipMemcpyDeviceToHost, c.stream));
	drain.armed = false;
	PSVR_HIP(hipStreamSynchronize(c.stream));
	return PSVR_OK;
}

extern "C" int psvr_signal_stats(psvr_signal_t *sg, uint64_t *isize_n, uint64_t *len_n)
{
	if (psvr_device_count() <= 0) return sg_no_device();
	if (!sg || !isize_n || !len_n) return set_error(PSVR_ERR_ARG, "psvr_signal_stats: null argument");
	DfwCtx &c = dfw_ctx();
	std::lock_guard<std::mutex> lk(c.mu);
	if (int rc = dfw_bind(c, sg->device)) return rc;
	StreamDrain drain{c.stream};
	PSVR_HIP(hipMemcpyAsync(isize_n, sg->isize_n.p, (size_t)kSgMaxIsize * 8, hipMemcpyDeviceToHost, c.stream));
	PSVR_HIP(hipMemcpyAsync(len_n, sg->len_n.p, (size_t)kSgMaxLen * 8, hipMemcpyDeviceToHost, c.stream));
	drain.armed = false;
	PSVR_HIP(hipStreamSynchronize(c.stream));
	return PSVR_OK;
}

// ---- psvr_signal_run_pos: the blocks of the position-sorted mode (signal_mate_device.h) -------------------------------------------------------
//   k_sg_mark, scan, k_sg_compact   the primaries behind first_record (as psvr_signal_run)     k_sm_end   the record that ends the block
//   k_sm_fill      a lane per record: pos / mpos / flag / tid == mtid side by side, filled once; the positions the rules do not serve
//   k_sm_cand      kFqGroup lanes per record: cand(i) over the 4-byte streams, names compared where the records lie; in-degrees by atomicAdd
//   k_sm_settle    a lane per record: the clean components' links, plain stores      k_sm_class   who is for the replay, whose turn failed
//   scan, k_sm_dlist, k_sm_replay   the replay list in index order; ONE lane walks it (launched only when the list is not empty)
//   k_sm_flags, scan x3, k_sm_lists   pair list (into prim, for the passes of psvr_signal_run), the unmated records' indices and lengths, notes
//   scan, k_sm_left   the unmated records side by side
// Bounds: every index a kernel follows (cand, mate, list entries) is checked against n where it is read from memory another kernel wrote.
namespace psvr {

// mctl[]: 0 the first primary that ends the block, 1 positions not served (1 decreasing, 2 index overflow), 2 2 x pairs, 3 unmated, 4 failed turns,
// 5 the block's last record behind first_record, 6 unmated bytes, 7 an index out of range
enum { kSmEnd = 0, kSmBad, kSmPairs2, kSmLeft, kSmFail, kSmLastRec, kSmLeftBytes, kSmRange, kSmCtl = 8 };

struct SmRec {
	const uint64_t *addr;
	long long first;
	const uint32_t *bprim;
	__device__ const uint8_t *operator()(int32_t i) const { return (const uint8_t *)(uintptr_t)addr[first + bprim[i]]; }
};

__global__ __launch_bounds__(256) void k_sm_end(SmRec R, const long long *n_prim, long long limit, long long span, long long *mctl)
{
	const long long j = (long long)blockIdx.x * 256 + threadIdx.x;
	if (j < 1 || j >= *n_prim || j >= limit) return;
	const uint8_t *r0 = R(0), *r = R((int32_t)j);
	if (sm_ends_block(bam_i32(r0 + 4), bam_i32(r0 + 8), bam_i32(r + 4), bam_i32(r + 8), span)) atomicMin((unsigned long long *)&mctl[kSmEnd], (unsigned long long)j);
}
__global__ __launch_bounds__(256) void k_sm_fill(SmRec R, long long n, int32_t *pos, int32_t *mpos, uint32_t *flag, int32_t *same, long long *mctl)
{
	const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
	if (i >= n) return;
	const uint8_t *r0 = R(0), *r = R((int32_t)i);
	const int32_t tid = bam_i32(r + 4), p = bam_i32(r + 8);
	pos[i] = p, mpos[i] = bam_i32(r + 28), flag[i] = bam_u16(r + 18), same[i] = tid == bam_i32(r + 24);
	const int bad = sm_pos_bad(n, i, bam_i32(r0 + 4), bam_i32(r0 + 8), i > 0 ? bam_i32(R((int32_t)i - 1) + 8) : 0, tid, p);
	if (bad) atomicMin((unsigned long long *)&mctl[kSmBad], (unsigned long long)bad);   // (the smaller code wins, as in the host build)
}
__global__ __launch_bounds__(256) void k_sm_cand(SmRec R, long long n, const int32_t *pos, const int32_t *mpos, const int32_t *same, int32_t *cand, int32_t *indeg)
{
	const SgGroupIds G = sg_group();
	if (G.p >= n) return;                                    // (the whole group)
	const int32_t c = sm_cand(G.g, (int32_t)n, bam_i32(R(0) + 4), pos, mpos, same, R, (int32_t)G.p);
	if (G.g.lane == 0) {
		cand[G.p] = c;
		if (c >= 0) atomicAdd(&indeg[c], 1);
	}
}
__global__ __launch_bounds__(256) void k_sm_settle(long long n, const int32_t *cand, const int32_t *indeg, int32_t *mate, long long *mctl)
{
	const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
	if (i >= n) return;
	const int32_t m = cand[i];
	if (m >= n || m == i) { mctl[kSmRange] = 1; return; }
	if (m >= 0 && (cand[m] >= n || cand[m] == m)) return;    // (that lane reports it)
	if (sm_clean(cand, indeg, (int32_t)i)) mate[i] = m, mate[m] = (int32_t)i;
}
__global__ __launch_bounds__(256) void k_sm_class(long long n, const int32_t *cand, const int32_t *indeg, const int32_t *mate, int32_t *dirty, int32_t *fail)
{
	const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
	if (i > n) return;
	int32_t f = 0;
	const bool d = i < n && sm_dirty(cand, indeg, mate, (int32_t)i, &f);
	dirty[i] = d, fail[i] = f;
}
__global__ __launch_bounds__(256) void k_sm_dlist(long long n, const int32_t *dirty, const long long *doff, int32_t *dlist)
{
	const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
	if (i < n && dirty[i] && doff[i] >= 0 && doff[i] < n) dlist[doff[i]] = (int32_t)i;
}
__global__ void k_sm_replay(const int32_t *dlist, long long n_list, const int32_t *cand, int32_t *mate, int32_t *fail) { sm_replay(dlist, n_list, cand, mate, fail); }
__global__ __launch_bounds__(256) void k_sm_flags(long long n, const int32_t *mate, const uint32_t *flag, int32_t *pflag, int32_t *lflag, int32_t *lbytes)
{
	const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
	if (i > n) return;
	pflag[i] = i < n && sm_is_pair(n, mate, flag, i), lflag[i] = i < n && mate[i] == kSmFree, lbytes[i] = 0;
}
__global__ __launch_bounds__(256) void k_sm_lists(SmRec R, long long n, const int32_t *pos, const int32_t *mate, const int32_t *pflag, const int32_t *lflag, const int32_t *fail, const long long *pfoff,
                                                  const long long *lfoff, const long long *ffoff, long long fail_base, long long note_cap, uint32_t *prim, uint32_t *llist, int32_t *lbytes,
                                                  psvr_signal_mate_note_t *notes, long long *mctl)
{
	const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
	if (i > n) return;
	if (i == n) {
		mctl[kSmPairs2] = 2 * pfoff[n], mctl[kSmLeft] = lfoff[n], mctl[kSmFail] = ffoff[n], mctl[kSmLastRec] = n > 0 ? (long long)R.bprim[n - 1] : -1;
		return;
	}
	if (pflag[i]) {
		const int32_t m = mate[i];
		const long long r = pfoff[i];
		if (m < 0 || m >= n || r < 0 || r >= n) mctl[kSmRange] = 1;
		else prim[2 * r] = R.bprim[i], prim[2 * r + 1] = R.bprim[m];
	}
	if (lflag[i]) {
		const long long r = lfoff[i];
		if (r < 0 || r >= n) mctl[kSmRange] = 1;
		else llist[r] = R.bprim[i], lbytes[r] = (int32_t)(4 + bam_u32(R((int32_t)i)));   // (a record the store holds has at most 0x7ffffff0 + 4 bytes)
	}
	if (fail[i]) {
		const long long turn = fail_base + ffoff[i] + 1, slot = sm_note_slot(fail_base, turn);
		if (slot >= note_cap) mctl[kSmRange] = 1;
		else if (slot >= 0) {
			const uint8_t *r = R((int32_t)i);
			psvr_signal_mate_note_t &o = notes[slot];
			o.number = turn, o.index = (int32_t)i, o.block = (int32_t)n, o.tid = bam_i32(r + 4), o.pos = pos[i];
			uint32_t k = 0;
			for (; k < r[12] && k < 255 && r[kBamRecHead + k]; ++k) o.name[k] = (char)r[kBamRecHead + k];
			for (; k < 256; ++k) o.name[k] = 0;
		}
	}
}
__global__ void k_sm_left_sum(const long long *lboff, long long n, long long *mctl) { mctl[kSmLeftBytes] = lboff[n]; }
__global__ __launch_bounds__(256) void k_sm_left(const uint64_t *addr, long long first, const uint32_t *llist, long long n_left, const int32_t *lbytes, const long long *lboff, uint8_t *left,
                                                 long long left_bytes, uint64_t *laddr, long long *mctl)
{
	const SgGroupIds G = sg_group();
	if (G.p >= n_left) return;                               // (the whole group)
	const uint8_t *r = (const uint8_t *)(uintptr_t)addr[first + llist[G.p]];
	const long long at = lboff[G.p], len = lbytes[G.p];
	if (at < 0 || len != 4 + (long long)bam_u32(r) || at + len > left_bytes) { if (G.g.lane == 0) mctl[kSmRange] = 1; return; }
	copy_aligned_lanes(r, left + at, len, G.g.lane, kFqGroup);
	if (G.g.lane == 0) laddr[G.p] = (uint64_t)(uintptr_t)(left + at);   // the left store's table: where the copy lies
}

// ---- psvr_signal_run_left: the by-name pass over the left store ----
//   sort_order_names_device   the host comparator's order: name by strcmp, records with 0x40 first, append order
//   k_sl_head      kFqGroup lanes per rank: does a run of equal names begin here?     scan, k_sl_start   where every run begins
//   k_sl_flags     a lane per rank: an even place in its run with a partner behind it is a pair; an even last place of a run that is not the
//                  last run is a pairing-error step     scan x2, k_sl_pairs   the pair list and, per pair, the error steps in front of it
struct SlRec {
	const uint64_t *laddr;
	const uint32_t *ord;                                     // nullptr: the append order stands
	__device__ uint32_t at(long long j) const { return ord ? ord[j] : (uint32_t)j; }
	__device__ const uint8_t *operator()(long long j) const { return (const uint8_t *)(uintptr_t)laddr[at(j)]; }
};
__global__ __launch_bounds__(256) void k_sl_head(SlRec R, long long n, int32_t *head)
{
	const SgGroupIds G = sg_group();
	if (G.p > n) return;                                     // (the whole group)
	bool h = G.p == 0 && n > 0;
	if (G.p > 0 && G.p < n) {
		if (R.at(G.p) >= n || R.at(G.p - 1) >= n) return;    // (an order is a permutation: always)
		h = !sg_same_name(G.g, R(G.p - 1), R(G.p));
	}
	if (G.g.lane == 0) head[G.p] = h;
}
__global__ __launch_bounds__(256) void k_sl_start(long long n, const int32_t *head, const long long *hoff, int32_t *start)
{
	const long long j = (long long)blockIdx.x * 256 + threadIdx.x;
	if (j < n && head[j] && hoff[j] >= 0 && hoff[j] < n) start[hoff[j]] = (int32_t)j;
}
__global__ __launch_bounds__(256) void k_sl_flags(long long n, const int32_t *head, const long long *hoff, const int32_t *start, int32_t *pflag, int32_t *eflag)
{
	const long long j = (long long)blockIdx.x * 256 + threadIdx.x;
	if (j > n) return;
	int32_t p = 0, e = 0;
	if (j < n) {
		const long long run = hoff[j] + head[j] - 1;         // (head[0] is 1: never negative)
		const long long off = run >= 0 && run < n ? j - start[run] : 1;   // (an odd place is neither)
		const bool partner = j + 1 < n && !head[j + 1];
		p = sm_left_is_pair(off, partner), e = sm_left_is_error(off, partner, j + 1 == n);
	}
	pflag[j] = p, eflag[j] = e;
}
__global__ __launch_bounds__(256) void k_sl_pairs(SlRec R, long long n, const int32_t *pflag, const long long *pfoff, const long long *efoff, uint32_t *lprim, long long *lerr, long long *lctl)
{
	const long long j = (long long)blockIdx.x * 256 + threadIdx.x;
	if (j > n) return;
	if (j == n) { lctl[0] = pfoff[n], lctl[1] = efoff[n]; return; }
	if (!pflag[j]) return;
	const long long r = pfoff[j];
	if (r < 0 || 2 * r + 1 >= n || R.at(j) >= n || R.at(j + 1) >= n) { lctl[2] = 1; return; }
	lprim[2 * r] = R.at(j), lprim[2 * r + 1] = R.at(j + 1), lerr[r] = efoff[j];
}

} // namespace psvr

extern "C" int psvr_signal_run_pos(psvr_signal_t *sg, psvr_bam_store_t *st, int64_t first_record, int32_t finish, const psvr_signal_pos_opt_t *opt, psvr_signal_info_t *info,
                                   psvr_signal_pos_info_t *pi)
{
	if (psvr_device_count() <= 0) return sg_no_device();
	if (!sg || !st || !info || !pi) return set_error(PSVR_ERR_ARG, "psvr_signal_run_pos: null argument");
	if (st->device != sg->device) return set_error(PSVR_ERR_ARG, "psvr_signal_run_pos: the store is on device %d, the signal object on device %d", st->device, sg->device);
	const long long limit = opt && opt->block_records ? opt->block_records : kSmRecords, span = opt && opt->block_span ? opt->block_span : kSmSpan;
	if (limit < 2 || limit >= (1ll << 31) - 1 || span < 0) return set_error(PSVR_ERR_ARG, "psvr_signal_run_pos: a block of %lld records and a span of %lld", limit, span);
	DfwCtx &c = dfw_ctx();
	std::lock_guard<std::mutex> lk(c.mu);
	if (int rc = dfw_bind(c, sg->device)) return rc;
	if (int rc = store_refresh(st, c, true)) return rc;
	sg->run_begins(), sg->pos_valid = false;
	if (st->ordered) return set_error(PSVR_ERR_ARG, "psvr_signal_run_pos: the store has been ordered: the blocks are those of its append order");
	if (first_record < 0 || first_record > st->n_rec) return set_error(PSVR_ERR_ARG, "psvr_signal_run_pos: first record %lld of %lld", (long long)first_record, st->n_rec);
	const long long m = st->n_rec - first_record;
	if (m >= (1ll << 31) - 1) return set_error(PSVR_ERR_UNSUPPORTED, "psvr_signal_run_pos: %lld records behind the first (at most 2^31 - 2)", m);
	*pi = psvr_signal_pos_info_t{0, 0, 0, 0, 0, sg->mate_failed, 0, 0};
	*info = psvr_signal_info_t{0, 0, 0, -1, 0, 0, 0};
	if (!sg->h_mctl && hipHostMalloc((void **)&sg->h_mctl, kSmCtl * 8, hipHostMallocDefault) != hipSuccess) { (void)hipGetLastError(); sg->h_mctl = nullptr; return set_error(PSVR_ERR_NOMEM, "psvr_signal_run_pos: no page-locked memory"); }
	if (sg->mark.ensure((size_t)(m + 1) * 4) || sg->poff.ensure((size_t)(m + 1) * 8) || sg->prim.ensure((size_t)(2 * m + 4) * 4) || sg->tmp.ensure(scan_tmp_bytes(3, m + 2)) || sg->mctl.ensure(kSmCtl * 8)) {
		(void)hipGetLastError();
		return set_error(PSVR_ERR_NOMEM, "psvr_signal_run_pos: device allocation failed for the tables of %lld records", m);
	}
	long long *ctl = sg->ctl.as<long long>(), *mctl = sg->mctl.as<long long>();
	long long *h = sg->h_ctl, *hm = sg->h_mctl;
	for (int k = 0; k < kSgCtl; ++k) h[k] = 0;
	h[kSgFirstErr] = h[kSgFirstWritten] = kSgNone, h[kSgStatPair] = -1, h[kSgLastPrim] = -1;
	for (int k = 0; k < kSmCtl; ++k) hm[k] = 0;
	hm[kSmEnd] = hm[kSmBad] = kSgNone;
	const uint64_t *addr = (const uint64_t *)st->addr.p;
	const long long *poff = (const long long *)sg->poff.p;
	const unsigned g_rec = (unsigned)((m + 256) / 256);
	StreamDrain drain{c.stream};
	// the primaries behind first_record and the record that ends the block
	PSVR_HIP(hipMemcpyAsync(ctl, h, kSgCtl * 8, hipMemcpyHostToDevice, c.stream));
	PSVR_HIP(hipMemcpyAsync(mctl, hm, kSmCtl * 8, hipMemcpyHostToDevice, c.stream));
	hipLaunchKernelGGL(k_sg_mark, dim3(g_rec), dim3(256), 0, c.stream, addr, (long long)first_record, m, sg->mark.as<int32_t>(), ctl);
	ScanSet X = {};
	X.cnt[0] = sg->mark.as<int32_t>(), X.out[0] = sg->poff.as<long long>(), X.stride[0] = 1;
	scan_launch(X, 1, m + 1, sg->tmp.as<long long>(), c.stream);
	hipLaunchKernelGGL(k_sg_compact, dim3(g_rec), dim3(256), 0, c.stream, (const int32_t *)sg->mark.p, poff, m, sg->prim.as<uint32_t>());
	SmRec R0{addr, (long long)first_record, (const uint32_t *)sg->prim.p};
	hipLaunchKernelGGL(k_sm_end, dim3((unsigned)((std::min(m, limit) + 256) / 256)), dim3(256), 0, c.stream, R0, poff + m, limit, span, mctl);
	PSVR_HIP(hipGetLastError());
	long long avail = 0;
	PSVR_HIP(hipMemcpyAsync(&avail, poff + m, 8, hipMemcpyDeviceToHost, c.stream));
	PSVR_HIP(hipMemcpyAsync(hm, mctl, kSmCtl * 8, hipMemcpyDeviceToHost, c.stream));
	PSVR_HIP(hipMemcpyAsync(h + kSgRefused, ctl + kSgRefused, 8, hipMemcpyDeviceToHost, c.stream));
	PSVR_HIP(hipStreamSynchronize(c.stream));
	if (h[kSgRefused]) return set_error(PSVR_ERR_IO, "psvr_signal_run_pos: malformed BAM record among records [%lld, %lld) of the store (BamReader's rules refuse it)", (long long)first_record, st->n_rec);
	if (avail < 0 || avail > m) return set_error(PSVR_ERR_DEVICE, "psvr_signal_run_pos: %lld primaries of %lld records", avail, m);
	bool complete = false;
	const long long end = hm[kSmEnd] == kSgNone ? avail : hm[kSmEnd];
	const long long n = sm_block_size(avail, end, limit, finish != 0, &complete);
	if (!complete) return PSVR_OK;
	pi->complete = 1, pi->primaries = n;
	if (n < 2) {                                             // (the input has ended: the host loop drops a single record)
		sg->valid = true, sg->pos_valid = true, sg->store = st, sg->store_generation = st->generation, sg->first_record = first_record;
		sg->pairs = sg->text_bytes = sg->side_bytes = sg->n_front = sg->written = sg->declined = sg->left_bytes = sg->n_notes = 0;
		pi->consumed = info->consumed = st->n_rec;
		return PSVR_OK;
	}
	const long long p_max = n, note_cap = n / 1000 + 2;   // (records without flag 0x80 on both sides of a link make two pairs: up to n - 1)
	const size_t n4 = (size_t)(n + 1) * 4, n8 = (size_t)(n + 1) * 8;
	if (sg->bprim.ensure(n4) || sg->spos.ensure(n4) || sg->smpos.ensure(n4) || sg->sflag.ensure(n4) || sg->ssame.ensure(n4) || sg->cand.ensure(n4) || sg->indeg.ensure(n4) || sg->mate.ensure(n4) ||
	    sg->dirty.ensure(n4) || sg->fail.ensure(n4) || sg->doff.ensure(n8) || sg->dlist.ensure(n4) || sg->pflag.ensure(n4) || sg->lflag.ensure(n4) || sg->pfoff.ensure(n8) || sg->lfoff.ensure(n8) ||
	    sg->ffoff.ensure(n8) || sg->lbytes.ensure(n4) || sg->lboff.ensure(n8) || sg->notes.ensure((size_t)note_cap * sizeof(psvr_signal_mate_note_t)) || sg->state.ensure((size_t)p_max + 1) ||
	    sg->note.ensure((size_t)p_max + 1) || sg->bytes.ensure((size_t)(p_max + 1) * 4) || sg->toff.ensure((size_t)(p_max + 1) * 8) || sg->sbytes.ensure((size_t)(p_max + 1) * 4) ||
	    sg->soff.ensure((size_t)(p_max + 1) * 8)) {
		(void)hipGetLastError();
		return set_error(PSVR_ERR_NOMEM, "psvr_signal_run_pos: device allocation failed for the tables of a block of %lld records", n);
	}
	const unsigned g_n = (unsigned)((n + 256) / 256), g_ngrp = (unsigned)((n + 256 / kFqGroup - 1) / (256 / kFqGroup));
	int32_t *pos = sg->spos.as<int32_t>(), *mpos = sg->smpos.as<int32_t>(), *same = sg->ssame.as<int32_t>(), *cand = sg->cand.as<int32_t>(), *indeg = sg->indeg.as<int32_t>(), *mate = sg->mate.as<int32_t>();
	uint32_t *flag = sg->sflag.as<uint32_t>();
	PSVR_HIP(hipMemcpyAsync(sg->bprim.p, sg->prim.p, (size_t)n * 4, hipMemcpyDeviceToDevice, c.stream));
	PSVR_HIP(hipMemsetAsync(indeg, 0, n4, c.stream));
	PSVR_HIP(hipMemsetAsync(mate, 0xff, n4, c.stream));
	SmRec R{addr, (long long)first_record, (const uint32_t *)sg->bprim.p};
	hipLaunchKernelGGL(k_sm_fill, dim3(g_n), dim3(256), 0, c.stream, R, n, pos, mpos, flag, same, mctl);
	hipLaunchKernelGGL(k_sm_cand, dim3(g_ngrp), dim3(256), 0, c.stream, R, n, (const int32_t *)pos, (const int32_t *)mpos, (const int32_t *)same, cand, indeg);
	hipLaunchKernelGGL(k_sm_settle, dim3(g_n), dim3(256), 0, c.stream, n, (const int32_t *)cand, (const int32_t *)indeg, mate, mctl);
	hipLaunchKernelGGL(k_sm_class, dim3(g_n), dim3(256), 0, c.stream, n, (const int32_t *)cand, (const int32_t *)indeg, (const int32_t *)mate, sg->dirty.as<int32_t>(), sg->fail.as<int32_t>());
	ScanSet D = {};
	D.cnt[0] = sg->dirty.as<int32_t>(), D.out[0] = sg->doff.as<long long>(), D.stride[0] = 1;
	scan_launch(D, 1, n + 1, sg->tmp.as<long long>(), c.stream);
	hipLaunchKernelGGL(k_sm_dlist, dim3(g_n), dim3(256), 0, c.stream, n, (const int32_t *)sg->dirty.p, (const long long *)sg->doff.p, sg->dlist.as<int32_t>());
	PSVR_HIP(hipGetLastError());
	long long n_dirty = 0;
	PSVR_HIP(hipMemcpyAsync(&n_dirty, sg->doff.as<long long>() + n, 8, hipMemcpyDeviceToHost, c.stream));
	PSVR_HIP(hipMemcpyAsync(hm, mctl, kSmCtl * 8, hipMemcpyDeviceToHost, c.stream));
	PSVR_HIP(hipStreamSynchronize(c.stream));
	if (hm[kSmBad] == kSgNone) hm[kSmBad] = 0;
	if (hm[kSmBad] == 1) return set_error(PSVR_ERR_UNSUPPORTED, "psvr_signal_run_pos: positions decrease inside a block of %lld records (is the input sorted by position?)", n);
	if (hm[kSmBad]) return set_error(PSVR_ERR_UNSUPPORTED, "psvr_signal_run_pos: a position of the block overflows the host loop's position index");
	if (hm[kSmRange] || n_dirty < 0 || n_dirty > n) return set_error(PSVR_ERR_DEVICE, "psvr_signal_run_pos: the candidate table of a block of %lld records is inconsistent", n);
	if (n_dirty > 0) hipLaunchKernelGGL(k_sm_replay, dim3(1), dim3(1), 0, c.stream, (const int32_t *)sg->dlist.p, n_dirty, (const int32_t *)cand, mate, sg->fail.as<int32_t>());
	hipLaunchKernelGGL(k_sm_flags, dim3(g_n), dim3(256), 0, c.stream, n, (const int32_t *)mate, (const uint32_t *)flag, sg->pflag.as<int32_t>(), sg->lflag.as<int32_t>(), sg->lbytes.as<int32_t>());
	ScanSet F = {};
	F.cnt[0] = sg->pflag.as<int32_t>(), F.out[0] = sg->pfoff.as<long long>(), F.stride[0] = 1;
	F.cnt[1] = sg->lflag.as<int32_t>(), F.out[1] = sg->lfoff.as<long long>(), F.stride[1] = 1;
	F.cnt[2] = sg->fail.as<int32_t>(), F.out[2] = sg->ffoff.as<long long>(), F.stride[2] = 1;
	scan_launch(F, 3, n + 1, sg->tmp.as<long long>(), c.stream);
	hipLaunchKernelGGL(k_sm_lists, dim3(g_n), dim3(256), 0, c.stream, R, n, (const int32_t *)pos, (const int32_t *)mate, (const int32_t *)sg->pflag.p, (const int32_t *)sg->lflag.p,
	                   (const int32_t *)sg->fail.p, (const long long *)sg->pfoff.p, (const long long *)sg->lfoff.p, (const long long *)sg->ffoff.p, sg->mate_failed, note_cap, sg->prim.as<uint32_t>(),
	                   sg->dlist.as<uint32_t>(), sg->lbytes.as<int32_t>(), sg->notes.as<psvr_signal_mate_note_t>(), mctl);
	ScanSet L = {};
	L.cnt[0] = sg->lbytes.as<int32_t>(), L.out[0] = sg->lboff.as<long long>(), L.stride[0] = 1;
	scan_launch(L, 1, n + 1, sg->tmp.as<long long>(), c.stream);
	hipLaunchKernelGGL(k_sm_left_sum, dim3(1), dim3(1), 0, c.stream, (const long long *)sg->lboff.p, n, mctl);
	PSVR_HIP(hipGetLastError());
	PSVR_HIP(hipMemcpyAsync(hm, mctl, kSmCtl * 8, hipMemcpyDeviceToHost, c.stream));
	PSVR_HIP(hipStreamSynchronize(c.stream));
	const long long n_left = hm[kSmLeft], left_bytes = hm[kSmLeftBytes], fails = hm[kSmFail];
	if (hm[kSmRange] || hm[kSmPairs2] < 0 || hm[kSmPairs2] / 2 > p_max || n_left < 0 || n_left > n || left_bytes < 0 || fails < 0 || fails > n || hm[kSmLastRec] < 0 || hm[kSmLastRec] >= m)
		return set_error(PSVR_ERR_DEVICE, "psvr_signal_run_pos: the lists of a block of %lld records are inconsistent", n);
	// the left store takes them, device to device: a chunk per block, and the table grows by doubling
	std::unique_ptr<DevBuf> chunk(new DevBuf);
	// (whole 8-byte words: k_name_chunk loads the aligned words a name touches)
	if (chunk->alloc(((size_t)left_bytes + 7) & ~(size_t)7)) { (void)hipGetLastError(); return set_error(PSVR_ERR_NOMEM, "psvr_signal_run_pos: device allocation failed for %lld bytes of unmated records", left_bytes); }
	if (sg->left_n + n_left > sg->laddr_cap) {
		const long long cap = std::max(2 * sg->laddr_cap, sg->left_n + n_left + 1024);
		DevBuf grown;
		if (grown.alloc((size_t)cap * 8)) { (void)hipGetLastError(); return set_error(PSVR_ERR_NOMEM, "psvr_signal_run_pos: device allocation failed for the table of %lld unmated records", cap); }
		if (sg->left_n) PSVR_HIP(hipMemcpyAsync(grown.p, sg->laddr.p, (size_t)sg->left_n * 8, hipMemcpyDeviceToDevice, c.stream));
		PSVR_HIP(hipStreamSynchronize(c.stream));
		std::swap(sg->laddr.p, grown.p), std::swap(sg->laddr.bytes, grown.bytes);
		sg->laddr_cap = cap;
	}
	if (n_left > 0) {
		hipLaunchKernelGGL(k_sm_left, dim3((unsigned)((n_left + 256 / kFqGroup - 1) / (256 / kFqGroup))), dim3(256), 0, c.stream, addr, (long long)first_record, (const uint32_t *)sg->dlist.p, n_left,
		                   (const int32_t *)sg->lbytes.p, (const long long *)sg->lboff.p, chunk->as<uint8_t>(), left_bytes, sg->laddr.as<uint64_t>() + sg->left_n, mctl);
		PSVR_HIP(hipGetLastError());
		PSVR_HIP(hipMemcpyAsync(hm + kSmRange, mctl + kSmRange, 8, hipMemcpyDeviceToHost, c.stream));
		PSVR_HIP(hipStreamSynchronize(c.stream));
		if (hm[kSmRange]) return set_error(PSVR_ERR_DEVICE, "psvr_signal_run_pos: the unmated records do not lie where their lengths said");
	}
	drain.armed = false;
	// the pairs through the passes of psvr_signal_run (the ctl upload lies in front of them on the stream)
	if (int rc = sg_run_pairs(sg, addr, st, c, first_record, (const long long *)(mctl + kSmPairs2), p_max, "psvr_signal_run_pos", info)) return rc;
	sg->left_chunks.push_back(std::move(chunk)), sg->left_n += n_left, sg->left_ordered = false, sg->left_valid = false;   // (a block whose pair passes failed keeps its unmated records out)
	sg->pos_valid = true, sg->left_bytes = left_bytes, sg->n_notes = sm_note_count(sg->mate_failed, fails), sg->mate_failed += fails;
	pi->consumed = info->consumed = first_record + hm[kSmLastRec] + 1;
	pi->unmated = n_left, pi->left_bytes = left_bytes, pi->mate_failed = sg->mate_failed, pi->notes = sg->n_notes, pi->replayed = n_dirty;
	return PSVR_OK;
}

extern "C" int psvr_signal_mate_notes(psvr_signal_t *sg, psvr_signal_mate_note_t *notes, int64_t cap)
{
	if (psvr_device_count() <= 0) return sg_no_device();
	if (!sg || cap < 0 || (cap > 0 && !notes)) return set_error(PSVR_ERR_ARG, "psvr_signal_mate_notes: bad argument");
	if (!sg->valid || !sg->pos_valid) return set_error(PSVR_ERR_ARG, "psvr_signal_mate_notes: no block");
	if (cap < sg->n_notes) return set_error(PSVR_ERR_OVERFLOW, "psvr_signal_mate_notes: the block has %lld notes, the table has room for %lld", sg->n_notes, (long long)cap);
	if (sg->n_notes == 0) return PSVR_OK;
	DfwCtx &c = dfw_ctx();
	std::lock_guard<std::mutex> lk(c.mu);
	if (int rc = dfw_bind(c, sg->device)) return rc;
	PSVR_HIP(hipMemcpyAsync(notes, sg->notes.p, (size_t)sg->n_notes * sizeof(psvr_signal_mate_note_t), hipMemcpyDeviceToHost, c.stream));
	PSVR_HIP(hipStreamSynchronize(c.stream));
	return PSVR_OK;
}

extern "C" int psvr_signal_left(psvr_signal_t *sg, void *bytes, int64_t cap)
{
	if (psvr_device_count() <= 0) return sg_no_device();
	if (!sg || cap < 0 || (cap > 0 && !bytes)) return set_error(PSVR_ERR_ARG, "psvr_signal_left: bad argument");
	if (!sg->valid || !sg->pos_valid) return set_error(PSVR_ERR_ARG, "psvr_signal_left: no block");
	if (cap < sg->left_bytes) return set_error(PSVR_ERR_OVERFLOW, "psvr_signal_left: the block's unmated records have %lld bytes, the buffer has %lld", sg->left_bytes, (long long)cap);
	if (sg->left_bytes == 0 || sg->left_chunks.empty()) return PSVR_OK;
	DfwCtx &c = dfw_ctx();
	std::lock_guard<std::mutex> lk(c.mu);
	if (int rc = dfw_bind(c, sg->device)) return rc;
	PSVR_HIP(hipMemcpyAsync(bytes, sg->left_chunks.back()->p, (size_t)sg->left_bytes, hipMemcpyDeviceToHost, c.stream));
	PSVR_HIP(hipStreamSynchronize(c.stream));
	return PSVR_OK;
}

extern "C" int psvr_signal_run_left(psvr_signal_t *sg, int64_t first_pair, int64_t max_pairs, psvr_signal_info_t *info, psvr_signal_left_info_t *li)
{
	if (psvr_device_count() <= 0) return sg_no_device();
	if (!sg || !info || !li || first_pair < 0 || max_pairs < 1) return set_error(PSVR_ERR_ARG, "psvr_signal_run_left: bad argument");
	DfwCtx &c = dfw_ctx();
	std::lock_guard<std::mutex> lk(c.mu);
	if (int rc = dfw_bind(c, sg->device)) return rc;
	sg->run_begins(), sg->pos_valid = false, sg->left_valid = false;
	const long long n = sg->left_n;
	if (n >= (1ll << 31) - 1) return set_error(PSVR_ERR_UNSUPPORTED, "psvr_signal_run_left: %lld unmated records (at most 2^31 - 2)", n);
	if (n & 1) return set_error(PSVR_ERR_UNSUPPORTED, "psvr_signal_run_left: an odd number of records found no mate (%lld): the host loop ends there", n);
	*info = psvr_signal_info_t{0, 0, 0, -1, 0, 0, 0};
	long long *hm = sg->h_mctl;
	if (!hm && n > 0) return set_error(PSVR_ERR_ARG, "psvr_signal_run_left: no block has been run");
	if (!sg->left_ordered && n > 0) {
		const size_t n4 = (size_t)(n + 1) * 4, n8 = (size_t)(n + 1) * 8;
		if (sg->lkeys.ensure(n8) || sg->dirty.ensure(n4) || sg->doff.ensure(n8) || sg->dlist.ensure(n4) || sg->pflag.ensure(n4) || sg->lflag.ensure(n4) || sg->pfoff.ensure(n8) || sg->lfoff.ensure(n8) ||
		    sg->lprim.ensure(n4 + 8) || sg->lerr.ensure(n8) || sg->lctl.ensure(32) || sg->tmp.ensure(scan_tmp_bytes(2, n + 1))) {
			(void)hipGetLastError();
			return set_error(PSVR_ERR_NOMEM, "psvr_signal_run_left: device allocation failed for the tables of %lld unmated records", n);
		}
		const NameSrc src = {(const uint64_t *)sg->laddr.p, nullptr, 0, nullptr, nullptr, 1};
		const uint32_t *ord = nullptr;
		if (int rc = sort_order_names_device(c.stream, n, src, sg->lkeys.as<uint64_t>(), sg->lN, sg->lS, sg->lhist, &ord, "psvr_signal_run_left")) return rc;
		const SlRec R{(const uint64_t *)sg->laddr.p, ord};
		const unsigned g_n = (unsigned)((n + 256) / 256), g_grp = (unsigned)((n + 1 + 256 / kFqGroup - 1) / (256 / kFqGroup));
		int32_t *head = sg->dirty.as<int32_t>(), *start = sg->dlist.as<int32_t>();
		StreamDrain drain{c.stream};
		PSVR_HIP(hipMemsetAsync(sg->lctl.p, 0, 32, c.stream));
		PSVR_HIP(hipMemsetAsync(head, 0, n4, c.stream));
		hipLaunchKernelGGL(k_sl_head, dim3(g_grp), dim3(256), 0, c.stream, R, n, head);
		ScanSet H = {};
		H.cnt[0] = head, H.out[0] = sg->doff.as<long long>(), H.stride[0] = 1;
		scan_launch(H, 1, n + 1, sg->tmp.as<long long>(), c.stream);
		hipLaunchKernelGGL(k_sl_start, dim3(g_n), dim3(256), 0, c.stream, n, (const int32_t *)head, (const long long *)sg->doff.p, start);
		hipLaunchKernelGGL(k_sl_flags, dim3(g_n), dim3(256), 0, c.stream, n, (const int32_t *)head, (const long long *)sg->doff.p, (const int32_t *)start, sg->pflag.as<int32_t>(), sg->lflag.as<int32_t>());
		ScanSet F = {};
		F.cnt[0] = sg->pflag.as<int32_t>(), F.out[0] = sg->pfoff.as<long long>(), F.stride[0] = 1;
		F.cnt[1] = sg->lflag.as<int32_t>(), F.out[1] = sg->lfoff.as<long long>(), F.stride[1] = 1;
		scan_launch(F, 2, n + 1, sg->tmp.as<long long>(), c.stream);
		hipLaunchKernelGGL(k_sl_pairs, dim3(g_n), dim3(256), 0, c.stream, R, n, (const int32_t *)sg->pflag.p, (const long long *)sg->pfoff.p, (const long long *)sg->lfoff.p, sg->lprim.as<uint32_t>(),
		                   sg->lerr.as<long long>(), sg->lctl.as<long long>());
		PSVR_HIP(hipGetLastError());
		PSVR_HIP(hipMemcpyAsync(hm, sg->lctl.p, 24, hipMemcpyDeviceToHost, c.stream));
		drain.armed = false;
		PSVR_HIP(hipStreamSynchronize(c.stream));
		if (hm[2] || hm[0] < 0 || 2 * hm[0] > n || hm[1] < 0 || hm[1] > n) return set_error(PSVR_ERR_DEVICE, "psvr_signal_run_left: the pair list of %lld unmated records is inconsistent", n);
		sg->left_pairs = hm[0], sg->left_errors = hm[1], sg->left_ordered = true;
	}
	if (n == 0) sg->left_pairs = sg->left_errors = 0, sg->left_ordered = true;
	const long long P = sg->left_pairs;
	if (first_pair > P) return set_error(PSVR_ERR_ARG, "psvr_signal_run_left: first pair %lld of %lld", (long long)first_pair, P);
	// A slice's text stays below 2 GiB whatever the file: a slice whose size pass counts more is halved until it fits (one pair always does:
	// a pair of 2 GiB of text is the host formatter's).  PSVR_SIGNAL_TEXT_LIMIT: a smaller limit, for the tests.
	const char *e_limit = getenv("PSVR_SIGNAL_TEXT_LIMIT");
	const long long text_limit = e_limit && atoll(e_limit) > 0 ? atoll(e_limit) : 0x7fffffffll;
	long long cnt = std::min<long long>(max_pairs, P - first_pair);
	if (cnt == 0) {
		*li = psvr_signal_left_info_t{n, P, sg->left_errors, first_pair, 0, 0};
		sg->slice_first = first_pair, sg->slice_pairs = 0;
		sg->valid = true, sg->left_valid = true, sg->store = nullptr;
		sg->pairs = sg->text_bytes = sg->side_bytes = sg->n_front = sg->written = sg->declined = 0;
		return PSVR_OK;
	}
	if (sg->prim.ensure((size_t)(2 * cnt + 4) * 4) || sg->state.ensure((size_t)cnt + 1) || sg->note.ensure((size_t)cnt + 1) || sg->bytes.ensure((size_t)(cnt + 1) * 4) || sg->toff.ensure((size_t)(cnt + 1) * 8) ||
	    sg->sbytes.ensure((size_t)(cnt + 1) * 4) || sg->soff.ensure((size_t)(cnt + 1) * 8) || sg->tmp.ensure(scan_tmp_bytes(2, cnt + 1)) || sg->mctl.ensure(kSmCtl * 8)) {
		(void)hipGetLastError();
		return set_error(PSVR_ERR_NOMEM, "psvr_signal_run_left: device allocation failed for the tables of %lld pairs", cnt);
	}
	for (;; cnt = (cnt + 1) / 2) {
		long long *h = sg->h_ctl;
		for (int k = 0; k < kSgCtl; ++k) h[k] = 0;
		h[kSgFirstErr] = h[kSgFirstWritten] = kSgNone, h[kSgStatPair] = -1, h[kSgLastPrim] = -1;
		for (int k = 0; k < kSmCtl; ++k) hm[k] = 0;
		hm[kSmPairs2] = 2 * cnt;
		{
			StreamDrain drain{c.stream};
			PSVR_HIP(hipMemcpyAsync(sg->ctl.p, h, kSgCtl * 8, hipMemcpyHostToDevice, c.stream));
			PSVR_HIP(hipMemcpyAsync(sg->mctl.p, hm, kSmCtl * 8, hipMemcpyHostToDevice, c.stream));
			PSVR_HIP(hipMemcpyAsync(sg->prim.p, sg->lprim.as<uint32_t>() + 2 * first_pair, (size_t)cnt * 8, hipMemcpyDeviceToDevice, c.stream));
			drain.armed = false;
		}
		const int rc = sg_run_pairs(sg, (const uint64_t *)sg->laddr.p, nullptr, c, 0, (const long long *)(sg->mctl.as<long long>() + kSmPairs2), cnt, "psvr_signal_run_left", info, cnt > 1 ? text_limit : 0);
		if (rc == PSVR_ERR_OVERFLOW && cnt > 1) continue;        // (every wait of the refused pass is over: the tables are free to be filled again)
		if (rc) return rc;
		break;
	}
	*li = psvr_signal_left_info_t{n, P, sg->left_errors, first_pair, cnt, first_pair + cnt < P};
	sg->slice_first = first_pair, sg->slice_pairs = cnt;
	sg->left_valid = true;
	return PSVR_OK;
}

extern "C" int psvr_signal_left_errors(psvr_signal_t *sg, int64_t *errors, int64_t cap)
{
	if (psvr_device_count() <= 0) return sg_no_device();
	if (!sg || cap < 0 || (cap > 0 && !errors)) return set_error(PSVR_ERR_ARG, "psvr_signal_left_errors: bad argument");
	if (!sg->valid || !sg->left_valid) return set_error(PSVR_ERR_ARG, "psvr_signal_left_errors: no slice");
	if (cap < sg->slice_pairs) return set_error(PSVR_ERR_OVERFLOW, "psvr_signal_left_errors: the slice has %lld pairs, the table has room for %lld", sg->slice_pairs, (long long)cap);
	if (sg->slice_pairs == 0) return PSVR_OK;
	DfwCtx &c = dfw_ctx();
	std::lock_guard<std::mutex> lk(c.mu);
	if (int rc = dfw_bind(c, sg->device)) return rc;
	PSVR_HIP(hipMemcpyAsync(errors, sg->lerr.as<long long>() + sg->slice_first, (size_t)sg->slice_pairs * 8, hipMemcpyDeviceToHost, c.stream));
	PSVR_HIP(hipStreamSynchronize(c.stream));
	return PSVR_OK;
}
