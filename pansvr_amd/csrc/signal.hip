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
// Bounds: a record is read only after k_sg_mark has vouched for name, CIGAR, bases and qualities; the tag walk (bam_aux_find) stays inside
// the record by its own rules; a pair's text is written into exactly the bytes the size pass counted for it, and a write pass that ends
// anywhere else raises the refusal flag.
#include <hip/hip_runtime.h>
#include <limits.h>
#include <algorithm>
#include <vector>
#include "../../include/psvr_engine.h"
#include "common.h"
#include "scan.h"
#include "bgzf_members.h"
#include "bam_store_run.h"
#include "signal_device.h"
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
__global__ __launch_bounds__(256) void k_sg_wseg(const long long *cut, const long long *host_off, long long n_host, long long text_bytes, long long host_bytes, SwSeg *seg, long long *ctl)
{
	const long long k = (long long)blockIdx.x * 256 + threadIdx.x;
	if (k > 2 * n_host) return;
	const SwSeg s = sw_segment(k, n_host, (const int64_t *)cut, (const int64_t *)host_off, text_bytes);
	// (inside its source and inside the window, whatever the tables say: the tiles trust the table)
	if (s.len < 0 || s.off < 0 || s.off + s.len > (s.src ? host_bytes : text_bytes) || s.out < 0 || s.out + s.len > text_bytes + host_bytes) ctl[kSgRefused] = 3;
	seg[k] = s;
}
__global__ __launch_bounds__(256) void k_sg_window(const SwSeg *seg, long long n_seg, const uint8_t *text, const uint8_t *host, uint8_t *out, long long n_out, const long long *ctl)
{
	if (ctl[kSgRefused] != 0) return;                        // (the whole launch)
	sw_tile(blockIdx.x, seg, n_seg, text, host, out, n_out, threadIdx.x, 256);
}

static int sg_no_device() { return set_error(PSVR_ERR_DEVICE, "no HIP device visible: the engine has no CPU path"); }

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
	sg->valid = false, sg->win_valid = false;
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
	const uint32_t *prim = (const uint32_t *)sg->prim.p;
	const long long *poff = (const long long *)sg->poff.p;
	const unsigned g_rec = (unsigned)((m + 256) / 256), g_grp = (unsigned)((p_max + 1 + 256 / kFqGroup - 1) / (256 / kFqGroup)), g_pair = (unsigned)((p_max + 256) / 256);
	StreamDrain drain{c.stream};
	PSVR_HIP(hipMemcpyAsync(ctl, h, kSgCtl * 8, hipMemcpyHostToDevice, c.stream));
	hipLaunchKernelGGL(k_sg_mark, dim3(g_rec), dim3(256), 0, c.stream, addr, (long long)first_record, m, sg->mark.as<int32_t>(), ctl);
	ScanSet X = {};
	X.cnt[0] = sg->mark.as<int32_t>(), X.out[0] = sg->poff.as<long long>(), X.stride[0] = 1;
	scan_launch(X, 1, m + 1, sg->tmp.as<long long>(), c.stream);
	hipLaunchKernelGGL(k_sg_compact, dim3(g_rec), dim3(256), 0, c.stream, (const int32_t *)sg->mark.p, poff, m, sg->prim.as<uint32_t>());
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
	if (h[kSgRefused]) return set_error(PSVR_ERR_IO, "psvr_signal_run: malformed BAM record among records [%lld, %lld) of the store (BamReader's rules refuse it)", (long long)first_record, st->n_rec);
	const long long n_prim = h[kSgPrim], P = n_prim / 2, first_err = h[kSgFirstErr] == kSgNone ? -1 : h[kSgFirstErr], text_bytes = h[kSgText];
	const long long n_front = first_err >= 0 ? first_err : P;
	const long long side_bytes = h[kSgSide];
	if (n_prim < 0 || n_prim > m || text_bytes < 0 || side_bytes < 0) return set_error(PSVR_ERR_DEVICE, "psvr_signal_run: the run's counts are inconsistent (%lld primaries of %lld records, %lld text bytes)", n_prim, m, text_bytes);
	if (sg->text.ensure((size_t)text_bytes) || sg->side.ensure((size_t)side_bytes)) { (void)hipGetLastError(); return set_error(PSVR_ERR_NOMEM, "psvr_signal_run: device allocation failed for %lld bytes of text and %lld of records", text_bytes, side_bytes); }
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
	if (h[kSgRefused]) return set_error(PSVR_ERR_DEVICE, "psvr_signal_run: the write pass did not end where the size pass said (the text is not used)");
	if (h[kSgStatPair] >= 0) sg->spent = true;
	sg->valid = true, sg->store = st, sg->store_generation = st->generation, sg->first_record = first_record, sg->pairs = P, sg->text_bytes = text_bytes, sg->side_bytes = side_bytes;
	sg->n_front = n_front, sg->written = h[kSgWritten], sg->declined = h[kSgDeclined];
	info->side_bytes = side_bytes;
	info->pairs = P, info->written = h[kSgWritten], info->declined = h[kSgDeclined], info->first_error = first_err, info->text_bytes = text_bytes;
	info->consumed = (n_prim & 1) ? first_record + h[kSgLastPrim] : st->n_rec;
	return PSVR_OK;
}

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

extern "C" int psvr_signal_window(psvr_signal_t *sg, const void *host_text, int64_t host_bytes, const int64_t *host_off, int64_t n_host, psvr_signal_window_info_t *info)
{
	if (psvr_device_count() <= 0) return sg_no_device();
	if (!sg || !info || (host_bytes > 0 && !host_text)) return set_error(PSVR_ERR_ARG, "psvr_signal_window: null argument");
	if (!sg->valid) return set_error(PSVR_ERR_ARG, "psvr_signal_window: no run");
	if (const char *bad = sw_args_bad(host_bytes, host_off, n_host, sg->declined))
		return set_error(PSVR_ERR_ARG, "psvr_signal_window: %s (%lld host pairs with %lld bytes, the run has %lld)", bad, (long long)n_host, (long long)host_bytes, sg->declined);
	const long long n_front = sg->n_front, text_bytes = sg->text_bytes, n_out = text_bytes + host_bytes, n_seg = 2 * n_host + 1;
	if (n_out >= (1ll << 32)) return set_error(PSVR_ERR_UNSUPPORTED, "psvr_signal_window: a window of %lld bytes (at most 2^32 - 1: the parser's offsets)", n_out);
	DfwCtx &c = dfw_ctx();
	std::lock_guard<std::mutex> lk(c.mu);
	if (int rc = dfw_bind(c, sg->device)) return rc;
	sg->win_valid = false;
	if (sg->wflag.ensure((size_t)(n_front + 1) * 4) || sg->wrank.ensure((size_t)(n_front + 1) * 8) || sg->wcut.ensure((size_t)(n_host + 1) * 8) || sg->wseg.ensure((size_t)n_seg * sizeof(SwSeg)) ||
	    sg->whost.ensure((size_t)host_bytes + 16) || sg->whoff.ensure((size_t)(n_host + 1) * 8) || sg->window.ensure((size_t)n_out + 16) || sg->tmp.ensure(scan_tmp_bytes(1, n_front + 1)) ||
	    (!sg->text.p && sg->text.ensure(16))) {             // (a run without text: the kernel still gets a pointer; a run's text is never reallocated here)
		(void)hipGetLastError();
		return set_error(PSVR_ERR_NOMEM, "psvr_signal_window: device allocation failed for a window of %lld bytes and %lld segments", n_out, n_seg);
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
	                   (long long)host_bytes, sg->wseg.as<SwSeg>(), ctl);
	if (n_out)
		hipLaunchKernelGGL(k_sg_window, dim3((unsigned)((n_out + kSwTileBytes - 1) / kSwTileBytes)), dim3(256), 0, c.stream, (const SwSeg *)sg->wseg.p, n_seg, (const uint8_t *)sg->text.p,
		                   (const uint8_t *)sg->whost.p, sg->window.as<uint8_t>(), n_out, (const long long *)ctl);
	PSVR_HIP(hipGetLastError());
	PSVR_HIP(hipMemcpyAsync(h + kSgRefused, ctl + kSgRefused, 8, hipMemcpyDeviceToHost, c.stream));
	drain.armed = false;
	PSVR_HIP(hipStreamSynchronize(c.stream));
	if (h[kSgRefused]) return set_error(PSVR_ERR_DEVICE, "psvr_signal_window: the segment table does not fit the run's text and the host text (the window is not used)");
	sg->win_valid = true, sg->win_bytes = n_out;
	info->n_bytes = n_out, info->n_pairs = sg->written + sg->declined, info->n_host_pairs = n_host;
	return PSVR_OK;
}

extern "C" int psvr_signal_window_text(psvr_signal_t *sg, void *dst, int64_t first, int64_t n)
{
	if (psvr_device_count() <= 0) return sg_no_device();
	if (!sg || first < 0 || n < 0 || (n > 0 && !dst)) return set_error(PSVR_ERR_ARG, "psvr_signal_window_text: bad argument");
	if (!sg->valid || !sg->win_valid) return set_error(PSVR_ERR_ARG, "psvr_signal_window_text: no window");
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
