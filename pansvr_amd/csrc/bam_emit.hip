// bam_emit.hip -- psvr_bam_emit_* (include/psvr_engine.h): the main BAM file's records of a run of pairs, encoded on the device from a
// parsed window (psvr_fastq_t: text, line index, name ends, original alignments) and a set of results (the caller's compact arrays, or an
// engine's in HBM).  The rules are bam_emit_device.h's, which the host build holds to SamEmitter::main_pair byte for byte; this file is
// their launch order on the emitter's own stream:
//   [upload of the caller's results] -> k_be_size -> scan (scan.h) -> read back the total -> k_be_write
// A group of kFqGroup lanes takes a pair (both of its reads, mate 0 first): the size pass gives the pair's state and the bytes of its
// records, their scan is pair_off, the write pass walks the same function with a sink that stores.  Bounds: be_plan_read checks every
// index a result holds before it is followed, so only the given arrays, the window's text (lines between two stored starts) and the
// index's string table are read; a pair writes bytes[pair_off[p], pair_off[p + 1]) and nothing else, because both passes walk be_record.
// psvr_bam_emit_ori_* are the same launch order over the second file's rules (bam_ori_device.h, held to SamEmitter::ori_pair): k_bo_size and
// k_bo_write walk bo_pair, which reads the pair's two comments, the results' pair record and -- for the `proper` rule -- one candidate's
// CIGAR words after the same index check.  An emitter holds the records of its last run, whichever file they are for.
#include <hip/hip_runtime.h>
#include "../../include/psvr_engine.h"
#include "common.h"
#include "bam_emit_device.h"
#include "bam_ori_device.h"
#include "bam_emit_hooks.h"
#include "bam_emit_run.h"
#include "fastq_parsed.h"
#include "scan.h"

namespace psvr {

static_assert(kFqGroup == 16, "the kernels below are written for 256 threads and four groups per wavefront");

// kFqGroup lanes per pair: its state, the bytes of its records; the run's counts (a workgroup adds up in LDS first)
__global__ __launch_bounds__(256) void k_be_size(BeInput in, int64_t P, int32_t *cnt, uint8_t *state, unsigned long long *counters)
{
	__shared__ unsigned int sum[3];
	if (threadIdx.x < 3) sum[threadIdx.x] = 0;
	__syncthreads();
	const int64_t p = ((int64_t)blockIdx.x * 256 + threadIdx.x) / kFqGroup;
	if (p < P) {
		FqGroup g;
		g.lane = threadIdx.x & (kFqGroup - 1), g.shift = threadIdx.x & 63 & ~(kFqGroup - 1);
		int32_t nb, nr;
		const int st = be_pair_size(g, in, p, &nb, &nr);
		if (g.lane == 0) {
			cnt[p] = nb, state[p] = (uint8_t)st;
			if (nr) atomicAdd(&sum[0], (unsigned int)nr);
			if (st) atomicAdd(&sum[st], 1u);
		}
	}
	__syncthreads();
	if (threadIdx.x < 3 && sum[threadIdx.x]) atomicAdd(&counters[threadIdx.x], (unsigned long long)sum[threadIdx.x]);
}

// kFqGroup lanes per written pair: its records at pair_off[p]
__global__ __launch_bounds__(256) void k_be_write(BeInput in, int64_t P, const long long *pair_off, const uint8_t *state, uint8_t *bytes)
{
	const int64_t p = ((int64_t)blockIdx.x * 256 + threadIdx.x) / kFqGroup;
	if (p >= P || state[p] != 1) return;
	FqGroup g;
	g.lane = threadIdx.x & (kFqGroup - 1), g.shift = threadIdx.x & 63 & ~(kFqGroup - 1);
	BeWrite w;
	w.out = bytes, w.pos = (uint64_t)pair_off[p];
	int32_t nr;
	be_pair(g, in, p, w, &nr);
}

// the same two passes by the second file's rules (bam_ori_device.h): same launch shape, same outputs
__global__ __launch_bounds__(256) void k_bo_size(BoInput in, int64_t P, int32_t *cnt, uint8_t *state, unsigned long long *counters)
{
	__shared__ unsigned int sum[3];
	if (threadIdx.x < 3) sum[threadIdx.x] = 0;
	__syncthreads();
	const int64_t p = ((int64_t)blockIdx.x * 256 + threadIdx.x) / kFqGroup;
	if (p < P) {
		FqGroup g;
		g.lane = threadIdx.x & (kFqGroup - 1), g.shift = threadIdx.x & 63 & ~(kFqGroup - 1);
		int32_t nb, nr;
		const int st = bo_pair_size(g, in, p, &nb, &nr);
		if (g.lane == 0) {
			cnt[p] = nb, state[p] = (uint8_t)st;
			if (nr) atomicAdd(&sum[0], (unsigned int)nr);
			if (st) atomicAdd(&sum[st], 1u);
		}
	}
	__syncthreads();
	if (threadIdx.x < 3 && sum[threadIdx.x]) atomicAdd(&counters[threadIdx.x], (unsigned long long)sum[threadIdx.x]);
}
__global__ __launch_bounds__(256) void k_bo_write(BoInput in, int64_t P, const long long *pair_off, const uint8_t *state, uint8_t *bytes)
{
	const int64_t p = ((int64_t)blockIdx.x * 256 + threadIdx.x) / kFqGroup;
	if (p >= P || state[p] != 1) return;
	FqGroup g;
	g.lane = threadIdx.x & (kFqGroup - 1), g.shift = threadIdx.x & 63 & ~(kFqGroup - 1);
	BeWrite w;
	w.out = bytes, w.pos = (uint64_t)pair_off[p];
	int32_t nr;
	bo_pair(g, in, p, w, &nr);
}

static inline unsigned be_grid(int64_t n) { return (unsigned)((n + 255) / 256); }

// the kernels of a set of rules, chosen by the type of their input
struct BeKernels {
	static void size(const BeInput &in, int64_t P, int32_t *cnt, uint8_t *state, unsigned long long *counters, hipStream_t st) { hipLaunchKernelGGL(k_be_size, dim3(be_grid(P * kFqGroup)), dim3(256), 0, st, in, P, cnt, state, counters); }
	static void size(const BoInput &in, int64_t P, int32_t *cnt, uint8_t *state, unsigned long long *counters, hipStream_t st) { hipLaunchKernelGGL(k_bo_size, dim3(be_grid(P * kFqGroup)), dim3(256), 0, st, in, P, cnt, state, counters); }
	static void write(const BeInput &in, int64_t P, const long long *pair_off, const uint8_t *state, uint8_t *bytes, hipStream_t st) { hipLaunchKernelGGL(k_be_write, dim3(be_grid(P * kFqGroup)), dim3(256), 0, st, in, P, pair_off, state, bytes); }
	static void write(const BoInput &in, int64_t P, const long long *pair_off, const uint8_t *state, uint8_t *bytes, hipStream_t st) { hipLaunchKernelGGL(k_bo_write, dim3(be_grid(P * kFqGroup)), dim3(256), 0, st, in, P, pair_off, state, bytes); }
};

// every emit call ends here: `in` (BeInput: the main file's rules, BoInput: the second file's) holds device pointers only
template <class In> static int be_run(psvr_bam_emit *em, const In &in, int64_t P, psvr_bam_emit_info_t *info)
{
	em->valid = false;
	if (em->cnt.ensure((size_t)(P + 1) * 4) || em->pair_off.ensure((size_t)(P + 1) * 8) || em->state.ensure((size_t)P + 1) || em->tmp.ensure(scan_tmp_bytes(1, P + 1)) ||
	    em->counters.ensure(3 * 8)) {
		(void)hipGetLastError();
		return set_error(PSVR_ERR_NOMEM, "psvr_bam_emit: device allocation failed for %lld pairs", (long long)P);
	}
	hipStream_t st = em->stream;
	StreamDrain drain{st};
	PSVR_HIP(hipMemsetAsync(em->counters.p, 0, 3 * 8, st));
	PSVR_HIP(hipMemsetAsync(em->cnt.as<int32_t>() + P, 0, 4, st));                             // the scan's last entry: its offset is the total
	if (P) BeKernels::size(in, P, em->cnt.as<int32_t>(), em->state.as<uint8_t>(), em->counters.as<unsigned long long>(), st);
	ScanSet S = {};
	S.cnt[0] = em->cnt.as<int32_t>(), S.out[0] = em->pair_off.as<long long>(), S.stride[0] = 1;
	scan_launch(S, 1, P + 1, em->tmp.as<long long>(), st);
	PSVR_HIP(hipGetLastError());
	PSVR_HIP(hipMemcpyAsync(em->h_back, em->pair_off.as<long long>() + P, 8, hipMemcpyDeviceToHost, st));
	PSVR_HIP(hipMemcpyAsync(em->h_back + 1, em->counters.p, 3 * 8, hipMemcpyDeviceToHost, st));
	PSVR_HIP(hipStreamSynchronize(st));
	const int64_t total = em->h_back[0];
	if (em->bytes.ensure((size_t)total + 64)) {
		(void)hipGetLastError();
		return set_error(PSVR_ERR_NOMEM, "psvr_bam_emit: device allocation failed for %lld bytes of records", (long long)total);
	}
	if (P && total) BeKernels::write(in, P, (const long long *)em->pair_off.p, (const uint8_t *)em->state.p, em->bytes.as<uint8_t>(), st);
	PSVR_HIP(hipGetLastError());
	drain.armed = false;
	PSVR_HIP(hipStreamSynchronize(st));
	em->n_pairs = P, em->n_bytes = total, em->valid = true;
	if (info) info->n_bytes = total, info->n_records = em->h_back[1], info->n_written_pairs = em->h_back[2], info->n_declined_pairs = em->h_back[3];
	return PSVR_OK;
}

static void be_window(const psvr_fastq *fq, int64_t first_pair, int32_t flags, const BeTables &T, BeInput *in)
{
	memset(in, 0, sizeof *in);
	in->text = fq->text.as<char>(), in->line_start = fq->line_start.as<uint64_t>(), in->name_end = fq->name_end.as<uint16_t>(), in->ori = fq->ori.as<psvr_ori_t>();
	in->first_pair = first_pair, in->not_ori = (flags & PSVR_EMIT_NOT_ORI) != 0, in->T = T;
}

} // namespace psvr

using namespace psvr;

static int be_no_device() { return set_error(PSVR_ERR_DEVICE, "no HIP device visible: the engine has no CPU path"); }

extern "C" int psvr_bam_emit_create(const psvr_index_t *idx, psvr_bam_emit_t **out)
{
	if (psvr_device_count() <= 0) return be_no_device();
	if (!idx || !out) return set_error(PSVR_ERR_ARG, "psvr_bam_emit_create: null argument");
	BeTables T;
	int device = 0;
	const int rc = index_emit_tables(idx, &T, &device);
	if (rc) return rc;
	PSVR_HIP(hipSetDevice(device));
	psvr_bam_emit *em = new psvr_bam_emit;
	em->device = device, em->T = T;
	hipError_t e = hipStreamCreateWithFlags(&em->stream, hipStreamNonBlocking);
	if (e == hipSuccess) e = hipHostMalloc((void **)&em->h_back, 4 * sizeof(long long), hipHostMallocDefault);
	if (e != hipSuccess) { psvr_bam_emit_destroy(em); return set_error(PSVR_ERR_DEVICE, "psvr_bam_emit_create: %s", hipGetErrorString(e)); }
	*out = em;
	return PSVR_OK;
}

extern "C" void psvr_bam_emit_destroy(psvr_bam_emit_t *em)
{
	if (!em) return;
	(void)hipSetDevice(em->device);
	if (em->stream) (void)hipStreamSynchronize(em->stream), (void)hipStreamDestroy(em->stream);
	if (em->h_back) (void)hipHostFree(em->h_back);
	delete em;                                               // (its DevBufs free themselves)
}

// the caller's compact results checked against the window and uploaded into the emitter's buffers (`who`: the call's name in messages)
struct BeResultsDev { const psvr_read_hdr_t *hdr; const psvr_pair_result_t *pairs; const psvr_cand_t *cands; const uint32_t *cig; };
static int be_upload_results(const char *who, psvr_bam_emit_t *em, const psvr_fastq_t *fq, int64_t first_pair, int64_t n_pairs, const psvr_read_hdr_t *hdr, const psvr_pair_result_t *pairs,
                             const psvr_cand_t *cands, int64_t n_cands, const uint32_t *cigar, int64_t n_cigar, BeResultsDev *r)
{
	if (!em || !fq || first_pair < 0 || n_pairs < 0 || n_cands < 0 || n_cigar < 0 || (n_pairs && (!hdr || !pairs)) || (n_cands && !cands) || (n_cigar && !cigar))
		return set_error(PSVR_ERR_ARG, "%s: bad argument", who);
	if (!fq->valid || first_pair + n_pairs > fq->last.n_pairs)
		return set_error(PSVR_ERR_ARG, "%s: pairs [%lld, %lld) are not in the parsed window (%lld pairs)", who, (long long)first_pair, (long long)(first_pair + n_pairs), fq->valid ? (long long)fq->last.n_pairs : 0ll);
	if (fq->device != em->device) return set_error(PSVR_ERR_ARG, "%s: the text was parsed on device %d, the emitter's index is on device %d", who, fq->device, em->device);
	PSVR_HIP(hipSetDevice(em->device));
	const size_t nh = (size_t)(2 * n_pairs) * sizeof(psvr_read_hdr_t), np = (size_t)n_pairs * sizeof(psvr_pair_result_t), nc = (size_t)n_cands * sizeof(psvr_cand_t), nw = (size_t)n_cigar * 4;
	if (em->hdr.ensure(nh) || em->pairs.ensure(np) || em->cands.ensure(nc) || em->cig.ensure(nw)) {
		(void)hipGetLastError();
		return set_error(PSVR_ERR_NOMEM, "%s: device allocation failed for the results of %lld pairs", who, (long long)n_pairs);
	}
	{
		StreamDrain drain{em->stream};
		if (nh) PSVR_HIP(hipMemcpyAsync(em->hdr.p, hdr, nh, hipMemcpyHostToDevice, em->stream));
		if (np) PSVR_HIP(hipMemcpyAsync(em->pairs.p, pairs, np, hipMemcpyHostToDevice, em->stream));
		if (nc) PSVR_HIP(hipMemcpyAsync(em->cands.p, cands, nc, hipMemcpyHostToDevice, em->stream));
		if (nw) PSVR_HIP(hipMemcpyAsync(em->cig.p, cigar, nw, hipMemcpyHostToDevice, em->stream));
	}                                                        // (drained: the caller's arrays are free whatever happens next)
	r->hdr = em->hdr.as<psvr_read_hdr_t>(), r->pairs = em->pairs.as<psvr_pair_result_t>(), r->cands = em->cands.as<psvr_cand_t>(), r->cig = em->cig.as<uint32_t>();
	return PSVR_OK;
}

extern "C" int psvr_bam_emit_results(psvr_bam_emit_t *em, const psvr_fastq_t *fq, int64_t first_pair, int64_t n_pairs, const psvr_read_hdr_t *hdr, const psvr_pair_result_t *pairs,
                                     const psvr_cand_t *cands, int64_t n_cands, const uint32_t *cigar, int64_t n_cigar, int32_t flags, psvr_bam_emit_info_t *info)
{
	if (psvr_device_count() <= 0) return be_no_device();
	BeResultsDev r;
	const int rc = be_upload_results("psvr_bam_emit_results", em, fq, first_pair, n_pairs, hdr, pairs, cands, n_cands, cigar, n_cigar, &r);
	if (rc) return rc;
	BeInput in;
	be_window(fq, first_pair, flags, em->T, &in);
	in.hdr = r.hdr, in.pairs = r.pairs, in.cands = r.cands, in.n_cands = n_cands, in.cig = r.cig, in.n_cig = n_cigar;
	return be_run(em, in, n_pairs, info);
}

// an engine's last results in HBM, checked against the window they came from (`who`: the call's name in messages)
static int be_engine_results(const char *who, psvr_bam_emit_t *em, psvr_engine_t *eng, const psvr_fastq_t *fq, EngineEmitView *v)
{
	if (!em || !eng || !fq) return set_error(PSVR_ERR_ARG, "%s: null argument", who);
	engine_emit_view(eng, v);
	if (!v->fq) return set_error(PSVR_ERR_ARG, "%s: the engine's last upload did not come from a psvr_fastq_t (psvr_engine_upload_fastq), the text of its reads is not on the device", who);
	if (v->fq != fq) return set_error(PSVR_ERR_ARG, "%s: the engine's last upload came from another psvr_fastq_t than the one given", who);
	if (!fq->valid || v->generation != fq->generation) return set_error(PSVR_ERR_ARG, "%s: the psvr_fastq_t has been parsed into since the engine's upload, the window of its reads is gone", who);
	if (v->device != em->device || fq->device != em->device)
		return set_error(PSVR_ERR_ARG, "%s: the engine runs on device %d, the text was parsed on device %d, the emitter's index is on device %d", who, v->device, fq->device, em->device);
	if (v->n_pairs > 0 && !v->ran) return set_error(PSVR_ERR_ARG, "%s: the engine has not run the batch it was given (psvr_engine_run)", who);
	PSVR_HIP(hipSetDevice(em->device));
	return PSVR_OK;
}

extern "C" int psvr_bam_emit_engine(psvr_bam_emit_t *em, psvr_engine_t *eng, const psvr_fastq_t *fq, int32_t flags, psvr_bam_emit_info_t *info)
{
	if (psvr_device_count() <= 0) return be_no_device();
	EngineEmitView v;
	const int rc = be_engine_results("psvr_bam_emit_engine", em, eng, fq, &v);
	if (rc) return rc;
	BeInput in;
	be_window(fq, v.first_pair, flags, em->T, &in);
	in.hdr = v.hdr, in.pairs = v.pairs, in.cands = v.cands, in.n_cands = v.n_cands, in.cig = v.cig, in.n_cig = v.n_cig;
	return be_run(em, in, v.n_pairs, info);
}

// ---- the second file's records: the same calls over bam_ori_device.h's rules --------------------------------------------------------------
static void bo_window(const psvr_fastq *fq, int64_t first_pair, int32_t min_filter_score, const BeTables &T, BoInput *in)
{
	memset(in, 0, sizeof *in);
	in->text = fq->text.as<char>(), in->line_start = fq->line_start.as<uint64_t>(), in->name_end = fq->name_end.as<uint16_t>(), in->ori = fq->ori.as<psvr_ori_t>();
	in->first_pair = first_pair, in->min_filter_score = min_filter_score, in->n_header = T.n_header;
}

extern "C" int psvr_bam_emit_ori_results(psvr_bam_emit_t *em, const psvr_fastq_t *fq, int64_t first_pair, int64_t n_pairs, const psvr_read_hdr_t *hdr, const psvr_pair_result_t *pairs,
                                         const psvr_cand_t *cands, int64_t n_cands, const uint32_t *cigar, int64_t n_cigar, int32_t min_filter_score, psvr_bam_emit_info_t *info)
{
	if (psvr_device_count() <= 0) return be_no_device();
	BeResultsDev r;
	const int rc = be_upload_results("psvr_bam_emit_ori_results", em, fq, first_pair, n_pairs, hdr, pairs, cands, n_cands, cigar, n_cigar, &r);
	if (rc) return rc;
	BoInput in;
	bo_window(fq, first_pair, min_filter_score, em->T, &in);
	in.hdr = r.hdr, in.pairs = r.pairs, in.cands = r.cands, in.n_cands = n_cands, in.cig = r.cig, in.n_cig = n_cigar;
	return be_run(em, in, n_pairs, info);
}

extern "C" int psvr_bam_emit_ori_engine(psvr_bam_emit_t *em, psvr_engine_t *eng, const psvr_fastq_t *fq, psvr_bam_emit_info_t *info)
{
	if (psvr_device_count() <= 0) return be_no_device();
	EngineEmitView v;
	const int rc = be_engine_results("psvr_bam_emit_ori_engine", em, eng, fq, &v);
	if (rc) return rc;
	BoInput in;
	bo_window(fq, v.first_pair, v.min_filter_score, em->T, &in);
	in.hdr = v.hdr, in.pairs = v.pairs, in.cands = v.cands, in.n_cands = v.n_cands, in.cig = v.cig, in.n_cig = v.n_cig;
	return be_run(em, in, v.n_pairs, info);
}

extern "C" int psvr_bam_emit_download(const psvr_bam_emit_t *em, void *bytes, int64_t cap, int64_t *pair_off, uint8_t *pair_state)
{
	if (psvr_device_count() <= 0) return be_no_device();
	if (!em || !em->valid) return set_error(PSVR_ERR_ARG, "psvr_bam_emit_download: no emitted run of pairs");
	if (bytes && cap < em->n_bytes) return set_error(PSVR_ERR_OVERFLOW, "psvr_bam_emit_download: the records take %lld bytes, the buffer has %lld", (long long)em->n_bytes, (long long)cap);
	PSVR_HIP(hipSetDevice(em->device));
	hipStream_t st = em->stream;
	StreamDrain drain{st};
	// (hipMemcpyDefault: a destination may be host memory or memory of this device)
	if (bytes && em->n_bytes) PSVR_HIP(hipMemcpyAsync(bytes, em->bytes.p, (size_t)em->n_bytes, hipMemcpyDefault, st));
	if (pair_off) PSVR_HIP(hipMemcpyAsync(pair_off, em->pair_off.p, (size_t)(em->n_pairs + 1) * 8, hipMemcpyDefault, st));
	if (pair_state && em->n_pairs) PSVR_HIP(hipMemcpyAsync(pair_state, em->state.p, (size_t)em->n_pairs, hipMemcpyDefault, st));
	drain.armed = false;
	PSVR_HIP(hipStreamSynchronize(st));
	return PSVR_OK;
}
