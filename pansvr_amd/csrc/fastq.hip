// fastq.hip -- psvr_fastq_* (include/psvr_engine.h): a window of interleaved FASTQ text parsed on the device into the arrays the engine
// takes (line index, name ends, base offsets, original alignments, bases).  The rules are fastq_device.h's, which the host build holds to
// fastq_batch.h byte for byte; this file is their launch order on one stream:
//   copy of the text (from the host, or device to device from a signal run's window: psvr_fastq_parse_signal) -> k_fq_count -> scan (scan.h) -> k_fq_lines -> k_fq_meta -> k_fq_slen -> scan -> k_fq_cut -> k_fq_extract -> info
// The host reads back the one psvr_fastq_info_t at the end; every count in between (newlines, pairs that count, pairs kept) stays on the
// device, and the launches that depend on one are sized by what the window's size and max_pairs allow (fq_line_cap, fq_pair_cap).
// Every phase hands over to the next at a kernel boundary.  Bounds: the newline passes read text[0, n) only (fq_newline_mask); line starts
// are stored at indices <= cap only; every later pass reads lines between two stored starts <= n.
#include <hip/hip_runtime.h>
#include <atomic>
#include "../../include/psvr_engine.h"
#include "common.h"
#include "fastq_device.h"
#include "fastq_parsed.h"
#include "signal_run.h"
#include "scan.h"

namespace psvr {

static_assert(kFqTileLanes == 256 && kFqGroup == 16, "the kernels below are written for 256 threads and four groups per wavefront");

// newlines of tile blockIdx.x
__global__ __launch_bounds__(kFqTileLanes) void k_fq_count(const char *text, uint64_t n, int32_t *cnt)
{
	__shared__ int red[kFqTileLanes / 64];
	const uint64_t pos = (uint64_t)blockIdx.x * kFqTileBytes + (uint64_t)threadIdx.x * kFqPiece;
	int c = (int)fq_popc(fq_newline_mask(text, pos, n));
	for (int d = 32; d > 0; d >>= 1) c += __shfl_down(c, d, 64);
	if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = c;
	__syncthreads();
	if (threadIdx.x == 0) cnt[blockIdx.x] = red[0] + red[1] + red[2] + red[3];
}

// the line starts behind tile blockIdx.x's newlines, in order: tile_off newlines lie in front of the tile, the lanes' counts are scanned here
__global__ __launch_bounds__(kFqTileLanes) void k_fq_lines(const char *text, uint64_t n, const long long *tile_off, uint64_t cap, uint64_t *line_start)
{
	__shared__ uint32_t wsum[kFqTileLanes / 64];
	const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
	const uint64_t pos = (uint64_t)blockIdx.x * kFqTileBytes + (uint64_t)threadIdx.x * kFqPiece;
	const uint32_t m = fq_newline_mask(text, pos, n), c = fq_popc(m);
	uint32_t s = c;
	for (int d = 1; d < 64; d <<= 1) { const uint32_t t = (uint32_t)__shfl_up((int)s, d, 64); if (lane >= d) s += t; }
	if (lane == 63) wsum[w] = s;
	__syncthreads();
	uint32_t before = 0;
	for (int q = 0; q < w; ++q) before += wsum[q];
	fq_emit_piece(m, pos, (uint64_t)tile_off[blockIdx.x] + before + s - c, cap, line_start);
}

// one thread: the window's tail, the lines and pairs that count; the record of a call that keeps no pair
__global__ void k_fq_meta(const char *text, uint64_t n, int at_end, const long long *n_newlines, int64_t max_pairs, int64_t max_bases, uint64_t cap, uint64_t *line_start,
                          FqMeta *meta, psvr_fastq_info_t *info, char *bases)
{
	const FqMeta m = fq_lines_meta(text, n, at_end, (uint64_t)*n_newlines, max_pairs, cap, line_start);
	*meta = m;
	const int64_t zero = 0;
	fq_fill_info(0, m, max_pairs, max_bases, &zero, line_start, info);
	bases[0] = 0;
}

// a lane per candidate read: the trimmed length of its sequence line (0 behind the pairs that count, so that one scan serves)
__global__ __launch_bounds__(256) void k_fq_slen(const char *text, const uint64_t *line_start, const FqMeta *meta, int64_t r_cap, int32_t *slen)
{
	const int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x;
	if (r > r_cap) return;
	slen[r] = r < 2 * meta->avail ? (int32_t)fq_trimmed_len(text, line_start[4 * r + 1], line_start[4 * r + 2]) : 0;
}

// a lane per candidate pair: the one that is the last kept writes the record and the NUL behind the bases
__global__ __launch_bounds__(256) void k_fq_cut(const FqMeta *meta, const long long *base_off, const uint64_t *line_start, int64_t max_pairs, int64_t max_bases,
                                                psvr_fastq_info_t *info, char *bases)
{
	const int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x;
	const FqMeta m = *meta;
	if (p >= m.avail || !fq_cut_here(p, m.avail, (const int64_t *)base_off, max_bases)) return;
	fq_fill_info(p + 1, m, max_pairs, max_bases, (const int64_t *)base_off, line_start, info);
	bases[base_off[2 * (p + 1)]] = 0;
}

// kFqGroup lanes per kept read: bases and header
__global__ __launch_bounds__(256) void k_fq_extract(const char *text, const uint64_t *line_start, const long long *base_off, const psvr_fastq_info_t *info, char *bases,
                                                    uint16_t *name_end, psvr_ori_t *ori)
{
	const int64_t r = ((int64_t)blockIdx.x * 256 + threadIdx.x) / kFqGroup;
	if (r >= 2 * info->n_pairs) return;
	FqGroup g;
	g.lane = threadIdx.x & (kFqGroup - 1), g.shift = threadIdx.x & 63 & ~(kFqGroup - 1);
	fq_extract_read(g, text, line_start, (const int64_t *)base_off, r, bases, name_end, ori);
}

// psvr_fastq::generation
static uint64_t fq_next_generation() { static std::atomic<uint64_t> g(0); return ++g; }

static inline unsigned fq_grid(int64_t n) { return (unsigned)((n + 255) / 256); }

} // namespace psvr

using namespace psvr;

static int fq_no_device() { return set_error(PSVR_ERR_DEVICE, "no HIP device visible: the engine has no CPU path"); }

extern "C" int psvr_fastq_create(int device, psvr_fastq_t **out)
{
	if (psvr_device_count() <= 0) return fq_no_device();
	if (!out || device < 0) return set_error(PSVR_ERR_ARG, "psvr_fastq_create: bad argument");
	PSVR_HIP(hipSetDevice(device));
	psvr_fastq *fq = new psvr_fastq;
	fq->device = device, fq->generation = fq_next_generation();
	hipError_t e = hipStreamCreateWithFlags(&fq->stream, hipStreamNonBlocking);
	if (e == hipSuccess) e = hipHostMalloc((void **)&fq->h_info, sizeof(psvr_fastq_info_t), hipHostMallocDefault);
	if (e != hipSuccess) { psvr_fastq_destroy(fq); return set_error(PSVR_ERR_DEVICE, "psvr_fastq_create: %s", hipGetErrorString(e)); }
	*out = fq;
	return PSVR_OK;
}

extern "C" void psvr_fastq_destroy(psvr_fastq_t *fq)
{
	if (!fq) return;
	(void)hipSetDevice(fq->device);
	if (fq->stream) (void)hipStreamSynchronize(fq->stream), (void)hipStreamDestroy(fq->stream);
	if (fq->h_info) (void)hipHostFree(fq->h_info);
	delete fq;                                               // (its DevBufs free themselves)
}

// the one body of psvr_fastq_parse and psvr_fastq_parse_signal: text[0, n_bytes) is host memory (kind: host to device) or memory of fq's
// device (device to device); the callers have looked at their arguments
static int fq_parse_from(const char *who, psvr_fastq_t *fq, const void *text, hipMemcpyKind kind, int64_t n_bytes, int at_end, int64_t max_pairs, int64_t max_bases, psvr_fastq_info_t *info)
{
	if (n_bytes >= ((int64_t)1 << 32)) return set_error(PSVR_ERR_UNSUPPORTED, "%s: a window of %lld bytes, offsets inside a call are 32-bit (at most 2^32 - 1 bytes)", who, (long long)n_bytes);
	PSVR_HIP(hipSetDevice(fq->device));
	fq->valid = false, fq->generation = fq_next_generation(), fq->n_text = 0;
	const uint64_t n = (uint64_t)n_bytes, cap = fq_line_cap(n, max_pairs);
	const int64_t ntile = (int64_t)((n + kFqTileBytes - 1) / kFqTileBytes), p_cap = fq_pair_cap(n, max_pairs), r_cap = 2 * p_cap;
	const size_t tmp_a = scan_tmp_bytes(1, ntile + 1), tmp_b = scan_tmp_bytes(1, r_cap + 1);
	if (fq->text.ensure(n + 16) || fq->cnt.ensure((size_t)(ntile + 1) * 4) || fq->tile_off.ensure((size_t)(ntile + 1) * 8) || fq->tmp.ensure(tmp_a > tmp_b ? tmp_a : tmp_b) ||
	    fq->line_start.ensure((size_t)(cap + 1) * 8) || fq->slen.ensure((size_t)(r_cap + 1) * 4) || fq->base_off.ensure((size_t)(r_cap + 1) * 8) ||
	    fq->name_end.ensure((size_t)(r_cap + 1) * 2) || fq->ori.ensure((size_t)(r_cap + 1) * sizeof(psvr_ori_t)) || fq->bases.ensure(n + 1 + 64) ||
	    fq->meta.ensure(sizeof(FqMeta)) || fq->info.ensure(sizeof(psvr_fastq_info_t))) {
		(void)hipGetLastError();
		return set_error(PSVR_ERR_NOMEM, "%s: device allocation failed for a window of %lld bytes and up to %lld pairs", who, (long long)n_bytes, (long long)p_cap);
	}
	hipStream_t st = fq->stream;
	const char *d_text = fq->text.as<char>();
	uint64_t *d_ls = fq->line_start.as<uint64_t>();
	long long *d_tile_off = fq->tile_off.as<long long>(), *d_off = fq->base_off.as<long long>();
	FqMeta *d_meta = fq->meta.as<FqMeta>();
	psvr_fastq_info_t *d_info = fq->info.as<psvr_fastq_info_t>();
	StreamDrain drain{st};
	if (n) PSVR_HIP(hipMemcpyAsync(fq->text.p, text, n, kind, st));
	PSVR_HIP(hipMemsetAsync(fq->cnt.as<int32_t>() + ntile, 0, 4, st));                    // the scan's last entry: its offset is the total
	if (ntile) hipLaunchKernelGGL(k_fq_count, dim3((unsigned)ntile), dim3(kFqTileLanes), 0, st, d_text, n, fq->cnt.as<int32_t>());
	ScanSet S = {};
	S.cnt[0] = fq->cnt.as<int32_t>(), S.out[0] = d_tile_off, S.stride[0] = 1;
	scan_launch(S, 1, ntile + 1, fq->tmp.as<long long>(), st);
	if (ntile) hipLaunchKernelGGL(k_fq_lines, dim3((unsigned)ntile), dim3(kFqTileLanes), 0, st, d_text, n, (const long long *)d_tile_off, cap, d_ls);
	hipLaunchKernelGGL(k_fq_meta, dim3(1), dim3(1), 0, st, d_text, n, at_end, (const long long *)(d_tile_off + ntile), max_pairs, max_bases, cap, d_ls, d_meta, d_info, fq->bases.as<char>());
	hipLaunchKernelGGL(k_fq_slen, dim3(fq_grid(r_cap + 1)), dim3(256), 0, st, d_text, (const uint64_t *)d_ls, (const FqMeta *)d_meta, r_cap, fq->slen.as<int32_t>());
	S.cnt[0] = fq->slen.as<int32_t>(), S.out[0] = d_off;
	scan_launch(S, 1, r_cap + 1, fq->tmp.as<long long>(), st);
	if (p_cap) {
		hipLaunchKernelGGL(k_fq_cut, dim3(fq_grid(p_cap)), dim3(256), 0, st, (const FqMeta *)d_meta, (const long long *)d_off, (const uint64_t *)d_ls, max_pairs, max_bases, d_info, fq->bases.as<char>());
		hipLaunchKernelGGL(k_fq_extract, dim3(fq_grid(r_cap * kFqGroup)), dim3(256), 0, st, d_text, (const uint64_t *)d_ls, (const long long *)d_off, (const psvr_fastq_info_t *)d_info,
		                   fq->bases.as<char>(), fq->name_end.as<uint16_t>(), fq->ori.as<psvr_ori_t>());
	}
	PSVR_HIP(hipGetLastError());
	PSVR_HIP(hipMemcpyAsync(fq->h_info, d_info, sizeof(psvr_fastq_info_t), hipMemcpyDeviceToHost, st));
	drain.armed = false;
	PSVR_HIP(hipStreamSynchronize(st));
	fq->last = *info = *fq->h_info;
	fq->valid = true, fq->n_text = n_bytes;
	return PSVR_OK;
}

extern "C" int psvr_fastq_parse(psvr_fastq_t *fq, const char *text, int64_t n_bytes, int at_end, int64_t max_pairs, int64_t max_bases, psvr_fastq_info_t *info)
{
	if (psvr_device_count() <= 0) return fq_no_device();
	if (!fq || !info || n_bytes < 0 || max_pairs < 0 || (n_bytes > 0 && !text)) return set_error(PSVR_ERR_ARG, "psvr_fastq_parse: bad argument");
	return fq_parse_from("psvr_fastq_parse", fq, text, hipMemcpyHostToDevice, n_bytes, at_end, max_pairs, max_bases, info);
}

extern "C" int psvr_fastq_parse_signal(psvr_fastq_t *fq, const psvr_signal_t *sg, int64_t first_byte, int64_t max_pairs, int64_t max_bases, psvr_fastq_info_t *info)
{
	if (psvr_device_count() <= 0) return fq_no_device();
	if (!fq || !sg || !info || max_pairs < 0) return set_error(PSVR_ERR_ARG, "psvr_fastq_parse_signal: bad argument");
	if (!sg->win_valid) return set_error(PSVR_ERR_ARG, "psvr_fastq_parse_signal: the signal object has no window");
	if (fq->device != sg->device) return set_error(PSVR_ERR_ARG, "psvr_fastq_parse_signal: the parser is on device %d, the signal object on device %d", fq->device, sg->device);
	if (first_byte < 0 || first_byte > sg->win_bytes) return set_error(PSVR_ERR_ARG, "psvr_fastq_parse_signal: first byte %lld of a window of %lld", (long long)first_byte, sg->win_bytes);
	// (the window is whole: psvr_signal_window waited for it)
	return fq_parse_from("psvr_fastq_parse_signal", fq, sg->window.as<char>() + first_byte, hipMemcpyDeviceToDevice, sg->win_bytes - first_byte, 1, max_pairs, max_bases, info);
}

extern "C" int psvr_fastq_text(const psvr_fastq_t *fq, void *dst, int64_t first, int64_t n)
{
	if (psvr_device_count() <= 0) return fq_no_device();
	if (!fq || first < 0 || n < 0 || (n > 0 && !dst)) return set_error(PSVR_ERR_ARG, "psvr_fastq_text: bad argument");
	if (!fq->valid) return set_error(PSVR_ERR_ARG, "psvr_fastq_text: no parsed window");
	if (first > fq->n_text || n > fq->n_text - first) return set_error(PSVR_ERR_ARG, "psvr_fastq_text: bytes [%lld, %lld) of a text of %lld", (long long)first, (long long)(first + n), (long long)fq->n_text);
	if (n == 0) return PSVR_OK;
	PSVR_HIP(hipSetDevice(fq->device));
	PSVR_HIP(hipMemcpyAsync(dst, fq->text.as<char>() + first, (size_t)n, hipMemcpyDeviceToHost, fq->stream));
	PSVR_HIP(hipStreamSynchronize(fq->stream));
	return PSVR_OK;
}

extern "C" int psvr_fastq_download(const psvr_fastq_t *fq, uint64_t *line_start, uint16_t *name_end, int64_t *base_off, psvr_ori_t *ori, char *bases)
{
	if (psvr_device_count() <= 0) return fq_no_device();
	if (!fq || !fq->valid) return set_error(PSVR_ERR_ARG, "psvr_fastq_download: no parsed window");
	PSVR_HIP(hipSetDevice(fq->device));
	const size_t P = (size_t)fq->last.n_pairs, R = 2 * P;
	hipStream_t st = fq->stream;
	StreamDrain drain{st};
	if (line_start) PSVR_HIP(hipMemcpyAsync(line_start, fq->line_start.p, (8 * P + 1) * 8, hipMemcpyDeviceToHost, st));
	if (name_end && R) PSVR_HIP(hipMemcpyAsync(name_end, fq->name_end.p, R * 2, hipMemcpyDeviceToHost, st));
	if (base_off) PSVR_HIP(hipMemcpyAsync(base_off, fq->base_off.p, (R + 1) * 8, hipMemcpyDeviceToHost, st));
	if (ori && R) PSVR_HIP(hipMemcpyAsync(ori, fq->ori.p, R * sizeof(psvr_ori_t), hipMemcpyDeviceToHost, st));
	if (bases) PSVR_HIP(hipMemcpyAsync(bases, fq->bases.p, (size_t)fq->last.total_bases + 1, hipMemcpyDeviceToHost, st));
	drain.armed = false;
	PSVR_HIP(hipStreamSynchronize(st));
	return PSVR_OK;
}
