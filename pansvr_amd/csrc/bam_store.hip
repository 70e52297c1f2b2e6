// bam_store.hip -- psvr_bam_store_* (include/psvr_engine.h): the main BAM file's records kept in HBM until the input ends, ordered there and
// handed to the device-resident BGZF stream (bgzf_stream.hip) in sorted order: the records of `panSVR aln --sort-device` never visit the host.
//   the records   lie in chunks of device memory that are allocated once and never moved (SortRecords::kChunk's idea); a range that is
//                 appended lies in one chunk, so a record is one address.  Records the encoder left in HBM are copied device to device
//                 (k_store_copy, k_bs_append's shape), host bytes are uploaded in place
//   the table     per record its address, its psvr_bam_rec_meta_t (the bin recomputed from position and CIGAR span) and samtools' key (what
//                 a record is, its span, bin and key: bam_record.h, the rules SortRecords runs on the host), built
//                 on the device for both sources: k_store_count walks the block_size chain of every pair of the range (bounded by the pair's
//                 own bytes), the scan of scan.h gives every pair its first slot, k_store_fill walks again and writes the entries
//   the counts    records, bytes of the current chunk in use and bytes in all live in ctl[] on the device; an append from an emitter queues
//                 count -> scan -> fill -> copy -> commit without the host having seen a length.  The host's copies are exact again after
//                 the next call that waits (info, a host append, order, download)
//   order         the keys sorted where they lie (sort_device.h), then per rank the source address, the meta and the exclusive scan of the
//                 lengths: where every record goes in the sorted stream, on the device for the gather and on the host for the window sizes
//   order_names   the same with name order (name_sort.hip: the names are read where the records lie, through the table's addresses; the keys'
//                 array is the runs' key buffer), for `panSVR sort --nsort-device`
//   the gather    k_store_gather: a group of 16 lanes per record, four records per wavefront; 16-byte stores aligned on the destination,
//                 16-byte loads from the unaligned source, at most 15 head and 15 tail bytes as byte stores, the bin patched in registers
// Bounds: a range that leaves the emitter's bytes or the chunk's room, a chain that leaves its pair, a block_size below 32 (or of 2 GiB and
// more), a CIGAR that leaves its record, a table without room: the launch that notices raises ctl[3], and every later launch of this and of
// all later appends does nothing.  The next call that waits sees the flag and marks the store unusable: from then on every call answers
// PSVR_ERR_DEVICE.  Everything runs under DfwCtx's mutex on its stream (bgzf_members.h), as the BGZF stream's calls do: the two are
// serialised, and psvr_bam_store_stream writes the stream's pending bytes directly (bgzf_stream_run.h).
//   from a BAM file  psvr_bam_store_append_bgzf: whole BGZF members are uploaded and inflated, a wavefront per member (inflate_device.h), straight
//                 into the chunk, behind everything inflated into it so far.  Where the records begin is found there too (bam_chain_device.h): a
//                 wavefront per segment guesses and walks (k_chain_guess), one wavefront settles the guesses (k_chain_settle), and the entries
//                 of the segments are the "pairs" of k_store_count / k_store_fill: the table is built by the same kernels, the bytes lie where
//                 they stay.  What is behind the last whole record (the tail: the start of a record that the next call completes) stays in
//                 the chunk behind its count, and the next call inflates right behind it; a call that does not fit the chunk moves the tail
//                 to a fresh one.  The call waits for the members' statuses and the chain's result: the host's counts are exact between calls.
#include <hip/hip_runtime.h>
#include <stdlib.h>
#include <algorithm>
#include <memory>
#include <vector>
#include "../../include/psvr_engine.h"
#include "common.h"
#include "scan.h"
#include "sort_device.h"
#include "bam_emit_run.h"
#include "bgzf_members.h"
#include "bgzf_stream_run.h"
#include "inflate_layout.h"
#include "bam_record.h"
#include "bam_chain_device.h"
#include "copy_aligned_device.h"
#include "bam_store_run.h"

namespace psvr {

static const size_t kStoreChunk = (size_t)256 << 20;
static const long long kStoreSeg = 16 << 10;                 // append_bgzf: a segment of the record-chain finder (PSVR_BAM_STORE_SEG_BYTES)

// the range of a run that an append takes: bytes[pair_off[first], pair_off[first + n_pairs]); state == nullptr: every pair is walked
struct StoreSrc {
	const uint8_t *bytes;
	long long n_bytes;
	const long long *pair_off;
	const uint8_t *state;
	long long first, n_pairs;
};

// the range itself: inside the run, and short enough for the chunk's room behind what is in use
__device__ inline bool st_range(const StoreSrc &S, const long long *ctl, long long room, long long *s0, long long *s1)
{
	*s0 = S.pair_off[S.first], *s1 = S.pair_off[S.first + S.n_pairs];
	return *s0 >= 0 && *s0 <= *s1 && *s1 <= S.n_bytes && ctl[1] >= 0 && ctl[1] <= room && *s1 - *s0 <= room - ctl[1];
}
// What the store takes, for the kernels' walks and the host's pre-walk alike: a whole record by the formatter's rule (bam_record.h, as
// SortRecords::add_stream), no longer than the cap (the lengths go through an int32 scan); `avail` bytes are there from rec on
enum { kStoreRecFine = 0, kStoreRecMalformed = 1, kStoreRecTooLong = 2 };
__host__ __device__ inline int st_record(const uint8_t *rec, long long avail)
{
	if (!bam_rec_frame(rec, (uint64_t)avail) || !bam_rec_cigar_inside(rec)) return kStoreRecMalformed;
	return bam_u32(rec) > kBamRecStoreMaxBlock ? kStoreRecTooLong : kStoreRecFine;
}

// records of pair first + i -> cnt[i] (cnt[n_pairs] = 0: the scan's last entry is the total); a lane per pair
__global__ __launch_bounds__(256) void k_store_count(StoreSrc S, long long *ctl, long long room, int32_t *cnt)
{
	const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
	if (i > S.n_pairs) return;
	long long s0, s1;
	const bool fine = ctl[3] == 0 && st_range(S, ctl, room, &s0, &s1);
	int32_t c = 0;
	bool refuse = !fine && i == 0;
	if (fine && i < S.n_pairs) {
		const long long a = S.pair_off[S.first + i], b = S.pair_off[S.first + i + 1];
		if (a < s0 || a > b || b > s1) refuse = true;
		else if (S.state && S.state[S.first + i] != 1) refuse = a != b;      // only a written pair has bytes
		else {
			long long at = a;
			while (at < b) {
				if (st_record(S.bytes + at, b - at) != kStoreRecFine) { refuse = true; break; }
				at += 4 + (long long)bam_u32(S.bytes + at), ++c;
			}
		}
	}
	if (refuse) ctl[3] = 1, c = 0;
	cnt[i] = c;
}

// the table's entries of the range; a lane per pair walks its records again
__global__ __launch_bounds__(256) void k_store_fill(StoreSrc S, long long *ctl, long long room, const long long *off, long long cap_rec, const uint8_t *chunk,
                                                    uint64_t *addr, psvr_bam_rec_meta_t *meta, uint64_t *key)
{
	const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
	long long s0, s1;
	if (ctl[3] != 0 || !st_range(S, ctl, room, &s0, &s1)) return;
	const long long n0 = ctl[0];
	if (n0 < 0 || off[S.n_pairs] > cap_rec - n0) {           // (the same for every lane of the launch)
		if (i == 0) ctl[3] = 1;
		return;
	}
	if (i >= S.n_pairs || (S.state && S.state[S.first + i] != 1)) return;
	const long long b = S.pair_off[S.first + i + 1];
	long long at = S.pair_off[S.first + i], slot = n0 + off[i];
	const long long last = n0 + off[i + 1];
	while (at < b && slot < last) {
		const uint8_t *r = S.bytes + at;
		if (st_record(r, b - at) != kStoreRecFine) return;   // (k_store_count has seen every record of the pair: never)
		psvr_bam_rec_meta_t m;
		bam_rec_derived(r, &m);
		m.index = (uint32_t)slot, m.pad = 0;
		meta[slot] = m;
		addr[slot] = (uint64_t)(uintptr_t)(chunk + ctl[1] + (at - s0));
		key[slot] = bam_sort_key(m.tid, m.pos, m.flag);
		if (!bam_key_exact(m.pos)) ctl[4] = 1;
		at += m.len, ++slot;
	}
}

// the range's bytes behind what the chunk holds: k_bs_append's copy (copy_aligned_device.h)
__global__ __launch_bounds__(256) void k_store_copy(StoreSrc S, const long long *ctl, long long room, uint8_t *__restrict__ chunk)
{
	long long s0, s1;
	if (ctl[3] != 0 || !st_range(S, ctl, room, &s0, &s1)) return;
	if (s1 == s0) return;
	copy_aligned_grid(S.bytes + s0, chunk + ctl[1], s1 - s0);
}

// the append counts: one lane, behind everything of the append that read the counts
__global__ void k_store_commit(StoreSrc S, long long *ctl, long long room, const long long *off)
{
	long long s0, s1;
	if (ctl[3] != 0 || !st_range(S, ctl, room, &s0, &s1)) return;
	ctl[0] += off[S.n_pairs], ctl[1] += s1 - s0, ctl[2] += s1 - s0;
}

// ---- append_bgzf: the members inflated into the chunk, and where the records begin in what they hold
// a wavefront per member, k_bgzf_inflate's body (inflate.hip); out is the chunk behind everything inflated into it so far
__global__ __launch_bounds__(64) void k_store_inflate(const uint8_t *__restrict__ in, const InfMember *__restrict__ mem, uint8_t *out, int32_t *status)
{
	__shared__ InfLds lds;
	const InfMember m = mem[blockIdx.x];
	const int rc = inf_member<64>(in + m.in_off, m.bsize, m.hdr, out + m.out_off, m.isize, &lds, (int)threadIdx.x);
	if (threadIdx.x == 0) status[blockIdx.x] = rc;
}
// a wavefront per segment of bytes[0, end) (four to a workgroup): its guess and the walk from it
__global__ __launch_bounds__(256) void k_chain_guess(const uint8_t *__restrict__ bytes, long long end, long long seg, int32_t n_ref, long long n_seg, ChainSeg *sg)
{
	const long long s = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
	if (s >= n_seg) return;                                  // (the whole wavefront)
	chain_guess<64>(bytes, end, seg, 0, n_ref, s, sg, (int)(threadIdx.x & 63u));
}
// one wavefront: the guesses settled into entry[0 .. n_seg], the result for the host
__global__ __launch_bounds__(64) void k_chain_settle(const uint8_t *__restrict__ bytes, long long end, long long seg, long long n_seg, const ChainSeg *sg, long long *entry, int32_t *cnt,
                                                     ChainResult *res)
{
	const ChainResult R = chain_settle<64>(bytes, end, seg, 0, n_seg, sg, entry, cnt, (int)threadIdx.x);
	if (threadIdx.x == 0) *res = R;
}
// bytes at the front of a file's first call that are no records (the BAM header's remainder) stay in the chunk, in front of the records
__global__ void k_store_skip(long long *ctl, long long skip)
{
	if (ctl[3] == 0) ctl[1] += skip;
}

// per list position r (a sorted rank, or the append index when order == nullptr and n_order == 0): address, meta and length of its record
__global__ __launch_bounds__(256) void k_store_rank(const uint32_t *order, const uint64_t *addr, const psvr_bam_rec_meta_t *meta, long long n, uint64_t *g_src, psvr_bam_rec_meta_t *smeta,
                                                    int32_t *slen)
{
	const long long r = (long long)blockIdx.x * 256 + threadIdx.x;
	if (r > n) return;
	if (r == n) { slen[r] = 0; return; }
	const long long i = order ? (long long)order[r] : r;
	if (i >= n) { slen[r] = 0; return; }                     // (an order is a permutation: never)
	const psvr_bam_rec_meta_t m = meta[i];
	slen[r] = (int32_t)m.len;
	if (g_src) g_src[r] = addr[i];
	if (smeta) smeta[r] = m;
}

__device__ inline void st_put_byte(uint4 &x, uint32_t idx, uint32_t val)   // byte idx (0..15) of x, without indexing it
{
	const uint32_t sh = (idx & 3u) * 8u, keep = ~(0xffu << sh), b = (val & 0xffu) << sh, w = idx >> 2;
	x.x = w == 0 ? (x.x & keep) | b : x.x;
	x.y = w == 1 ? (x.y & keep) | b : x.y;
	x.z = w == 2 ? (x.z & keep) | b : x.z;
	x.w = w == 3 ? (x.w & keep) | b : x.w;
}
__device__ inline uint8_t st_rec_byte(const uint8_t *s, uint32_t k, uint32_t bin) { return k == 14 ? (uint8_t)bin : k == 15 ? (uint8_t)(bin >> 8) : s[k]; }

// The gather: record first + r of the list goes to dst + (off[first + r] - base), with its bin (bytes 14 and 15) replaced.  16 lanes per record,
// 16 records per workgroup and step; a lane stores 16 aligned bytes at a time (two loads in flight), the group loops over a long record;
// the head up to the destination's next 16-byte boundary and the tail are byte stores of the group's first lanes.  The caller has made sure
// that dst holds off[first + n] - base bytes; a record's loads stay inside the record.
__global__ __launch_bounds__(256) void k_store_gather(const uint64_t *__restrict__ src, const psvr_bam_rec_meta_t *__restrict__ M, const long long *__restrict__ off, long long first,
                                                      long long n, long long base, uint8_t *__restrict__ dst)
{
	const uint32_t sub = threadIdx.x & 15u;
	for (long long r = (long long)blockIdx.x * 16 + (threadIdx.x >> 4); r < n; r += (long long)gridDim.x * 16) {
		const long long i = first + r;
		const uint8_t *s = (const uint8_t *)(uintptr_t)src[i];
		uint8_t *d = dst + (off[i] - base);
		const uint32_t len = M[i].len, bin = M[i].bin;
		const uint32_t lead = copy_lead(d, len), nv = (len - lead) / 16u, done = lead + 16u * nv;
		for (uint32_t v = sub; v < nv; v += 32u) {
			const bool two = v + 16u < nv;
			uint4 x, y = {0, 0, 0, 0};
			__builtin_memcpy(&x, s + lead + 16u * v, 16);
			if (two) __builtin_memcpy(&y, s + lead + 16u * (v + 16u), 16);
			if (v == 0) {                                    // record bytes [lead, lead + 16): the only vector that can hold the bin
				if (lead <= 14u) st_put_byte(x, 14u - lead, bin);
				if (lead <= 15u) st_put_byte(x, 15u - lead, bin >> 8);
			}
			*(uint4 *)(d + lead + 16u * v) = x;
			if (two) *(uint4 *)(d + lead + 16u * (v + 16u)) = y;
		}
		if (sub < lead) d[sub] = st_rec_byte(s, sub, bin);
		if (sub < len - done) d[done + sub] = st_rec_byte(s, done + sub, bin);
	}
}

// drop: the table's entries [n_front, n) slide to the front of its other half, index counting from the first one kept; the dropped records'
// bytes are added up into ctl[5]
__global__ __launch_bounds__(256) void k_store_slide(const uint64_t *addr, const psvr_bam_rec_meta_t *meta, const uint64_t *key, long long n_front, long long n, uint64_t *addr2,
                                                     psvr_bam_rec_meta_t *meta2, uint64_t *key2, long long *ctl)
{
	__shared__ unsigned long long sum;
	if (threadIdx.x == 0) sum = 0;
	__syncthreads();
	unsigned long long mine = 0;
	for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long long)gridDim.x * 256) {
		psvr_bam_rec_meta_t m = meta[i];
		if (i < n_front) { mine += m.len; continue; }
		m.index = (uint32_t)(i - n_front);
		addr2[i - n_front] = addr[i], meta2[i - n_front] = m, key2[i - n_front] = key[i];
	}
	if (mine) atomicAdd(&sum, mine);
	__syncthreads();
	if (threadIdx.x == 0 && sum) atomicAdd((unsigned long long *)&ctl[5], sum);
}
__global__ void k_store_dropped(long long *ctl, long long n_front)
{
	if (ctl[3] != 0) return;
	ctl[0] -= n_front, ctl[2] -= ctl[5];
}

// ---- host side: everything below runs under DfwCtx's mutex, on its stream, bound to the store's device
static int st_bad()
{
	return set_error(PSVR_ERR_DEVICE, "psvr_bam_store: the store is unusable: an append was refused on the device (a range or a record chain out of bounds) and was not made, or an earlier call failed while it changed the store");
}
static int st_open_tail(const char *who, const psvr_bam_store *st)
{
	return set_error(PSVR_ERR_ARG, "%s: the last append_bgzf ended %lld bytes into a record: only append_bgzf can complete it", who, st->tail);
}
static int st_no_device() { return set_error(PSVR_ERR_DEVICE, "no HIP device visible: the engine has no CPU path"); }
static int st_refresh(psvr_bam_store *st, DfwCtx &c, bool wait)   // the counts as the device holds them; an unusable store says so
{
	if (st->bad) return st_bad();
	if (st->exact) {
		if (wait && hipStreamSynchronize(c.stream) != hipSuccess) { st->bad = true; return st_bad(); }
		return PSVR_OK;
	}
	hipError_t e = hipMemcpyAsync(st->h_ctl, st->ctl.p, 5 * 8, hipMemcpyDeviceToHost, c.stream);
	if (e == hipSuccess) e = hipStreamSynchronize(c.stream);
	if (e != hipSuccess || st->h_ctl[3]) { st->bad = true; return st_bad(); }
	st->n_rec = st->rec_upper = st->h_ctl[0], st->fill = st->fill_upper = st->h_ctl[1], st->n_bytes = st->h_ctl[2];
	st->key_exact = st->h_ctl[4] == 0, st->exact = true;
	return PSVR_OK;
}
int store_refresh(psvr_bam_store *st, DfwCtx &c, bool wait) { return st_refresh(st, c, wait); }
// a chunk whose room behind `used` holds `need` bytes: the last one, or a fresh one (nothing stored moves)
static int st_chunk(psvr_bam_store *st, DfwCtx &c, long long used, long long need)
{
	if (!st->chunks.empty() && (long long)st->chunks.back()->bytes - used >= need) return PSVR_OK;
	std::unique_ptr<DevBuf> b;
	// (whole 8-byte words: k_name_chunk loads the aligned words that a name touches, also of a record that ends with its name at the chunk's end)
	const size_t n = (((size_t)need > st->chunk_bytes ? (size_t)need : st->chunk_bytes) + 7) / 8 * 8;
	if (st->spare && st->spare->bytes >= n) b = std::move(st->spare);   // (what psvr_bam_store_drop kept)
	else b.reset(new DevBuf);
	if (!b->p && b->alloc(n) != hipSuccess) {
		(void)hipGetLastError();
		return set_error(PSVR_ERR_NOMEM, "psvr_bam_store: device allocation failed for a chunk of %zu bytes (%lld bytes of records are stored)", n, st->n_bytes);
	}
	PSVR_HIP(hipMemsetAsync(st->ctl.as<long long>() + 1, 0, 8, c.stream));   // (behind every queued append that counts in the old chunk)
	st->chunks.push_back(std::move(b));
	st->fill = st->fill_upper = 0;
	return PSVR_OK;
}
// the table holds `need` records; the entries of the records stored are kept
static int st_table(psvr_bam_store *st, DfwCtx &c, long long need)
{
	if (need <= st->cap_rec) return PSVR_OK;
	long long cap = st->cap_rec ? st->cap_rec : 1 << 16;
	while (cap < need) cap *= 2;
	DevBuf a, m, k;
	if (a.alloc((size_t)cap * 8) || m.alloc((size_t)cap * sizeof(psvr_bam_rec_meta_t)) || k.alloc((size_t)cap * 8)) {
		(void)hipGetLastError();
		return set_error(PSVR_ERR_NOMEM, "psvr_bam_store: device allocation failed for a table of %lld records (%zu bytes)", cap, (size_t)cap * 48);
	}
	if (st->rec_upper) {
		PSVR_HIP(hipMemcpyAsync(a.p, st->addr.p, (size_t)st->rec_upper * 8, hipMemcpyDeviceToDevice, c.stream));
		PSVR_HIP(hipMemcpyAsync(m.p, st->meta.p, (size_t)st->rec_upper * sizeof(psvr_bam_rec_meta_t), hipMemcpyDeviceToDevice, c.stream));
		PSVR_HIP(hipMemcpyAsync(k.p, st->key.p, (size_t)st->rec_upper * 8, hipMemcpyDeviceToDevice, c.stream));
	}
	PSVR_HIP(hipStreamSynchronize(c.stream));
	std::swap(a.p, st->addr.p), std::swap(a.bytes, st->addr.bytes);
	std::swap(m.p, st->meta.p), std::swap(m.bytes, st->meta.bytes);
	std::swap(k.p, st->key.p), std::swap(k.bytes, st->key.bytes);
	st->cap_rec = cap;
	return PSVR_OK;
}
static int st_scratch(psvr_bam_store *st, long long n_pairs)
{
	if (st->cnt.ensure((size_t)(n_pairs + 1) * 4) || st->off.ensure((size_t)(n_pairs + 1) * 8) || st->tmp.ensure(scan_tmp_bytes(1, n_pairs + 1))) {
		(void)hipGetLastError();
		return set_error(PSVR_ERR_NOMEM, "psvr_bam_store: device allocation failed for the scratch of an append of %lld pairs", n_pairs);
	}
	return PSVR_OK;
}
// count -> scan -> fill -> [copy] -> commit, queued
static int st_queue_append(psvr_bam_store *st, DfwCtx &c, const StoreSrc &S, bool copy)
{
	DevBuf &chunk = *st->chunks.back();
	const long long room = (long long)chunk.bytes, n1 = S.n_pairs + 1;
	const unsigned grid = (unsigned)((n1 + 255) / 256);
	long long *ctl = st->ctl.as<long long>();
	hipLaunchKernelGGL(k_store_count, dim3(grid), dim3(256), 0, c.stream, S, ctl, room, st->cnt.as<int32_t>());
	ScanSet X = {};
	X.cnt[0] = st->cnt.as<int32_t>(), X.out[0] = st->off.as<long long>(), X.stride[0] = 1;
	scan_launch(X, 1, n1, st->tmp.as<long long>(), c.stream);
	hipLaunchKernelGGL(k_store_fill, dim3(grid), dim3(256), 0, c.stream, S, ctl, room, (const long long *)st->off.p, st->cap_rec, chunk.as<uint8_t>(), st->addr.as<uint64_t>(),
	                   st->meta.as<psvr_bam_rec_meta_t>(), st->key.as<uint64_t>());
	if (copy) {
		const long long nv = S.n_bytes / 16 + 1;
		const unsigned g = (unsigned)(nv / 256 + 1 < 2048 ? nv / 256 + 1 : 2048);
		hipLaunchKernelGGL(k_store_copy, dim3(g), dim3(256), 0, c.stream, S, (const long long *)ctl, room, chunk.as<uint8_t>());
	}
	hipLaunchKernelGGL(k_store_commit, dim3(1), dim3(1), 0, c.stream, S, ctl, room, (const long long *)st->off.p);
	PSVR_HIP(hipGetLastError());
	return PSVR_OK;
}
static void st_gather(DfwCtx &c, const uint64_t *src, const psvr_bam_rec_meta_t *M, const long long *off, long long first, long long n, long long base, uint8_t *dst)
{
	const long long g = (n + 15) / 16;
	hipLaunchKernelGGL(k_store_gather, dim3((unsigned)(g < 4096 ? g : 4096)), dim3(256), 0, c.stream, src, M, off, first, n, base, dst);
}

} // namespace psvr

using namespace psvr;

extern "C" int psvr_bam_store_create(int device, psvr_bam_store_t **out)
{
	if (!out) return set_error(PSVR_ERR_ARG, "psvr_bam_store_create: null argument");
	if (psvr_device_count() <= 0) return st_no_device();
	DfwCtx &c = dfw_ctx();
	std::lock_guard<std::mutex> lk(c.mu);
	if (int rc = dfw_bind(c, device)) return rc;
	psvr_bam_store *st = new psvr_bam_store;
	st->device = device;
	// PSVR_BAM_STORE_CHUNK_BYTES: the size of a chunk (the tests fill several small ones)
	const char *e_chunk = getenv("PSVR_BAM_STORE_CHUNK_BYTES");
	st->chunk_bytes = e_chunk && atoll(e_chunk) > 0 ? (size_t)atoll(e_chunk) : kStoreChunk;
	// PSVR_BAM_STORE_SEG_BYTES: the segment of append_bgzf's record-chain finder (the tests make it small: few records, many segments)
	const char *e_seg = getenv("PSVR_BAM_STORE_SEG_BYTES");
	st->seg_bytes = e_seg && atoll(e_seg) > 0 ? std::max((long long)atoll(e_seg), kChainMinSeg) : kStoreSeg;
	hipError_t e = st->ctl.alloc(8 * 8);
	if (e == hipSuccess) e = hipHostMalloc((void **)&st->h_ctl, 8 * sizeof(long long) + sizeof(ChainResult), hipHostMallocDefault);
	if (e == hipSuccess) st->h_res = (ChainResult *)(st->h_ctl + 8);
	if (e == hipSuccess) e = hipMemsetAsync(st->ctl.p, 0, 8 * 8, c.stream);
	if (e == hipSuccess) e = hipStreamSynchronize(c.stream);
	if (e != hipSuccess) {
		if (st->h_ctl) (void)hipHostFree(st->h_ctl);
		delete st;
		return set_error(PSVR_ERR_DEVICE, "psvr_bam_store_create: %s", hipGetErrorString(e));
	}
	*out = st;
	return PSVR_OK;
}

extern "C" void psvr_bam_store_destroy(psvr_bam_store_t *st)
{
	if (!st) return;
	DfwCtx &c = dfw_ctx();
	std::lock_guard<std::mutex> lk(c.mu);
	(void)hipSetDevice(st->device);
	if (c.stream) (void)hipStreamSynchronize(c.stream);      // (an append may still be queued)
	if (st->h_ctl) (void)hipHostFree(st->h_ctl);
	delete st;                                               // (its DevBufs free themselves)
}

extern "C" int psvr_bam_store_append(psvr_bam_store_t *st, const void *bytes, int64_t n_bytes)
{
	if (!st || n_bytes < 0 || (n_bytes > 0 && !bytes)) return set_error(PSVR_ERR_ARG, "psvr_bam_store_append: bad argument");
	if (st->bad) return st_bad();
	if (st->ordered) return set_error(PSVR_ERR_ARG, "psvr_bam_store_append: the store has been ordered, it takes no more records");
	if (st->tail) return st_open_tail("psvr_bam_store_append", st);
	// the kernels' own rule (st_record), before anything is uploaded; every record is a "pair" of the device's walk
	const uint8_t *p = (const uint8_t *)bytes;
	std::vector<long long> off(1, 0);
	for (size_t i = 0, n = (size_t)n_bytes; i < n;) {
		const int v = st_record(p + i, (long long)(n - i));
		if (v == kStoreRecMalformed) return set_error(PSVR_ERR_ARG, "psvr_bam_store_append: malformed record at byte %zu of %zu (nothing was appended)", i, n);
		const uint32_t bs = bam_u32(p + i);
		if (v == kStoreRecTooLong) return set_error(PSVR_ERR_UNSUPPORTED, "psvr_bam_store_append: a record of %u bytes at byte %zu (2 GiB and more are not stored; nothing was appended)", bs, i);
		i += 4 + (size_t)bs;
		off.push_back((long long)i);
	}
	if (n_bytes == 0) return PSVR_OK;
	DfwCtx &c = dfw_ctx();
	std::lock_guard<std::mutex> lk(c.mu);
	if (int rc = dfw_bind(c, st->device)) return rc;
	if (int rc = st_refresh(st, c, false)) return rc;            // (where the bytes go is the chunk's count)
	const long long n_rec = (long long)off.size() - 1;
	if (int rc = st_chunk(st, c, st->fill, n_bytes)) return rc;
	if (int rc = st_table(st, c, st->n_rec + n_rec)) return rc;
	if (int rc = st_scratch(st, n_rec)) return rc;
	if (st->poff.ensure(off.size() * 8)) { (void)hipGetLastError(); return set_error(PSVR_ERR_NOMEM, "psvr_bam_store_append: device allocation failed for %zu record offsets", off.size()); }
	// (bytes behind the chunk's count are not part of the store: a failure before the commit leaves it as it was)
	uint8_t *at = st->chunks.back()->as<uint8_t>() + st->fill;
	hipError_t e = hipMemcpyAsync(st->poff.p, off.data(), off.size() * 8, hipMemcpyHostToDevice, c.stream);
	if (e == hipSuccess) e = hipMemcpyAsync(at, bytes, (size_t)n_bytes, hipMemcpyHostToDevice, c.stream);
	if (e != hipSuccess) { (void)hipStreamSynchronize(c.stream); return set_error(PSVR_ERR_DEVICE, "psvr_bam_store_append: %s", hipGetErrorString(e)); }
	// the records are walked where they lie now: the run is the upload, its offsets count from its start (the fill kernel adds the chunk's count)
	const StoreSrc S = {at, (long long)n_bytes, (const long long *)st->poff.p, nullptr, 0, n_rec};
	st->exact = false;
	int rc = st_queue_append(st, c, S, false);
	if (!rc) rc = st_refresh(st, c, true);                       // the caller's bytes are free again, and the counts are the host's
	if (rc) { st->bad = true; return rc; }
	return PSVR_OK;
}

extern "C" int psvr_bam_store_append_emit(psvr_bam_store_t *st, const psvr_bam_emit_t *em, int64_t first_pair, int64_t n_pairs)
{
	if (!st || !em) return set_error(PSVR_ERR_ARG, "psvr_bam_store_append_emit: null argument");
	if (st->bad) return st_bad();
	if (st->ordered) return set_error(PSVR_ERR_ARG, "psvr_bam_store_append_emit: the store has been ordered, it takes no more records");
	if (st->tail) return st_open_tail("psvr_bam_store_append_emit", st);
	if (!em->valid) return set_error(PSVR_ERR_ARG, "psvr_bam_store_append_emit: no emitted run of pairs");
	if (em->device != st->device) return set_error(PSVR_ERR_ARG, "psvr_bam_store_append_emit: the records were encoded on device %d, the store is on device %d", em->device, st->device);
	if (first_pair < 0 || n_pairs < 0 || first_pair > em->n_pairs || n_pairs > em->n_pairs - first_pair)
		return set_error(PSVR_ERR_ARG, "psvr_bam_store_append_emit: pairs [%lld, %lld) are not in the emitted run (%lld pairs)", (long long)first_pair, (long long)(first_pair + n_pairs), (long long)em->n_pairs);
	if (n_pairs == 0 || em->n_bytes == 0) return PSVR_OK;
	DfwCtx &c = dfw_ctx();
	std::lock_guard<std::mutex> lk(c.mu);
	if (int rc = dfw_bind(c, st->device)) return rc;
	// the range's length and its records are known on the device only: room for the whole run, in the chunk and in the table, behind the
	// most that can be there.  Until the next call that waits every append adds the run's size to those bounds
	const long long run_records = em->h_back[1] > 0 ? em->h_back[1] : 0;
	if (int rc = st_chunk(st, c, st->fill_upper, em->n_bytes)) return rc;
	if (int rc = st_table(st, c, st->rec_upper + run_records)) return rc;
	if (int rc = st_scratch(st, n_pairs)) return rc;
	const StoreSrc S = {em->bytes.as<uint8_t>(), (long long)em->n_bytes, (const long long *)em->pair_off.p, em->state.as<uint8_t>(), (long long)first_pair, (long long)n_pairs};
	st->exact = false, st->fill_upper += em->n_bytes, st->rec_upper += run_records;
	if (int rc = st_queue_append(st, c, S, true)) { st->bad = true; return rc; }
	return PSVR_OK;
}

extern "C" int psvr_bam_store_append_bgzf(psvr_bam_store_t *st, const void *in_, int64_t n_bytes, int64_t skip, int32_t n_ref, int64_t *in_used, int64_t *bad_member)
{
	if (psvr_device_count() <= 0) return st_no_device();
	if (!st || n_bytes < 0 || (n_bytes > 0 && !in_) || skip < 0 || !in_used) return set_error(PSVR_ERR_ARG, "psvr_bam_store_append_bgzf: bad argument");
	*in_used = 0;
	if (bad_member) *bad_member = -1;
	if (st->bad) return st_bad();
	if (st->ordered) return set_error(PSVR_ERR_ARG, "psvr_bam_store_append_bgzf: the store has been ordered, it takes no more records");
	const uint8_t *in = (const uint8_t *)in_;
	// the BSIZE chain, by psvr_bgzf_decompress's rules: whole members only, a header that is none ends the call before anything is done
	std::vector<InfMember> &mem = st->h_mem;
	mem.clear();
	long long used = 0, total = 0;
	const long long bad = inf_layout(in, n_bytes, mem, &used, &total);
	const long long nm = (long long)mem.size();
	auto io_error = [&](long long m, int status) {
		if (bad_member) *bad_member = m;
		return set_error(PSVR_ERR_IO, "psvr_bam_store_append_bgzf: corrupt BGZF block: member %lld at byte %lld (status %d; nothing of this call was appended)", m, m < nm ? mem[(size_t)m].in_off : used, status);
	};
	if (bad >= 0) return io_error(bad, kInfHeader);
	if (nm == 0) return PSVR_OK;                                 // (no whole member: the caller's to complete)
	if (skip > 0 && (skip >= (long long)mem[0].isize || st->tail))
		return set_error(PSVR_ERR_ARG, "psvr_bam_store_append_bgzf: skip = %lld: it lies inside the first member (%lld bytes) of a call that continues no record", (long long)skip,
		                 (long long)mem[0].isize);
	*in_used = used;
	DfwCtx &c = dfw_ctx();
	std::lock_guard<std::mutex> lk(c.mu);
	if (int rc = dfw_bind(c, st->device)) return rc;
	if (int rc = st_refresh(st, c, false)) return rc;            // (where the bytes go is the chunk's count)
	// the stream of this call: the tail, then what the members hold, less the skipped bytes; it lies at chunk + fill + skip
	const long long end = st->tail + total - skip, n_seg = chain_segments(end, st->seg_bytes);
	if (st->zin.ensure((size_t)used) || st->zmem.ensure((size_t)nm * sizeof(InfMember)) || st->zstatus.ensure((size_t)nm * 4) || st->cseg.ensure((size_t)(n_seg + 1) * sizeof(ChainSeg)) ||
	    st->centry.ensure((size_t)(n_seg + 1) * 8) || st->ccnt.ensure((size_t)(n_seg + 1) * 4) || st->cres.ensure(sizeof(ChainResult))) {
		(void)hipGetLastError();
		return set_error(PSVR_ERR_NOMEM, "psvr_bam_store_append_bgzf: device allocation failed for a call of %lld bytes in %lld members and %lld segments", used, nm, n_seg);
	}
	const uint8_t *old_tail = st->tail ? st->chunks.back()->as<uint8_t>() + st->fill : nullptr;
	if (int rc = st_chunk(st, c, st->fill, st->tail + total)) return rc;
	uint8_t *base = st->chunks.back()->as<uint8_t>() + st->fill;
	StreamDrain drain{c.stream};
	if (old_tail && old_tail != base) PSVR_HIP(hipMemcpyAsync(base, old_tail, (size_t)st->tail, hipMemcpyDeviceToDevice, c.stream));   // a fresh chunk: at most one record moves
	st->h_status.assign((size_t)nm, -1);
	PSVR_HIP(hipMemcpyAsync(st->zin.p, in, (size_t)used, hipMemcpyHostToDevice, c.stream));
	PSVR_HIP(hipMemcpyAsync(st->zmem.p, mem.data(), (size_t)nm * sizeof(InfMember), hipMemcpyHostToDevice, c.stream));
	hipLaunchKernelGGL(k_store_inflate, dim3((unsigned)nm), dim3(64), 0, c.stream, st->zin.as<uint8_t>(), st->zmem.as<InfMember>(), base + st->tail, st->zstatus.as<int32_t>());
	const uint8_t *bytes = base + skip;
	if (n_seg) {
		hipLaunchKernelGGL(k_chain_guess, dim3((unsigned)((n_seg + 3) / 4)), dim3(256), 0, c.stream, bytes, end, st->seg_bytes, n_ref, n_seg, st->cseg.as<ChainSeg>());
		hipLaunchKernelGGL(k_chain_settle, dim3(1), dim3(64), 0, c.stream, bytes, end, st->seg_bytes, n_seg, (const ChainSeg *)st->cseg.p, st->centry.as<long long>(), st->ccnt.as<int32_t>(),
		                   st->cres.as<ChainResult>());
		PSVR_HIP(hipMemcpyAsync(st->h_res, st->cres.p, sizeof(ChainResult), hipMemcpyDeviceToHost, c.stream));
	}
	PSVR_HIP(hipGetLastError());
	PSVR_HIP(hipMemcpyAsync(st->h_status.data(), st->zstatus.p, (size_t)nm * 4, hipMemcpyDeviceToHost, c.stream));
	drain.armed = false;
	PSVR_HIP(hipStreamSynchronize(c.stream));
	// (bytes behind the chunk's count and the tail are not part of the store: a refused call leaves it as it was)
	for (long long i = 0; i < nm; ++i) if (st->h_status[(size_t)i] != kInfOk) { *in_used = 0; return io_error(i, st->h_status[(size_t)i]); }
	if (n_seg == 0) return PSVR_OK;
	const ChainResult R = *st->h_res;
	st->chain.segments += n_seg, st->chain.no_guess += R.no_guess, st->chain.wrong_guess += R.wrong_guess, st->chain.rewalked += R.rewalked;
	if (R.bad_seg >= 0) {                                        // the store's rule for a record chain that cannot be followed
		st->bad = true;
		return set_error(PSVR_ERR_DEVICE, "psvr_bam_store_append_bgzf: malformed BAM record at byte %lld of this call's stream, behind %lld whole records (the store is unusable from here on)",
		                 R.bad_at + (long long)skip - st->tail, R.total);
	}
	if (R.total < 0 || R.tail < 0 || R.tail > end) { st->bad = true; return st_bad(); }
	if (int rc = st_table(st, c, st->n_rec + R.total)) return rc;
	if (int rc = st_scratch(st, n_seg)) return rc;
	// the records are walked where they lie: the run is this call's stream, its "pairs" are the segments' entries
	const StoreSrc S = {bytes, end, (const long long *)st->centry.p, nullptr, 0, n_seg};
	const long long want_rec = st->n_rec + R.total, want_bytes = st->n_bytes + (end - R.tail);
	st->exact = false;
	if (skip) hipLaunchKernelGGL(k_store_skip, dim3(1), dim3(1), 0, c.stream, st->ctl.as<long long>(), (long long)skip);
	int rc = st_queue_append(st, c, S, false);
	if (!rc) rc = st_refresh(st, c, true);
	if (!rc && (st->n_rec != want_rec || st->n_bytes != want_bytes))
		rc = set_error(PSVR_ERR_DEVICE, "psvr_bam_store_append_bgzf: the table holds %lld records in %lld bytes, the chain has %lld in %lld", st->n_rec, st->n_bytes, want_rec, want_bytes);
	if (rc) { st->bad = true; return rc; }
	st->tail = R.tail;
	return PSVR_OK;
}

extern "C" int psvr_bam_store_chain_info(psvr_bam_store_t *st, psvr_bam_chain_info_t *info)
{
	if (psvr_device_count() <= 0) return st_no_device();
	if (!st) return set_error(PSVR_ERR_ARG, "psvr_bam_store_chain_info: null argument");
	DfwCtx &c = dfw_ctx();
	std::lock_guard<std::mutex> lk(c.mu);
	if (int rc = dfw_bind(c, st->device)) return rc;
	if (int rc = st_refresh(st, c, true)) return rc;
	if (info) *info = st->chain, info->tail_bytes = st->tail;
	return PSVR_OK;
}

extern "C" int psvr_bam_store_info(psvr_bam_store_t *st, psvr_bam_store_info_t *info)
{
	if (!st) return set_error(PSVR_ERR_ARG, "psvr_bam_store_info: null argument");
	DfwCtx &c = dfw_ctx();
	std::lock_guard<std::mutex> lk(c.mu);
	if (int rc = dfw_bind(c, st->device)) return rc;
	if (int rc = st_refresh(st, c, true)) return rc;
	if (info) info->n_records = st->n_rec, info->n_bytes = st->n_bytes, info->key_exact = st->key_exact ? 1 : 0, info->ordered = st->ordered;
	return PSVR_OK;
}

// what both orders share: the store can be ordered now, and its sorted table has room.  *done: nothing more to do (ordered this way already, or empty)
static int st_order_begin(psvr_bam_store *st, DfwCtx &c, int kind, const char *who, bool *done)
{
	*done = false;
	if (int rc = dfw_bind(c, st->device)) return rc;
	if (int rc = st_refresh(st, c, true)) return rc;
	if (st->ordered == kind) { *done = true; return PSVR_OK; }
	if (st->ordered) return set_error(PSVR_ERR_ARG, "%s: the store has been ordered %s already", who, st->ordered == 2 ? "by name" : "by coordinate");
	if (st->tail) return set_error(PSVR_ERR_ARG, "%s: truncated BAM stream: the last append_bgzf ended %lld bytes into a record", who, st->tail);
	if (kind == 1 && !st->key_exact) return set_error(PSVR_ERR_UNSUPPORTED, "%s: a position outside [-1, 2^31 - 2]: the 64-bit key does not order as samtools' comparator", who);
	if (st->n_rec >= (1ll << 32)) return set_error(PSVR_ERR_UNSUPPORTED, "%s: %lld records, the order is 32-bit (at most 2^32 - 1 records)", who, st->n_rec);
	if (st->keys_spent) return set_error(PSVR_ERR_DEVICE, "%s: an earlier order failed after it had begun to move the keys", who);
	const long long n = st->n_rec;
	st->h_rank_off.assign((size_t)n + 1, 0);
	if (n == 0) { st->ordered = kind, *done = true; return PSVR_OK; }
	if (st->g_src.alloc((size_t)n * 8) || st->smeta.alloc((size_t)n * sizeof(psvr_bam_rec_meta_t)) || st->slen.alloc((size_t)(n + 1) * 4) || st->rank_off.alloc((size_t)(n + 1) * 8) ||
	    st->tmp.ensure(scan_tmp_bytes(1, n + 1))) {
		(void)hipGetLastError();
		return set_error(PSVR_ERR_NOMEM, "%s: device allocation failed for the sorted table of %lld records (%zu bytes)", who, n, (size_t)n * 52);
	}
	return PSVR_OK;
}
// ... and the order applied: per rank the address, the meta and where the record goes in the sorted stream
static int st_order_apply(psvr_bam_store *st, DfwCtx &c, const uint32_t *d_order, int kind, const char *who)
{
	const long long n = st->n_rec;
	StreamDrain drain{c.stream};
	hipLaunchKernelGGL(k_store_rank, dim3((unsigned)((n + 256) / 256)), dim3(256), 0, c.stream, d_order, (const uint64_t *)st->addr.p, (const psvr_bam_rec_meta_t *)st->meta.p, n,
	                   st->g_src.as<uint64_t>(), st->smeta.as<psvr_bam_rec_meta_t>(), st->slen.as<int32_t>());
	ScanSet X = {};
	X.cnt[0] = st->slen.as<int32_t>(), X.out[0] = st->rank_off.as<long long>(), X.stride[0] = 1;
	scan_launch(X, 1, n + 1, st->tmp.as<long long>(), c.stream);
	PSVR_HIP(hipGetLastError());
	PSVR_HIP(hipMemcpyAsync(st->h_rank_off.data(), st->rank_off.p, (size_t)(n + 1) * 8, hipMemcpyDeviceToHost, c.stream));
	drain.armed = false;
	PSVR_HIP(hipStreamSynchronize(c.stream));
	if (st->h_rank_off[(size_t)n] != st->n_bytes) return set_error(PSVR_ERR_DEVICE, "%s: the sorted lengths add up to %lld bytes, the store holds %lld", who, st->h_rank_off[(size_t)n], st->n_bytes);
	st->S.release();                                              // (the order has been applied: its scratch and the keys go back)
	st->key.release(), st->slen.release();
	st->ordered = kind;
	return PSVR_OK;
}

extern "C" int psvr_bam_store_order(psvr_bam_store_t *st)
{
	const char *who = "psvr_bam_store_order";
	if (!st) return set_error(PSVR_ERR_ARG, "%s: null argument", who);
	DfwCtx &c = dfw_ctx();
	std::lock_guard<std::mutex> lk(c.mu);
	bool done = false;
	if (int rc = st_order_begin(st, c, 1, who, &done)) return rc;
	if (done) return PSVR_OK;
	const uint32_t *d_order = nullptr;
	if (int rc = sort_order_device(c.stream, st->n_rec, st->key.as<uint64_t>(), st->S, st->h_hist, &d_order, who)) {
		st->keys_spent = rc != PSVR_ERR_NOMEM;                     // (nothing has been launched when the scratch does not fit)
		return rc;
	}
	st->keys_spent = true;
	return st_order_apply(st, c, d_order, 1, who);
}

// name order: the names are read where the records lie (the table's addresses), the keys' array is the runs' key buffer
extern "C" int psvr_bam_store_order_names(psvr_bam_store_t *st)
{
	const char *who = "psvr_bam_store_order_names";
	if (psvr_device_count() <= 0) return st_no_device();
	if (!st) return set_error(PSVR_ERR_ARG, "%s: null argument", who);
	DfwCtx &c = dfw_ctx();
	std::lock_guard<std::mutex> lk(c.mu);
	bool done = false;
	if (int rc = st_order_begin(st, c, 2, who, &done)) return rc;
	if (done) return PSVR_OK;
	const NameSrc src = {(const uint64_t *)st->addr.p, nullptr, 0, nullptr, nullptr};
	NameScratch N;
	const uint32_t *d_order = nullptr;
	// the first k_name_chunk overwrites the coordinate keys; every allocation of the call comes before it (sort_device.h), so a call that
	// failed for want of memory has not written them, and N says whether a write was queued
	const int rc_sort = sort_order_names_device(c.stream, st->n_rec, src, st->key.as<uint64_t>(), N, st->S, st->h_hist, &d_order, who);
	st->keys_spent = N.keys_written;
	if (rc_sort) return rc_sort;
	return st_order_apply(st, c, d_order, 2, who);                 // (it waits: N's entries are free to go)
}

extern "C" int psvr_bam_store_meta(psvr_bam_store_t *st, int64_t first_rank, int64_t n, psvr_bam_rec_meta_t *meta)
{
	if (!st || (n > 0 && !meta)) return set_error(PSVR_ERR_ARG, "psvr_bam_store_meta: null argument");
	if (st->bad) return st_bad();
	if (!st->ordered) return set_error(PSVR_ERR_ARG, "psvr_bam_store_meta: the store has not been ordered");
	if (first_rank < 0 || n < 0 || first_rank > st->n_rec || n > st->n_rec - first_rank)
		return set_error(PSVR_ERR_ARG, "psvr_bam_store_meta: ranks [%lld, %lld) of %lld records", (long long)first_rank, (long long)(first_rank + n), st->n_rec);
	if (n == 0) return PSVR_OK;
	DfwCtx &c = dfw_ctx();
	std::lock_guard<std::mutex> lk(c.mu);
	if (int rc = dfw_bind(c, st->device)) return rc;
	PSVR_HIP(hipMemcpyAsync(meta, st->smeta.as<psvr_bam_rec_meta_t>() + first_rank, (size_t)n * sizeof(psvr_bam_rec_meta_t), hipMemcpyDeviceToHost, c.stream));
	PSVR_HIP(hipStreamSynchronize(c.stream));
	return PSVR_OK;
}

extern "C" int psvr_bam_store_stream(psvr_bam_store_t *st, psvr_bgzf_stream_t *s, int64_t first_rank, int64_t n)
{
	if (!st || !s) return set_error(PSVR_ERR_ARG, "psvr_bam_store_stream: null argument");
	if (st->bad) return st_bad();
	if (!st->ordered) return set_error(PSVR_ERR_ARG, "psvr_bam_store_stream: the store has not been ordered");
	if (s->device != st->device) return set_error(PSVR_ERR_ARG, "psvr_bam_store_stream: the store is on device %d, the stream is on device %d", st->device, s->device);
	if (first_rank < 0 || n < 0 || first_rank > st->n_rec || n > st->n_rec - first_rank)
		return set_error(PSVR_ERR_ARG, "psvr_bam_store_stream: ranks [%lld, %lld) of %lld records", (long long)first_rank, (long long)(first_rank + n), st->n_rec);
	const long long base = st->h_rank_off[(size_t)first_rank], len = st->h_rank_off[(size_t)(first_rank + n)] - base;
	if (len == 0) return PSVR_OK;
	DfwCtx &c = dfw_ctx();
	std::lock_guard<std::mutex> lk(c.mu);
	if (int rc = dfw_bind(c, st->device)) return rc;
	if (int rc = bs_refresh(s, c)) return rc;                    // (where the records go is the stream's count)
	if (int rc = bs_room(s, c, s->n + len)) return rc;           // the host knows every length: the bytes themselves, nothing on top
	StreamDrain drain{c.stream};
	// (bytes behind the stream's count are not part of it: a failure before the count is set leaves it as it was)
	st_gather(c, (const uint64_t *)st->g_src.p, (const psvr_bam_rec_meta_t *)st->smeta.p, (const long long *)st->rank_off.p, first_rank, n, base, s->pend.as<uint8_t>() + s->n);
	PSVR_HIP(hipGetLastError());
	if (int rc = bs_set_count(s, c, s->n + len)) return rc;
	drain.armed = false;
	if (hipStreamSynchronize(c.stream) != hipSuccess) { s->bad = true; return bs_bad(s); }   // (the count may or may not have arrived)
	s->n += len, s->upper = s->n;
	return PSVR_OK;
}

extern "C" int psvr_bam_store_download(psvr_bam_store_t *st, void *bytes, int64_t cap, int64_t *n_bytes)
{
	if (!st || !n_bytes || cap < 0 || (cap > 0 && !bytes)) return set_error(PSVR_ERR_ARG, "psvr_bam_store_download: bad argument");
	*n_bytes = 0;
	DfwCtx &c = dfw_ctx();
	std::lock_guard<std::mutex> lk(c.mu);
	if (int rc = dfw_bind(c, st->device)) return rc;
	if (int rc = st_refresh(st, c, true)) return rc;
	*n_bytes = st->n_bytes;
	if (cap < st->n_bytes) return set_error(PSVR_ERR_OVERFLOW, "psvr_bam_store_download: the store holds %lld bytes, the buffer has %lld", st->n_bytes, (long long)cap);
	const long long n = st->n_rec;
	if (n == 0) return PSVR_OK;
	// append order: the scan of the lengths as they lie in the table, then windows of records gathered side by side and copied out
	DevBuf len, aoff, win;
	std::vector<long long> h_off((size_t)n + 1);
	if (len.alloc((size_t)(n + 1) * 4) || aoff.alloc((size_t)(n + 1) * 8) || st->tmp.ensure(scan_tmp_bytes(1, n + 1))) {
		(void)hipGetLastError();
		return set_error(PSVR_ERR_NOMEM, "psvr_bam_store_download: device allocation failed for the offsets of %lld records", n);
	}
	StreamDrain drain{c.stream};
	hipLaunchKernelGGL(k_store_rank, dim3((unsigned)((n + 256) / 256)), dim3(256), 0, c.stream, (const uint32_t *)nullptr, (const uint64_t *)st->addr.p, (const psvr_bam_rec_meta_t *)st->meta.p, n,
	                   (uint64_t *)nullptr, (psvr_bam_rec_meta_t *)nullptr, len.as<int32_t>());
	ScanSet X = {};
	X.cnt[0] = len.as<int32_t>(), X.out[0] = aoff.as<long long>(), X.stride[0] = 1;
	scan_launch(X, 1, n + 1, st->tmp.as<long long>(), c.stream);
	PSVR_HIP(hipGetLastError());
	PSVR_HIP(hipMemcpyAsync(h_off.data(), aoff.p, (size_t)(n + 1) * 8, hipMemcpyDeviceToHost, c.stream));
	PSVR_HIP(hipStreamSynchronize(c.stream));
	if (h_off[(size_t)n] != st->n_bytes) return set_error(PSVR_ERR_DEVICE, "psvr_bam_store_download: the lengths add up to %lld bytes, the store holds %lld", h_off[(size_t)n], st->n_bytes);
	long long longest = 0;
	for (long long i = 0; i < n; ++i) if (h_off[(size_t)i + 1] - h_off[(size_t)i] > longest) longest = h_off[(size_t)i + 1] - h_off[(size_t)i];
	long long window = st->n_bytes < ((long long)256 << 20) ? st->n_bytes : (long long)256 << 20;
	if (window < longest) window = longest;
	if (win.alloc((size_t)window)) { (void)hipGetLastError(); return set_error(PSVR_ERR_NOMEM, "psvr_bam_store_download: device allocation failed for a window of %lld bytes", window); }
	for (long long a = 0; a < n;) {
		long long b = a + 1;                                     // records [a, b): as many as the window holds
		if (h_off[(size_t)n] - h_off[(size_t)a] <= window) b = n;
		else b = (long long)(std::upper_bound(h_off.begin() + a + 1, h_off.end(), h_off[(size_t)a] + window) - h_off.begin()) - 1;
		if (b <= a) b = a + 1;
		const long long got = h_off[(size_t)b] - h_off[(size_t)a];
		st_gather(c, (const uint64_t *)st->addr.p, (const psvr_bam_rec_meta_t *)st->meta.p, (const long long *)aoff.p, a, b - a, h_off[(size_t)a], win.as<uint8_t>());
		PSVR_HIP(hipGetLastError());
		PSVR_HIP(hipMemcpyAsync((uint8_t *)bytes + h_off[(size_t)a], win.p, (size_t)got, hipMemcpyDeviceToHost, c.stream));
		PSVR_HIP(hipStreamSynchronize(c.stream));
		a = b;
	}
	drain.armed = false;
	return PSVR_OK;
}

extern "C" int psvr_bam_store_drop(psvr_bam_store_t *st, int64_t n_front)
{
	if (psvr_device_count() <= 0) return st_no_device();
	if (!st) return set_error(PSVR_ERR_ARG, "psvr_bam_store_drop: null argument");
	DfwCtx &c = dfw_ctx();
	std::lock_guard<std::mutex> lk(c.mu);
	if (int rc = dfw_bind(c, st->device)) return rc;
	if (int rc = st_refresh(st, c, true)) return rc;
	if (st->ordered) return set_error(PSVR_ERR_ARG, "psvr_bam_store_drop: the store has been ordered: its sorted table names every record");
	if (n_front < 0 || n_front > st->n_rec) return set_error(PSVR_ERR_ARG, "psvr_bam_store_drop: %lld records of %lld", (long long)n_front, st->n_rec);
	if (n_front == 0) return PSVR_OK;
	const long long n = st->n_rec;
	if (st->addr2.ensure((size_t)st->cap_rec * 8) || st->meta2.ensure((size_t)st->cap_rec * sizeof(psvr_bam_rec_meta_t)) || st->key2.ensure((size_t)st->cap_rec * 8)) {
		(void)hipGetLastError();
		return set_error(PSVR_ERR_NOMEM, "psvr_bam_store_drop: device allocation failed for the table of %lld records (%zu bytes); nothing was dropped", st->cap_rec, (size_t)st->cap_rec * 48);
	}
	// the first record kept says which chunks are free: records lie in the chunks in append order
	st->h_ctl[6] = 0;                                            // (page-locked, behind what st_refresh reads back)
	if (n_front < n) PSVR_HIP(hipMemcpyAsync(st->h_ctl + 6, st->addr.as<uint64_t>() + n_front, 8, hipMemcpyDeviceToHost, c.stream));
	long long *ctl = st->ctl.as<long long>();
	PSVR_HIP(hipMemsetAsync(ctl + 5, 0, 8, c.stream));
	const long long g = (n + 255) / 256;
	hipLaunchKernelGGL(k_store_slide, dim3((unsigned)(g < 1024 ? g : 1024)), dim3(256), 0, c.stream, (const uint64_t *)st->addr.p, (const psvr_bam_rec_meta_t *)st->meta.p, (const uint64_t *)st->key.p,
	                   (long long)n_front, n, st->addr2.as<uint64_t>(), st->meta2.as<psvr_bam_rec_meta_t>(), st->key2.as<uint64_t>(), ctl);
	hipLaunchKernelGGL(k_store_dropped, dim3(1), dim3(1), 0, c.stream, ctl, (long long)n_front);
	st->exact = false;
	int rc = hipGetLastError() == hipSuccess ? PSVR_OK : set_error(PSVR_ERR_DEVICE, "psvr_bam_store_drop: launch failed");
	if (!rc) rc = st_refresh(st, c, true);
	if (!rc && st->n_rec != n - n_front) rc = set_error(PSVR_ERR_DEVICE, "psvr_bam_store_drop: the table holds %lld records, %lld were to stay", st->n_rec, n - (long long)n_front);
	if (rc) { st->bad = true; return rc; }
	const uint64_t first_kept = (uint64_t)st->h_ctl[6];
	++st->generation;
	std::swap(st->addr.p, st->addr2.p), std::swap(st->addr.bytes, st->addr2.bytes);
	std::swap(st->meta.p, st->meta2.p), std::swap(st->meta.bytes, st->meta2.bytes);
	std::swap(st->key.p, st->key2.p), std::swap(st->key.bytes, st->key2.bytes);
	// every chunk in front of the first record kept's -- without one: in front of the chunk being filled, which also holds a pending tail
	size_t keep_from = st->chunks.empty() ? 0 : st->chunks.size() - 1;
	if (st->n_rec > 0)
		for (size_t k = 0; k < st->chunks.size(); ++k) {
			const uint64_t b = (uint64_t)(uintptr_t)st->chunks[k]->p;
			if (first_kept >= b && first_kept < b + st->chunks[k]->bytes) { keep_from = k; break; }
		}
	const size_t standard = (st->chunk_bytes + 7) / 8 * 8;
	for (size_t k = 0; k < keep_from; ++k)
		if (!st->spare && st->chunks[k]->bytes == standard) st->spare = std::move(st->chunks[k]);
	st->chunks.erase(st->chunks.begin(), st->chunks.begin() + (long)keep_from);   // (the others free themselves)
	return PSVR_OK;
}

extern "C" int psvr_bam_store_footprint(psvr_bam_store_t *st, int64_t *chunks, int64_t *bytes)
{
	if (psvr_device_count() <= 0) return st_no_device();
	if (!st) return set_error(PSVR_ERR_ARG, "psvr_bam_store_footprint: null argument");
	DfwCtx &c = dfw_ctx();
	std::lock_guard<std::mutex> lk(c.mu);
	long long n = 0, b = 0;
	for (auto &ch : st->chunks) ++n, b += (long long)ch->bytes;
	if (st->spare) ++n, b += (long long)st->spare->bytes;
	if (chunks) *chunks = n;
	if (bytes) *bytes = b;
	return PSVR_OK;
}
