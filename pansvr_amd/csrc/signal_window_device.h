// signal_window_device.h -- the window of a signal run: the FASTQ text SignalStep's host loop would have written for the pairs in front of
// the run's first error pair, complete and in pair order, put together from two sources without either leaving its memory:
//   source 0   the run's text buffer: the state-1 pairs back to back (signal.hip: k_sg_write), pair p's bytes at toff[p]
//   source 1   the host formatter's text of the state-2 pairs (base codes without a letter, quality 223), pair by pair, with offsets
// State-0 pairs have no bytes in either.  The rule, in the form the device runs it: the bodies of the kernels of signal.hip's
// psvr_signal_window and, compiled for the host with one lane, of the checker that holds them to plain concatenation
// (tests/tools/signal_window_check.cpp).  No HIP calls.
//   1 flags, scan   flag[p] = pair p lies in front and is in state 2; the exclusive scan is the pair's rank i among them (scan.h on the device)
//   2 cuts          cut[i] = toff[p]: where in the run's text the i-th host pair belongs (a state-2 pair has zero bytes there)
//   3 segments      2 H + 1 of them for H host pairs (sw_segment): device text [cut[i - 1], cut[i]) in front of host text i, and the rest
//                   of the device text last; a segment is (source, offset, length, output offset), an empty one is kept (two adjacent
//                   state-2 pairs have an empty device segment between them), so segment k's place never depends on the data
//   4 tiles         output tiles of kSwTileBytes: a tile finds the last segment that starts at or in front of its first byte (sw_first_segment,
//                   a binary search over the output offsets, which are monotone) and copies what the segments from there on have inside the
//                   tile with copy_aligned_device.h's body: the tile's first byte is 16-byte aligned, so only a segment's own edges take byte
//                   stores
// Bounds: sw_args_bad has refused offsets that are not monotone or do not end at host_bytes; cut[] comes from the run's own scan and is
// monotone inside [0, text_bytes]; so every segment lies inside its source, the output offsets run from 0 to text_bytes + host_bytes
// without a gap, and a tile writes out[a, b) only.
//
// The add (psvr_signal_window_add): the same passes write a run's window behind the bytes a kept window already holds, at `base`.  The output
// is window bytes [base, base + n_out); the segments' output offsets are the ones above plus base (sw_segment_add); the tiles are the
// kSwTileBytes-aligned tiles of the whole window that meet that range (sw_add_tiles), so only an add's first tile can begin off a 16-byte
// boundary -- copy_aligned_lanes takes any destination residue, and a later tile pays a comparison for it; a tile writes
// [max(a, base), min(b, base + n_out)) and nothing else (sw_tile_add), so two adds that share a tile never touch each other's bytes.  The
// window of a run is the add at base 0: sw_tile and sw_window_host are that.
#pragma once
#include <stdint.h>
#include "copy_aligned_device.h"

namespace psvr {

static const int kSwTileBytes = 16384;                       // output bytes per workgroup: four vector stores per lane

struct SwSeg { int64_t off, len, out; int32_t src, pad; };   // 32 bytes

// what psvr_signal_window refuses before anything is uploaded: a reason, or null.  declined: the last run's state-2 pairs in front.
PSVR_COPY const char *sw_args_bad(int64_t host_bytes, const int64_t *host_off, int64_t n_host, int64_t declined)
{
	if (n_host < 0 || host_bytes < 0) return "a negative count";
	if (n_host != declined) return "n_host is not the number of state-2 pairs in front of the run's first error pair";
	if (n_host == 0) return host_bytes == 0 ? nullptr : "host text without a host pair";
	if (!host_off) return "no offsets";
	if (host_off[0] != 0) return "the first offset is not 0";
	for (int64_t i = 0; i < n_host; ++i) if (host_off[i + 1] < host_off[i]) return "the offsets are not monotone";
	if (host_off[n_host] != host_bytes) return "the last offset is not host_bytes";
	return nullptr;
}

PSVR_COPY int32_t sw_flag(int64_t p, int64_t n_front, const uint8_t *state) { return p < n_front && state[p] == 2 ? 1 : 0; }

// segment k of 2 H + 1.  host_off may be null when H == 0.
PSVR_COPY SwSeg sw_segment(int64_t k, int64_t H, const int64_t *cut, const int64_t *host_off, int64_t text_bytes)
{
	const int64_t i = k >> 1;
	SwSeg s;
	s.pad = 0;
	if (k & 1) {
		s.src = 1, s.off = host_off[i], s.len = host_off[i + 1] - host_off[i], s.out = cut[i] + host_off[i];
	} else {
		const int64_t a = i ? cut[i - 1] : 0, b = i < H ? cut[i] : text_bytes;
		s.src = 0, s.off = a, s.len = b - a, s.out = a + (H ? host_off[i] : 0);
	}
	return s;
}

// segment k of an add at base: the same segment, its place in the window base bytes further on
PSVR_COPY SwSeg sw_segment_add(int64_t k, int64_t H, const int64_t *cut, const int64_t *host_off, int64_t text_bytes, int64_t base)
{
	SwSeg s = sw_segment(k, H, cut, host_off, text_bytes);
	s.out += base;
	return s;
}

// the tiles of the whole window that meet [base, base + n_out): the first one, and how many
PSVR_COPY int64_t sw_add_first_tile(int64_t base) { return base / kSwTileBytes; }
PSVR_COPY int64_t sw_add_tiles(int64_t base, int64_t n_out) { return n_out > 0 ? (base + n_out + kSwTileBytes - 1) / kSwTileBytes - base / kSwTileBytes : 0; }

// the last segment whose output offset is <= at (segment 0 starts at the first byte anybody asks for: there always is one)
PSVR_COPY int64_t sw_first_segment(const SwSeg *seg, int64_t n_seg, int64_t at)
{
	int64_t lo = 0, hi = n_seg;                              // seg[lo].out <= at < seg[hi].out
	while (hi - lo > 1) {
		const int64_t mid = lo + (hi - lo) / 2;
		if (seg[mid].out <= at) lo = mid; else hi = mid;
	}
	return lo;
}

// tile t of the whole window, for the add whose bytes are out[base, end): by lanes [0, n_lanes) that all come here
PSVR_COPY void sw_tile_add(int64_t t, const SwSeg *seg, int64_t n_seg, const uint8_t *text, const uint8_t *host, uint8_t *out, int64_t base, int64_t end, long long lane, long long n_lanes)
{
	const int64_t ta = t * kSwTileBytes, tb = ta + kSwTileBytes;
	const int64_t a = ta > base ? ta : base, b = tb < end ? tb : end;
	if (a >= b) return;
	for (int64_t k = sw_first_segment(seg, n_seg, a); k < n_seg && seg[k].out < b; ++k) {
		const SwSeg s = seg[k];
		const int64_t lo = s.out > a ? s.out : a, hi = s.out + s.len < b ? s.out + s.len : b;
		if (hi <= lo) continue;
		copy_aligned_lanes((s.src ? host : text) + s.off + (lo - s.out), out + lo, hi - lo, lane, n_lanes);
	}
}

// tile t of the window out[0, n_out) by lanes [0, n_lanes) that all come here
PSVR_COPY void sw_tile(int64_t t, const SwSeg *seg, int64_t n_seg, const uint8_t *text, const uint8_t *host, uint8_t *out, int64_t n_out, long long lane, long long n_lanes)
{
	sw_tile_add(t, seg, n_seg, text, host, out, 0, n_out, lane, n_lanes);
}

} // namespace psvr

#if !defined(__HIPCC__)
// ---- the host build: the same passes in the same order, one lane --------------------------------------------------------------------------
#include <vector>
namespace psvr {

// state[n_front], toff[n_front] of a run with text[0, text_bytes), added at base: out is the whole window and has base + text_bytes +
// host_off[n_host] bytes, of which [0, base) are not touched.  The segment table comes back.
inline std::vector<SwSeg> sw_window_add_host(const uint8_t *state, const int64_t *toff, int64_t n_front, const uint8_t *text, int64_t text_bytes, const uint8_t *host,
                                             const int64_t *host_off, int64_t n_host, uint8_t *out, int64_t base)
{
	std::vector<int64_t> rank((size_t)n_front + 1, 0), cut((size_t)n_host, 0);
	for (int64_t p = 0; p < n_front; ++p) rank[(size_t)p + 1] = rank[(size_t)p] + sw_flag(p, n_front, state);
	for (int64_t p = 0; p < n_front; ++p) if (sw_flag(p, n_front, state)) cut[(size_t)rank[(size_t)p]] = toff[p];
	std::vector<SwSeg> seg((size_t)(2 * n_host + 1));
	for (int64_t k = 0; k < 2 * n_host + 1; ++k) seg[(size_t)k] = sw_segment_add(k, n_host, cut.data(), host_off, text_bytes, base);
	const int64_t n_out = text_bytes + (n_host ? host_off[n_host] : 0), t0 = sw_add_first_tile(base);
	for (int64_t t = 0; t < sw_add_tiles(base, n_out); ++t) sw_tile_add(t0 + t, seg.data(), (int64_t)seg.size(), text, host, out, base, base + n_out, 0, 1);
	return seg;
}

// the window of a run: the add at base 0.  out has text_bytes + host_off[n_host] bytes.
inline std::vector<SwSeg> sw_window_host(const uint8_t *state, const int64_t *toff, int64_t n_front, const uint8_t *text, int64_t text_bytes, const uint8_t *host,
                                         const int64_t *host_off, int64_t n_host, uint8_t *out)
{
	return sw_window_add_host(state, toff, n_front, text, text_bytes, host, host_off, n_host, out, 0);
}

} // namespace psvr
#endif
