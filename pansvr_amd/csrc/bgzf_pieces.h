// bgzf_pieces.h -- a BAM file's own BGZF members, a piece at a time, for the routes that inflate them on the device (bam_sort.h:
// sort_device_route; signal_device_route.h): find the member that holds the first record's first byte, then read pieces of PSVR_INFLATE_BATCH
// compressed bytes (bam_reader.h's batch) with a second thread while the caller's call on the piece before runs; what lies behind a piece's
// last whole member (less than a member: below 64 KiB) is put in front of the next piece.  Host C++ only.
#pragma once
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <future>
#include <string>
#include <vector>
#include "inflate_device.h"

namespace psvr {

struct PieceFail { std::string call, why; };                 // what ended the walk: the call and the reason, for the caller's one line

// f is left at the first member to send: the one that holds byte header_bytes of the inflated stream; *skip bytes of it are the header's.
// (A header that ends the file: f is at its end, no member to send.)
inline bool bgzf_seek_first_record(FILE *f, size_t header_bytes, long long *skip, PieceFail *fail)
{
	long long first_off = 0, cum = 0;
	*skip = 0;
	for (std::vector<uint8_t> h(12 + 65536);;) {
		const size_t k = fread(h.data(), 1, 12, f);
		if (k == 0) break;
		uint32_t bsize = 0, xlen = k == 12 ? h[10] | (uint32_t)h[11] << 8 : 0;
		uint8_t t[4];
		if (k != 12 || fread(h.data() + 12, 1, xlen, f) != xlen || bgzf_member_header(h.data(), 12 + (uint64_t)xlen, &bsize, &xlen) != 0 || fseek(f, first_off + bsize - 4, SEEK_SET) != 0 ||
		    fread(t, 1, 4, f) != 4) {
			*fail = {"finding the first record's member", "not a whole BGZF block"};
			return false;
		}
		const long long isize = t[0] | (uint32_t)t[1] << 8 | (uint32_t)t[2] << 16 | (uint32_t)t[3] << 24;
		if (cum + isize > (long long)header_bytes) { *skip = (long long)header_bytes - cum; break; }
		cum += isize, first_off += bsize;
	}
	if (fseek(f, first_off, SEEK_SET) != 0) { *fail = {"finding the first record's member", "seek"}; return false; }
	return true;
}

// The pieces from f's position to its end.  take(p, have, skip, &used, fail): p[0, have) holds whole members and perhaps the start of one more;
// it sets *used to the whole members' bytes (skip: inflated bytes at the front of the first piece that took any that are no records) or
// returns false with *fail.  Buffers come from be.host_alloc / host_free.  false: *fail says what ended the walk
template <class Backend, class Take> bool bgzf_for_pieces(Backend &be, FILE *f, long long skip, PieceFail *fail, Take &&take)
{
	const char *e_piece = getenv("PSVR_INFLATE_BATCH");
	const size_t piece = e_piece && atoll(e_piece) >= 1 ? (size_t)atoll(e_piece) : (size_t)16 << 20, front = 65536;
	struct Bufs { Backend &be; uint8_t *buf[2]; ~Bufs() { for (uint8_t *b : buf) if (b) be.host_free(b); } } B{be, {nullptr, nullptr}};
	for (uint8_t *&b : B.buf) if (!(b = (uint8_t *)be.host_alloc(front + piece))) { *fail = {"host_alloc", be.last_error()}; return false; }
	auto read_piece = [&](int b) { return fread(B.buf[b] + front, 1, piece, f); };
	size_t carry = 0, got = read_piece(0);
	bool first = true;
	for (int cur = 0;; cur ^= 1) {
		const bool eof = got < piece;
		uint8_t *p = B.buf[cur] + front - carry;
		const size_t have = carry + got;
		std::future<size_t> next;
		if (!eof) next = std::async(std::launch::async, read_piece, cur ^ 1);
		int64_t used = 0;
		const bool fine = have ? take(p, have, first ? skip : 0, &used, fail) : true;
		if (!eof) got = next.get();                              // (the reader is through before anything is given up)
		if (!fine) return false;
		if (used > 0) first = false;
		carry = have - (size_t)used;
		if (eof) {
			if (carry) { *fail = {"reading the input", carry < 18 ? "not a BGZF block" : "truncated BGZF block"}; return false; }
			return true;
		}
		if (carry >= front) { *fail = {"reading the input", "a BGZF block of more than 64 KiB"}; return false; }
		memcpy(B.buf[cur ^ 1] + front - carry, p + used, carry);
	}
}

} // namespace psvr
