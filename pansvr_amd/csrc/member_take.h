// member_take.h -- one take from a device-resident BGZF stream (psvr_bgzf_stream_take, include/psvr_engine.h) into page-locked memory and on
// into the file: what bgzf_stream_sink.h does after a piece and sorted_bam.h's store writer does after a window of ranks.  It owns the
// page-locked buffer and the table of member offsets, and counts what it wrote.  Of the backend it asks int64_t bound(int64_t n),
// int take(int finish, void *out, int64_t cap, int64_t *got, int64_t *member_off, int64_t member_cap, int64_t *n_members, int64_t *used),
// void *host_alloc(size_t) and void host_free(void *).
#pragma once
#include <stdint.h>
#include <stdio.h>
#include <vector>
#include "bam_writer.h"

namespace psvr {

template <class Backend> class MemberTake {
public:
	uint64_t fpos = 0;                                   // bytes written so far: the file offset of the next member
	long long members = 0;                               // members written so far
	bool wrote = true;                                   // every fwrite was whole
	explicit MemberTake(Backend &be) : be_(be) {}
	~MemberTake() { if (pin_) be_.host_free(pin_); }
	MemberTake(const MemberTake &) = delete;

	// the members of the stream's `pending` bytes (finish: the tail as a last, shorter member) into f; *used: the pending bytes they held.
	// starts: the file offset of every member is logged there, or null for no table.  false: no buffer, or the backend's take failed
	bool operator()(FILE *f, int finish, int64_t pending, int64_t *used, std::vector<uint64_t> *starts = nullptr)
	{
		*used = 0;
		if (pending == 0) return true;
		const size_t need = (size_t)be_.bound(pending);
		if (need > pin_cap_) {
			if (pin_) be_.host_free(pin_);
			pin_ = (uint8_t *)be_.host_alloc(need + need / 4), pin_cap_ = pin_ ? need + need / 4 : 0;
			if (!pin_) return false;
		}
		const int64_t cap_m = starts ? pending / (int64_t)kBgzfBlock + 1 : 0;
		if (starts) moff_.assign((size_t)cap_m + 1, 0);
		int64_t got = 0, nm = 0;
		if (be_.take(finish, pin_, (int64_t)pin_cap_, &got, starts ? moff_.data() : nullptr, cap_m, &nm, used)) return false;
		for (int64_t m = 0; starts && m < nm; ++m) starts->push_back(fpos + (uint64_t)moff_[(size_t)m]);
		if (fwrite(pin_, 1, (size_t)got, f) != (size_t)got) wrote = false;
		fpos += (uint64_t)got, members += nm;
		return true;
	}

private:
	Backend &be_;
	uint8_t *pin_ = nullptr;
	size_t pin_cap_ = 0;
	std::vector<int64_t> moff_;
};

} // namespace psvr
