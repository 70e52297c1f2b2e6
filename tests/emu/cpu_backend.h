// tests/emu/cpu_backend.h -- TEST INFRASTRUCTURE ONLY.
//
// CpuBE, the host backend for pansvr_amd/csrc/engine_core.h: the very same stage functions (aln_device.h) and batch orchestration the
// GPU engine uses, as plain loops on the CPU, with the oracle's DP (oracle/ksw_oracle.c) standing in for the HIP DP kernel.  Shared by
// emu_aln (emu_main.cpp) and the pipeline check (tests/tools/aln_pipeline_check.cpp); never linked into libpsvr_engine.so.
#pragma once
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include "../../pansvr_amd/csrc/engine_core.h"
#include "../../oracle/ksw_oracle.h"

using namespace psvr;

struct CpuBE {
	static constexpr unsigned int kArenaShards = 1;
	void dzero(void *p, size_t n) { memset(p, 0, n); }
	void scatter_u8_dev(uint8_t *a, const int32_t *idx, long long n, uint8_t v) { scatter_u8(a, idx, n, v); }
	void h2d(void *d, const void *h, size_t n) { memcpy(d, h, n); }
	void h2d_start(void *d, const void *h, size_t n) { memcpy(d, h, n); }
	void h2d_wait() {}
	// the pass over an uploaded batch (k_scan_batch on the device): longest read, pairs whose reads will draw for N bases
	bool scan_batch(const char *bases, const long long *off, const psvr_ori_t *ori, long long P, int match, int32_t *, int *lmax, std::vector<int32_t> &out)
	{
		out.clear();
		*lmax = 0;
		for (long long p = 0; p < P; ++p) {
			int nn[2] = {0, 0};
			for (int k = 0; k < 2; ++k) {
				const long long r = 2 * p + k, L = off[r + 1] - off[r];
				if (L > *lmax) *lmax = (int)L;
				const bool unm = ori[r].unmapped || (uint32_t)ori[r].chr_id > 24u;
				if ((!unm && ori[r].align_score == (uint32_t)(L * match)) || L < kLenKmer || L > kMaxReadLen) continue;
				int n = 0;
				for (long long i = 0; i < L; ++i) n += bases[off[r] + i] == 'N';
				nn[k] = n < 255 ? n : 255;
			}
			if (nn[0] + nn[1] >= 1) out.push_back((int32_t)p), out.push_back(nn[0] | (nn[1] << 8));
		}
		return true;
	}
	static long long pr(const int32_t *w, long long i) { return w ? w[i] : i; }
	void run_init(const RunInit &r)
	{
		long long n = r.S;
		for (long long k : {r.nsp, (long long)r.n_tops, (long long)r.n_atops, (long long)kFlagWords}) if (k > n) n = k;
		for (long long s = 0; s < n; ++s) run_init_slot(r, s);
	}
	void append_iota(int32_t *w, long long at, long long start, long long n) { for (long long i = 0; i < n; ++i) w[at + i] = (int32_t)(start + i); }
	void st_special_class(const Ctx &c, const SpecialPair *sp, long long n, uint8_t *mask, uint8_t *cls)
	{
		for (long long i = 0; i < n; ++i) { cls[i] = (uint8_t)special_is_const(c, sp[i]); if (cls[i]) mask[sp[i].pair] = 0; }
	}
	void st_adopt_auto(const Ctx &c, const SpecialPair *sp, long long n, const uint8_t *cls, const uint8_t *mask, const long long *noff, int32_t *adopted, long long *adopted_at, unsigned long long *count,
	                   const int32_t *host_pairs, const int32_t *host_slots, long long n_host)
	{
		st_adopt(c, host_pairs, host_slots, n_host, noff);
		for (long long i = 0; i < n; ++i) if (cls[i] && !mask[sp[i].pair]) { const int did = adopt_auto(c, sp[i], noff, adopted + i, adopted_at + i, 0, 1); if (count) *count += (unsigned long long)did; }
	}
	void scatter_u8(uint8_t *a, const int32_t *idx, long long n, uint8_t v) { for (long long i = 0; i < n; ++i) a[idx[i]] = v; }
	void st_mask_totals(const int32_t *ctot, const uint8_t *mask, long long n, int32_t *out) { for (long long i = 0; i < n; ++i) out[i] = mask[i] ? 0 : ctot[i]; }
	void copy_hoff_to_shadows(const Ctx &c, long long P, long long n)
	{
		for (long long j = 0; j < n; ++j) for (int k = 0; k < 2; ++k) c.hoff[2 * (P + j) + k] = c.hoff[2 * (long long)c.src[P + j] + k];
	}
	void st_prep(const Ctx &c, const int32_t *w, long long n, int mate) { for (long long i = 0; i < n; ++i) prep_read(c, pr(w, i) * 2 + mate); }
	void st_str(const Ctx &c, const int32_t *w, long long n, int mate) { for (long long i = 0; i < n; ++i) str_detect(c, pr(w, i) * 2 + mate); }
	void st_seed(const Ctx &c, const int32_t *w, long long n, int mate) { for (long long i = 0; i < 2 * n; ++i) seed_strand(c, (pr(w, i >> 1) * 2 + mate) * 2 + (i & 1)); }
	// chaining + chain selection of a read in one go, like the GPU backend: the register-resident small case first, the generic pair for what
	// it declines (PSVR_EMU_NO_SMALL=1: the generic pair for every read)
	long long n_small = 0, n_generic = 0;
	void st_chain(const Ctx &c, const int32_t *w, long long n, int mate)
	{
		static const bool no_small = getenv("PSVR_EMU_NO_SMALL") != nullptr;
		for (long long i = 0; i < n; ++i) {
			const long long r = pr(w, i) * 2 + mate;
			if (!no_small && chain_select_small(c, r)) { ++n_small; continue; }
			++n_generic;
			chain_read(c, r), select_read(c, r);
		}
	}
	void st_walk(const Ctx &c, const int32_t *w, long long n)
	{
		for (long long i = 0; i < 2 * n; ++i) walk_read(c, pr(w, i >> 1) * 2 + (i & 1));
	}
	void st_totals(const Ctx &c, const int32_t *w, long long n, int32_t *ctot, int32_t *hprev, uint8_t *sens, int32_t *slist, unsigned long long *cnt, bool detect)
	{
		for (long long i = 0; i < n; ++i) {
			long long s = pr(w, i);
			int32_t t = c.rcnt[3 * s] + c.rcnt[3 * s + 1] + c.rcnt[3 * s + 2];
			const int32_t h0 = c.hcnt[2 * s], h1 = c.hcnt[2 * s + 1];
			if (t != ctot[s] || h0 != hprev[2 * s] || h1 != hprev[2 * s + 1]) cnt[kTopChanged - kTopNewSens] = 1;
			if (detect && s < c.n_pairs && t != ctot[s] && !sens[s]) sens[s] = 1, slist[(*cnt)++] = (int32_t)s;
			ctot[s] = t, hprev[2 * s] = h0, hprev[2 * s + 1] = h1;
		}
	}
	void st_totals_dev(const Ctx &c, const int32_t *list, const unsigned long long *n_dev, long long, int32_t *ctot, int32_t *hprev, uint8_t *sens, int32_t *slist, unsigned long long *cnt)
	{
		st_totals(c, list, (long long)*n_dev, ctot, hprev, sens, slist, cnt, true);
	}
	void st_assemble(const Ctx &c, long long b, long long e) { for (long long i = b; i < e; ++i) assemble_candidate(c, i); }
	void st_pair(const Ctx &c, const int32_t *w, long long n) { for (long long i = 0; i < n; ++i) pair_reads(c, pr(w, i)); }
	// as k_finalize_pair does it: both headers built in place, the pairing's items handed on from finalize_read
	void st_finalize_pair(const Ctx &c, const int32_t *w, long long n)
	{
		for (long long i = 0; i < n; ++i) {
			const long long p = pr(w, i);
			PeItem it0[3], it1[3];
			finalize_read(c, 2 * p, c.rh[2 * p], it0), finalize_read(c, 2 * p + 1, c.rh[2 * p + 1], it1);
			pair_reads(c, p, c.rh[2 * p], c.rh[2 * p + 1], it0, it1);
		}
	}
	void st_scan(const int32_t *cnt, long long n, int stride, int off, long long base, long long *out)
	{
		long long acc = base;
		for (long long i = 0; i < n; ++i) { out[off + i * stride] = acc; acc += cnt[off + i * stride]; }
	}
	void st_dirty(const Ctx &c, const long long *noff, const long long *nhoff, int32_t *out, unsigned long long *cnt, int32_t *outp, unsigned long long *cntp,
	              const uint8_t *has_n, int32_t *out3, unsigned long long *cnt3, long long cap3, int32_t *out4, unsigned long long *cnt4)
	{
		for (long long p = 0; p < c.n_pairs; ++p) {
			int d = mark_dirty(c, p, noff, nhoff, has_n);
			if (d == 3 && (long long)*cnt3 >= cap3) d = 2;
			if (d == 3) out3[(*cnt3)++] = (int32_t)p;
			else if (d == 2) out[(*cnt)++] = (int32_t)p;
			else if (d == 1) outp[(*cntp)++] = (int32_t)p;
		}
		for (unsigned long long i = 0; i < *cnt3; ++i) {
			const long long p = out3[i];
			if (reselect_pair(c, p) != 2) outp[(*cntp)++] = (int32_t)p;
			else out4[(*cnt4)++] = (int32_t)p;
		}
	}
	void append_list(int32_t *w, long long at, const int32_t *src, long long n) { for (long long i = 0; i < n; ++i) w[at + i] = src[i]; }
	void st_pair_dev(const Ctx &c, const int32_t *list, const unsigned long long *cnt) { for (unsigned long long i = 0; i < *cnt; ++i) pair_reads(c, list[i]); }
	void st_adopt(const Ctx &c, const int32_t *pairs, const int32_t *slots, long long n, const long long *noff) { for (long long i = 0; i < n; ++i) adopt_variant(c, pairs[i], slots[i], noff, 0, 1); }
	bool side_begin() { return false; }       // one queue
	void side_end() {}
	void side_wait() {}
	template <class Core> int st_dp(Core &core)
	{
		const Ctx &c = core.c;
		DpIO &d = core.dp;
		long long n = d.end - d.begin, qb = 0, tb = 0;
		for (long long i = 0; i < n; ++i) { const DpDesc &x = c.dp.base[d.begin + i]; qb += x.qlen, tb += x.tlen; }
		if (!core.ensure_dp(n, qb, tb, qb + tb + 2 * n)) return PSVR_ERR_NOMEM;
		long long qo = 0, to = 0;
		static FILE *shapes = getenv("EMU_DP_SHAPES") ? fopen(getenv("EMU_DP_SHAPES"), "w") : nullptr;   // one "qlen tlen" line per DP problem, for tools/team_fill.py
		for (long long i = 0; i < n; ++i) {
			const DpDesc &x = c.dp.base[d.begin + i];
			if (shapes) fprintf(shapes, "%d %d\n", x.qlen, x.tlen);
			d.qlen[i] = x.qlen, d.tlen[i] = x.tlen, d.q_off[i] = qo, d.t_off[i] = to;
			dp_fetch_one(c, x, d.qbuf + qo, d.tbuf + to);
			orc_extz_t ez;
			psvr_extz_t &o = d.ez[i];
			o.cigar_off = qo + to + 2 * i;
			orc_extd2(x.qlen, d.qbuf + qo, x.tlen, d.tbuf + to, 5, c.mat, (int8_t)c.par.gap_open, (int8_t)c.par.gap_ex, (int8_t)c.par.gap_open2, (int8_t)c.par.gap_ex2,
			          200, c.par.zdrop, -1, 0, &ez, d.cig + o.cigar_off, x.qlen + x.tlen + 2);
			o.max = ez.max, o.zdropped = ez.zdropped, o.max_q = ez.max_q, o.max_t = ez.max_t, o.mqe = ez.mqe, o.mqe_t = ez.mqe_t;
			o.mte = ez.mte, o.mte_q = ez.mte_q, o.score = ez.score, o.n_cigar = ez.n_cigar, o.reach_end = ez.reach_end;
			qo += x.qlen, to += x.tlen;
		}
		return PSVR_OK;
	}
};
