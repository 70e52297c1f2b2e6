// signal_device_check -- holds the host build of pansvr_amd/csrc/signal_device.h (the rules the kernels of signal.hip run, compiled with one
// "lane") to SignalStep::pair, pair by pair, on the records of a BAM file: state, note and text.  A program of its own, built plain and with
// -fsanitize=address,undefined (tests/test_signal_device_rules.py); both builds must write the same summary.
//   signal_device_check in.bam [-D] [-U] [-I n] [--dump prefix] [--opt isize_min,isize_max,s0,s1,s2,s3]
// (--opt: the -U window and the four STAT_ numbers as given instead of what the file's first records say, for a file that is part of another)
// The pairing is SignalStep::run's name-sorted loop: consecutive primary records, a lone last one is dropped; the first pair the host
// would abort on (states 3, 4, 5) ends the walk.  stdout: one summary line; --dump: prefix.tab ("state note bytes rec1 rec2" per pair) and
// prefix.fq (the device text: the state-1 pairs).  Exit status 0: every pair agreed.
#include <sys/wait.h>
#include <unistd.h>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>
#include "../../pansvr_amd/csrc/signal_step.h"
#include "../../pansvr_amd/csrc/signal_device.h"

using namespace psvr;

static std::vector<uint8_t> raw_of(const BamRecord &r)       // the record as it lay in the file (its bin is not kept: no rule reads it)
{
	std::vector<uint8_t> v(kBamRecHead + r.data.size());
	const uint32_t bs = (uint32_t)(32 + r.data.size());
	const uint16_t bin = 0;
	memcpy(&v[0], &bs, 4), memcpy(&v[4], &r.tid, 4), memcpy(&v[8], &r.pos, 4);
	v[12] = r.l_qname, v[13] = r.mapq;
	memcpy(&v[14], &bin, 2), memcpy(&v[16], &r.n_cigar, 2), memcpy(&v[18], &r.flag, 2), memcpy(&v[20], &r.l_qseq, 4), memcpy(&v[24], &r.mtid, 4), memcpy(&v[28], &r.mpos, 4);
	memcpy(&v[32], &r.isize, 4);
	if (!r.data.empty()) memcpy(&v[kBamRecHead], r.data.data(), r.data.size());
	return v;
}

// does SignalStep::pair abort on this pair?  (in a child process: the checker itself goes on)
static bool host_aborts(SignalStep &S, const BamRecord &a, const BamRecord &b)
{
	fflush(stdout), fflush(stderr);
	const pid_t pid = fork();
	if (pid == 0) {
		if (!freopen("/dev/null", "w", stderr)) _exit(3);
		S.out = fopen("/dev/null", "w");
		S.pair(a, b, true);
		_exit(0);
	}
	int status = 0;
	waitpid(pid, &status, 0);
	return !(WIFEXITED(status) && WEXITSTATUS(status) == 0);
}

int main(int argc, char **argv)
{
	if (argc < 2) { fprintf(stderr, "usage: signal_device_check in.bam [-D] [-U] [-I n] [--dump prefix]\n"); return 2; }
	SignalStep S;
	S.o.input = argv[1], S.o.sort_by_name = true;
	std::string dump;
	int given[6], have_given = 0;
	for (int i = 2; i < argc; ++i) {
		if (!strcmp(argv[i], "-D")) S.o.not_use_filter = true;
		else if (!strcmp(argv[i], "-U")) S.o.discard_full_match = true;
		else if (!strcmp(argv[i], "-I") && i + 1 < argc) S.o.max_tid = atoi(argv[++i]);
		else if (!strcmp(argv[i], "--dump") && i + 1 < argc) dump = argv[++i];
		else if (!strcmp(argv[i], "--opt") && i + 1 < argc && sscanf(argv[++i], "%d,%d,%d,%d,%d,%d", &given[0], &given[1], &given[2], &given[3], &given[4], &given[5]) == 6) have_given = 1;
		else { fprintf(stderr, "unknown argument %s\n", argv[i]); return 2; }
	}
	FILE *const real_err = stderr;
	{                                                        // SignalStep::run's preamble, its status line kept off the terminal
		char *eb = nullptr; size_t en = 0;
		FILE *em = open_memstream(&eb, &en);
		stderr = em;
		const bool ok = S.sample_stats();
		stderr = real_err;
		fclose(em), free(eb);
		if (!ok) { fprintf(stderr, "cannot sample %s\n", argv[1]); return 2; }
	}
	psvr_signal_opt_t opt;
	opt.gap_open = S.o.gap_open, opt.gap_ex = S.o.gap_ex, opt.gap_open2 = S.o.gap_open2, opt.gap_ex2 = S.o.gap_ex2, opt.match = S.o.match, opt.mismatch = S.o.mismatch;
	opt.max_tid = S.o.max_tid, opt.not_use_filter = S.o.not_use_filter, opt.discard_full_match = S.o.discard_full_match;
	opt.stat[0] = S.bs.read_len, opt.stat[1] = (int32_t)S.bs.min_i, opt.stat[2] = (int32_t)S.bs.mid_i, opt.stat[3] = (int32_t)S.bs.max_i;
	S.bs.reset();
	S.isize_max = (int)(S.bs.max_i + 150), S.isize_min = (int)(S.bs.min_i - 150);
	if (S.isize_min < 1) S.isize_min = 1;
	if (have_given) {
		S.isize_min = given[0], S.isize_max = given[1];
		S.bs.read_len = given[2], S.bs.min_i = (uint32_t)given[3], S.bs.mid_i = (uint32_t)given[4], S.bs.max_i = (uint32_t)given[5];
		for (int k = 0; k < 4; ++k) opt.stat[k] = given[2 + k];
	}
	opt.isize_min = S.isize_min, opt.isize_max = S.isize_max;

	BamReader rd;
	if (!rd.open(argv[1])) { fprintf(stderr, "%s\n", rd.error().c_str()); return 2; }
	FILE *tab = nullptr, *fq = nullptr;
	if (!dump.empty() && (!(tab = fopen((dump + ".tab").c_str(), "w")) || !(fq = fopen((dump + ".fq").c_str(), "w")))) { fprintf(stderr, "cannot write %s.*\n", dump.c_str()); return 2; }
	const FqGroup g;
	long long n_state[6] = {0, 0, 0, 0, 0, 0}, pairs = 0, notes = 0, bytes = 0, first_error = -1, mismatches = 0, rec_index = -1, stat_pairs = 0;
	uint64_t fnv = 1469598103934665603ull;
	bool spent = false;
	BamRecord b1, b2;
	for (;;) {
		bool g1, g2;
		long long i1, i2;
		do { g1 = rd.next(b1), ++rec_index; } while (g1 && !SignalStep::primary(b1));
		i1 = rec_index;
		do { g2 = rd.next(b2), ++rec_index; } while (g2 && !SignalStep::primary(b2));
		i2 = rec_index;
		if (!g1 || !g2) break;
		const std::vector<uint8_t> r1 = raw_of(b1), r2 = raw_of(b2);
		if (!bam_rec_reader_fits(r1.data()) || !bam_rec_name_ends(r1.data()) || !bam_rec_reader_fits(r2.data()) || !bam_rec_name_ends(r2.data())) { fprintf(stderr, "record rules\n"); return 2; }
		// ---- the host: SignalStep::run's two tests, then pair() into memory
		int want = 0;
		uint32_t want_note = 0;
		std::string want_text;
		if (strcmp(b1.qname(), b2.qname())) want = 3;
		else if (!(b1.flag & 0x40) || !(b2.flag & 0x80)) want = 4;
		else if (b1.l_qseq >= 2048 && host_aborts(S, b1, b2)) want = 5;
		else {
			char *ob = nullptr, *eb = nullptr; size_t on = 0, en = 0;
			FILE *om = open_memstream(&ob, &on), *em = open_memstream(&eb, &en);
			S.out = om, S.stat_written = spent, stderr = em;
			S.pair(b1, b2, true);
			stderr = real_err;
			fclose(om), fclose(em);
			want_text.assign(ob, on);
			const std::string err(eb, en);
			free(ob), free(eb);
			if (err.find(" wrong ISIZE: ") != std::string::npos) want_note |= kSgNoteIsize;
			want = want_text.empty() ? 0 : err.find("Wrong base!") != std::string::npos ? 2 : 1;
		}
		// ---- the rules: the size pass, then the write pass into exactly that many bytes
		int32_t nb = 0;
		uint32_t note = 0;
		const int st = sg_pair_size(g, opt, r1.data(), r2.data(), &nb, &note);
		const bool stat_here = !spent && (st == 1 || st == 2);
		if (st == 1 && stat_here) nb += sg_stat_bytes(g, opt);
		std::string text((size_t)nb, '\xEE');
		if (st == 1) {
			BeWrite w;
			w.out = (uint8_t *)&text[0], w.pos = 0;
			uint32_t note2 = 0;
			const int st2 = sg_pair(g, opt, r1.data(), r2.data(), stat_here, w, &note2);
			if (st2 != 1 || note2 != note || w.pos != (uint64_t)nb) { fprintf(stderr, "pair %lld: the passes disagree (%d, %llu of %d bytes)\n", pairs, st2, (unsigned long long)w.pos, nb); ++mismatches; }
		}
		if (stat_here) spent = true, ++stat_pairs;
		bool same = st == want && (st >= 3 || note == want_note);
		if (same && st == 1) same = text == want_text;
		if (!same && mismatches++ < 5) {
			fprintf(stderr, "pair %lld [%s]: state %d note %u, the host says %d note %u\n", pairs, b1.qname(), st, note, want, want_note);
			if (st == 1 && want == 1) fprintf(stderr, "--- rules\n%s--- host\n%s", text.c_str(), want_text.c_str());
		}
		n_state[st]++, notes += (st < 3 && note) ? 1 : 0, bytes += nb;
		for (char ch : text) fnv = (fnv ^ (uint8_t)ch) * 1099511628211ull;
		fnv = (fnv ^ (uint64_t)(st * 4 + (int)note)) * 1099511628211ull;
		if (tab) fprintf(tab, "%d %u %d %lld %lld\n", st, note, nb, i1, i2);
		if (fq && st == 1) fwrite(text.data(), 1, text.size(), fq);
		++pairs;
		if (st >= 3 || want >= 3) { first_error = pairs - 1; break; }
	}
	if (first_error < 0 && !rd.error().empty()) { fprintf(stderr, "%s\n", rd.error().c_str()); return 2; }
	if (tab) fclose(tab);
	if (fq) fclose(fq);
	printf("pairs %lld state0 %lld state1 %lld state2 %lld state3 %lld state4 %lld state5 %lld notes %lld bytes %lld stat_pairs %lld first_error %lld mismatches %lld isize_min %d isize_max %d stat0 %d stat1 %d stat2 %d stat3 %d fnv %016llx\n", pairs,
	       n_state[0], n_state[1], n_state[2], n_state[3], n_state[4], n_state[5], notes, bytes, stat_pairs, first_error, mismatches, opt.isize_min, opt.isize_max, opt.stat[0], opt.stat[1], opt.stat[2], opt.stat[3], (unsigned long long)fnv);
	return mismatches ? 1 : 0;
}
