// signal_mate_check -- the mate rules of pansvr_amd/csrc/signal_mate_device.h (host build, one lane) against SignalStep::run_pos_sorted, the
// specification, through what that loop writes: its FASTQ text and its stderr.
//   signal_mate_check in.bam [-D] [-U] [--block-records N]
// The host loop runs over the file with its stdout in memory and its stderr in a file.  Then the model runs: blocks cut, mates found, turns
// counted and lists made by the header's rules (signal_mate_host.h walks them as psvr_signal_run_pos does), the by-name pass by runs of
// equal names -- and for every pair it decides on, SignalStep::pair formats; the messages are printed in the host loop's words.  Both
// texts and both stderr files must be equal byte for byte.  Prints a summary; exit 0: equal, 1: not, 2: a block the rules decline (which
// one is said).
#include <unistd.h>
#include <fcntl.h>
#include <string>
#include <vector>
#include "../../pansvr_amd/csrc/signal_step.h"
#include "signal_mate_host.h"

using namespace psvr;

static std::string slurp(const char *fn)
{
	std::string s;
	FILE *f = fopen(fn, "rb");
	if (!f) return s;
	char buf[65536];
	size_t n;
	while ((n = fread(buf, 1, sizeof buf, f)) > 0) s.append(buf, n);
	fclose(f);
	return s;
}
struct StderrTo {                                            // fd 2 goes to a file while this lives
	int saved;
	explicit StderrTo(const char *fn) { fflush(stderr); saved = dup(2); const int fd = open(fn, O_WRONLY | O_CREAT | O_TRUNC, 0600); dup2(fd, 2); close(fd); }
	~StderrTo() { fflush(stderr); dup2(saved, 2); close(saved); }
};

int main(int argc, char **argv)
{
	if (argc < 2) { fprintf(stderr, "usage: signal_mate_check in.bam [-D] [-U] [--block-records N]\n"); return 2; }
	SignalStep S;
	S.o.input = argv[1];
	for (int a = 2; a < argc; ++a) {
		const std::string s = argv[a];
		if (s == "-D") S.o.not_use_filter = true;
		else if (s == "-U") S.o.discard_full_match = true;
		else if (s == "--block-records" && a + 1 < argc) S.o.block_records = atoi(argv[++a]);
		else { fprintf(stderr, "unknown argument %s\n", s.c_str()); return 2; }
	}
	const std::string tmp = std::string(getenv("TMPDIR") ? getenv("TMPDIR") : "/tmp") + "/signal_mate_check." + std::to_string((long)getpid());
	const std::string err_host = tmp + ".host", err_model = tmp + ".model";
	{
		StderrTo quiet(err_host.c_str());
		if (!S.sample_stats()) return 2;
	}
	S.bs.reset();
	S.isize_max = (int)(S.bs.max_i + 150), S.isize_min = (int)(S.bs.min_i - 150);
	if (S.isize_min < 1) S.isize_min = 1;
	SignalStep M = S;                                        // the model's formatter: the same options and statistics
	// the host loop
	char *host_buf = nullptr, *model_buf = nullptr;
	size_t host_len = 0, model_len = 0;
	{
		BamReader rd;
		if (!rd.open(S.o.input.c_str())) { fprintf(stderr, "%s\n", rd.error().c_str()); return 2; }
		S.out = open_memstream(&host_buf, &host_len);
		StderrTo capture(err_host.c_str());
		if (!S.run_pos_sorted(rd)) return 2;
		fclose(S.out);
	}
	// the model
	std::vector<std::vector<uint8_t>> bytes;
	std::vector<BamRecord> recs;
	{
		BamReader rd;
		if (!rd.open(S.o.input.c_str())) return 2;
		BamRecord r;
		while (rd.next(r)) if (SignalStep::primary(r)) bytes.push_back(sm_record_bytes(r)), recs.push_back(r);
	}
	M.out = open_memstream(&model_buf, &model_len);
	long long fails = 0, pairs = 0, blocks = 0, replayed = 0, left_pairs = 0, pair_errors = 0;
	int declined = 0;
	std::vector<size_t> left;
	{
		StderrTo capture(err_model.c_str());
		size_t front = 0;
		for (;;) {
			std::vector<const uint8_t *> prim;
			const size_t look = std::min(bytes.size(), front + (size_t)S.o.block_records);   // (a block never looks further than its record limit)
			for (size_t i = front; i < look; ++i) prim.push_back(bytes[i].data());
			const SmHostBlock B = sm_host_block(prim, S.o.block_records, kSmSpan, true);
			if (B.n < 2) break;
			if (B.bad) { declined = B.bad; break; }
			++blocks, replayed += B.replayed;
			long long rank = 0;
			for (int64_t i = 0; i < B.n; ++i) {
				if (!B.fail[(size_t)i]) continue;
				const long long turn = fails + ++rank;
				if (sm_note_slot(fails, turn) < 0) continue;
				const BamRecord &c = recs[front + (size_t)i];
				fprintf(stderr, "NUM: [%lld]: Mate failed, index:[%d] in [%d] size block, tid: [ %d ], pos [%d] name [%s]\n", turn, (int)i, (int)B.n, c.tid, c.pos, c.qname());
			}
			fails += B.fails;
			if (sm_too_many_unmated((int64_t)B.left.size(), B.n)) fprintf(stderr, "WARNING, too many total_unmated_read![ %d %d %f]\n", (int)B.left.size(), (int)B.n, (float)(int)B.left.size() / (float)(int)B.n);
			for (const auto &p : B.pairs) {
				M.bs.total += 2;
				if (M.bs.total % 100000 == 0) fprintf(stderr, "%ld\n", (long)M.bs.total);
				M.pair(recs[front + (size_t)p.first], recs[front + (size_t)p.second], true);
				++pairs;
			}
			for (int32_t i : B.left) left.push_back(front + (size_t)i);
			front += (size_t)B.n;
		}
		if (!declined) {
			fprintf(stderr, "phase 2:\nSort all unpaired records: [%zu] in total\n", left.size());
			std::stable_sort(left.begin(), left.end(), [&](size_t a, size_t b) {
				const int c = strcmp(recs[a].qname(), recs[b].qname());
				if (c) return c < 0;
				return (recs[a].flag & 0x40) != 0 && !(recs[b].flag & 0x40);
			});
			const FqGroup g;
			for (const auto &ev : sm_phase2_events(left.size(), [&](size_t a, size_t b) { return sg_same_name(g, bytes[left[a]].data(), bytes[left[b]].data()); })) {
				M.bs.total += 2;
				if (M.bs.total % 100000 == 0) fprintf(stderr, "%ld\n", (long)M.bs.total);
				if (!ev.second) { ++pair_errors; fprintf(stderr, "Read Pairing error!, reads names are not same, please confirm the completeness of BAM/CRAM file.\n"); continue; }
				M.pair(recs[left[ev.first]], recs[left[ev.first + 1]], true);
				++left_pairs;
			}
		}
		fclose(M.out);
	}
	const std::string eh = slurp(err_host.c_str()), em = slurp(err_model.c_str());
	unlink(err_host.c_str()), unlink(err_model.c_str());
	if (declined) { printf("declined %d\n", declined); free(host_buf), free(model_buf); return 2; }
	const bool same_text = host_len == model_len && !memcmp(host_buf, model_buf, host_len), same_err = eh == em;
	printf("blocks %lld pairs %lld left %zu left_pairs %lld pair_errors %lld fails %lld replayed %lld text_bytes %zu same_text %d same_stderr %d\n", blocks, pairs, left.size(), left_pairs, pair_errors, fails,
	       replayed, host_len, (int)same_text, (int)same_err);
	if (!same_err) fprintf(stderr, "---- host loop's stderr\n%s---- model's stderr\n%s", eh.c_str(), em.c_str());
	free(host_buf), free(model_buf);
	return same_text && same_err ? 0 : 1;
}
