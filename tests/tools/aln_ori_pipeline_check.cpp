// tests/tools/aln_ori_pipeline_check.cpp -- TEST INFRASTRUCTURE ONLY.
//
// `panSVR aln --ori-device` without a GPU: the PRODUCT's pipeline (pansvr_amd/csrc/aln_pipeline.h) over aln_pipeline_check.cpp's driver of
// CPU emulations, extended by the two device routes the option needs -- both as the host builds of the rules the kernels run:
//   parse_window / emit_encode / emit_download    the host parser's batch marked as a device batch; the main file's records by bam_emit_device.h
//   OriSource                                     the second file's records by bam_ori_device.h
// Every piece behind the first is handed to the pipeline with a POISONED text pointer and text_pending set, as the window routes hand it
// out under the option: the pipeline must fetch the text (fetch_text, counted) before anything on the host reads it, and must not fetch it
// for a resident piece.  The driver's download is counted as well: a resident piece's results are not asked for (its Block keeps the
// results of an earlier piece, so a formatter that looked at them would write other records than the plain pipeline).
//
// Usage: aln_ori_pipeline_check [--ori-device] [--fail-ori N] <aln_pipeline_check's options and arguments>
//   --fail-ori N: the OriSource's N-th encode and every later one fail
// stderr, last line: "ori_pipeline pieces <n> resident <n> text_fetches <n> downloads <n> ori_device_pairs <n> ori_declined_pairs <n> ori_spliced_pairs <n> ori_pieces <n> ori_host_pieces <n>"
#define main aln_pipeline_check_main
#include "aln_pipeline_check.cpp"
#undef main
#include "../../pansvr_amd/csrc/bam_ori_device.h"

static const char *const kPoison = (const char *)16;         // (reading through it faults)

struct OriDriver : CpuDriver {
	const HostIndex &hi;
	int n_header;
	BeTableHost tab;
	const char *real_text[aln::kSlots] = {};
	long long text_bytes[aln::kSlots] = {};
	BeHostResult main_rec[aln::kSlots], ori_rec[aln::kSlots];
	long long n_parsed = 0, n_fetches = 0, n_downloads = 0, n_ori_calls = 0, fail_ori_from = -1;
	int mfs = 0;
	OriDriver(const HostIndex &h, int nh, int D) : CpuDriver(h.view(), D), hi(h), n_header(nh)
	{
		tab.build((int)h.svh.size(), [&](int i) { return h.svh[(size_t)i].vcf_print_string.c_str(); }, [&](int i) { return h.svh[(size_t)i].vcf_id.c_str(); });
	}
	int create(const psvr_aln_params_t &par, int64_t pos[3]) { mfs = par.min_filter_score; return CpuDriver::create(par, pos); }
	int download(int d, aln::Block &bk, bool full, long long *bytes) { ++n_downloads; return CpuDriver::download(d, bk, full, bytes); }
	int parse_window(int slot, FastqReader &rd, FastqBatch &fb, long long pairs, long long bases, int threads, std::string *)
	{
		if (!rd.read(fb, pairs, bases, threads)) return 0;
		fb.dev = (const psvr_fastq_t *)this;                     // (never followed: the emulation's upload reads fb.bases)
		fb_of[slot] = &fb, real_text[slot] = fb.text, text_bytes[slot] = (long long)fb.ls[(size_t)(4 * fb.R)];
		if (n_parsed++) fb.text = kPoison, fb.text_pending = text_bytes[slot];
		return 1;
	}
	const FastqBatch *fb_of[aln::kSlots] = {};
	int slot_of(const FastqBatch &fb) const { for (int s = 0; s < aln::kSlots; ++s) if (fb_of[s] == &fb) return s; return -1; }
	template <class In> void window(int slot, const FastqBatch &fb, In *in)
	{
		const Ctx &c = eng[0]->core.c;
		memset(in, 0, sizeof *in);
		in->text = real_text[slot], in->line_start = fb.ls.data(), in->name_end = fb.name_end.data(), in->ori = fb.ori, in->first_pair = 0;
		in->hdr = c.rh, in->pairs = c.pres, in->cands = c.cand, in->n_cands = (int64_t)c.cw.cap, in->cig = c.cig.base, in->n_cig = (int64_t)c.cig.cap;
	}
	int emit_encode(int slot, const FastqBatch &fb, bool not_ori)
	{
		BeInput in;
		window(slot, fb, &in);
		in.not_ori = not_ori, in.T = tab.view(n_header);
		be_emit_host(in, fb.n_pairs(), &main_rec[slot]);
		return 0;
	}
	static void view_of(const BeHostResult &r, aln::EmitView *v) { v->bytes = r.bytes.data(), v->off = r.pair_off.data(), v->state = r.state.data(); }
	int emit_download(int slot, long long, aln::EmitView *v) { view_of(main_rec[slot], v); return 0; }
};

struct HostOriSource : aln::OriSource {
	OriDriver &drv;
	explicit HostOriSource(OriDriver &d) : drv(d) {}
	int encode(int slot, const FastqBatch &fb, long long *declined) override
	{
		if (drv.fail_ori_from >= 0 && ++drv.n_ori_calls >= drv.fail_ori_from) { CpuDriver::err() = "injected failure of the ori encode"; return 7; }
		BoInput in;
		drv.window(slot, fb, &in);
		in.min_filter_score = drv.mfs, in.n_header = drv.n_header;
		bo_emit_host(in, fb.n_pairs(), &drv.ori_rec[slot]);
		*declined = drv.ori_rec[slot].n_declined;
		return 0;
	}
	long long main_declined(int slot) override { return drv.main_rec[slot].n_declined; }
	int download(int slot, long long, aln::EmitView *v) override { OriDriver::view_of(drv.ori_rec[slot], v); return 0; }
	int fetch_text(FastqBatch &fb) override
	{
		const int slot = drv.slot_of(fb);
		if (slot < 0 || fb.text != kPoison) { CpuDriver::err() = "fetch_text: not a piece whose text is pending"; return 7; }
		fb.text = drv.real_text[slot], fb.text_fetched += fb.text_pending, fb.text_pending = 0, ++drv.n_fetches;
		return 0;
	}
	const char *last_error() override { return CpuDriver::err().c_str(); }
};

int main(int argc, char **argv)
{
	aln::PipeOpt o;
	std::string out = "./output.bam", out_ori = "./output_ori.bam", records;
	std::vector<const char *> pos;
	long long fail_from = -1;
	for (int i = 1; i < argc; ++i) {
		const bool arg = i + 1 < argc;
		if (!strcmp(argv[i], "--ori-device")) o.ori_device = o.emit_device = o.parse_device = true;
		else if (!strcmp(argv[i], "--fail-ori") && arg) fail_from = atoll(argv[++i]);
		else if (!strcmp(argv[i], "-Q")) o.not_ori = true;
		else if (!strcmp(argv[i], "-t") && arg) o.thread_n = atoi(argv[++i]);
		else if (!strcmp(argv[i], "-o") && arg) out = argv[++i];
		else if (!strcmp(argv[i], "-p") && arg) out_ori = argv[++i];
		else if (!strcmp(argv[i], "--batch") && arg) o.batch_pairs = atoll(argv[++i]);
		else if (!strcmp(argv[i], "--sub-batch") && arg) o.sub_pairs = atoll(argv[++i]);
		else if (!strcmp(argv[i], "--records") && arg) records = argv[++i];
		else pos.push_back(argv[i]);
	}
	if (pos.size() != 3 || o.thread_n < 1 || o.batch_pairs < 1) { fprintf(stderr, "usage: aln_ori_pipeline_check [--ori-device] [--fail-ori N] [options] <index_dir> <reads.fq> <header.sam>\n"); return 1; }
	HostIndex hi;
	hi.keep_sparse = true;
	std::string err;
	if (!hi.load_dir(pos[0], pos[2], &err)) { fprintf(stderr, "%s\n", err.c_str()); return 2; }
	HeaderInfo H;
	if (!H.load(pos[2])) { fprintf(stderr, "cannot read %s\n", pos[2]); return 2; }
	std::vector<BamRef> refs;
	for (size_t i = 0; i < H.names.size(); ++i) refs.push_back({H.names[i], H.lens[i]});
	aln::RunStats st;
	st.devices = 1, st.threads = o.thread_n;
	st.wall0 = aln::walltime();
	FastqReader fq;
	if (!fq.open(pos[1])) { fprintf(stderr, "%s\n", fq.error().c_str()); return 2; }
	aln::OutFile fo, fo_ori;
	if (!fo.open(out, true, H, refs, o.thread_n) || !fo_ori.open(out_ori, true, H, refs, o.thread_n)) { fprintf(stderr, "fail to open output file\n"); return 2; }
	FILE *frec = records.empty() ? nullptr : fopen(records.c_str(), "w");
	psvr_aln_params_t par;
	aln_params_default(&par);
	HostSvNames svn;
	svn.h = &hi;
	SamEmitter em;
	em.H = &H, em.sv = &svn, em.as_bam = true, em.not_ori = o.not_ori, em.stats = &st.emit;
	OriDriver drv(hi, (int)H.names.size(), 1);
	drv.fail_ori_from = fail_from;
	HostOriSource src(drv);
	aln::AlnPipeline<OriDriver> pipe(o, drv, fq, par, em, fo, fo_ori, nullptr, frec, st, true, nullptr, o.ori_device ? &src : nullptr);
	pipe.run();
	if (!fo.close() || !fo_ori.close()) { fprintf(stderr, "fail to write output file\n"); return 2; }
	if (frec) fclose(frec);
	st.wall = aln::walltime() - st.wall0;
	st.print(0);
	fprintf(stderr, "ori_pipeline pieces %lld resident %lld text_fetches %lld downloads %lld ori_device_pairs %lld ori_declined_pairs %lld ori_spliced_pairs %lld ori_pieces %lld ori_host_pieces %lld\n", st.n_batches,
	        st.resident_pieces, drv.n_fetches, drv.n_downloads, st.ori_device_pairs, st.ori_declined_pairs, st.ori_spliced_pairs, st.n_ori_pieces, st.n_ori_host_pieces);
	return 0;
}
