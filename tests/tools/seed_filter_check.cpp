// seed_filter_check -- host checks of the seeding filter of pansvr_amd/csrc/aln_device.h (driven by tests/test_seed_filter.py):
//   rc20             rc20 is an involution, a 20-mer and its reverse complement share their filter word (palindromes included)
//   index DIR [OUT]  the filter of an index fixture, built on the host by the build rule (the mask of every indexed 20-mer, in the word
//                    bloom_slot names), passes every indexed 20-mer; OUT: the filter's words, for the comparison with the device's
//   rates            pass rates of absent k-mers under the canonical rule and under the rule it replaced, same keys and queries
//   pair             the lane-pair scheme (two "lanes" running seed_pair_half, halves exchanged) against kmer_maybe_present per strand
// Exit status 0 = every check of the mode held; the figures are printed either way.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>
#include "../../pansvr_amd/csrc/aln_device.h"

using namespace psvr;

static uint64_t rng_state = 0x243F6A8885A308D3ull;
static uint64_t rnd()                                    // splitmix64
{
	uint64_t z = (rng_state += 0x9E3779B97F4A7C15ull);
	z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
	z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
	return z ^ (z >> 31);
}
static const uint64_t kMask40 = (1ull << 40) - 1;

// the engine's sizing rule (index_upload): ~10 bits per key, a power of two of 64-bit words, 1 MB to 1 GB
static int filter_lg(uint64_t n_keys)
{
	int lg = 20;
	while (lg < 30 && ((uint64_t)8 << lg) < n_keys * 10) ++lg;
	return lg;
}

static uint64_t rc20_slow(uint64_t x)
{
	uint64_t r = 0;
	for (int i = 0; i < 20; ++i) r = (r << 2) | (3 - ((x >> (2 * i)) & 3));
	return r;
}

static int mode_rc20()
{
	int bad = 0;
	std::vector<uint64_t> xs = {0, kMask40, 1, 1ull << 39, 0x123456789aull};
	for (int i = 0; i < 200000; ++i) xs.push_back(rnd() & kMask40);
	for (int i = 0; i < 2000; ++i) {                        // palindromes: second half = reverse complement of the first
		uint64_t h = rnd() & ((1ull << 20) - 1), x = h << 20;
		for (int b = 0; b < 10; ++b) x |= (3 - ((h >> (2 * b)) & 3)) << (2 * (9 - b));
		if (rc20(x) != x) { printf("not a palindrome: %010llx\n", (unsigned long long)x); ++bad; }
		xs.push_back(x);
	}
	for (uint64_t x : xs) {
		const uint64_t r = rc20(x);
		if (r != rc20_slow(x) || rc20(r) != x || (r >> 40)) { ++bad; continue; }
		for (uint32_t shift = 34; shift <= 47; shift += 13) {
			uint64_t w0, m0, w1, m1, w2, a, b;
			bloom_slot(x, shift, w0, m0), bloom_slot(r, shift, w1, m1), bloom_slot2(x, shift, w2, a, b);
			if (w0 != w1 || w2 != w0 || a != m0 || b != m1 || (x == r && m0 != m1)) ++bad;
			if (__builtin_popcountll(m0) > 3 || m0 == 0) ++bad;
		}
	}
	printf("rc20: %zu k-mers, %d failures\n", xs.size(), bad);
	return bad != 0;
}

static std::vector<unsigned char> slurp(const std::string &p)
{
	std::vector<unsigned char> v;
	FILE *f = fopen(p.c_str(), "rb");
	if (!f) { fprintf(stderr, "cannot read %s\n", p.c_str()); exit(2); }
	unsigned char buf[1 << 16];
	size_t n;
	while ((n = fread(buf, 1, sizeof buf, f)) > 0) v.insert(v.end(), buf, buf + n);
	fclose(f);
	return v;
}

static int mode_index(const char *dir, const char *out)
{
	const std::vector<unsigned char> sp = slurp(std::string(dir) + "/unipath_g.hash.sparse"), km = slurp(std::string(dir) + "/unipath_g.kmer");
	const uint32_t *spw = (const uint32_t *)sp.data(), *kmer = (const uint32_t *)km.data();
	const size_t nb = sp.size() / 8, n_kmer = km.size() / 4;
	const int lg = filter_lg(n_kmer);
	const uint32_t shift = (uint32_t)(64 - (lg - 3));
	std::vector<uint64_t> bloom((size_t)1 << (lg - 3), 0), keys;
	size_t i = 0;
	for (size_t b = 0; b < nb; ++b)
		for (uint32_t k = 0; k < spw[2 * b + 1]; ++k, ++i) keys.push_back(((uint64_t)spw[2 * b] << 12) | (uint64_t)(kmer[i] >> 4));
	if (i != n_kmer) { printf("index: %zu entries in the buckets, %zu in the k-mer file\n", i, n_kmer); return 1; }
	for (uint64_t x : keys) { uint64_t w, m; bloom_slot(x, shift, w, m); bloom[w] |= m; }
	DevIndex ix;
	memset(&ix, 0, sizeof ix);
	ix.bloom = bloom.data(), ix.bloom_shift = shift;
	size_t miss = 0, rc_pass = 0;
	for (uint64_t x : keys) miss += !kmer_maybe_present(ix, x), rc_pass += kmer_maybe_present(ix, rc20(x));
	printf("index: %zu indexed 20-mers, %zu words, shift %u, false negatives %zu, reverse complements passing %zu\n", keys.size(), bloom.size(), shift, miss, rc_pass);
	if (out) {
		FILE *f = fopen(out, "wb");
		if (!f || fwrite(bloom.data(), 8, bloom.size(), f) != bloom.size()) { fprintf(stderr, "cannot write %s\n", out); return 2; }
		fclose(f);
	}
	return miss != 0;
}

// the rule this filter replaced, as the baseline: word and bits from the k-mer itself
static void parent_slot(uint64_t kmer, uint32_t shift, uint64_t &word, uint64_t &mask)
{
	const uint64_t h = kmer * 0x9E3779B97F4A7C15ull;
	const uint64_t g = (h ^ (h >> 32)) * 0xD6E8FEB86659FD93ull;
	word = h >> shift;
	mask = (1ull << (g >> 58)) | (1ull << ((g >> 52) & 63)) | (1ull << ((g >> 46) & 63));
}

static int mode_rates()
{
	const size_t n = 800000;
	std::vector<uint64_t> keys(n), sorted;
	for (auto &k : keys) k = rnd() & kMask40;
	const int lg = filter_lg(n);
	const uint32_t shift = (uint32_t)(64 - (lg - 3));
	std::vector<uint64_t> fnew((size_t)1 << (lg - 3), 0), fold(fnew.size(), 0);
	for (uint64_t x : keys) {
		uint64_t w, m;
		bloom_slot(x, shift, w, m), fnew[w] |= m;
		parent_slot(x, shift, w, m), fold[w] |= m;
	}
	auto pass_new = [&](uint64_t x) { uint64_t w, m; bloom_slot(x, shift, w, m); return (fnew[w] & m) == m; };
	auto pass_old = [&](uint64_t x) { uint64_t w, m; parent_slot(x, shift, w, m); return (fold[w] & m) == m; };
	// absent = not a key (40-bit random k-mers hit one of 800 k keys with probability 1e-6: they are screened out all the same)
	sorted = keys;
	std::sort(sorted.begin(), sorted.end());
	auto is_key = [&](uint64_t x) { return std::binary_search(sorted.begin(), sorted.end(), x); };
	size_t nq = 0, a_new = 0, a_old = 0, nr = 0, r_new = 0, r_old = 0, fn = 0;
	for (size_t i = 0; i < 2000000; ++i) {
		const uint64_t x = rnd() & kMask40;
		if (is_key(x)) continue;
		++nq, a_new += pass_new(x), a_old += pass_old(x);
	}
	for (uint64_t k : keys) {
		fn += !pass_new(k);
		const uint64_t x = rc20(k);
		if (is_key(x)) continue;
		++nr, r_new += pass_new(x), r_old += pass_old(x);
	}
	const double s_an = (double)a_new / nq, s_ao = (double)a_old / nq, s_rn = (double)r_new / nr, s_ro = (double)r_old / nr;
	printf("rates: keys %zu bits_per_key %.2f false_negatives %zu\n", n, 64.0 * fnew.size() / n, fn);
	printf("rates: absent_canonical %.6f absent_parent %.6f revcomp_canonical %.6f revcomp_parent %.6f\n", s_an, s_ao, s_rn, s_ro);
	const bool ok = fn == 0 && s_an <= 2 * s_ao + 1e-3 && s_rn <= 2 * s_ro + 1e-3;
	printf("rates: bound 2 x parent + 1e-3 %s\n", ok ? "held" : "MISSED");
	return !ok;
}

static void pack(const std::vector<uint8_t> &b, std::vector<uint64_t> &w)
{
	w.assign(b.size() / 32 + 2, 0);
	for (size_t i = 0; i < b.size(); ++i) w[i >> 5] |= (uint64_t)b[i] << ((31 - (i & 31)) << 1);
}

static int mode_pair()
{
	// a "genome" whose 20-mers fill a small filter, reads cut from it (either strand, a few substitutions) and random ones
	const int G = 60000;
	std::vector<uint8_t> genome(G);
	for (auto &b : genome) b = (uint8_t)(rnd() & 3);
	for (int i = 0; i < 200; ++i) {                         // some palindromic stretches, so that palindromic 20-mers are looked up too
		const int p = 100 + (int)(rnd() % (G - 200));
		for (int k = 0; k < 12; ++k) genome[p + 12 + k] = (uint8_t)(3 - genome[p + 11 - k]);
	}
	std::vector<uint64_t> gw;
	pack(genome, gw);
	const int lg = 16;                                       // 8192 words for 60 k keys: dense enough that absent k-mers pass now and then
	const uint32_t shift = (uint32_t)(64 - (lg - 3));
	std::vector<uint64_t> bloom((size_t)1 << (lg - 3), 0);
	for (int i = 0; i + 20 <= G; ++i) { uint64_t w, m; bloom_slot(get_kmer((uint32_t)i, gw.data()), shift, w, m); bloom[w] |= m; }
	DevIndex ix;
	memset(&ix, 0, sizeof ix);
	ix.bloom = bloom.data(), ix.bloom_shift = shift;
	const int lens[] = {20, 24, 25, 100, 150, 250, 339};
	int bad = 0;
	size_t bits = 0, set = 0, paired = 0, pal = 0;
	for (int L : lens)
		for (int rep = 0; rep < 300; ++rep) {
			std::vector<uint8_t> b0(L), b1(L);
			const int kind = rep % 3;                         // from the genome forward, from its reverse strand, random
			const int p = (int)(rnd() % (G - L));
			for (int i = 0; i < L; ++i) b0[i] = kind == 2 ? (uint8_t)(rnd() & 3) : kind == 0 ? genome[p + i] : (uint8_t)(3 - genome[p + L - 1 - i]);
			if (kind != 2) for (int s = 0; s < (int)(rnd() % 4); ++s) b0[rnd() % L] = (uint8_t)(rnd() & 3);
			for (int i = 0; i < L; ++i) b1[L - 1 - i] = b0[i] ^ 3;      // prep_read
			std::vector<uint64_t> w[2];
			pack(b0, w[0]), pack(b1, w[1]);
			const int T = (L - kLenKmer) / kSeedStep + 1;
			uint64_t want[2] = {0, 0}, got[2] = {0, 0};
			for (int s = 0; s < 2; ++s)
				for (int t = 0; t < T && t < 64; ++t) {
					const uint64_t x = get_kmer((uint32_t)(t * kSeedStep), w[s].data());
					want[s] |= (uint64_t)kmer_maybe_present(ix, x) << t, pal += x == rc20(x);
				}
			if (seed_pair_applies(ix, L)) {
				uint64_t own[2], other[2];
				for (int s = 0; s < 2; ++s) seed_pair_half(ix, w[s].data(), T, s, own[s], other[s]);
				got[0] = own[0] | other[1], got[1] = own[1] | other[0];   // the neighbour swap
				++paired;
			} else {
				got[0] = want[0], got[1] = want[1];                         // per-strand loop: kmer_maybe_present itself
			}
			for (int s = 0; s < 2; ++s) {
				if (got[s] != want[s]) { if (bad < 5) printf("pair: L %d rep %d strand %d: %016llx != %016llx\n", L, rep, s, (unsigned long long)got[s], (unsigned long long)want[s]); ++bad; }
				bits += (size_t)(T < 64 ? T : 64), set += (size_t)__builtin_popcountll(want[s]);
			}
		}
	printf("pair: %zu answers (%zu pass, %zu of palindromes), %zu of %zu reads by the lane pair, %d strands differ\n", bits, set, pal, paired, (size_t)(7 * 300), bad);
	// lengths 20, 25, 100, 150, 250 mirror; 24 and 339 do not
	return bad != 0 || paired != 5 * 300 || set == 0 || set == bits;
}

int main(int argc, char **argv)
{
	const std::string mode = argc > 1 ? argv[1] : "";
	if (mode == "rc20") return mode_rc20();
	if (mode == "index" && argc > 2) return mode_index(argv[2], argc > 3 ? argv[3] : nullptr);
	if (mode == "rates") return mode_rates();
	if (mode == "pair") return mode_pair();
	fprintf(stderr, "usage: seed_filter_check rc20 | index DIR [OUT] | rates | pair\n");
	return 2;
}
