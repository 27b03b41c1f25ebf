// sr_replay.cpp -- a stand-alone program that replays the short-read host forms, for runs of the host code under a sanitizer (no Python, nothing preloaded).
//   sr_replay seeds batch.bin [threads]: one batch of seed matches through mm2gb_collect_seeds_heap_host.  Input: the file tests/sr_cases.py's dump_batch() writes -- six
//     int64 (reads, seeds, hits, anchors, the option flag, tied reads), then seed_off, the seed records, hit_off, the hits, the reads' lengths, and the expected offsets
//     and anchors (the plain-Python restatement's).  Every offset, every anchor and the count of tied reads are compared with the file's.
//   sr_replay align batch.bin [threads]: one batch of records and anchors through mm2gb_align_regs_sr_host.  Input: the file tests/align_cases.py's dump_batch() writes
//     (as tests/tools/align_replay.cpp reads it); a digest of the record offsets, records and words is compared with the file's.
// Either runs at 1 and at the given number of threads; exit status 0 when all agree.
//   hipcc -O1 -g -std=c++17 -ffp-contract=off -fsanitize=address,undefined -fno-omit-frame-pointer -I include tests/tools/sr_replay.cpp mm2-gb_amd/csrc/seed_heap_host.cpp \
//       mm2-gb_amd/csrc/align_host.cpp mm2-gb_amd/csrc/ksw_host.cpp mm2-gb_amd/csrc/host_chain.cpp -o sr_replay -lpthread
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>
#include "mm2gb_chain.h"

namespace mm2gb {          // what the library's engine unit provides to the host units
static std::string g_err;
void set_error(const std::string &msg) { g_err = msg; }
int fail(const std::string &msg) { g_err = msg; return -1; }
}
extern "C" const char *mm2gb_last_error(void) { return mm2gb::g_err.c_str(); }

template <class T> static std::vector<T> take(FILE *f, int64_t n)
{
	std::vector<T> v((size_t)n);
	if (n > 0 && fread(v.data(), sizeof(T), (size_t)n, f) != (size_t)n) { fprintf(stderr, "short file\n"); exit(2); }
	return v;
}

static uint64_t fold(uint64_t h, const void *p, size_t n)
{
	const unsigned char *b = (const unsigned char*)p;
	for (size_t i = 0; i < n; ++i) h = (h ^ b[i]) * 1099511628211ULL;
	return h;
}

static int replay_align(FILE *f, int threads)
{
	const std::vector<int64_t> h = take<int64_t>(f, 8);      // k, hpc, n_ref, n_reads, n_regs, n_anchors, digest, sizeof opt
	if (h[7] != (int64_t)sizeof(mm2gb_align_opt_t)) { fprintf(stderr, "option block of another size\n"); return 2; }
	mm2gb_align_opt_t opt = take<mm2gb_align_opt_t>(f, 1)[0];
	const std::vector<int32_t> ref_len = take<int32_t>(f, h[2]), read_len = take<int32_t>(f, h[3]);
	const std::vector<int64_t> reg_off = take<int64_t>(f, h[3] + 1), a_off = take<int64_t>(f, h[3] + 1);
	const std::vector<mm2gb_reg_t> regs = take<mm2gb_reg_t>(f, h[4]);
	const std::vector<mm2gb_anchor_t> anchors = take<mm2gb_anchor_t>(f, h[5]);
	std::vector<std::vector<char>> refs, reads;
	std::vector<const char*> ref_p, read_p;
	for (int32_t n : ref_len) refs.push_back(take<char>(f, n));
	for (int32_t n : read_len) reads.push_back(take<char>(f, n));
	for (auto &v : refs) ref_p.push_back(v.data());
	for (auto &v : reads) read_p.push_back(v.data());
	int bad = 0;
	for (int nt : { 1, threads }) {
		mm2gb_align_out_t out;
		int64_t cnt[MM2GB_SR_N_COUNTS];
		if (mm2gb_align_regs_sr_host(&opt, (int)h[0], (int)h[1], (int32_t)h[2], ref_p.data(), ref_len.data(), h[3], read_p.data(), read_len.data(), reg_off.data(), regs.data(),
		                             a_off.data(), anchors.data(), nt, &out, cnt)) { fprintf(stderr, "error: %s\n", mm2gb_last_error()); return 1; }
		uint64_t d = 1469598103934665603ULL;
		d = fold(d, out.reg_off, (size_t)(h[3] + 1) * 8);
		d = fold(d, out.regs, (size_t)out.n_regs * sizeof(mm2gb_reg_t));
		d = fold(d, out.cigar, (size_t)out.n_cigar * 4);
		printf("%d threads: records %lld words %lld fills ungapped %lld run again %lld short stretches %lld digest %016llx expected %016llx\n", nt, (long long)out.n_regs, (long long)out.n_cigar,
		       (long long)cnt[MM2GB_SR_N_FILL_UNGAPPED], (long long)cnt[MM2GB_SR_N_FILL_RERUN], (long long)cnt[MM2GB_SR_N_STRETCH_SHORT], (unsigned long long)d, (unsigned long long)h[6]);
		bad += d != (uint64_t)h[6];
		mm2gb_align_out_free(&out);
	}
	return bad ? 1 : 0;
}

int main(int argc, char **argv)
{
	if (argc < 3 || (strcmp(argv[1], "seeds") != 0 && strcmp(argv[1], "align") != 0)) { fprintf(stderr, "usage: sr_replay seeds|align batch.bin [threads]\n"); return 2; }
	const bool align = !strcmp(argv[1], "align");
	++argv; --argc;
	FILE *f = fopen(argv[1], "rb");
	if (!f) { perror(argv[1]); return 2; }
	if (align) { const int rc = replay_align(f, argc > 2 ? atoi(argv[2]) : 16); fclose(f); return rc; }
	const std::vector<int64_t> h = take<int64_t>(f, 6);
	const int64_t n_reads = h[0], n_seeds = h[1], n_hits = h[2], n_anchors = h[3], flag = h[4], n_tied = h[5];
	const std::vector<int64_t> seed_off = take<int64_t>(f, n_reads + 1);
	const std::vector<mm2gb_seed_t> seeds = take<mm2gb_seed_t>(f, n_seeds);
	const std::vector<int64_t> hit_off = take<int64_t>(f, n_seeds + 1);
	// the arrays are exactly as long as the batch says: a read or write past a read's last hit is one past an allocation
	const std::vector<uint64_t> hits = take<uint64_t>(f, n_hits);
	const std::vector<int32_t> qlen = take<int32_t>(f, n_reads);
	const std::vector<int64_t> want_off = take<int64_t>(f, n_reads + 1);
	const std::vector<mm2gb_anchor_t> want = take<mm2gb_anchor_t>(f, n_anchors);
	fclose(f);
	const int threads = argc > 2 ? atoi(argv[2]) : 16;
	int64_t bad = 0;
	for (int nt : { 1, threads }) {
		std::vector<int64_t> off((size_t)n_reads + 1, -1);
		std::vector<mm2gb_anchor_t> out((size_t)n_hits);
		int64_t tied = -1;
		if (mm2gb_collect_seeds_heap_host(flag, n_reads, seed_off.data(), seeds.data(), hit_off.data(), hits.data(), qlen.data(), nullptr, 0, nullptr, nullptr, nt, off.data(), out.data(), &tied)) {
			fprintf(stderr, "error: %s\n", mm2gb_last_error());
			return 1;
		}
		int64_t bad_off = 0, bad_a = 0;
		for (int64_t r = 0; r <= n_reads; ++r) bad_off += off[(size_t)r] != want_off[(size_t)r];
		if (!bad_off) for (int64_t k = 0; k < n_anchors; ++k) bad_a += out[(size_t)k].x != want[(size_t)k].x || out[(size_t)k].y != want[(size_t)k].y;
		printf("%d threads: %lld reads, %lld hits, %lld anchors, %lld tied reads (file: %lld), %lld offsets differ, %lld anchors differ\n", nt, (long long)n_reads, (long long)n_hits,
		       (long long)off[(size_t)n_reads], (long long)tied, (long long)n_tied, (long long)bad_off, (long long)bad_a);
		bad += bad_off + bad_a + (tied != n_tied);
	}
	return bad ? 1 : 0;
}
