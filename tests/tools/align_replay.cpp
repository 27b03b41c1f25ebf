// align_replay.cpp -- a stand-alone program that replays one batch through mm2gb_align_regs_host, for runs of the host code under a sanitizer
// (no Python, nothing preloaded).  Input: the file tests/align_cases.py's dump_batch() writes -- int64 counts, then the arrays.  It prints a
// digest of the results and compares with the digest stored in the file; exit status 0 when they agree.
//   hipcc -O1 -g -std=c++17 -ffp-contract=off -fsanitize=address,undefined -I include tests/tools/align_replay.cpp \
//       mm2-gb_amd/csrc/align_host.cpp mm2-gb_amd/csrc/ksw_host.cpp mm2-gb_amd/csrc/host_chain.cpp -o align_replay -lpthread
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

int main(int argc, char **argv)
{
	if (argc < 2) { fprintf(stderr, "usage: align_replay batch.bin [threads]\n"); return 2; }
	FILE *f = fopen(argv[1], "rb");
	if (!f) { perror(argv[1]); return 2; }
	const std::vector<int64_t> h = take<int64_t>(f, 8);      // k, hpc, n_ref, n_reads, n_regs, n_anchors, digest, sizeof opt
	if (h[7] != (int64_t)sizeof(mm2gb_align_opt_t)) { fprintf(stderr, "option block of another size\n"); return 2; }
	mm2gb_align_opt_t opt = take<mm2gb_align_opt_t>(f, 1)[0];
	const std::vector<int32_t> ref_len = take<int32_t>(f, h[2]), read_len = take<int32_t>(f, h[3]);
	const std::vector<int64_t> reg_off = take<int64_t>(f, h[3] + 1), a_off = take<int64_t>(f, h[3] + 1);
	const std::vector<mm2gb_reg_t> regs = take<mm2gb_reg_t>(f, h[4]);
	const std::vector<mm2gb_anchor_t> anchors = take<mm2gb_anchor_t>(f, h[5]);
	std::vector<std::vector<char>> refs, reads;
	std::vector<const char*> ref_p, read_p;
	for (int32_t n : ref_len) { refs.push_back(take<char>(f, n)); }
	for (int32_t n : read_len) { reads.push_back(take<char>(f, n)); }
	for (auto &v : refs) ref_p.push_back(v.data());
	for (auto &v : reads) read_p.push_back(v.data());
	fclose(f);
	mm2gb_align_out_t out;
	const int threads = argc > 2 ? atoi(argv[2]) : 4;
	if (mm2gb_align_regs_host(&opt, (int)h[0], (int)h[1], (int32_t)h[2], ref_p.data(), ref_len.data(), h[3], read_p.data(), read_len.data(), reg_off.data(), regs.data(),
	                          a_off.data(), anchors.data(), threads, &out)) { fprintf(stderr, "error: %s\n", mm2gb_last_error()); return 1; }
	uint64_t d = 1469598103934665603ULL;
	d = fold(d, out.reg_off, (size_t)(h[3] + 1) * 8);
	d = fold(d, out.regs, (size_t)out.n_regs * sizeof(mm2gb_reg_t));
	d = fold(d, out.cigar, (size_t)out.n_cigar * 4);
	printf("records %lld words %lld digest %016llx expected %016llx\n", (long long)out.n_regs, (long long)out.n_cigar, (unsigned long long)d, (unsigned long long)h[6]);
	mm2gb_align_out_free(&out);
	return d == (uint64_t)h[6] ? 0 : 1;
}
