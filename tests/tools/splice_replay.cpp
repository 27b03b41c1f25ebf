// splice_replay.cpp -- a stand-alone program that replays one spliced batch through mm2gb_align_regs_splice_host and its records through
// mm2gb_aln_text_splice_host (cg + cs, then MD), for runs of the host code under a sanitizer (no Python, nothing preloaded).  Input: the file
// tests/splice_cases.py's dump_batch() writes -- int64 counts, the option record, then the arrays.  It prints a digest of the results (record
// offsets, records, trans_strand of every record, words) and one of the two texts, and compares with the digests stored in the file; exit
// status 0 when both agree.
//   hipcc -O1 -g -std=c++17 -ffp-contract=off -fsanitize=address,undefined -I include tests/tools/splice_replay.cpp \
//       mm2-gb_amd/csrc/align_host.cpp mm2-gb_amd/csrc/aln_text_host.cpp mm2-gb_amd/csrc/ksw_host.cpp mm2-gb_amd/csrc/host_chain.cpp -o splice_replay -lpthread
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
	if (argc < 2) { fprintf(stderr, "usage: splice_replay batch.bin [threads]\n"); return 2; }
	FILE *f = fopen(argv[1], "rb");
	if (!f) { perror(argv[1]); return 2; }
	const std::vector<int64_t> h = take<int64_t>(f, 8);      // k, hpc, n_ref, n_reads, n_regs, n_anchors, digest, sizeof opt
	if (h[7] != (int64_t)sizeof(mm2gb_align_splice_opt_t)) { fprintf(stderr, "option block of another size\n"); return 2; }
	mm2gb_align_splice_opt_t opt = take<mm2gb_align_splice_opt_t>(f, 1)[0];
	const uint64_t want_text = take<uint64_t>(f, 1)[0];
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
	int64_t paths[MM2GB_SPL_N_COUNTS];
	if (mm2gb_align_regs_splice_host(&opt, (int)h[0], (int)h[1], (int32_t)h[2], ref_p.data(), ref_len.data(), h[3], read_p.data(), read_len.data(), reg_off.data(), regs.data(),
	                          a_off.data(), anchors.data(), threads, &out, paths)) { fprintf(stderr, "error: %s\n", mm2gb_last_error()); return 1; }
	uint64_t d = 1469598103934665603ULL;
	d = fold(d, out.reg_off, (size_t)(h[3] + 1) * 8);
	d = fold(d, out.regs, (size_t)out.n_regs * sizeof(mm2gb_reg_t));
	for (int64_t i = 0; i < out.n_regs; ++i) d = fold(d, &out.aln[i].trans_strand, 4);
	d = fold(d, out.cigar, (size_t)out.n_cigar * 4);
	int64_t trials = 0;
	for (int k = MM2GB_SPL_N_TRIAL_FOR_WON; k <= MM2GB_SPL_N_TRIAL_TIE_KEPT_1; ++k) trials += paths[k];
	printf("records %lld words %lld chains with two trials %lld digest %016llx expected %016llx\n", (long long)out.n_regs, (long long)out.n_cigar, (long long)trials, (unsigned long long)d, (unsigned long long)h[6]);
	std::vector<int32_t> read_of((size_t)out.n_regs);
	for (int64_t r = 0; r < h[3]; ++r) for (int64_t i = out.reg_off[r]; i < out.reg_off[r + 1]; ++i) read_of[(size_t)i] = (int32_t)r;
	uint64_t dt = 1469598103934665603ULL;
	for (int what : { MM2GB_TEXT_CG | MM2GB_TEXT_CS, MM2GB_TEXT_MD }) {
		int64_t *off = nullptr; char *text = nullptr;
		if (mm2gb_aln_text_splice_host(what, (int32_t)h[2], ref_p.data(), ref_len.data(), h[3], read_p.data(), read_len.data(), out.n_regs, out.regs, read_of.data(), out.aln, out.cigar,
		                               threads, &off, &text)) { fprintf(stderr, "error: %s\n", mm2gb_last_error()); return 1; }
		dt = fold(dt, off, (size_t)(out.n_regs + 1) * 8);
		dt = fold(dt, text, (size_t)off[out.n_regs]);
		free(off); free(text);
	}
	printf("text digest %016llx expected %016llx\n", (unsigned long long)dt, (unsigned long long)want_text);
	mm2gb_align_out_free(&out);
	return d == (uint64_t)h[6] && dt == want_text ? 0 : 1;
}
