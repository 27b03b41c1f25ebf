// ksw_single_replay.cpp -- a stand-alone program that replays one batch of single-affine DP jobs through mm2gb_ksw_extz2_host, for runs of the
// host code under a sanitizer (no Python, nothing preloaded).  Input: the file tests/ksw_single_cases.py's dump_batch() writes -- five int64
// counts (jobs, query bytes, target bytes, words, size of the parameter record), the parameter record, the job records, both sequence
// arrays, then the expected result records and CIGAR words.  It runs the batch at 1 and at the given number of threads and compares every
// record and every word with the file's; exit status 0 when all agree.
//   hipcc -O1 -g -std=c++17 -ffp-contract=off -fsanitize=address,undefined -fno-omit-frame-pointer -I include tests/tools/ksw_single_replay.cpp \
//       mm2-gb_amd/csrc/ksw_host.cpp -o ksw_single_replay -lpthread
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

int main(int argc, char **argv)
{
	if (argc < 2) { fprintf(stderr, "usage: ksw_single_replay batch.bin [threads]\n"); return 2; }
	FILE *f = fopen(argv[1], "rb");
	if (!f) { perror(argv[1]); return 2; }
	const std::vector<int64_t> h = take<int64_t>(f, 5);
	if (h[4] != (int64_t)sizeof(mm2gb_ksw_param_t)) { fprintf(stderr, "parameter record of another size\n"); return 2; }
	const mm2gb_ksw_param_t param = take<mm2gb_ksw_param_t>(f, 1)[0];
	const std::vector<mm2gb_ksw_job_t> jobs = take<mm2gb_ksw_job_t>(f, h[0]);
	// the arrays are exactly as long as the batch says: a read or write past a job's last residue is one past an allocation
	const std::vector<uint8_t> queries = take<uint8_t>(f, h[1]), targets = take<uint8_t>(f, h[2]);
	const std::vector<mm2gb_ksw_res_t> want = take<mm2gb_ksw_res_t>(f, h[0]);
	const std::vector<uint32_t> want_words = take<uint32_t>(f, h[3]);
	fclose(f);
	const int threads = argc > 2 ? atoi(argv[2]) : 16;
	int64_t bad = 0;
	for (int nt : { 1, threads }) {
		std::vector<mm2gb_ksw_res_t> res((size_t)h[0]);
		uint32_t *words = nullptr;
		int64_t n_words = 0;
		if (mm2gb_ksw_extz2_host(&param, h[0], jobs.data(), queries.data(), targets.data(), nt, res.data(), &words, &n_words)) { fprintf(stderr, "error: %s\n", mm2gb_last_error()); return 1; }
		int64_t bad_res = 0, bad_words = n_words != h[3];
		for (int64_t j = 0; j < h[0]; ++j) bad_res += memcmp(&res[(size_t)j], &want[(size_t)j], sizeof(mm2gb_ksw_res_t)) != 0;
		if (n_words == h[3]) for (int64_t k = 0; k < n_words; ++k) bad_words += words[k] != want_words[(size_t)k];
		printf("%d threads: %lld jobs, %lld words, %lld records differ, %lld words differ\n", nt, (long long)h[0], (long long)n_words, (long long)bad_res, (long long)bad_words);
		bad += bad_res + bad_words;
		free(words);
	}
	return bad ? 1 : 0;
}
