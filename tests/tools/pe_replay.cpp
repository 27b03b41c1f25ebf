// pe_replay.cpp -- a stand-alone program that replays the host code of the paired-end path, for runs under a sanitizer (no Python, nothing preloaded).
//   pe_replay batch.bin: the file tests/pe_cases.py's dump_replay() writes -- the contigs and the fixture's reads as they are mapped, the seed options, per fragment the
//   expected number of seeds, hits and rep_len, and the recorded input and output of mm_select_sub_multi and mm_seg_gen.  The program forms the fragments from the names
//   (mm2gb_frag_offsets), builds the index, seeds every fragment (mm2gb_collect_matches_frag), and runs mm2gb_select_sub_multi_host and mm2gb_seg_gen_host; everything is
//   compared with the file's.  The arrays are exactly as long as the file says, so a read or write past a fragment's last record is one past an allocation.
//   Exit status 0 when all agree.  The calls live in the library's host units; build those under the sanitizer (make -C mm2-gb_amd host-asan) and link this program to them:
//   hipcc -O1 -g -std=c++17 -fsanitize=address,undefined -fno-omit-frame-pointer -I include tests/tools/pe_replay.cpp -o pe_replay \
//       -L mm2-gb_amd/build/asan -lmm2gb_chain_asan -Wl,-rpath,$PWD/mm2-gb_amd/build/asan
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>
#include "mm2gb_chain.h"

template <class T> static std::vector<T> take(FILE *f, int64_t n)
{
	std::vector<T> v((size_t)n);
	if (n > 0 && fread(v.data(), sizeof(T), (size_t)n, f) != (size_t)n) { fprintf(stderr, "short file\n"); exit(2); }
	return v;
}

static std::vector<std::string> take_strings(FILE *f, int64_t n)
{
	const std::vector<int32_t> len = take<int32_t>(f, n);
	std::vector<std::string> out;
	for (int32_t l : len) { const std::vector<char> s = take<char>(f, l); out.emplace_back(s.begin(), s.end()); }
	return out;
}

int main(int argc, char **argv)
{
	if (argc < 2) { fprintf(stderr, "usage: pe_replay batch.bin\n"); return 2; }
	FILE *f = fopen(argv[1], "rb");
	if (!f) { perror(argv[1]); return 2; }
	// n_ctg, n_reads, n_frag, k, w, mid_occ, max_max_occ, occ_dist, n_pairs, n_in, n_kept, n_anchors, n_seg_regs, n_seg_anchors, min_diff, best_n
	const std::vector<int64_t> h = take<int64_t>(f, 16);
	const std::vector<float> fl = take<float>(f, 4);               // q_occ_frac, pri_ratio, pri1, pri2
	const std::vector<std::string> ctg = take_strings(f, h[0]), names = take_strings(f, h[1]), seqs = take_strings(f, h[1]);
	const std::vector<int32_t> want_frag_off = take<int32_t>(f, h[2] + 1), want_seeds = take<int32_t>(f, h[2]), want_rep = take<int32_t>(f, h[2]);
	const std::vector<int64_t> want_hits = take<int64_t>(f, h[2]);
	const int64_t P = h[8];
	const std::vector<int32_t> qlens = take<int32_t>(f, 2 * P), n_segs = take<int32_t>(f, P), max_gap_ref = take<int32_t>(f, P);
	const std::vector<uint32_t> hash = take<uint32_t>(f, P);
	const std::vector<int64_t> in_off = take<int64_t>(f, P + 1), kept_off = take<int64_t>(f, P + 1), a_off = take<int64_t>(f, P + 1);
	std::vector<mm2gb_reg_t> regs_in = take<mm2gb_reg_t>(f, h[9]);
	const std::vector<mm2gb_reg_t> regs_kept = take<mm2gb_reg_t>(f, h[10]);
	const std::vector<mm2gb_anchor_t> anchors = take<mm2gb_anchor_t>(f, h[11]);
	const std::vector<int64_t> seg_r_off = take<int64_t>(f, 2 * P + 1), seg_a_off = take<int64_t>(f, 2 * P + 1);
	const std::vector<mm2gb_reg_t> seg_regs = take<mm2gb_reg_t>(f, h[12]);
	const std::vector<mm2gb_anchor_t> seg_anchors = take<mm2gb_anchor_t>(f, h[13]);
	fclose(f);
	int64_t bad = 0;
	// fragments
	std::vector<const char*> name_p, seq_p, ctg_p;
	std::vector<int32_t> lens, ctg_len;
	for (const std::string &s : names) name_p.push_back(s.c_str());
	for (const std::string &s : seqs) { seq_p.push_back(s.data()); lens.push_back((int32_t)s.size()); }
	for (const std::string &s : ctg) { ctg_p.push_back(s.data()); ctg_len.push_back((int32_t)s.size()); }
	std::vector<int32_t> frag_off((size_t)h[1] + 1, -1);
	int32_t n_frag = -1;
	if (mm2gb_frag_offsets((int32_t)h[1], name_p.data(), frag_off.data(), &n_frag)) { fprintf(stderr, "error: %s\n", mm2gb_last_error()); return 1; }
	bad += n_frag != h[2];
	for (int64_t i = 0; i <= h[2] && n_frag == h[2]; ++i) bad += frag_off[(size_t)i] != want_frag_off[(size_t)i];
	printf("%d fragments of %lld reads (file: %lld)\n", n_frag, (long long)h[1], (long long)h[2]);
	if (bad) return 1;
	// seeding
	mm2gb_index_t *ix = mm2gb_index_build((int)h[3], (int)h[4], (int32_t)h[0], ctg_p.data(), ctg_len.data(), 4);
	if (!ix) { fprintf(stderr, "error: %s\n", mm2gb_last_error()); return 1; }
	const mm2gb_seed_opt_t so = { (int32_t)h[5], (int32_t)h[6], (int32_t)h[7], fl[0] };
	int64_t bad_seed = 0, all_seeds = 0;
	for (int32_t u = 0; u < n_frag; ++u) {
		mm2gb_matches_t m;
		const int32_t r0 = frag_off[(size_t)u], n = frag_off[(size_t)u + 1] - r0;
		if (mm2gb_collect_matches_frag(ix, n, seq_p.data() + r0, lens.data() + r0, &so, &m)) { fprintf(stderr, "error: %s\n", mm2gb_last_error()); return 1; }
		bad_seed += m.n_seeds != want_seeds[(size_t)u] || m.rep_len != want_rep[(size_t)u] || m.n_hits != want_hits[(size_t)u];
		all_seeds += m.n_seeds;
		mm2gb_matches_free(&m);
	}
	mm2gb_index_destroy(ix);
	printf("seeding: %lld seeds, %lld fragments differ\n", (long long)all_seeds, (long long)bad_seed);
	// mm_select_sub_multi
	std::vector<int32_t> n_kept((size_t)P, -1);
	if (mm2gb_select_sub_multi_host(fl[1], fl[2], fl[3], (int32_t)h[14], (int32_t)h[15], P, n_segs.data(), qlens.data(), max_gap_ref.data(), in_off.data(), regs_in.data(), n_kept.data())) {
		fprintf(stderr, "error: %s\n", mm2gb_last_error());
		return 1;
	}
	int64_t bad_sel = 0;
	for (int64_t p = 0; p < P; ++p) {
		const int64_t want_n = kept_off[(size_t)p + 1] - kept_off[(size_t)p];
		if (n_kept[(size_t)p] != want_n || (want_n > 0 && memcmp(regs_in.data() + in_off[(size_t)p], regs_kept.data() + kept_off[(size_t)p], (size_t)want_n * sizeof(mm2gb_reg_t)) != 0)) ++bad_sel;
	}
	printf("mm_select_sub_multi: %lld records in, %lld kept, %lld fragments differ\n", (long long)h[9], (long long)h[10], (long long)bad_sel);
	// mm_seg_gen
	mm2gb_seg_out_t so_out;
	if (mm2gb_seg_gen_host(P, n_segs.data(), qlens.data(), hash.data(), kept_off.data(), regs_kept.data(), a_off.data(), anchors.data(), &so_out)) { fprintf(stderr, "error: %s\n", mm2gb_last_error()); return 1; }
	int64_t bad_seg = memcmp(so_out.reg_off, seg_r_off.data(), (size_t)(2 * P + 1) * 8) != 0 || memcmp(so_out.anchor_off, seg_a_off.data(), (size_t)(2 * P + 1) * 8) != 0;
	if (!bad_seg) bad_seg = (h[12] > 0 && memcmp(so_out.regs, seg_regs.data(), (size_t)h[12] * sizeof(mm2gb_reg_t)) != 0) || (h[13] > 0 && memcmp(so_out.anchors, seg_anchors.data(), (size_t)h[13] * sizeof(mm2gb_anchor_t)) != 0);
	mm2gb_seg_out_free(&so_out);
	printf("mm_seg_gen: %lld per-mate records, %lld anchors, %s\n", (long long)h[12], (long long)h[13], bad_seg ? "differ" : "equal");
	return bad + bad_seed + bad_sel + bad_seg ? 1 : 0;
}
