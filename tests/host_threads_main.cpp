// The fork-join helper of the host side (csrc/host_threads.h) alone: every index once, worker numbers 0 .. max(1, nt) - 1 each once,
// worker 0 and the one-thread case on the calling thread, never more workers than runs of `grain`.  Exit status 0 and "ok" when all hold.
#include <atomic>
#include <cstdio>
#include <mutex>
#include <set>
#include <thread>
#include <vector>
#include "host_threads.h"

static int failures = 0;
#define CHECK(cond, ...) do { if (!(cond)) { ++failures; fprintf(stderr, "FAILED %s: ", #cond); fprintf(stderr, __VA_ARGS__); fputc('\n', stderr); } } while (0)

static void check_run(int nt)
{
	const int want = nt > 1 ? nt : 1;
	const std::thread::id me = std::this_thread::get_id();
	std::vector<std::atomic<int>> seen((size_t)want);
	for (auto &s : seen) s = 0;
	std::atomic<int> outside(0), zero_elsewhere(0);
	std::mutex lock;
	std::set<std::thread::id> ids;
	mm2gb::run_on_threads(nt, [&](int k) {
		if (k < 0 || k >= want) { ++outside; return; }
		++seen[(size_t)k];
		if (k == 0 && std::this_thread::get_id() != me) ++zero_elsewhere;
		std::lock_guard<std::mutex> g(lock);
		ids.insert(std::this_thread::get_id());
	});
	CHECK(outside == 0, "run_on_threads(%d): a worker number outside 0..%d", nt, want - 1);
	for (int k = 0; k < want; ++k) CHECK(seen[(size_t)k] == 1, "run_on_threads(%d): worker %d ran %d times", nt, k, seen[(size_t)k].load());
	CHECK(zero_elsewhere == 0, "run_on_threads(%d): worker 0 is not the calling thread", nt);
	CHECK((int)ids.size() == want, "run_on_threads(%d): %zu threads for %d workers", nt, ids.size(), want);
}

static void check_each(size_t n, size_t grain, int nt)
{
	const std::thread::id me = std::this_thread::get_id();
	std::vector<std::atomic<int>> visits(n);
	for (auto &v : visits) v = 0;
	std::atomic<int> outside(0);
	std::mutex lock;
	std::set<std::thread::id> ids;
	mm2gb::for_each_on_threads(n, nt, grain, [&](size_t i) {
		if (i >= n) { ++outside; return; }
		++visits[i];
		std::lock_guard<std::mutex> g(lock);
		ids.insert(std::this_thread::get_id());
	});
	const size_t runs = (n + grain - 1) / grain, most = std::min<size_t>(runs, (size_t)(nt > 1 ? nt : 1));
	CHECK(outside == 0, "n %zu grain %zu nt %d: an index outside [0, n)", n, grain, nt);
	for (size_t i = 0; i < n; ++i) CHECK(visits[i] == 1, "n %zu grain %zu nt %d: index %zu visited %d times", n, grain, nt, i, visits[i].load());
	CHECK(ids.size() <= most, "n %zu grain %zu nt %d: %zu threads worked, at most %zu may", n, grain, nt, ids.size(), most);
	if (most <= 1 && n > 0) CHECK(ids.size() == 1 && *ids.begin() == me, "n %zu grain %zu nt %d: not inline on the calling thread", n, grain, nt);
	if (n == 0) CHECK(ids.empty(), "n 0: fn was called");
}

int main()
{
	const size_t ns[] = { 0, 1, 15, 16, 17, 1000 }, grains[] = { 1, 16, 64 };
	int cases = 0;
	for (size_t n : ns) {
		for (int nt : { 0, 1, 2, 16, (int)n + 5 }) check_run(nt);
		for (size_t grain : grains)
			for (int nt : { 0, 1, 2, 16, (int)n + 5 }) { check_each(n, grain, nt); ++cases; }
	}
	check_run(-3);
	if (failures) { fprintf(stderr, "%d checks failed\n", failures); return 1; }
	printf("ok %d cases\n", cases);
	return 0;
}
