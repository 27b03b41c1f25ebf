// host_threads.h -- the host side's one fork-join: the calling thread is worker 0, the others are spawned and joined before the return.
// An exception that leaves a spawned worker ends the process.
#pragma once
#include <algorithm>
#include <atomic>
#include <cstddef>
#include <thread>
#include <vector>

namespace mm2gb {

// work(k) for k in [0, max(1, nt)); nt <= 1: on the calling thread, nothing spawned
template <typename F>
void run_on_threads(int nt, F work)
{
	std::vector<std::thread> th;
	for (int k = 1; k < nt; ++k) th.emplace_back([&work, k]() { work(k); });
	work(0);
	for (std::thread &t : th) t.join();
}

// fn(i) once for every i in [0, n), dealt in runs of `grain` through one counter to min(nt, ceil(n / grain)) workers
template <typename F>
void for_each_on_threads(size_t n, int nt, size_t grain, F fn)
{
	if (n == 0) return;
	if (grain < 1) grain = 1;
	const size_t runs = (n + grain - 1) / grain;
	std::atomic<size_t> next(0);
	run_on_threads((int)std::min<size_t>((size_t)std::max(nt, 1), runs), [&](int) {
		for (;;) {
			const size_t lo = next.fetch_add(grain);
			if (lo >= n) break;
			for (size_t i = lo; i < std::min(n, lo + grain); ++i) fn(i);
		}
	});
}

} // namespace mm2gb
