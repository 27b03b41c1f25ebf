// index_dev.h -- internal: the minimizer index as the host holds it (seeding.cpp) and the kernels that build it on a device
// (index_kernels.hip): the sort's input split from the sketch's pairs, the tables keys / first / bucket from the sorted keys, and the
// occurrence threshold's quantile by radix select.  The host build (mm2gb_index_build) stays the definition of every array.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <algorithm>
#include <mutex>
#include <vector>

namespace mm2gb {

struct SeedIndex {
	int k = 15, w = 10;
	int flag = 0;                           // MM2GB_I_*: how the sequences were sketched, and how every read mapped against it is
	std::vector<int32_t> lens;
	std::vector<uint64_t> keys;             // distinct minimizers (x >> 8), ascending
	std::vector<int64_t> first;             // keys.size() + 1: where each one's occurrences begin
	std::vector<uint64_t> where;            // occurrences, ascending within a minimizer
	// keys by their top bits: bucket[b] = first key with (key >> bucket_shift) >= b.  The hash spreads minimizers evenly over their 2k bits,
	// so a bucket holds a key or two and a look-up is one probe of this table and a search among those (a binary search over all keys:
	// ~20 dependent probes of a table that does not fit the cache, ~200 ns per minimizer of a read, most of what seeding cost)
	std::vector<uint32_t> bucket;
	int bucket_shift = 0;
	// the four arrays as they are, in a device's memory (index_on_device): one copy per device, made on first use -- or born there
	// (mm2gb_index_build_gpu) --, given up by mm2gb_index_destroy
	struct DevCopy { int device; void *ptr[4]; size_t bytes[4]; };
	mutable std::mutex dev_mu;
	mutable std::vector<DevCopy> dev;
	int built_on = -1;                      // the device mm2gb_index_build_gpu made it on (-1: the host build)
	mutable int64_t uploads = 0;            // host -> device copies index_on_device has made
	double build_ms[5] = { 0, 0, 0, 0, 0 }; // the device build's stages: H2D, sketch, sort, tables, D2H
	// bits of a key the bucket table is indexed by: about one key per bucket
	static int bucket_bits(int k, size_t n_keys)
	{
		int bits = 1;
		while (bits < 2 * k && ((size_t)1 << bits) < n_keys) ++bits;
		return std::min(bits, 26);
	}
	void build_buckets()
	{
		const int bits = bucket_bits(k, keys.size());
		bucket_shift = 2 * k - bits;
		bucket.assign(((size_t)1 << bits) + 1, 0);
		size_t at = 0;
		for (size_t b = 0; b <= (size_t)1 << bits; ++b) {
			while (at < keys.size() && (keys[at] >> bucket_shift) < b) ++at;
			bucket[b] = (uint32_t)at;
		}
	}
	const uint64_t *find(uint64_t minier, int *n) const
	{
		const uint64_t b = minier >> bucket_shift;
		if (b + 1 >= bucket.size()) { *n = 0; return nullptr; }
		const auto lo = keys.begin() + bucket[(size_t)b], hi = keys.begin() + bucket[(size_t)b + 1];
		const auto it = std::lower_bound(lo, hi, minier);
		if (it == hi || *it != minier) { *n = 0; return nullptr; }
		const size_t at = (size_t)(it - keys.begin());
		*n = (int)(first[at + 1] - first[at]);
		return where.data() + first[at];
	}
};

// ---- index_kernels.hip.  Every launch is on the stream given; a function that returns int returns -1 when a library call refused.
// the sketch's pairs (x, y) as the sort's input: key_out[i] = x >> 8, val_out[i] = y
void launch_ix_split(const ulonglong2 *mini, int64_t n, unsigned long long *key_out, unsigned long long *val_out, hipStream_t s);
// stable sort by bits [0, 2k) of the key (tmp == nullptr: only the work space's size, in tmp_bytes)
int  ix_sort_pairs(void *tmp, size_t &tmp_bytes, const unsigned long long *key_in, unsigned long long *key_out, const unsigned long long *val_in,
                   unsigned long long *val_out, int64_t n, int k, hipStream_t s);
// head[i] = key[i] != key[i-1] for i in [0, n), head[n] = 0; pos = exclusive scan of head over n + 1 entries (pos[n] = distinct keys)
int  ix_heads_scan(void *tmp, size_t &tmp_bytes, const unsigned long long *key, int64_t n, unsigned char *head, long long *pos, hipStream_t s);
// keys, first (with first[n_keys] = n) and every entry of bucket (2^bits + 1), as SeedIndex::build_buckets defines them
void launch_ix_tables(const unsigned long long *key, const unsigned char *head, const long long *pos, int64_t n, int64_t n_keys, int bits, int bucket_shift,
                      unsigned long long *keys_out, long long *first_out, uint32_t *bucket_out, hipStream_t s);
// the value of rank `rank` (0-based) among the counts first[i+1] - first[i], i in [0, n_keys): four histogram passes of 8 bits from the top.
// work: IX_SELECT_WORDS 64-bit words of device memory; the value is left in work[0]
constexpr int IX_SELECT_WORDS = 2 + 256;
void launch_ix_select(const long long *first, int64_t n_keys, unsigned long long rank, unsigned long long *work, int n_cu, hipStream_t s);

} // namespace mm2gb
