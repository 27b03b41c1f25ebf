// kmer.h -- internal: a base's code and the hash of a k-mer, one definition for the host sketch (seeding.cpp) and the device's (seed_kernels.hip).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace mm2gb {

__host__ __device__ inline int base_code(unsigned char c)      // A C G T (either case, U as T) -> 0..3, anything else 4
{
	switch (c) {
	case 'A': case 'a': return 0;
	case 'C': case 'c': return 1;
	case 'G': case 'g': return 2;
	case 'T': case 't': case 'U': case 'u': return 3;
	default: return 4;
	}
}

// invertible integer hash of a 2k-bit k-mer (sketch.c:29-39)
__host__ __device__ inline uint64_t mix(uint64_t key, uint64_t mask)
{
	key = (~key + (key << 21)) & mask;
	key ^= key >> 24;
	key = (key + (key << 3) + (key << 8)) & mask;
	key ^= key >> 14;
	key = (key + (key << 2) + (key << 4)) & mask;
	key ^= key >> 28;
	key = (key + (key << 31)) & mask;
	return key;
}

} // namespace mm2gb
