// checksum.hpp — the content checksum of a sealed container (include/density_hip.h: DENSITY_HIP_FLAG_CHECKSUM), as host and device code share it.
//   C(B), B of L bytes: m = ceil(L / 4) little-endian words w_i, the last one zero-padded;  S = sum of fmix32(w_i + kSumStep * (i + 1));  C = fmix32(S + (u32)L),
//   all mod 2^32.  A sum, so any split of B over lanes, waves, work-groups or host slices combines with one add; fmix32 is a bijection and the word's
//   index goes in, so one damaged word, or two different words exchanged, always change S.  An integrity check, not a MAC.
#pragma once
#include <stdint.h>

namespace density {

constexpr uint32_t kSumStep = 0x9E3779B1u;

// the finaliser of MurmurHash3 (public domain): a bijection of the 32-bit words
__host__ __device__ inline uint32_t fmix32(uint32_t h) {
    h ^= h >> 16;
    h *= 0x85ebca6bu;
    h ^= h >> 13;
    h *= 0xc2b2ae35u;
    h ^= h >> 16;
    return h;
}
// what word `w` at index `i` of its chunk adds to S
__host__ __device__ inline uint32_t sum_term(uint32_t w, uint32_t i) { return fmix32(w + kSumStep * (i + 1u)); }

}  // namespace density
