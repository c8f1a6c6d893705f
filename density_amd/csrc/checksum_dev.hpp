// checksum_dev.hpp — what the kernels that sum, blank and rebuild chunks of a device buffer share (checksum.hip, parity.hip): 16 bytes from any address,
// a chunk's length, and the sum kernel's tile — so that a chunk summed again after it was rebuilt is summed by the same arithmetic.
#pragma once
#include "checksum.hpp"
#include "common.hpp"

namespace density {

constexpr uint32_t kSumThreads = 256, kSumLoads = 8;
constexpr uint32_t kSumTile = kSumThreads * 16u * kSumLoads;   // 32 KiB per work-group and trip

typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));

// 16 bytes from any address: one global_load_dwordx4 (gfx950 global memory takes unaligned accesses, as for the dwords of common.hpp)
__device__ __forceinline__ u32x4 load16(const uint8_t* p) {
    u32x4 v;
    __builtin_memcpy(&v, p, 16);
    return v;
}

// bytes of chunk `c` of a buffer of `size` bytes cut every `chunk` bytes
__device__ __forceinline__ uint32_t chunk_len(uint64_t size, uint32_t chunk, uint32_t c) {
    const uint64_t begin = (uint64_t)c * chunk;
    return size - begin < chunk ? (uint32_t)(size - begin) : chunk;
}

// The tile [t0, t0 + kSumTile) of the chunk of `len` bytes at `p` (t0 < len), summed by a work-group of kSumThreads: every lane has kSumLoads 16-byte
// loads in flight and mixes each word with its index IN THE CHUNK; the work-group adds its partial sum to *acc with one global atomic.  `part`:
// kSumThreads / 64 words of LDS, free again on return.
__device__ __forceinline__ void sum_tile(const uint8_t* p, uint32_t len, uint32_t t0, uint32_t* part, uint32_t* acc) {
    u32x4 v[kSumLoads];
#pragma unroll
    for (uint32_t j = 0; j < kSumLoads; ++j) {
        const uint32_t off = t0 + (j * kSumThreads + threadIdx.x) * 16u;
        v[j] = (off < len && len - off >= 16u) ? load16(p + off) : u32x4{0u, 0u, 0u, 0u};
    }
    uint32_t sum = 0;
#pragma unroll
    for (uint32_t j = 0; j < kSumLoads; ++j) {
        const uint32_t off = t0 + (j * kSumThreads + threadIdx.x) * 16u, i = off / 4u;
        if (off >= len) continue;
        if (len - off >= 16u) {
            sum += sum_term(v[j].x, i) + sum_term(v[j].y, i + 1u) + sum_term(v[j].z, i + 2u) + sum_term(v[j].w, i + 3u);
        } else {                                                         // the chunk's last 1..15 bytes: whole words, then one padded with zeros
            const uint32_t rem = len - off;
            for (uint32_t k = 0; k < rem; k += 4u) {
                uint32_t w = 0;
                for (uint32_t b = 0; b < 4u && k + b < rem; ++b) w |= (uint32_t)p[off + k + b] << (8u * b);
                sum += sum_term(w, i + k / 4u);
            }
        }
    }
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) sum += __shfl_down(sum, d, 64);
    if ((threadIdx.x & 63u) == 0) part[threadIdx.x >> 6] = sum;
    __syncthreads();
    if (threadIdx.x == 0) atomicAdd(acc, part[0] + part[1] + part[2] + part[3]);
    __syncthreads();                                                     // (part is written again in the next trip)
}

}  // namespace density
