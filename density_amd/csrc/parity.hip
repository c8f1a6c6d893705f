// parity.hip — recovery records for gfx950: the parity blob "DHP1" of a device buffer (include/density_hip.h: n_groups rows, row g the XOR of the input
// chunks i with i % n_groups == g, each zero-padded to the row's length), and the kernels that use it behind a verdict decode: a chunk that is the
// only damaged one of its group is rebuilt as its row XOR the output regions of the group's other members, summed again, and held against its
// trailer entry once more.  Adjacent chunks lie in different groups, so a burst of up to n_groups neighbouring chunks is rebuilt whole.
//
// Both bulk kernels only stream: a row (a victim's region) is cut into tiles of 16 KiB, a work-group takes tiles in a grid-stride loop, every lane keeps four
// 16-byte accumulators and walks the group's members with four independent 16-byte loads in flight per member (eight with the loop unrolled twice).
// The input and the blob may lie at any address.  The ragged last chunk is the only member that can end inside a tile: it contributes zeros past
// its end and its last 1..15 bytes bytewise.
//
// Recovery never reads more than the verdict words to decide: recover_plan_kernel turns them into one word per group — the group's only damaged
// member, or kNoVictim where it has none or several — and clears that chunk's accumulator; the kernels behind it leave at that word.
#include "checksum_dev.hpp"
#include "kernels.hpp"

namespace density {

namespace {

constexpr uint32_t kParThreads = 256, kParLoads = 4;
constexpr uint32_t kParTile = kParThreads * 16u * kParLoads;   // 16 KiB per work-group and trip
constexpr uint32_t kParMaxGroups = 256u * 8u;                  // eight work-groups a CU; what is left is taken in the grid-stride loop
constexpr uint32_t kNoVictim = 0xffffffffu;
constexpr uint32_t kHeaderBytes = sizeof(density_hip_parity_header_t);

__device__ __forceinline__ void store16(uint8_t* p, u32x4 v) { __builtin_memcpy(p, &v, 16); }   // (any address, as load16)

// the 16 bytes at `off` of a chunk of `len` bytes at `p`, zeros past its end
__device__ __forceinline__ u32x4 load16_clipped(const uint8_t* p, uint32_t off, uint32_t len) {
    if (off < len && len - off >= 16u) return load16(p + off);
    uint32_t w[4];
#pragma unroll
    for (uint32_t q = 0; q < 4u; ++q) {
        w[q] = 0u;
#pragma unroll
        for (uint32_t b = 0; b < 4u; ++b)
            if (off + 4u * q + b < len) w[q] |= (uint32_t)p[off + 4u * q + b] << (8u * b);
    }
    const u32x4 v{w[0], w[1], w[2], w[3]};
    return v;
}

// acc[j] ^= the 16 bytes at off[j] (where off[j] < limit) of every chunk m of `data` with m % n_groups == g, but `skip`
__device__ __forceinline__ void xor_members(u32x4 (&acc)[kParLoads], const uint32_t (&off)[kParLoads], uint32_t limit, const uint8_t* data, uint64_t size,
                                            uint32_t chunk, uint32_t n_chunks, uint32_t g, uint32_t n_groups, uint32_t skip) {
#pragma unroll 2
    for (uint64_t m = g; m < n_chunks; m += n_groups) {
        if (m == skip) continue;
        const uint32_t len = chunk_len(size, chunk, (uint32_t)m);
        const uint8_t* p = data + m * chunk;
        u32x4 v[kParLoads];
#pragma unroll
        for (uint32_t j = 0; j < kParLoads; ++j) v[j] = off[j] < limit ? load16_clipped(p, off[j], len) : u32x4{0u, 0u, 0u, 0u};
#pragma unroll
        for (uint32_t j = 0; j < kParLoads; ++j) acc[j] ^= v[j];
    }
}
// the same for one byte
__device__ __forceinline__ uint8_t xor_members_byte(uint8_t b, uint32_t off, const uint8_t* data, uint64_t size, uint32_t chunk, uint32_t n_chunks, uint32_t g,
                                                    uint32_t n_groups, uint32_t skip) {
    for (uint64_t m = g; m < n_chunks; m += n_groups)
        if (m != skip && off < chunk_len(size, chunk, (uint32_t)m)) b ^= data[m * chunk + off];
    return b;
}

// The blob of `data`: the header (work-group 0) and n_groups rows of hdr.row_bytes bytes behind it, every byte of them written.
__global__ __launch_bounds__(kParThreads) void parity_rows_kernel(const uint8_t* __restrict__ data, density_hip_parity_header_t hdr, uint8_t* __restrict__ blob) {
    const uint64_t size = hdr.total_len;
    const uint32_t chunk = hdr.chunk_size, n_chunks = hdr.n_chunks, n_groups = hdr.n_groups, row_bytes = hdr.row_bytes;
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        st32u(blob, hdr.magic);
        st32u(blob + 4, hdr.version);                                         // (version, then three zero bytes)
        st32u(blob + 8, chunk);
        st32u(blob + 12, n_chunks);
        st32u(blob + 16, (uint32_t)size);
        st32u(blob + 20, (uint32_t)(size >> 32));
        st32u(blob + 24, n_groups);
        st32u(blob + 28, row_bytes);
    }
    const uint32_t tiles = (row_bytes + kParTile - 1) / kParTile;
    const uint64_t units = (uint64_t)n_groups * tiles;
    for (uint64_t u = blockIdx.x; u < units; u += gridDim.x) {
        const uint32_t g = (uint32_t)(u / tiles), t0 = (uint32_t)(u % tiles) * kParTile;
        u32x4 acc[kParLoads];
        uint32_t off[kParLoads];
#pragma unroll
        for (uint32_t j = 0; j < kParLoads; ++j) {
            acc[j] = u32x4{0u, 0u, 0u, 0u};
            off[j] = t0 + (j * kParThreads + threadIdx.x) * 16u;
        }
        xor_members(acc, off, row_bytes, data, size, chunk, n_chunks, g, n_groups, kNoVictim);
        uint8_t* row = blob + kHeaderBytes + (uint64_t)g * row_bytes;
#pragma unroll
        for (uint32_t j = 0; j < kParLoads; ++j)
            if (off[j] < row_bytes) store16(row + off[j], acc[j]);               // (row_bytes is a multiple of 16: a slot that begins inside the row ends inside it)
    }
}

// victim[g] = the only chunk of group g whose verdict is DENSITY_HIP_CHUNK_DAMAGED — its accumulator is cleared for the sum that follows the rebuild —,
// kNoVictim where the group has none or more than one.  A work-group per group, in a grid-stride loop; the lanes share out the group's verdict words.
__global__ __launch_bounds__(kParThreads) void recover_plan_kernel(const uint32_t* __restrict__ verdict, uint32_t n_chunks, uint32_t n_groups,
                                                                   uint32_t* __restrict__ victim, uint32_t* __restrict__ acc) {
    __shared__ uint32_t s_count, s_who;
    for (uint32_t g = blockIdx.x; g < n_groups; g += gridDim.x) {
        if (threadIdx.x == 0) s_count = s_who = 0u;
        __syncthreads();
        uint32_t count = 0, who = 0;
        for (uint64_t m = g + (uint64_t)threadIdx.x * n_groups; m < n_chunks; m += (uint64_t)kParThreads * n_groups)
            if (verdict[m] == DENSITY_HIP_CHUNK_DAMAGED) { ++count; who = (uint32_t)m; }
        if (count) { atomicAdd(&s_count, count); atomicAdd(&s_who, who); }      // (s_who is read only where one lane found one chunk)
        __syncthreads();
        if (threadIdx.x == 0) {
            const bool one = s_count == 1u;
            victim[g] = one ? s_who : kNoVictim;
            if (one) acc[s_who] = 0u;
        }
        __syncthreads();                                                     // (s_count is cleared again in the next trip)
    }
}

// Group g's victim k (recover_plan_kernel), where it has one: the bytes of k's region of `out` become row g XOR the regions of the group's other members, the
// last chunk at its true length, `out` and the rows at any alignment.  Inside a tile, as in blank_chunks_kernel: bytes up to the first 16-byte boundary
// of the ADDRESS (the other members' regions are whole chunks away: the same phase), 16-byte stores, bytes behind the last whole one.  `out` is read
// and written, but never the same chunk: no other chunk of the group is rebuilt.
__global__ __launch_bounds__(kParThreads) void recover_rebuild_kernel(uint8_t* out, uint64_t size, uint32_t chunk, uint32_t n_chunks, const uint8_t* __restrict__ rows,
                                                                      uint32_t n_groups, uint32_t row_bytes, const uint32_t* __restrict__ victim) {
    const uint32_t tiles = (chunk + kParTile - 1) / kParTile;
    const uint64_t units = (uint64_t)n_groups * tiles;
    for (uint64_t u = blockIdx.x; u < units; u += gridDim.x) {
        const uint32_t g = (uint32_t)(u / tiles), t0 = (uint32_t)(u % tiles) * kParTile;
        const uint32_t k = victim[g];
        if (k == kNoVictim) continue;
        const uint32_t len = chunk_len(size, chunk, k);
        if (t0 >= len) continue;                                             // (the ragged last chunk)
        const uint32_t n = len - t0 < kParTile ? len - t0 : kParTile;
        uint8_t* p = out + (uint64_t)k * chunk + t0;
        const uint8_t* row = rows + (uint64_t)g * row_bytes + t0;            // (len <= row_bytes: the row covers the tile)
        const uint32_t lead = (16u - (uint32_t)((uintptr_t)p & 15u)) & 15u, head = lead < n ? lead : n;
        const uint32_t full = (n - head) / 16u, tail_at = head + full * 16u; // (full <= 1024: four stores a lane cover it)
        if (threadIdx.x < head) p[threadIdx.x] = xor_members_byte(row[threadIdx.x], t0 + threadIdx.x, out, size, chunk, n_chunks, g, n_groups, k);
        u32x4 acc[kParLoads];
        uint32_t off[kParLoads];
#pragma unroll
        for (uint32_t j = 0; j < kParLoads; ++j) {
            const uint32_t i = j * kParThreads + threadIdx.x;
            off[j] = t0 + head + 16u * i;
            acc[j] = i < full ? load16(row + head + 16u * i) : u32x4{0u, 0u, 0u, 0u};
        }
        xor_members(acc, off, t0 + tail_at, out, size, chunk, n_chunks, g, n_groups, k);
        u32x4* q = reinterpret_cast<u32x4*>(p + head);
#pragma unroll
        for (uint32_t j = 0; j < kParLoads; ++j) {
            const uint32_t i = j * kParThreads + threadIdx.x;
            if (i < full) q[i] = acc[j];
        }
        if (threadIdx.x < n - tail_at) p[tail_at + threadIdx.x] = xor_members_byte(row[tail_at + threadIdx.x], t0 + tail_at + threadIdx.x, out, size, chunk, n_chunks, g, n_groups, k);
    }
}

// The rebuilt chunks summed again, by checksum_tiles_kernel's tile: a work-group takes the tiles of the groups' victims in a grid-stride loop
__global__ __launch_bounds__(kSumThreads) void recover_sum_kernel(const uint8_t* __restrict__ out, uint64_t size, uint32_t chunk, uint32_t n_groups,
                                                                  const uint32_t* __restrict__ victim, uint32_t* __restrict__ acc) {
    __shared__ uint32_t part[kSumThreads / 64];
    const uint32_t tiles = (chunk + kSumTile - 1) / kSumTile;
    const uint64_t units = (uint64_t)n_groups * tiles;
    for (uint64_t u = blockIdx.x; u < units; u += gridDim.x) {
        const uint32_t g = (uint32_t)(u / tiles), t0 = (uint32_t)(u % tiles) * kSumTile;
        const uint32_t k = victim[g];
        if (k == kNoVictim) continue;                                        // (the same for the whole work-group, like every test in front of sum_tile)
        const uint32_t len = chunk_len(size, chunk, k);
        if (t0 >= len) continue;
        sum_tile(out + (uint64_t)k * chunk, len, t0, part, acc + k);
    }
}

// ... and held against the trailer once more, a thread per group: a victim whose bytes now have the trailer's checksum becomes DENSITY_HIP_CHUNK_RECOVERED and
// moves from *damaged to *recovered; one whose bytes have not (a damaged row, a damaged trailer entry) stays DENSITY_HIP_CHUNK_DAMAGED.
__global__ __launch_bounds__(256) void recover_verify_kernel(const uint32_t* __restrict__ acc, uint64_t size, uint32_t chunk, uint32_t n_groups,
                                                             const uint32_t* __restrict__ victim, const uint8_t* __restrict__ expect, uint32_t* __restrict__ verdict,
                                                             uint32_t* __restrict__ damaged, uint32_t* __restrict__ recovered) {
    const uint32_t g = blockIdx.x * 256u + threadIdx.x;
    if (g >= n_groups) return;
    const uint32_t k = victim[g];
    if (k == kNoVictim) return;
    if (fmix32(acc[k] + chunk_len(size, chunk, k)) != ld32u(expect + 4ull * k)) return;
    verdict[k] = DENSITY_HIP_CHUNK_RECOVERED;
    atomicSub(damaged, 1u);
    atomicAdd(recovered, 1u);
}

uint32_t grid_for(uint64_t units) { return (uint32_t)(units < 1 ? 1 : units < kParMaxGroups ? units : kParMaxGroups); }

}  // namespace

hipError_t launch_parity_rows(const uint8_t* d_data, const density_hip_parity_header_t& hdr, uint8_t* d_blob, hipStream_t stream) {
    const uint64_t units = (uint64_t)hdr.n_groups * ((hdr.row_bytes + kParTile - 1) / kParTile);
    hipLaunchKernelGGL(parity_rows_kernel, dim3(grid_for(units)), dim3(kParThreads), 0, stream, d_data, hdr, d_blob);
    return hipGetLastError();
}

hipError_t launch_recover_rebuild(uint8_t* d_out, uint64_t size, uint32_t chunk, uint32_t n_chunks, const uint8_t* d_rows, uint32_t n_groups, uint32_t row_bytes,
                                  const uint32_t* d_verdicts, uint32_t* d_victim, uint32_t* d_acc, hipStream_t stream) {
    if (n_chunks == 0) return hipSuccess;
    hipLaunchKernelGGL(recover_plan_kernel, dim3(grid_for(n_groups)), dim3(kParThreads), 0, stream, d_verdicts, n_chunks, n_groups, d_victim, d_acc);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    const uint64_t units = (uint64_t)n_groups * ((chunk + kParTile - 1) / kParTile);
    hipLaunchKernelGGL(recover_rebuild_kernel, dim3(grid_for(units)), dim3(kParThreads), 0, stream, d_out, size, chunk, n_chunks, d_rows, n_groups, row_bytes, d_victim);
    return hipGetLastError();
}

hipError_t launch_recover_verify(const uint8_t* d_out, uint64_t size, uint32_t chunk, uint32_t n_chunks, uint32_t n_groups, const uint32_t* d_victim, uint32_t* d_acc,
                                 const uint8_t* d_expect, uint32_t* d_verdicts, uint32_t* d_damaged, uint32_t* d_recovered, hipStream_t stream) {
    hipError_t e = hipMemsetAsync(d_recovered, 0, sizeof(uint32_t), stream);
    if (e != hipSuccess || n_chunks == 0) return e;
    const uint64_t units = (uint64_t)n_groups * ((chunk + kSumTile - 1) / kSumTile);
    hipLaunchKernelGGL(recover_sum_kernel, dim3(grid_for(units)), dim3(kSumThreads), 0, stream, d_out, size, chunk, n_groups, d_victim, d_acc);
    e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(recover_verify_kernel, dim3((n_groups + 255u) / 256u), dim3(256), 0, stream, d_acc, size, chunk, n_groups, d_victim, d_expect, d_verdicts, d_damaged,
                       d_recovered);
    return hipGetLastError();
}

}  // namespace density
