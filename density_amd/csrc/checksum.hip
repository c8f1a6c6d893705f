// checksum.hip — content checksums for gfx950: C (checksum.hpp) of every chunk of a device buffer, and the small kernels that seal a container
// with them (a trailer of one word per chunk behind the container: include/density_hip.h, DENSITY_HIP_FLAG_CHECKSUM), carry a trailer along when a
// slotted container is packed, and hold a decoder's output against one.
//
// The sum kernel only reads: a chunk is cut into tiles of 32 KiB, a work-group takes tiles in a grid-stride loop, every lane has eight 16-byte loads
// in flight, mixes each word with its index IN THE CHUNK (not its address: the buffer may start anywhere), and the work-group adds its partial sum
// to the chunk's accumulator with one global atomic (the tile: checksum_dev.hpp, shared with parity.hip).  The sum commutes, so neither the tiles nor
// the atomics need an order.  A second, tiny kernel turns the accumulators into C = fmix32(S + L), or compares them with a trailer.
//
// Verdicts (density_hip_decode_device_verdicts): the accumulators a verifying decode leaves behind are held against the trailer once more, this time with
// one word per chunk as the answer, and a fill kernel puts zeros where a damaged chunk's bytes stand.
#include "checksum_dev.hpp"
#include "kernels.hpp"

namespace density {

namespace {

constexpr uint32_t kSumMaxGroups = 256u * 8u;                  // eight work-groups a CU; what is left is taken in the grid-stride loop
constexpr uint32_t kSmallThreads = 1024;

__device__ __forceinline__ uint64_t align16(uint64_t v) { return (v + 15ull) & ~15ull; }
__device__ __forceinline__ uint64_t ld64u(const uint8_t* p) { return *reinterpret_cast<const u64_u*>(p); }
__device__ __forceinline__ void st64u(uint8_t* p, uint64_t v) { *reinterpret_cast<u64_u*>(p) = v; }

// d_geom (nullable; the asynchronous seal, whose geometry only the device knows): {chunk size, chunks} as seal_prepare_kernel took them from the
// container's header, {.., 0} where that header is not to be followed
__global__ __launch_bounds__(kSumThreads) void checksum_tiles_kernel(const uint8_t* __restrict__ data, uint64_t size, uint32_t chunk, uint32_t n_chunks,
                                                                     const uint32_t* __restrict__ d_geom, uint32_t* __restrict__ acc) {
    __shared__ uint32_t part[kSumThreads / 64];
    if (d_geom) { chunk = d_geom[0]; n_chunks = d_geom[1]; }
    if (n_chunks == 0) return;
    const uint32_t tiles = (chunk + kSumTile - 1) / kSumTile;
    const uint64_t units = (uint64_t)n_chunks * tiles;
    for (uint64_t u = blockIdx.x; u < units; u += gridDim.x) {
        const uint32_t c = (uint32_t)(u / tiles), t0 = (uint32_t)(u % tiles) * kSumTile;
        const uint32_t len = chunk_len(size, chunk, c);
        if (t0 >= len) continue;                                             // (the ragged last chunk: the same for the whole work-group)
        const uint8_t* p = data + (uint64_t)c * chunk;
        sum_tile(p, len, t0, part, acc + c);
    }
}

// acc[c] = S of chunk c -> C = fmix32(S + L); with `expect` (n_chunks words at any alignment: a trailer) nothing is written but *err, where they differ
__global__ __launch_bounds__(256) void checksum_finish_kernel(uint32_t* __restrict__ acc, uint64_t size, uint32_t chunk, uint32_t n_chunks,
                                                              const uint8_t* __restrict__ expect, uint32_t* __restrict__ err) {
    const uint32_t c = blockIdx.x * 256u + threadIdx.x;
    if (c >= n_chunks) return;
    const uint32_t sum = fmix32(acc[c] + chunk_len(size, chunk, c));
    if (!expect) acc[c] = sum;
    else if (sum != ld32u(expect + 4ull * c)) atomicOr(err, kErrChecksum);
}

// The same comparison with an answer per chunk: verdict[c] = DENSITY_HIP_CHUNK_DAMAGED where chunk c's sum is not the trailer's, 0 where it is; *count
// (cleared by the launcher) receives the number of damaged chunks.  acc is only read: it holds what checksum_tiles_kernel left for the verifying decode.
__global__ __launch_bounds__(256) void checksum_verdict_kernel(const uint32_t* __restrict__ acc, uint64_t size, uint32_t chunk, uint32_t n_chunks,
                                                               const uint8_t* __restrict__ expect, uint32_t* __restrict__ verdict, uint32_t* __restrict__ count,
                                                               uint32_t* __restrict__ err) {
    const uint32_t c = blockIdx.x * 256u + threadIdx.x;
    if (c >= n_chunks) return;
    const bool damaged = fmix32(acc[c] + chunk_len(size, chunk, c)) != ld32u(expect + 4ull * c);
    verdict[c] = damaged ? DENSITY_HIP_CHUNK_DAMAGED : 0u;
    if (damaged) { atomicAdd(count, 1u); atomicOr(err, kErrChecksum); }
}

// Zeros over the output region of every chunk whose verdict is DENSITY_HIP_CHUNK_DAMAGED — a chunk that parity.hip has rebuilt is kept — (the last chunk at its
// true length, `out` at any alignment): a chunk is cut into tiles of 16 KiB, a work-group takes tiles in a grid-stride loop and leaves a tile of an intact
// chunk at its first load — the verdict word.  Inside a tile: bytes up to the first 16-byte boundary of the ADDRESS, 16-byte stores, bytes behind the last
// whole one.
constexpr uint32_t kBlankThreads = 256, kBlankStores = 4;
constexpr uint32_t kBlankTile = kBlankThreads * 16u * kBlankStores;   // 16 KiB per work-group and trip
constexpr uint32_t kBlankMaxGroups = 256u * 32u;
__global__ __launch_bounds__(kBlankThreads) void blank_chunks_kernel(uint8_t* __restrict__ out, uint64_t size, uint32_t chunk, uint32_t n_chunks,
                                                                     const uint32_t* __restrict__ verdict) {
    const uint32_t tiles = (chunk + kBlankTile - 1) / kBlankTile;
    const uint64_t units = (uint64_t)n_chunks * tiles;
    for (uint64_t u = blockIdx.x; u < units; u += gridDim.x) {
        const uint32_t c = (uint32_t)(u / tiles), t0 = (uint32_t)(u % tiles) * kBlankTile;
        if (verdict[c] != DENSITY_HIP_CHUNK_DAMAGED) continue;
        const uint32_t len = chunk_len(size, chunk, c);
        if (t0 >= len) continue;                                             // (the ragged last chunk)
        const uint32_t n = len - t0 < kBlankTile ? len - t0 : kBlankTile;
        uint8_t* p = out + (uint64_t)c * chunk + t0;
        const uint32_t lead = (16u - (uint32_t)((uintptr_t)p & 15u)) & 15u, head = lead < n ? lead : n;
        const uint32_t full = (n - head) / 16u, tail_at = head + full * 16u; // (full <= 1024: four stores a lane cover it)
        if (threadIdx.x < head) p[threadIdx.x] = 0;
        u32x4* q = reinterpret_cast<u32x4*>(p + head);
#pragma unroll
        for (uint32_t j = 0; j < kBlankStores; ++j) {
            const uint32_t i = j * kBlankThreads + threadIdx.x;
            if (i < full) q[i] = u32x4{0u, 0u, 0u, 0u};
        }
        if (threadIdx.x < n - tail_at) p[tail_at + threadIdx.x] = 0;
    }
}

// The seal, first step: the header the encoder left on the device says where the trailer goes.  A header that is not this input's (or is sealed
// already) raises bit 1 of *err, a capacity that does not hold the trailer bit 2; either way d_geom says "no chunks" and nothing more happens.
// Otherwise the accumulators are cleared for the sum kernel.  One work-group.
__global__ __launch_bounds__(kSmallThreads) void seal_prepare_kernel(const uint8_t* __restrict__ container, uint64_t capacity, uint64_t input_size,
                                                                     uint32_t* __restrict__ d_geom, uint32_t* __restrict__ acc, uint32_t* __restrict__ err) {
    const uint32_t magic = ld32u(container), version = container[5], flags = ld16u(container + 6), chunk = ld32u(container + 8), n = ld32u(container + 12);
    const uint64_t total = ld64u(container + 16), len = ld64u(container + 24);
    const bool bad = magic != DENSITY_HIP_MAGIC || version != 1 || chunk < 256u || chunk % 256u != 0 || (flags & DENSITY_HIP_FLAG_CHECKSUM) || total != input_size ||
                     n != (total + chunk - 1) / chunk || len < sizeof(density_hip_header_t) || len > capacity;
    const bool fits = !bad && align16(len) + align16(4ull * n) <= capacity;
    if (threadIdx.x == 0) {
        d_geom[0] = chunk;
        d_geom[1] = fits ? n : 0u;
        d_geom[2] = fits ? 1u : 0u;
        if (bad) atomicOr(err, 1u);
        else if (!fits) atomicOr(err, 2u);
    }
    if (fits) for (uint32_t i = threadIdx.x; i < n; i += kSmallThreads) acc[i] = 0u;
}

// ... last step: the trailer behind the container (the gap in front of it and its own padding are zeros: they are wire bytes now), then the flag
// and the new length.  The container may lie at any address.
__global__ __launch_bounds__(kSmallThreads) void seal_finish_kernel(uint8_t* __restrict__ container, uint64_t input_size, const uint32_t* __restrict__ d_geom,
                                                                    const uint32_t* __restrict__ acc) {
    if (!d_geom[2]) return;
    const uint32_t chunk = d_geom[0], n = d_geom[1];
    const uint64_t len = ld64u(container + 24), at = align16(len), bytes = align16(4ull * n);
    const uint32_t flags = ld16u(container + 6);
    __syncthreads();                                                         // (everyone has the old length before thread 0 replaces it)
    for (uint32_t i = threadIdx.x; i < n; i += kSmallThreads) st32u(container + at + 4ull * i, fmix32(acc[i] + chunk_len(input_size, chunk, i)));
    if (threadIdx.x < at - len) container[len + threadIdx.x] = 0;
    if (threadIdx.x < bytes - 4ull * n) container[at + 4ull * n + threadIdx.x] = 0;
    if (threadIdx.x == 0) {
        st16u(container + 6, flags | DENSITY_HIP_FLAG_CHECKSUM);
        st64u(container + 24, at + bytes);
    }
}

// The trailer of a packed container: n_parts runs of trailer words, run p to entries [entry, entry + count) of the n-word trailer behind the container the
// layout and gather kernels have just written into `dst`; the gap in front and the padding once.  Nothing where they raised *err, bit 2 where the capacity
// does not hold it.
__global__ __launch_bounds__(kSmallThreads) void place_trailer_kernel(TrailerRuns runs, uint32_t n_parts, uint8_t* __restrict__ dst, uint64_t capacity, uint32_t n,
                                                                      uint32_t* __restrict__ err) {
    if (*err) return;
    const uint64_t len = ld64u(dst + 24), at = align16(len), bytes = align16(4ull * n);
    const uint32_t flags = ld16u(dst + 6);
    if (at + bytes > capacity) { if (threadIdx.x == 0) atomicOr(err, 2u); return; }
    __syncthreads();
    for (uint32_t p = 0; p < n_parts; ++p) {
        const TrailerRun r = runs.p[p];
        if ((uint64_t)r.entry + r.count > n) continue;                       // (never from this library's host side)
        for (uint32_t i = threadIdx.x; i < r.count; i += kSmallThreads) st32u(dst + at + 4ull * (r.entry + i), ld32u(r.src + 4ull * i));
    }
    if (threadIdx.x < at - len) dst[len + threadIdx.x] = 0;
    if (threadIdx.x < bytes - 4ull * n) dst[at + 4ull * n + threadIdx.x] = 0;
    if (threadIdx.x == 0) {
        st16u(dst + 6, flags | DENSITY_HIP_FLAG_CHECKSUM);
        st64u(dst + 24, at + bytes);
    }
}

hipError_t launch_tiles(const uint8_t* d_data, uint64_t size, uint32_t chunk, uint32_t n_chunks, const uint32_t* d_geom, uint32_t* d_acc, hipStream_t stream) {
    // with the geometry on the device alone, the tiles of the input as a whole stand in for the tiles of its chunks: the loop takes the rest
    const uint64_t units = d_geom ? (size + kSumTile - 1) / kSumTile : (uint64_t)n_chunks * ((chunk + kSumTile - 1) / kSumTile);
    const uint32_t groups = (uint32_t)(units < 1 ? 1 : units < kSumMaxGroups ? units : kSumMaxGroups);
    hipLaunchKernelGGL(checksum_tiles_kernel, dim3(groups), dim3(kSumThreads), 0, stream, d_data, size, chunk, n_chunks, d_geom, d_acc);
    return hipGetLastError();
}

}  // namespace

hipError_t launch_checksum(const uint8_t* d_data, uint64_t size, uint32_t chunk, uint32_t n_chunks, uint32_t* d_sums, const uint8_t* d_expect, uint32_t* d_err,
                           hipStream_t stream) {
    if (n_chunks == 0) return hipSuccess;
    hipError_t e = hipMemsetAsync(d_sums, 0, 4ull * n_chunks, stream);
    if (e == hipSuccess) e = launch_tiles(d_data, size, chunk, n_chunks, nullptr, d_sums, stream);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(checksum_finish_kernel, dim3((n_chunks + 255u) / 256u), dim3(256), 0, stream, d_sums, size, chunk, n_chunks, d_expect, d_err);
    return hipGetLastError();
}

hipError_t launch_chunk_verdicts(const uint32_t* d_acc, uint64_t size, uint32_t chunk, uint32_t n_chunks, const uint8_t* d_expect, uint32_t* d_verdicts,
                                 uint32_t* d_count, uint32_t* d_err, hipStream_t stream) {
    const hipError_t e = hipMemsetAsync(d_count, 0, sizeof(uint32_t), stream);
    if (e != hipSuccess || n_chunks == 0) return e;
    hipLaunchKernelGGL(checksum_verdict_kernel, dim3((n_chunks + 255u) / 256u), dim3(256), 0, stream, d_acc, size, chunk, n_chunks, d_expect, d_verdicts, d_count, d_err);
    return hipGetLastError();
}

hipError_t launch_blank_chunks(uint8_t* d_out, uint64_t size, uint32_t chunk, uint32_t n_chunks, const uint32_t* d_verdicts, hipStream_t stream) {
    if (n_chunks == 0) return hipSuccess;
    const uint64_t units = (uint64_t)n_chunks * ((chunk + kBlankTile - 1) / kBlankTile);
    hipLaunchKernelGGL(blank_chunks_kernel, dim3((uint32_t)(units < kBlankMaxGroups ? units : kBlankMaxGroups)), dim3(kBlankThreads), 0, stream, d_out, size, chunk, n_chunks,
                       d_verdicts);
    return hipGetLastError();
}

hipError_t launch_seal(const uint8_t* d_in, uint64_t input_size, uint8_t* d_container, uint64_t capacity, uint32_t* d_geom, uint32_t* d_acc, uint32_t* d_err,
                       hipStream_t stream) {
    hipLaunchKernelGGL(seal_prepare_kernel, dim3(1), dim3(kSmallThreads), 0, stream, d_container, capacity, input_size, d_geom, d_acc, d_err);
    hipError_t e = hipGetLastError();
    if (e == hipSuccess) e = launch_tiles(d_in, input_size, 0, 0, d_geom, d_acc, stream);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(seal_finish_kernel, dim3(1), dim3(kSmallThreads), 0, stream, d_container, input_size, d_geom, d_acc);
    return hipGetLastError();
}

hipError_t launch_place_trailer(const TrailerRuns& runs, uint32_t n_parts, uint8_t* d_container, uint64_t capacity, uint32_t n_chunks, uint32_t* d_err,
                                hipStream_t stream) {
    hipLaunchKernelGGL(place_trailer_kernel, dim3(1), dim3(kSmallThreads), 0, stream, runs, n_parts, d_container, capacity, n_chunks, d_err);
    return hipGetLastError();
}

}  // namespace density
