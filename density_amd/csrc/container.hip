// container.hip — layout (size scan), stitch (compaction) and self-test kernels for gfx950.
//
// The encode kernels write every chunk's stream into a worst-case sized slot; chunk sizes are known only afterwards
// (write_buffer.rs:29-31 keeps a running total; in parallel that becomes an exclusive scan).  layout_* computes the
// payload offsets (16-byte aligned so the gather and the decoder's loads are aligned), compact gathers the streams.
#include "common.hpp"
#include "kernels.hpp"

namespace density {

namespace {

constexpr uint32_t kScanThreads = 1024;
constexpr uint32_t kHeaderBytes = 32;
static_assert(sizeof(density_hip_header_t) == kHeaderBytes, "container header is 32 bytes");

__device__ __forceinline__ uint64_t align16(uint64_t v) { return (v + 15ull) & ~15ull; }

// inclusive scan of one u64 per thread across a 1024-thread block; returns inclusive value, *total = block sum
__device__ __forceinline__ uint64_t block_inclusive_scan(uint64_t v, uint64_t* wave_sums /* [16] LDS */, uint64_t* total) {
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const uint32_t lo = bperm(lane >= (uint32_t)d ? lane - d : lane, (uint32_t)v);
        const uint32_t hi = bperm(lane >= (uint32_t)d ? lane - d : lane, (uint32_t)(v >> 32));
        if (lane >= (uint32_t)d) v += ((uint64_t)hi << 32) | lo;
    }
    if (lane == 63) wave_sums[wave] = v;
    __syncthreads();
    uint64_t prefix = 0, sum = 0;
    for (uint32_t i = 0; i < kScanThreads / 64; ++i) {
        const uint64_t s = wave_sums[i];
        if (i < wave) prefix += s;
        sum += s;
    }
    __syncthreads();
    *total = sum;
    return v + prefix;
}

// slot_stride != 0: a SLOTTED container (DENSITY_HIP_FLAG_SLOTTED) — payload i sits in its worst-case slot at base + i * slot_stride, no scan
template <typename SizeT>
__device__ __forceinline__ void layout_common(const SizeT* __restrict__ sizes_in, uint32_t n, uint64_t base,
                                              uint64_t* __restrict__ sizes_out, uint32_t* __restrict__ table_out,
                                              uint64_t* __restrict__ offsets, uint64_t* end_out, uint64_t limit, uint32_t* __restrict__ err,
                                              uint64_t slot_stride = 0) {
    __shared__ uint64_t wave_sums[kScanThreads / 64];
    uint64_t carry = base, last_end = base;
    for (uint32_t t0 = 0; t0 < n; t0 += kScanThreads) {
        const uint32_t i = t0 + threadIdx.x;
        const uint64_t sz = i < n ? (uint64_t)sizes_in[i] : 0ull;
        uint64_t tile_total = 0;
        const uint64_t incl = slot_stride ? 0ull : block_inclusive_scan(align16(sz), wave_sums, &tile_total);
        if (i < n) {
            uint64_t off = slot_stride ? base + (uint64_t)i * slot_stride : carry + incl - align16(sz);
            uint64_t keep = sz;
            if (slot_stride && sz > slot_stride) { off = base; keep = 0; atomicOr(err, 4u); }   // a size table entry larger than its slot (never from this library): not followed
            if (off + sz > limit) {                     // a size table that runs past the container: the codec kernels must not follow it
                off = base; keep = 0;
                atomicOr(err, 4u);
            }
            offsets[i] = off;
            if (sizes_out) sizes_out[i] = keep;
            if (table_out) table_out[i] = (uint32_t)sz;
            if (i == n - 1) *end_out = off + sz;     // single writer
        }
        carry += tile_total;
    }
    (void)last_end;
}

__global__ __launch_bounds__(kScanThreads) void layout_encode_kernel(const uint64_t* __restrict__ sizes, uint32_t n,
                                                                     density_hip_header_t hdr, uint64_t base, uint8_t* __restrict__ container,
                                                                     uint64_t capacity, uint64_t* __restrict__ offsets,
                                                                     uint64_t* __restrict__ end_scratch, uint32_t* __restrict__ err, uint64_t slot_stride) {
    if (threadIdx.x == 0) *end_scratch = base;
    __syncthreads();
    layout_common<uint64_t>(sizes, n, base, nullptr, reinterpret_cast<uint32_t*>(container + kHeaderBytes), offsets, end_scratch, ~0ull, err, slot_stride);
    __syncthreads();
    if (threadIdx.x == 0) {
        hdr.container_len = *end_scratch;
        *reinterpret_cast<density_hip_header_t*>(container) = hdr;
        if (hdr.container_len > capacity) atomicOr(err, 2u);
    }
    // the gaps in front of the payloads — size table to block index, block index to the first stream — are part of the container: zeros
    const uint64_t table_end = kHeaderBytes + 4ull * n, ibase = (table_end + 15) / 16 * 16;
    const uint64_t iend = ibase + ((hdr.flags & DENSITY_HIP_FLAG_BLOCK_INDEX) ? (hdr.total_len + 255) / 256 : 0);
    if (threadIdx.x < ibase - table_end) container[table_end + threadIdx.x] = 0;
    if (threadIdx.x >= 32 && threadIdx.x - 32 < base - iend && base <= capacity) container[iend + threadIdx.x - 32] = 0;
}

// A slice [first, first + count) of the chunks (encode in batches: api.hip): offsets continue from *carry (the end of the previous
// batch's last payload; `base` for the first batch), the size-table entries of the slice are written, *carry moves on.  The last
// batch writes the header.
__global__ __launch_bounds__(kScanThreads) void layout_encode_batch_kernel(const uint64_t* __restrict__ sizes, uint32_t first, uint32_t count,
                                                                           uint32_t is_first, uint32_t is_last, density_hip_header_t hdr, uint64_t base,
                                                                           uint8_t* __restrict__ container, uint64_t capacity, uint64_t* __restrict__ offsets,
                                                                           uint64_t* __restrict__ carry, uint32_t* __restrict__ err) {
    __shared__ uint64_t end_scratch;
    const uint64_t start = is_first ? base : align16(*carry);
    if (threadIdx.x == 0) end_scratch = start;
    __syncthreads();
    layout_common<uint64_t>(sizes + first, count, start, nullptr, reinterpret_cast<uint32_t*>(container + kHeaderBytes) + first, offsets + first, &end_scratch, ~0ull, err);
    __syncthreads();
    if (threadIdx.x == 0) {
        *carry = end_scratch;
        if (is_last) {
            hdr.container_len = end_scratch;
            *reinterpret_cast<density_hip_header_t*>(container) = hdr;
        }
        if (end_scratch > capacity) atomicOr(err, 2u);
    }
    if (is_first) {                                              // (as in layout_encode_kernel: the gaps in front of the payloads are zeros)
        const uint64_t table_end = kHeaderBytes + 4ull * hdr.n_chunks, ibase = (table_end + 15) / 16 * 16;
        const uint64_t iend = ibase + ((hdr.flags & DENSITY_HIP_FLAG_BLOCK_INDEX) ? (hdr.total_len + 255) / 256 : 0);
        if (threadIdx.x < ibase - table_end) container[table_end + threadIdx.x] = 0;
        if (threadIdx.x >= 32 && threadIdx.x - 32 < base - iend && base <= capacity) container[iend + threadIdx.x - 32] = 0;
    }
}

// A PAGED container's front matter: size table, header (its length: the pages the encoder took from the counter), zeroed gaps.  The directory and the
// pages were written by the encode kernel itself.
__global__ __launch_bounds__(kScanThreads) void layout_encode_paged_kernel(const uint64_t* __restrict__ sizes, uint32_t n, density_hip_header_t hdr, uint64_t dir_base,
                                                                           uint64_t dir_end, uint64_t pages_base, uint8_t* __restrict__ container, uint64_t capacity,
                                                                           const uint32_t* __restrict__ page_counter, uint32_t* __restrict__ err) {
    uint32_t* table = reinterpret_cast<uint32_t*>(container + kHeaderBytes);
    for (uint32_t i = threadIdx.x; i < n; i += kScanThreads) table[i] = (uint32_t)sizes[i];
    if (threadIdx.x == 0) {
        hdr.container_len = pages_base + (uint64_t)*page_counter * kPageBytes;
        *reinterpret_cast<density_hip_header_t*>(container) = hdr;
        if (hdr.container_len > capacity) atomicOr(err, 2u);
    }
    const uint64_t table_end = kHeaderBytes + 4ull * n, ibase = (table_end + 15) / 16 * 16;
    const uint64_t iend = ibase + (hdr.total_len + 255) / 256;
    if (threadIdx.x < ibase - table_end) container[table_end + threadIdx.x] = 0;
    if (threadIdx.x >= 32 && threadIdx.x - 32 < dir_base - iend) container[iend + threadIdx.x - 32] = 0;
    for (uint64_t i = dir_end + threadIdx.x; i < pages_base; i += kScanThreads) container[i] = 0;
}
// the directory entries behind a chunk's last page are part of the wire bytes too: zeros, not what the buffer held.  A wave per chunk (in the layout kernel's
// one work-group this loop was 33 of its 39 µs — 4 % of the headline's round trip)
__global__ __launch_bounds__(256) void clear_directory_tails_kernel(uint32_t n, uint64_t dir_base, uint64_t dir_end, uint8_t* __restrict__ container) {
    const uint32_t c = blockIdx.x * 4u + (threadIdx.x >> 6), lane = threadIdx.x & 63u;
    if (c >= n) return;
    const uint32_t words = (uint32_t)((dir_end - dir_base) / 4 / n);
    uint32_t* dir = reinterpret_cast<uint32_t*>(container + dir_base) + (uint64_t)c * words;
    const uint32_t used = dir[0];                                                     // pages of chunk c (word 0 of its directory; never rewritten here)
    for (uint32_t w = 4u * (used + 1u) + lane; w < words; w += 64u) dir[w] = 0u;
}

__global__ __launch_bounds__(kScanThreads) void layout_decode_kernel(const uint8_t* __restrict__ container, uint64_t container_size,
                                                                     uint32_t n, uint64_t base, uint64_t* __restrict__ sizes,
                                                                     uint64_t* __restrict__ offsets, uint64_t* __restrict__ end_scratch,
                                                                     uint32_t* __restrict__ err, uint64_t slot_stride) {
    if (threadIdx.x == 0) *end_scratch = base;
    __syncthreads();
    layout_common<uint32_t>(reinterpret_cast<const uint32_t*>(container + kHeaderBytes), n, base, sizes, nullptr, offsets, end_scratch, container_size, err, slot_stride);
    __syncthreads();
    if (threadIdx.x == 0 && *end_scratch > container_size) atomicOr(err, 4u);   // truncated container
}

constexpr uint32_t kCopyThreads = 256;
constexpr uint32_t kCopyTile = kCopyThreads * 16u * 4u;   // 16 KiB per work-group

__global__ __launch_bounds__(kCopyThreads) void compact_kernel(const uint8_t* __restrict__ slots, uint64_t slot_stride,
                                                               const uint64_t* __restrict__ sizes, const uint64_t* __restrict__ offsets,
                                                               uint32_t tiles_per_chunk, uint8_t* __restrict__ container,
                                                               const uint32_t* __restrict__ err, uint32_t more_follow) {
    if (*err) return;                                          // layout overflowed the capacity: do not write
    const uint32_t chunk = blockIdx.x / tiles_per_chunk, tile = blockIdx.x % tiles_per_chunk;
    const uint64_t size = sizes[chunk];
    const uint64_t begin = (uint64_t)tile * kCopyTile;
    if (begin >= size) return;
    const uint8_t* s = slots + chunk * slot_stride;           // 16-byte aligned (stride and base are)
    uint8_t* d = container + offsets[chunk];                   // 16-byte aligned by layout
    const uint64_t full = size / 16;                           // whole uint4's
    const uint4* s4 = reinterpret_cast<const uint4*>(s);
    uint4* d4 = reinterpret_cast<uint4*>(d);
    const uint64_t i0 = begin / 16 + threadIdx.x;
    uint4 v[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) { const uint64_t i = i0 + (uint64_t)j * kCopyThreads; if (i < full) v[j] = s4[i]; }
#pragma unroll
    for (int j = 0; j < 4; ++j) { const uint64_t i = i0 + (uint64_t)j * kCopyThreads; if (i < full) d4[i] = v[j]; }
    // ragged tail (< 16 bytes) handled by the tile that contains it
    const uint64_t tail_at = full * 16;
    if (tail_at >= begin && tail_at < begin + kCopyTile) {
        const uint32_t r = (uint32_t)(size - tail_at);
        if (threadIdx.x < r) d[tail_at + threadIdx.x] = s[tail_at + threadIdx.x];
        // the gap up to the next stream's 16-byte boundary is part of the container: zeros, not whatever the buffer held
        // (`more_follow`: this launch gathers a batch and another batch's streams come behind its last one)
        else if (threadIdx.x < 16 && r != 0 && (chunk + 1 < gridDim.x / tiles_per_chunk || more_follow)) d[tail_at + threadIdx.x] = 0;
    }
}

// ---- PAGED container -> packed container (density_hip_unpage_device): a check of the page directory, then a gather over it ----
constexpr uint32_t kPageTiles = kPageBytes / kCopyTile;   // work-groups per page
static_assert(kPageBytes % kCopyTile == 0, "a page is whole copy tiles");
typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
typedef u32x4 u32x4_u __attribute__((aligned(1)));         // a 16-byte load at any byte phase (gfx950 global memory takes it)

__device__ __forceinline__ uint32_t wave_sum(uint32_t v) {
    const uint32_t lane = threadIdx.x & 63u;
#pragma unroll
    for (uint32_t d = 32; d; d >>= 1) v += bperm(lane ^ d, v);
    return v;
}

// A wave per chunk: may the gather follow this chunk's directory?  1 .. pages_per_chunk pages, every page inside the container, at most a page of bytes in
// each, the bytes adding up to the size table's entry, and that no more than the chunk's worst case (the packed output is sized by it).  sizes[c]: the
// stream's length for the layout kernel, 0 where the directory is refused — then with bit 4 of *err, and the gather writes nothing at all.  Nothing is
// read through the directory here, and nothing outside it: `used` is checked before the entries it counts are read.
__global__ __launch_bounds__(256) void check_directory_kernel(const uint8_t* __restrict__ container, uint32_t n, uint64_t chunk_bytes, uint64_t total_len,
                                                              uint64_t dir_base, uint32_t pages_per_chunk, uint32_t n_pages, uint64_t* __restrict__ sizes,
                                                              uint32_t* __restrict__ err) {
    const uint32_t c = blockIdx.x * 4u + (threadIdx.x >> 6), lane = threadIdx.x & 63u;
    if (c >= n) return;
    const uint8_t* dir = container + dir_base + 16ull * (pages_per_chunk + 1u) * c;
    const uint32_t size = ld32u(container + kHeaderBytes + 4ull * c), used = ld32u(dir);
    bool bad = used == 0 || used > pages_per_chunk;
    uint32_t sum = 0;                                          // (at most pages_per_chunk pages of 64 KiB: a chunk is at most 1 GiB, its worst case below 2^31)
    if (!bad)
        for (uint32_t k = lane; k < used; k += 64u) {
            const uint8_t* e = dir + 16ull * (k + 1u);
            const uint32_t page = ld32u(e), bytes = ld32u(e + 8);
            if (page >= n_pages || bytes > kPageBytes) bad = true;
            else sum += bytes;
        }
    sum = wave_sum(sum);
    bad = ballot64(bad) != 0;
    const uint64_t first = (uint64_t)c * chunk_bytes, len = total_len - first < chunk_bytes ? total_len - first : chunk_bytes;
    if (sum != size || size > safe_size(DENSITY_HIP_CHAMELEON, len)) bad = true;
    if (lane == 0) {
        sizes[c] = bad ? 0ull : size;
        if (bad) atomicOr(err, 4u);
    }
}

// The gather: one work-group per (chunk, directory slot, 16 KiB tile of the page); slots and tiles not in use leave at once.  A page's used bytes go to the
// chunk's packed offset plus the bytes of the pages in front of it in the chunk's directory (summed here: a few dozen entries).  The destination has any
// byte phase: the stores are 16-byte aligned uint4, fed from loads at whatever phase that gives the source; the segment's first and last bytes (less than
// 16 each) go bytewise, with tile 0.  Every byte of the streams is written once; the zero gap up to the next stream's 16-byte boundary by the work-group
// that holds the stream's last byte.  The directory was checked (check_directory_kernel): with *err set nothing is read through it.
__global__ __launch_bounds__(kCopyThreads) void unpage_kernel(const uint8_t* __restrict__ in, uint64_t dir_base, uint64_t pages_base, uint32_t pages_per_chunk,
                                                              uint32_t n, const uint64_t* __restrict__ sizes, const uint64_t* __restrict__ offsets,
                                                              uint8_t* __restrict__ out, const uint32_t* __restrict__ err) {
    if (*err) return;
    const uint32_t tile = blockIdx.x % kPageTiles, slot = blockIdx.x / kPageTiles % pages_per_chunk, chunk = blockIdx.x / (kPageTiles * pages_per_chunk);
    const uint8_t* dir = in + dir_base + 16ull * (pages_per_chunk + 1u) * chunk;
    if (slot >= ld32u(dir)) return;
    const uint8_t* e = dir + 16ull * (slot + 1u);
    const uint32_t bytes = ld32u(e + 8);
    if ((uint64_t)tile * kCopyTile >= bytes) return;           // (an empty page too)
    __shared__ uint32_t wave_sums[kCopyThreads / 64];
    uint32_t before = 0;
    for (uint32_t j = threadIdx.x; j < slot; j += kCopyThreads) before += ld32u(dir + 16ull * (j + 1u) + 8);
    before = wave_sum(before);
    if ((threadIdx.x & 63u) == 0) wave_sums[threadIdx.x >> 6] = before;
    __syncthreads();
    before = 0;
#pragma unroll
    for (uint32_t w = 0; w < kCopyThreads / 64; ++w) before += wave_sums[w];
    const uint8_t* s = in + pages_base + (uint64_t)ld32u(e) * kPageBytes;
    const uint64_t size = sizes[chunk], end = offsets[chunk] + size;
    uint8_t* d = out + offsets[chunk] + before;
    const uint32_t phase = (uint32_t)(0u - (uint32_t)(uintptr_t)d) & 15u, head = phase < bytes ? phase : bytes;
    const uint32_t full = (bytes - head) / 16u, tail = bytes - head - 16u * full;
    const uint32_t i0 = tile * (kCopyTile / 16u) + threadIdx.x;
    u32x4 v[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) { const uint32_t i = i0 + (uint32_t)j * kCopyThreads; if (i < full) v[j] = *reinterpret_cast<const u32x4_u*>(s + head + 16ull * i); }
#pragma unroll
    for (int j = 0; j < 4; ++j) { const uint32_t i = i0 + (uint32_t)j * kCopyThreads; if (i < full) *reinterpret_cast<u32x4*>(d + head + 16ull * i) = v[j]; }
    if (tile != 0) return;
    if (threadIdx.x < head) d[threadIdx.x] = s[threadIdx.x];
    const uint32_t t1 = threadIdx.x - 64u, t2 = threadIdx.x - 128u;
    if (t1 < tail) d[bytes - tail + t1] = s[bytes - tail + t1];
    // the gap behind the chunk's stream is part of the container: zeros, not whatever the buffer held (none behind the last stream: container_len ends there)
    if (before + (uint64_t)bytes == size && chunk + 1u < n && t2 < ((0u - (uint32_t)end) & 15u)) out[end + t2] = 0;
}

// ---- chunk windows [first, first + count) of one or several containers of any form -> one packed container (density_hip_slice_device, density_hip_join_device) ----
// The windows' layout, one work-group.  The parts are walked in order.  Where chunk `first`'s stream lies in a packed part only its size table says: the
// 16-byte-rounded entries are scanned from chunk 0 on (tiles of kScanThreads, the carry of layout_common), from chunk `first` for the other forms (slotted:
// src_base + i * slot_stride; paged: the gather follows the directory, which check_directory_kernel has held against the table — lens comes from there, 0
// where it refused).  A second carry runs across the parts: K, the output's chunk number of the part's first chunk, and `at`, the offset in `out` where its
// first stream goes — the 16-byte boundary behind the part in front.  Left on the device for the gather, per output chunk: lens, src (the stream's ADDRESS, 0
// for a paged part's chunk: unpage_kernel moves those) and dst_off (offset in `out`: packed, from out_base); and, where `run` is not null, *run = the bytes
// from the first stream's start to the last one's end where there is ONE part, 0 for more (a caller with one packed part may move its window as that one
// run: the streams lie as the output wants them).  Written to `out` (any byte alignment): the header `hdr` with container_len = the last stream's end, every window's
// size-table entries, zeros over the gaps in front of the payloads and behind each stream but the last, the parts' seams included — what stands behind a
// source's stream is its own gap, another part's business, the trailer's padding or nothing at all.  Refused, with bit 4 of *err, and then no gap written,
// container_len = out_base and *run = 0: a window entry above its chunk's worst case or its slot, a window stream that ends behind its part's `limit`.
// Entries in front of a window are summed, not judged.
__global__ __launch_bounds__(kScanThreads) void window_layout_kernel(JoinSources parts, uint32_t n_parts, uint32_t algo, uint64_t chunk_bytes, uint8_t* __restrict__ out,
                                                                     uint64_t capacity, density_hip_header_t hdr, uint64_t out_base, uint64_t* lens,
                                                                     uint64_t* __restrict__ src, uint64_t* dst_off, uint64_t* __restrict__ run, uint32_t* __restrict__ err) {
    __shared__ uint64_t wave_sums[kScanThreads / 64];
    __shared__ uint64_t s_first, s_end;
    __shared__ uint32_t s_bad;
    if (threadIdx.x == 0) { s_first = 0; s_end = 0; s_bad = *err; }                              // (paged parts: what the directory checks raised)
    __syncthreads();
    uint64_t K = 0, at = out_base, end = out_base, span = 0;
    for (uint32_t p = 0; p < n_parts; ++p) {
        const JoinSource& part = parts.p[p];
        const uint8_t* in = part.in;
        const bool paged = part.slot_stride == kJoinPaged;
        const uint64_t slot_stride = paged ? 0ull : part.slot_stride, limit = part.limit, total_len = part.total_len, src_base = part.src_base;
        const uint64_t first = part.first, count = part.count;
        const uint64_t from = (slot_stride || paged) ? first : 0u, to = first + count;
        uint64_t carry = 0;
        for (uint64_t t0 = from; t0 < to; t0 += kScanThreads) {
            const uint64_t i = t0 + threadIdx.x;
            const bool in_window = i >= first && i < to;
            uint64_t raw = 0, keep = 0;
            if (i < to) {
                keep = raw = ld32u(in + kHeaderBytes + 4ull * i);
                if (in_window) {
                    const uint64_t a = i * chunk_bytes, len = total_len - a < chunk_bytes ? total_len - a : chunk_bytes;
                    if (paged) keep = lens[K + (i - first)];
                    else if (raw > safe_size((int)algo, len) || (slot_stride && raw > slot_stride)) { keep = 0; atomicOr(&s_bad, 4u); }
                }
            }
            uint64_t tile_total = 0;
            const uint64_t excl = carry + block_inclusive_scan(align16(keep), wave_sums, &tile_total) - align16(keep);
            if (in_window) {
                const uint64_t k = K + (i - first);
                const uint64_t so = paged ? 0ull : slot_stride ? src_base + i * slot_stride : src_base + excl;
                if (!paged && (so > limit || keep > limit - so)) { keep = 0; atomicOr(&s_bad, 4u); }  // the stream runs past its container: the gather must not follow it
                src[k] = paged ? 0ull : (uint64_t)(uintptr_t)(in + so);
                dst_off[k] = excl;                                                               // (from the scan's start: made the output's below)
                if (!paged) lens[k] = keep;
                st32u(out + kHeaderBytes + 4ull * k, (uint32_t)raw);
                if (i == first) s_first = excl;
                if (i == to - 1) s_end = excl + keep;
            }
            carry += tile_total;
        }
        __syncthreads();
        const uint64_t first_at = s_first;
        span = s_end - first_at;
        for (uint64_t k = threadIdx.x; k < count; k += kScanThreads) dst_off[K + k] = at + (dst_off[K + k] - first_at);
        end = at + span;
        at = align16(end);
        K += count;
        __syncthreads();                                                                         // (s_first and s_end are the next part's now)
    }
    const bool bad = s_bad != 0 || end > capacity;
    for (uint64_t k = threadIdx.x; k < K; k += kScanThreads) {
        const uint64_t e = dst_off[k] + lens[k];
        if (!bad && k + 1 < K) for (uint64_t q = e; q < align16(e); ++q) out[q] = 0;             // the gap behind the stream is part of the container: zeros
    }
    if (threadIdx.x == 0) {
        if (run) *run = bad || n_parts != 1 ? 0ull : span;
        if (bad) atomicOr(err, s_bad ? 4u : 2u);
        const uint64_t len = bad ? out_base : end;
        st32u(out, hdr.magic);
        st32u(out + 4, (uint32_t)hdr.algo | (uint32_t)hdr.version << 8 | (uint32_t)hdr.flags << 16);
        st32u(out + 8, hdr.chunk_size);
        st32u(out + 12, hdr.n_chunks);
        st32u(out + 16, (uint32_t)hdr.total_len);
        st32u(out + 20, (uint32_t)(hdr.total_len >> 32));
        st32u(out + 24, (uint32_t)len);
        st32u(out + 28, (uint32_t)(len >> 32));
    }
    // (as in layout_encode_kernel: the gaps in front of the payloads are zeros)
    const uint64_t table_end = kHeaderBytes + 4ull * hdr.n_chunks, ibase = (table_end + 15) / 16 * 16;
    const uint64_t iend = ibase + ((hdr.flags & DENSITY_HIP_FLAG_BLOCK_INDEX) ? (hdr.total_len + 255) / 256 : 0);
    if (threadIdx.x < ibase - table_end) out[table_end + threadIdx.x] = 0;
    if (threadIdx.x >= 32 && threadIdx.x - 32 < out_base - iend) out[iend + threadIdx.x - 32] = 0;
}

// The gather of `runs` byte runs: run r is lens[r] bytes from the address src[r] (the parts lie in different allocations) to out + dst_off[r], both at any byte
// phase.  A join's run is one output chunk's stream, so no run carries a gap; a packed slice's window is ONE run (the three words are the layout kernel's
// src[0], *run and dst_off[0], read here, so the host never learns them) and takes the gaps between its streams along as they stand.  src[r] == 0: a paged
// part's chunk, not moved here.  A run is cut into tiles of kCopyTile (tiles_per_run covers the longest a run can be); work-groups take tiles in a grid-stride
// loop and leave the tiles behind a run's end at once.  Inside a tile: bytes up to the first 16-byte boundary of the DESTINATION's address, 16-byte stores fed
// from loads at whatever phase that gives the source, bytes behind the last whole one (blank_chunks_kernel's cut).  Nothing where *err is set.
constexpr uint32_t kGatherMaxGroups = 256u * 32u;
__global__ __launch_bounds__(kCopyThreads) void run_gather_kernel(const uint64_t* __restrict__ src, const uint64_t* __restrict__ lens, const uint64_t* __restrict__ dst_off,
                                                                  uint32_t runs, uint64_t tiles_per_run, uint8_t* __restrict__ out, const uint32_t* __restrict__ err) {
    if (*err) return;
    const uint64_t units = (uint64_t)runs * tiles_per_run;
    for (uint64_t u = blockIdx.x; u < units; u += gridDim.x) {
        const uint64_t r = u / tiles_per_run, t0 = (u % tiles_per_run) * kCopyTile, len = lens[r], from = src[r];
        if (t0 >= len || from == 0) continue;
        const uint32_t n = len - t0 < kCopyTile ? (uint32_t)(len - t0) : kCopyTile;
        const uint8_t* s = reinterpret_cast<const uint8_t*>((uintptr_t)from) + t0;
        uint8_t* d = out + dst_off[r] + t0;
        const uint32_t lead = (0u - (uint32_t)(uintptr_t)d) & 15u, head = lead < n ? lead : n;
        const uint32_t full = (n - head) / 16u, tail_at = head + 16u * full;                     // (full <= 1024: four stores a lane cover it)
        u32x4 v[4];
#pragma unroll
        for (uint32_t j = 0; j < 4; ++j) { const uint32_t i = j * kCopyThreads + threadIdx.x; if (i < full) v[j] = *reinterpret_cast<const u32x4_u*>(s + head + 16ull * i); }
#pragma unroll
        for (uint32_t j = 0; j < 4; ++j) { const uint32_t i = j * kCopyThreads + threadIdx.x; if (i < full) *reinterpret_cast<u32x4*>(d + head + 16ull * i) = v[j]; }
        if (threadIdx.x < head) d[threadIdx.x] = s[threadIdx.x];
        if (threadIdx.x < n - tail_at) d[tail_at + threadIdx.x] = s[tail_at + threadIdx.x];
    }
}

// LDS ordering assumptions of chameleon.hip, checked on the device the library is running on.
__global__ __launch_bounds__(64) void selftest_kernel(uint32_t* __restrict__ fail) {
    __shared__ __attribute__((aligned(16))) uint16_t cells[256];
    const uint32_t lane = threadIdx.x;
    for (uint32_t i = lane; i < 256; i += 64) cells[i] = 0xffffu;
    __syncthreads();
    const uint32_t base = lds_addr(cells);
    uint32_t bad = 0, r0, r1, r2, r3;
    // (a) all lanes, one u16 cell: highest lane's write must survive; (b) lane pairs share a cell; (c) neighbours in
    // one dword do not clobber each other; (d) the read between two writes of one instruction stream sees the first.
    asm volatile(
        "ds_write_b16 %4, %8\n\t"
        "ds_read_u16 %0, %4\n\t"
        "ds_write_b16 %5, %8\n\t"
        "ds_read_u16 %1, %5\n\t"
        "ds_write_b16 %6, %8\n\t"
        "ds_read_u16 %2, %6\n\t"
        "ds_write_b16 %7, %8\n\t"
        "ds_read_u16 %3, %7\n\t"
        "ds_write_b16 %7, %9\n\t"
        "s_waitcnt lgkmcnt(0)"
        : "=&v"(r0), "=&v"(r1), "=&v"(r2), "=&v"(r3)
        : "v"(base), "v"(base + 64u + 2u * (lane >> 1)), "v"(base + 192u + 2u * lane), "v"(base + 2u * 200u + 2u * (lane & 7u)),
          "v"(lane), "v"(lane + 100u)
        : "memory");
    if (r0 != 63u) bad |= 1u;
    if (r1 != (lane | 1u)) bad |= 2u;
    if (r2 != lane) bad |= 4u;
    if (r3 != (56u + (lane & 7u))) bad |= 8u;
    __syncthreads();
    if (cells[200 + (lane & 7u)] != 156u + (lane & 7u)) bad |= 16u;
    if (bad) atomicOr(fail, bad);
}

}  // namespace

hipError_t launch_layout_encode(const uint64_t* d_sizes, uint32_t n_chunks, density_hip_header_t hdr, uint64_t payload_base, uint8_t* d_container,
                                uint64_t capacity, uint64_t* d_offsets, uint32_t* d_err, hipStream_t stream, uint64_t slot_stride) {
    // d_offsets has n_chunks + 1 entries; the extra one is scratch for the end offset
    hipLaunchKernelGGL(layout_encode_kernel, dim3(1), dim3(kScanThreads), 0, stream, d_sizes, n_chunks, hdr, payload_base, d_container, capacity,
                       d_offsets, d_offsets + n_chunks, d_err, slot_stride);
    return hipGetLastError();
}

hipError_t launch_layout_encode_paged(const uint64_t* d_sizes, uint32_t n_chunks, density_hip_header_t hdr, uint64_t dir_base, uint64_t dir_end, uint64_t pages_base, uint8_t* d_container,
                                      uint64_t capacity, const uint32_t* d_page_counter, uint32_t* d_err, hipStream_t stream) {
    hipLaunchKernelGGL(layout_encode_paged_kernel, dim3(1), dim3(kScanThreads), 0, stream, d_sizes, n_chunks, hdr, dir_base, dir_end, pages_base, d_container, capacity, d_page_counter, d_err);
    if (n_chunks) hipLaunchKernelGGL(clear_directory_tails_kernel, dim3((n_chunks + 3) / 4), dim3(256), 0, stream, n_chunks, dir_base, dir_end, d_container);
    return hipGetLastError();
}

// PAGED container, decode side: the streams' lengths from the u32 table; every chunk reads from page 0 on (the kernel follows the directory)
__global__ __launch_bounds__(kScanThreads) void layout_decode_paged_kernel(const uint8_t* __restrict__ container, uint32_t n, uint64_t* __restrict__ sizes, uint64_t* __restrict__ offsets) {
    const uint32_t* table = reinterpret_cast<const uint32_t*>(container + kHeaderBytes);
    for (uint32_t i = threadIdx.x; i < n; i += kScanThreads) { sizes[i] = table[i]; offsets[i] = 0; }
}
hipError_t launch_layout_decode_paged(const uint8_t* d_container, uint32_t n_chunks, uint64_t* d_sizes, uint64_t* d_offsets, hipStream_t stream) {
    hipLaunchKernelGGL(layout_decode_paged_kernel, dim3(1), dim3(kScanThreads), 0, stream, d_container, n_chunks, d_sizes, d_offsets);
    return hipGetLastError();
}

hipError_t launch_layout_encode_batch(const uint64_t* d_sizes, uint32_t first, uint32_t count, bool is_first, bool is_last, density_hip_header_t hdr,
                                      uint64_t payload_base, uint8_t* d_container, uint64_t capacity, uint64_t* d_offsets, uint64_t* d_carry, uint32_t* d_err,
                                      hipStream_t stream) {
    hipLaunchKernelGGL(layout_encode_batch_kernel, dim3(1), dim3(kScanThreads), 0, stream, d_sizes, first, count, is_first ? 1u : 0u, is_last ? 1u : 0u, hdr,
                       payload_base, d_container, capacity, d_offsets, d_carry, d_err);
    return hipGetLastError();
}

hipError_t launch_layout_decode(const uint8_t* d_container, uint64_t container_size, uint32_t n_chunks, uint64_t payload_base, uint64_t* d_sizes,
                                uint64_t* d_offsets, uint32_t* d_err, hipStream_t stream, uint64_t slot_stride) {
    hipLaunchKernelGGL(layout_decode_kernel, dim3(1), dim3(kScanThreads), 0, stream, d_container, container_size, n_chunks, payload_base, d_sizes,
                       d_offsets, d_offsets + n_chunks, d_err, slot_stride);
    return hipGetLastError();
}

hipError_t launch_compact(const uint8_t* d_slots, uint64_t slot_stride, const uint64_t* d_sizes, const uint64_t* d_offsets,
                          uint32_t n_chunks, uint8_t* d_container, const uint32_t* d_err, hipStream_t stream, bool more_follow) {
    if (n_chunks == 0) return hipSuccess;
    const uint32_t tiles = (uint32_t)((slot_stride + kCopyTile - 1) / kCopyTile);
    const uint64_t blocks = (uint64_t)tiles * n_chunks;
    if (blocks > 0x7fffffffull) return hipErrorInvalidValue;
    hipLaunchKernelGGL(compact_kernel, dim3((uint32_t)blocks), dim3(kCopyThreads), 0, stream, d_slots, slot_stride, d_sizes, d_offsets, tiles,
                       d_container, d_err, more_follow ? 1u : 0u);
    return hipGetLastError();
}

hipError_t launch_check_directory(const uint8_t* d_container, uint32_t n_chunks, uint64_t chunk_bytes, uint64_t total_len, uint64_t dir_base,
                                  uint32_t pages_per_chunk, uint32_t n_pages, uint64_t* d_sizes, uint32_t* d_err, hipStream_t stream) {
    if (n_chunks == 0) return hipSuccess;
    hipLaunchKernelGGL(check_directory_kernel, dim3((n_chunks + 3) / 4), dim3(256), 0, stream, d_container, n_chunks, chunk_bytes, total_len, dir_base,
                       pages_per_chunk, n_pages, d_sizes, d_err);
    return hipGetLastError();
}

hipError_t launch_unpage(const uint8_t* d_container, uint32_t n_chunks, uint64_t dir_base, uint64_t pages_base, uint32_t pages_per_chunk,
                         const uint64_t* d_sizes, const uint64_t* d_offsets, uint8_t* d_out, const uint32_t* d_err, hipStream_t stream) {
    if (n_chunks == 0) return hipSuccess;
    const uint64_t blocks = (uint64_t)n_chunks * pages_per_chunk * kPageTiles;
    if (blocks > 0x7fffffffull) return hipErrorInvalidValue;
    hipLaunchKernelGGL(unpage_kernel, dim3((uint32_t)blocks), dim3(kCopyThreads), 0, stream, d_container, dir_base, pages_base, pages_per_chunk, n_chunks,
                       d_sizes, d_offsets, d_out, d_err);
    return hipGetLastError();
}

hipError_t launch_window_layout(const JoinSources& parts, uint32_t n_parts, uint32_t algo, uint64_t chunk_bytes, uint8_t* d_out, uint64_t capacity,
                                density_hip_header_t hdr, uint64_t out_base, uint64_t* d_lens, uint64_t* d_src, uint64_t* d_dst_off, uint64_t* d_run, uint32_t* d_err,
                                hipStream_t stream) {
    hipLaunchKernelGGL(window_layout_kernel, dim3(1), dim3(kScanThreads), 0, stream, parts, n_parts, algo, chunk_bytes, d_out, capacity, hdr, out_base, d_lens, d_src,
                       d_dst_off, d_run, d_err);
    return hipGetLastError();
}

hipError_t launch_run_gather(const uint64_t* d_src, const uint64_t* d_lens, const uint64_t* d_dst_off, uint32_t runs, uint64_t longest_run, uint8_t* d_out,
                             const uint32_t* d_err, hipStream_t stream) {
    const uint64_t tiles = (longest_run + kCopyTile - 1) / kCopyTile, units = tiles * runs;
    if (units == 0) return hipSuccess;
    hipLaunchKernelGGL(run_gather_kernel, dim3((uint32_t)(units < kGatherMaxGroups ? units : kGatherMaxGroups)), dim3(kCopyThreads), 0, stream, d_src, d_lens, d_dst_off,
                       runs, tiles, d_out, d_err);
    return hipGetLastError();
}

hipError_t launch_selftest(uint32_t* d_fail, hipStream_t stream) {
    hipLaunchKernelGGL(selftest_kernel, dim3(1), dim3(64), 0, stream, d_fail);
    return hipGetLastError();
}

}  // namespace density
