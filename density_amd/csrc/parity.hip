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
//
// Version 2 of the blob ("double parity") carries a second set of rows Q behind the first (P): Q row g = XOR of 2^j · D over the group's members, j the member's
// place in its group, the product bytewise in GF(2^8) (polynomial 0x11D, generator 2).  The kernels that know it are the <true> instances of the templates
// below; the <false> instances are the version-1 kernels.  One pass makes both rows: the members are walked from the last down and Q follows Horner's rule,
// Q = 2·Q ^ D, on four packed bytes a word (xtime), so no member needs a constant of its own.  With both rows a group's plan word may name TWO damaged members
// at places a < b, with the two constants of the solve  D_a = c1·Pxy ^ c2·Qxy,  D_b = Pxy ^ D_a  (Pxy, Qxy: the rows XOR the sums over the intact members).
//
// The blob is a linear code over the zero-padded input, so a blob is kept current after an edit of its input by the same code applied to old ^ new
// (parity_update_kernel): only the rows of the edited chunks are read and written, in the same tiles and slots, each slot by the one lane that owns it.
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

// GF(2^8) with polynomial 0x11D on the four bytes of a word (of each of four words): v times 2, and v times the constant c by shift-and-add
__device__ __forceinline__ uint32_t xtime(uint32_t v) { return ((v & 0x7f7f7f7fu) << 1) ^ (((v >> 7) & 0x01010101u) * 0x1du); }
__device__ __forceinline__ u32x4 xtime(u32x4 v) { return ((v & 0x7f7f7f7fu) << 1) ^ (((v >> 7) & 0x01010101u) * 0x1du); }
template <class T>
__device__ __forceinline__ T gf_times(uint32_t c, T v) {
    T r = v ^ v;
#pragma unroll
    for (uint32_t bit = 0; bit < 8u; ++bit) {
        r ^= v & (0u - ((c >> bit) & 1u));
        v = xtime(v);
    }
    return r;
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

// Both rows at once: p[j] ^= D and q[j] = 2·q[j] ^ D for the members of group g from the LAST down, D as in xor_members — q ends as q·2^members ^ the XOR of
// 2^place · D —; the members `skip_a` and `skip_b` count as zeros (they keep their places).
__device__ __forceinline__ void horner_members(u32x4 (&p)[kParLoads], u32x4 (&q)[kParLoads], const uint32_t (&off)[kParLoads], uint32_t limit, const uint8_t* data,
                                               uint64_t size, uint32_t chunk, uint32_t n_chunks, uint32_t g, uint32_t n_groups, uint32_t skip_a, uint32_t skip_b) {
    const uint32_t members = (uint32_t)(((uint64_t)n_chunks - g + n_groups - 1u) / n_groups);
#pragma unroll 2
    for (uint32_t place = members; place-- > 0u;) {
        const uint64_t m = g + (uint64_t)place * n_groups;
#pragma unroll
        for (uint32_t j = 0; j < kParLoads; ++j) q[j] = xtime(q[j]);
        if (m == skip_a || m == skip_b) continue;
        const uint32_t len = chunk_len(size, chunk, (uint32_t)m);
        const uint8_t* d = data + m * chunk;
        u32x4 v[kParLoads];
#pragma unroll
        for (uint32_t j = 0; j < kParLoads; ++j) v[j] = off[j] < limit ? load16_clipped(d, off[j], len) : u32x4{0u, 0u, 0u, 0u};
#pragma unroll
        for (uint32_t j = 0; j < kParLoads; ++j) {
            p[j] ^= v[j];
            q[j] ^= v[j];
        }
    }
}
// the same for one byte (in the low byte of p and q)
__device__ __forceinline__ void horner_members_byte(uint32_t& p, uint32_t& q, uint32_t off, const uint8_t* data, uint64_t size, uint32_t chunk, uint32_t n_chunks, uint32_t g,
                                                    uint32_t n_groups, uint32_t skip_a, uint32_t skip_b) {
    const uint32_t members = (uint32_t)(((uint64_t)n_chunks - g + n_groups - 1u) / n_groups);
    for (uint32_t place = members; place-- > 0u;) {
        const uint64_t m = g + (uint64_t)place * n_groups;
        q = xtime(q);
        if (m == skip_a || m == skip_b || off >= chunk_len(size, chunk, (uint32_t)m)) continue;
        const uint32_t b = data[m * chunk + off];
        p ^= b;
        q ^= b;
    }
}

// The blob of `data`: the header (work-group 0) and n_groups rows of hdr.row_bytes bytes behind it — with kQ (hdr.version 2) the n_groups Q rows behind those, from
// the same loads —, every byte of them written.
template <bool kQ>
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
        u32x4 acc[kParLoads], q[kParLoads];
        uint32_t off[kParLoads];
#pragma unroll
        for (uint32_t j = 0; j < kParLoads; ++j) {
            acc[j] = q[j] = u32x4{0u, 0u, 0u, 0u};
            off[j] = t0 + (j * kParThreads + threadIdx.x) * 16u;
        }
        if (kQ) horner_members(acc, q, off, row_bytes, data, size, chunk, n_chunks, g, n_groups, kNoVictim, kNoVictim);
        else xor_members(acc, off, row_bytes, data, size, chunk, n_chunks, g, n_groups, kNoVictim);
        uint8_t* row = blob + kHeaderBytes + (uint64_t)g * row_bytes;
#pragma unroll
        for (uint32_t j = 0; j < kParLoads; ++j) {
            if (off[j] >= row_bytes) continue;                               // (row_bytes is a multiple of 16: a slot that begins inside the row ends inside it)
            store16(row + off[j], acc[j]);
            if (kQ) store16(row + (uint64_t)n_groups * row_bytes + off[j], q[j]);
        }
    }
}

// A group's plan word.  Version 1 (kQ false): the group's only damaged chunk.  Version 2: a | b << 8 | c1 << 16 | c2 << 24 — the places a <= b (below 255) of
// its one (a == b, the constants 0) or two damaged members in the group, and for two the constants of the solve.  kNoVictim either way: nothing to rebuild.
// victims_of: how many, and which chunks.
template <bool kQ>
__device__ __forceinline__ uint32_t victims_of(uint32_t word, uint32_t g, uint32_t n_groups, uint32_t (&k)[2]) {
    if (word == kNoVictim) return 0u;
    if (!kQ) { k[0] = k[1] = word; return 1u; }
    const uint32_t a = word & 255u, b = (word >> 8) & 255u;
    k[0] = g + a * n_groups;
    k[1] = g + b * n_groups;
    return a == b ? 1u : 2u;
}
// The word of the pair at places a < b < 255: with d = 2^(b-a) ^ 1 (not 0: 2 has order 255), c1 = 2^(b-a) / d and c2 = 2^(-a) / d, by the logarithm of d — a
// walk along the powers of 2, once per group and by one lane.
__device__ uint32_t gf_pow2(uint32_t e) {
    uint32_t r = 1u;
    for (; e; --e) r = xtime(r);
    return r;
}
__device__ uint32_t pair_word(uint32_t a, uint32_t b) {
    const uint32_t d = gf_pow2(b - a) ^ 1u;
    uint32_t log_d = 0;
    for (uint32_t r = 1u; r != d; r = xtime(r)) ++log_d;
    const uint32_t c1 = gf_pow2((b - a + 255u - log_d) % 255u), c2 = gf_pow2((510u - a - log_d) % 255u);
    return a | b << 8 | c1 << 16 | c2 << 24;
}

// victim[g] = group g's plan word: the only chunk of the group whose verdict is DENSITY_HIP_CHUNK_DAMAGED — with kQ: the only one or the only two —, kNoVictim where
// there are none or more; the accumulators of the chunks it names are cleared for the sum that follows the rebuild.  A work-group per group, in a grid-stride
// loop; the lanes share out the group's verdict words.
template <bool kQ>
__global__ __launch_bounds__(kParThreads) void recover_plan_kernel(const uint32_t* __restrict__ verdict, uint32_t n_chunks, uint32_t n_groups,
                                                                   uint32_t* __restrict__ victim, uint32_t* __restrict__ acc) {
    __shared__ uint32_t s_count, s_first, s_last;
    for (uint32_t g = blockIdx.x; g < n_groups; g += gridDim.x) {
        if (threadIdx.x == 0) { s_count = s_last = 0u; s_first = kNoVictim; }
        __syncthreads();
        uint32_t count = 0, first = kNoVictim, last = 0;
        for (uint64_t m = g + (uint64_t)threadIdx.x * n_groups; m < n_chunks; m += (uint64_t)kParThreads * n_groups)
            if (verdict[m] == DENSITY_HIP_CHUNK_DAMAGED) {
                ++count;
                first = first < (uint32_t)m ? first : (uint32_t)m;
                last = (uint32_t)m;
            }
        if (count) { atomicAdd(&s_count, count); atomicMin(&s_first, first); atomicMax(&s_last, last); }
        __syncthreads();
        if (threadIdx.x == 0) {
            uint32_t word = kNoVictim;
            if (s_count == 1u) {
                word = kQ ? (s_first - g) / n_groups * 0x101u : s_first;
                acc[s_first] = 0u;
            } else if (kQ && s_count == 2u) {
                word = pair_word((s_first - g) / n_groups, (s_last - g) / n_groups);
                acc[s_first] = acc[s_last] = 0u;
            }
            victim[g] = word;
        }
        __syncthreads();                                                     // (s_count is cleared again in the next trip)
    }
}

// One tile of a pair: group g's damaged members ka < kb (so ka is a whole chunk and the tile, which begins inside the chunk size, inside it; kb may be the ragged
// last one), neither read, both written by the lane that holds their position: from zeros the walk gives the sums over the intact members, the rows make them
// Pxy and Qxy, and D_a = c1·Pxy ^ c2·Qxy, D_b = Pxy ^ D_a.  The tile is cut as in recover_rebuild_kernel, by ka's address: kb's region is whole chunks away.
// kb is written at its true length — where that ends inside a 16-byte slot, bytewise.
__device__ __forceinline__ void rebuild_pair_tile(uint8_t* out, uint64_t size, uint32_t chunk, uint32_t n_chunks, const uint8_t* __restrict__ rows, uint32_t n_groups,
                                                  uint32_t row_bytes, uint32_t g, uint32_t t0, uint32_t ka, uint32_t kb, uint32_t c1, uint32_t c2) {
    const uint32_t len_b = chunk_len(size, chunk, kb);
    const uint32_t n = chunk - t0 < kParTile ? chunk - t0 : kParTile, n_b = t0 >= len_b ? 0u : len_b - t0 < n ? len_b - t0 : n;
    uint8_t *pa = out + (uint64_t)ka * chunk + t0, *pb = out + (uint64_t)kb * chunk + t0;
    const uint8_t *prow = rows + (uint64_t)g * row_bytes + t0, *qrow = prow + (uint64_t)n_groups * row_bytes;   // (two chunks and more: row_bytes == chunk)
    const uint32_t lead = (16u - (uint32_t)((uintptr_t)pa & 15u)) & 15u, head = lead < n ? lead : n;
    const uint32_t full = (n - head) / 16u, tail_at = head + full * 16u;
    const auto byte_at = [&](uint32_t i) {
        uint32_t p = 0u, q = 0u;
        horner_members_byte(p, q, t0 + i, out, size, chunk, n_chunks, g, n_groups, ka, kb);
        p ^= prow[i];
        q ^= qrow[i];
        const uint32_t da = gf_times(c1, p) ^ gf_times(c2, q);
        pa[i] = (uint8_t)da;
        if (i < n_b) pb[i] = (uint8_t)(da ^ p);
    };
    if (threadIdx.x < head) byte_at(threadIdx.x);
    u32x4 p[kParLoads], q[kParLoads];
    uint32_t off[kParLoads];
#pragma unroll
    for (uint32_t j = 0; j < kParLoads; ++j) {
        off[j] = t0 + head + 16u * (j * kParThreads + threadIdx.x);
        p[j] = q[j] = u32x4{0u, 0u, 0u, 0u};
    }
    horner_members(p, q, off, t0 + tail_at, out, size, chunk, n_chunks, g, n_groups, ka, kb);
#pragma unroll
    for (uint32_t j = 0; j < kParLoads; ++j) {
        const uint32_t i = j * kParThreads + threadIdx.x, at = head + 16u * i;
        if (i >= full) continue;
        p[j] ^= load16(prow + at);
        q[j] ^= load16(qrow + at);
        const u32x4 da = gf_times(c1, p[j]) ^ gf_times(c2, q[j]), db = da ^ p[j];
        *reinterpret_cast<u32x4*>(pa + at) = da;
        if (at + 16u <= n_b) *reinterpret_cast<u32x4*>(pb + at) = db;
        else if (at < n_b) {
            const uint32_t w[4] = {db.x, db.y, db.z, db.w};
#pragma unroll
            for (uint32_t b = 0; b < 16u; ++b)
                if (at + b < n_b) pb[at + b] = (uint8_t)(w[b / 4u] >> (8u * (b % 4u)));
        }
    }
    if (threadIdx.x < n - tail_at) byte_at(tail_at + threadIdx.x);
}

// Group g's victim k (recover_plan_kernel), where it has one: the bytes of k's region of `out` become row g XOR the regions of the group's other members, the
// last chunk at its true length, `out` and the rows at any alignment.  Inside a tile, as in blank_chunks_kernel: bytes up to the first 16-byte boundary
// of the ADDRESS (the other members' regions are whole chunks away: the same phase), 16-byte stores, bytes behind the last whole one.  `out` is read
// and written, but never the same chunk: no other chunk of the group is rebuilt.  With kQ a group may have a pair instead: rebuild_pair_tile, and the Q rows
// are read for nothing else.
template <bool kQ>
__global__ __launch_bounds__(kParThreads) void recover_rebuild_kernel(uint8_t* out, uint64_t size, uint32_t chunk, uint32_t n_chunks, const uint8_t* __restrict__ rows,
                                                                      uint32_t n_groups, uint32_t row_bytes, const uint32_t* __restrict__ victim) {
    const uint32_t tiles = (chunk + kParTile - 1) / kParTile;
    const uint64_t units = (uint64_t)n_groups * tiles;
    for (uint64_t u = blockIdx.x; u < units; u += gridDim.x) {
        const uint32_t g = (uint32_t)(u / tiles), t0 = (uint32_t)(u % tiles) * kParTile;
        const uint32_t word = victim[g];
        uint32_t ks[2];
        const uint32_t count = victims_of<kQ>(word, g, n_groups, ks);
        if (count == 0u) continue;
        if (kQ && count == 2u) {
            rebuild_pair_tile(out, size, chunk, n_chunks, rows, n_groups, row_bytes, g, t0, ks[0], ks[1], (word >> 16) & 255u, word >> 24);
            continue;
        }
        const uint32_t k = ks[0];
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
template <bool kQ>
__global__ __launch_bounds__(kSumThreads) void recover_sum_kernel(const uint8_t* __restrict__ out, uint64_t size, uint32_t chunk, uint32_t n_groups,
                                                                  const uint32_t* __restrict__ victim, uint32_t* __restrict__ acc) {
    __shared__ uint32_t part[kSumThreads / 64];
    const uint32_t tiles = (chunk + kSumTile - 1) / kSumTile;
    const uint64_t units = (uint64_t)n_groups * tiles;
    for (uint64_t u = blockIdx.x; u < units; u += gridDim.x) {
        const uint32_t g = (uint32_t)(u / tiles), t0 = (uint32_t)(u % tiles) * kSumTile;
        uint32_t ks[2];
        const uint32_t count = victims_of<kQ>(victim[g], g, n_groups, ks);   // (the same for the whole work-group, like every test in front of sum_tile)
        for (uint32_t v = 0; v < count; ++v) {
            const uint32_t len = chunk_len(size, chunk, ks[v]);
            if (t0 < len) sum_tile(out + (uint64_t)ks[v] * chunk, len, t0, part, acc + ks[v]);
        }
    }
}

// ... and held against the trailer once more, a thread per group: a victim whose bytes now have the trailer's checksum becomes DENSITY_HIP_CHUNK_RECOVERED and
// moves from *damaged to *recovered; one whose bytes have not (a damaged row, a damaged trailer entry) stays DENSITY_HIP_CHUNK_DAMAGED — each of a pair for itself.
template <bool kQ>
__global__ __launch_bounds__(256) void recover_verify_kernel(const uint32_t* __restrict__ acc, uint64_t size, uint32_t chunk, uint32_t n_groups,
                                                             const uint32_t* __restrict__ victim, const uint8_t* __restrict__ expect, uint32_t* __restrict__ verdict,
                                                             uint32_t* __restrict__ damaged, uint32_t* __restrict__ recovered) {
    const uint32_t g = blockIdx.x * 256u + threadIdx.x;
    if (g >= n_groups) return;
    uint32_t ks[2];
    const uint32_t count = victims_of<kQ>(victim[g], g, n_groups, ks);
    for (uint32_t v = 0; v < count; ++v) {
        const uint32_t k = ks[v];
        if (fmix32(acc[k] + chunk_len(size, chunk, k)) != ld32u(expect + 4ull * k)) continue;
        verdict[k] = DENSITY_HIP_CHUNK_RECOVERED;
        atomicSub(damaged, 1u);
        atomicAdd(recovered, 1u);
    }
}

// The 16 bytes at input position `pos` of an edit's side: `p` holds the input's bytes [base, base + size) and every other position counts as zero — clipped on BOTH
// sides, where load16_clipped clips at the end only.
__device__ __forceinline__ u32x4 load16_window(const uint8_t* p, uint64_t base, uint64_t size, uint64_t pos) {
    if (pos >= base + size || pos + 16u <= base) return u32x4{0u, 0u, 0u, 0u};
    if (pos >= base && base + size - pos >= 16u) return load16(p + (pos - base));
    uint32_t w[4];
#pragma unroll
    for (uint32_t q = 0; q < 4u; ++q) {
        w[q] = 0u;
#pragma unroll
        for (uint32_t b = 0; b < 4u; ++b) {
            const uint64_t i = pos + 4u * q + b - base;                      // (in front of the window: wraps to a value no size reaches)
            if (i < size) w[q] |= (uint32_t)p[i] << (8u * b);
        }
    }
    const u32x4 v{w[0], w[1], w[2], w[3]};
    return v;
}

// An edit of the blob's input, as launch_parity_update hands it over: input bytes [offset, offset + old_size) held `old_data` and hold `new_data` (new_size bytes,
// the shorter of the two zero-padded) now — chunks [m0, m1) are touched, of tg = min(m1 - m0, n_groups) groups, and of every row the tiles [tile0, tile0 + tiles).
struct ParityEdit {
    const uint8_t *old_data, *new_data;
    uint64_t offset, old_size, new_size, total_len;                          // total_len, n_chunks: of the input after the edit
    uint32_t chunk, n_groups, row_bytes, n_chunks, m0, m1, tg, tile0, tiles;
};

// The blob brought up to date after an edit of its input.  The blob is linear over the zero-padded input, so the edit's effect on it is the same code applied to
// delta = old ^ new: P row g ^= delta of every touched member, Q row g ^= 2^place · delta.  A unit is a tile of a touched group's row; every 16-byte slot of it
// belongs to one lane, which reads, modifies and writes it — no atomics, and rows of groups no touched chunk belongs to are not written.  The touched members of a
// group stand at consecutive places, so Q follows Horner from the last one down, q = 2·q ^ delta, and one product with 2^(place of the first) a slot ends it.
// Work-group 0 writes the header words the edit changes (nobody reads the header here).
template <bool kQ>
__global__ __launch_bounds__(kParThreads) void parity_update_kernel(uint8_t* blob, ParityEdit e) {
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        st32u(blob + 12, e.n_chunks);
        st32u(blob + 16, (uint32_t)e.total_len);
        st32u(blob + 20, (uint32_t)(e.total_len >> 32));
    }
    const uint64_t units = (uint64_t)e.tg * e.tiles;
    for (uint64_t u = blockIdx.x; u < units; u += gridDim.x) {
        const uint32_t first = e.m0 + (uint32_t)(u / e.tiles), t0 = (e.tile0 + (uint32_t)(u % e.tiles)) * kParTile;   // (first: the group's first touched member)
        const uint32_t g = first % e.n_groups, members = (uint32_t)(((uint64_t)e.m1 - first + e.n_groups - 1u) / e.n_groups);
        u32x4 p[kParLoads], q[kParLoads];
        uint32_t off[kParLoads];
#pragma unroll
        for (uint32_t j = 0; j < kParLoads; ++j) {
            p[j] = q[j] = u32x4{0u, 0u, 0u, 0u};
            off[j] = t0 + (j * kParThreads + threadIdx.x) * 16u;
        }
#pragma unroll 2
        for (uint32_t i = members; i-- > 0u;) {
            const uint64_t at = ((uint64_t)first + (uint64_t)i * e.n_groups) * e.chunk;   // (a slot that begins inside the row ends inside the member's chunk: row_bytes <= chunk)
            u32x4 d[kParLoads];
#pragma unroll
            for (uint32_t j = 0; j < kParLoads; ++j)
                d[j] = off[j] < e.row_bytes ? load16_window(e.old_data, e.offset, e.old_size, at + off[j]) ^ load16_window(e.new_data, e.offset, e.new_size, at + off[j])
                                            : u32x4{0u, 0u, 0u, 0u};
#pragma unroll
            for (uint32_t j = 0; j < kParLoads; ++j) {
                p[j] ^= d[j];
                if (kQ) q[j] = xtime(q[j]) ^ d[j];
            }
        }
        const uint32_t c = kQ ? gf_pow2(first / e.n_groups) : 1u;
        uint8_t* row = blob + kHeaderBytes + (uint64_t)g * e.row_bytes;
#pragma unroll
        for (uint32_t j = 0; j < kParLoads; ++j) {
            if (off[j] >= e.row_bytes) continue;
            store16(row + off[j], load16(row + off[j]) ^ p[j]);
            if (kQ) {
                uint8_t* qrow = row + (uint64_t)e.n_groups * e.row_bytes;
                store16(qrow + off[j], load16(qrow + off[j]) ^ gf_times(c, q[j]));
            }
        }
    }
}

uint32_t grid_for(uint64_t units) { return (uint32_t)(units < 1 ? 1 : units < kParMaxGroups ? units : kParMaxGroups); }

template <bool kQ>
hipError_t recover_rebuild(uint8_t* d_out, uint64_t size, uint32_t chunk, uint32_t n_chunks, const uint8_t* d_rows, uint32_t n_groups, uint32_t row_bytes,
                           const uint32_t* d_verdicts, uint32_t* d_victim, uint32_t* d_acc, hipStream_t stream) {
    hipLaunchKernelGGL(recover_plan_kernel<kQ>, dim3(grid_for(n_groups)), dim3(kParThreads), 0, stream, d_verdicts, n_chunks, n_groups, d_victim, d_acc);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    const uint64_t units = (uint64_t)n_groups * ((chunk + kParTile - 1) / kParTile);
    hipLaunchKernelGGL(recover_rebuild_kernel<kQ>, dim3(grid_for(units)), dim3(kParThreads), 0, stream, d_out, size, chunk, n_chunks, d_rows, n_groups, row_bytes, d_victim);
    return hipGetLastError();
}

template <bool kQ>
hipError_t recover_verify(const uint8_t* d_out, uint64_t size, uint32_t chunk, uint32_t n_groups, const uint32_t* d_victim, uint32_t* d_acc, const uint8_t* d_expect,
                          uint32_t* d_verdicts, uint32_t* d_damaged, uint32_t* d_recovered, hipStream_t stream) {
    const uint64_t units = (uint64_t)n_groups * ((chunk + kSumTile - 1) / kSumTile);
    hipLaunchKernelGGL(recover_sum_kernel<kQ>, dim3(grid_for(units)), dim3(kSumThreads), 0, stream, d_out, size, chunk, n_groups, d_victim, d_acc);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(recover_verify_kernel<kQ>, dim3((n_groups + 255u) / 256u), dim3(256), 0, stream, d_acc, size, chunk, n_groups, d_victim, d_expect, d_verdicts, d_damaged,
                       d_recovered);
    return hipGetLastError();
}

}  // namespace

hipError_t launch_parity_rows(const uint8_t* d_data, const density_hip_parity_header_t& hdr, uint8_t* d_blob, hipStream_t stream) {
    const uint64_t units = (uint64_t)hdr.n_groups * ((hdr.row_bytes + kParTile - 1) / kParTile);
    if (hdr.version == 2) hipLaunchKernelGGL(parity_rows_kernel<true>, dim3(grid_for(units)), dim3(kParThreads), 0, stream, d_data, hdr, d_blob);
    else hipLaunchKernelGGL(parity_rows_kernel<false>, dim3(grid_for(units)), dim3(kParThreads), 0, stream, d_data, hdr, d_blob);
    return hipGetLastError();
}

hipError_t launch_parity_update(uint8_t* d_blob, const density_hip_parity_header_t& after, uint64_t offset, const uint8_t* d_old, uint64_t old_size, const uint8_t* d_new,
                                uint64_t new_size, hipStream_t stream) {
    const uint64_t span = old_size > new_size ? old_size : new_size, chunk = after.chunk_size;
    if (span == 0 || after.n_groups == 0) return hipSuccess;
    const uint64_t m0 = offset / chunk, m1 = (offset + span + chunk - 1) / chunk;
    ParityEdit e{d_old, d_new, offset, old_size, new_size, after.total_len, after.chunk_size, after.n_groups, after.row_bytes, after.n_chunks, (uint32_t)m0, (uint32_t)m1,
                 (uint32_t)std::min<uint64_t>(m1 - m0, after.n_groups), 0u, (after.row_bytes + kParTile - 1) / kParTile};
    if (m1 - m0 == 1) {                                                      // one chunk: only the tiles of its row the edit covers — a 100-byte edit is one work-group
        const uint64_t lo = offset - m0 * chunk, hi = std::min<uint64_t>(lo + span, after.row_bytes);
        e.tile0 = (uint32_t)(lo / kParTile);
        e.tiles = hi > lo ? (uint32_t)((hi + kParTile - 1) / kParTile) - e.tile0 : 0u;
    }
    const uint32_t grid = grid_for((uint64_t)e.tg * e.tiles);
    if (after.version == 2) hipLaunchKernelGGL(parity_update_kernel<true>, dim3(grid), dim3(kParThreads), 0, stream, d_blob, e);
    else hipLaunchKernelGGL(parity_update_kernel<false>, dim3(grid), dim3(kParThreads), 0, stream, d_blob, e);
    return hipGetLastError();
}

hipError_t launch_recover_rebuild(uint8_t* d_out, uint64_t size, uint32_t chunk, uint32_t n_chunks, const uint8_t* d_rows, uint32_t n_groups, uint32_t row_bytes, bool with_q,
                                  const uint32_t* d_verdicts, uint32_t* d_victim, uint32_t* d_acc, hipStream_t stream) {
    if (n_chunks == 0) return hipSuccess;
    return with_q ? recover_rebuild<true>(d_out, size, chunk, n_chunks, d_rows, n_groups, row_bytes, d_verdicts, d_victim, d_acc, stream)
                  : recover_rebuild<false>(d_out, size, chunk, n_chunks, d_rows, n_groups, row_bytes, d_verdicts, d_victim, d_acc, stream);
}

hipError_t launch_recover_verify(const uint8_t* d_out, uint64_t size, uint32_t chunk, uint32_t n_chunks, uint32_t n_groups, bool with_q, const uint32_t* d_victim,
                                 uint32_t* d_acc, const uint8_t* d_expect, uint32_t* d_verdicts, uint32_t* d_damaged, uint32_t* d_recovered, hipStream_t stream) {
    const hipError_t e = hipMemsetAsync(d_recovered, 0, sizeof(uint32_t), stream);
    if (e != hipSuccess || n_chunks == 0) return e;
    return with_q ? recover_verify<true>(d_out, size, chunk, n_groups, d_victim, d_acc, d_expect, d_verdicts, d_damaged, d_recovered, stream)
                  : recover_verify<false>(d_out, size, chunk, n_groups, d_victim, d_acc, d_expect, d_verdicts, d_damaged, d_recovered, stream);
}

}  // namespace density
