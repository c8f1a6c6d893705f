// rotor.hip — Chameleon wave-rotation kernels for gfx950 (MI355X): the default encode / index-fed decode path.
//
// This file: the design notes, the start-up self-test of what the kernels assume about the LDS, two small kernels of the segmented
// whole-stream encode (offset scan, byte gather) and the host side of the cycle accounting.  The encoder is rotor_encode.hip, the
// decoder rotor_decode.hip, the device code they share rotor_dev.hpp.
//
// One work-group owns one chunk (= one independent reference stream, chameleon.rs:45-53) and its dictionary (64 Ki exact 16-bit
// entries = 128 KiB of LDS, chameleon_dev.hpp).  The chunk is cut into ROUNDS of R blocks that rotate over W wavefronts: R = 16 on
// W = 8 for the encoder (4 KiB rounds, 256 registers per wave: the quads of a round stay in registers from the hash to the emit),
// R = 12 on W = 12 for the decoder (rotor_dev.hpp: kEncRound .. kDecWaves; the geometries that lost against these: DESIGN.md 4.3).
// Wave w takes the rounds r = w, w + W, w + 2W, ... and does EVERYTHING for its round itself, in registers: global loads, hashing,
// the dictionary step, signatures, the copy-mode FSM, record offsets, stores.  There are no staging rings and no per-round
// work-group barrier.  What IS sequential in the reference — the dictionary (every quad sees the table its predecessors left,
// chameleon.rs:88-100) and the running output position / ProtectionState (codec.rs:34-70) — is passed from round to round by
// two token chains through LDS:
//
//   D chain  "dictionary token".  The holder issues its R ordered exchanges (ds_mskor_rtn_b32: one instruction = the 64
//            sequential dictionary steps of a block, LDS lane order; chameleon_dev.hpp) back to back from prepared registers
//            and writes the token for the next round BEHIND them in its own LDS instruction stream.  A wave's LDS
//            instructions execute in issue order, so whoever sees the new token also sees the table after those exchanges.
//            This chain is the critical path of the kernel: ~R x 23 cycles of exchanges + one LDS write->read hand-off per round.
//   O chain  "commit token" + payload {output position, FSM state}.  After its exchanges a wave turns the R answers into R
//            signatures (hit == answer equals own entry; __ballot == the signature word, io/write_signature.rs:14-17), waits for
//            the commit token, runs the FSM over its R blocks in closed form, passes position + state on, and only then stores.
//
// Copy mode (protection_state.rs) is a feedback from the signatures to "which blocks touch the dictionary at all", so the
// exchanges of a round are speculative: "no raw-copy block in this round".  The commit step knows the truth.  When it finds
// a block that had to be a raw copy it raises an abort: all waves meet at a barrier, the rounds that exchanged after the
// last committed one roll their blocks back in reverse order (the lowest lane of a slot holds the pre-block entry, so the
// answers are written back lane-reversed with one ds_write_b16 per block), and the chain restarts at the failed round in SLOW
// mode: the token holder first waits for its commit payload and then takes its round in order — in batches against a prediction
// of the FSM, or block by block (rotor_encode.hip: ordered rounds).  Slow mode ends after a few rounds that leave the FSM calm.
// Every chunk starts in slow mode (its first blocks are incompressible by construction: empty dictionary).  Rounds that contain a
// zero entry outside slot 0 (zero-entry map, about one quad in 64 Ki) and the chunk's last partial round are also walked in order.
//
// The split encoder (kernel variant 2048) runs the same rounds on 8 CHAIN waves (hash, exchange, signatures, commit) and 8 EMIT
// waves (loads, records), the quads handed over through an LDS ring (rotor_dev.hpp).
//
// Decode (index-fed: the container's block index gives record lengths and raw-copy blocks, include/density_hip.h) uses the
// same D chain for the dictionary (MAP lanes exchange with mask 0 = read, PLAIN lanes write: chameleon.rs:56-68); record
// positions of the whole chunk come from one prefix sum over the index at kernel start; a Z chain orders the rare
// zero-entry-map accesses.  Streams without an index, chunks above 4 MiB and unaligned buffers run on chameleon.hip's kernels.
#include <cstdio>
#include <cstdlib>

#include "rotor_dev.hpp"

namespace density {

// where the streams of segments [first, first + count) go: one behind the other from *carry on, which moves to their end (write_buffer.rs:29-31's
// running total, a few dozen sizes at a time)
__global__ void scan_offsets_kernel(const uint64_t* __restrict__ sizes, uint32_t first, uint32_t count, uint64_t* __restrict__ carry, uint64_t* __restrict__ offsets) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    uint64_t at = *carry;
    for (uint32_t i = 0; i < count; ++i) { offsets[first + i] = at; at += sizes[first + i]; }
    *carry = at;
}

// 16 bytes per lane: aligned stores, unaligned loads (the streams start at any even offset of the destination); head and tail by bytes
__global__ __launch_bounds__(256) void compact_bytes_kernel(const uint8_t* __restrict__ src, uint64_t src_stride, const uint64_t* __restrict__ sizes,
                                                            const uint64_t* __restrict__ offsets, uint8_t* __restrict__ dst) {
    typedef uint4 uint4_u __attribute__((aligned(1)));
    const uint64_t chunk = blockIdx.y;
    const uint64_t n = sizes[chunk];
    const uint8_t* s = src + chunk * src_stride;
    uint8_t* d = dst + offsets[chunk];
    uint64_t head = (16 - (reinterpret_cast<uintptr_t>(d) & 15)) & 15;
    if (head > n) head = n;
    const uint64_t vecs = (n - head) / 16;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < vecs; i += (uint64_t)gridDim.x * blockDim.x)
    {
        const uint4_u* sp = reinterpret_cast<const uint4_u*>(s + head + 16 * i);
        const uint4 v = {sp->x, sp->y, sp->z, sp->w};
        *reinterpret_cast<uint4*>(d + head + 16 * i) = v;
    }
    if (blockIdx.x == 0) {
        if (threadIdx.x < head) d[threadIdx.x] = s[threadIdx.x];
        const uint64_t tail0 = head + 16 * vecs;
        if (tail0 + threadIdx.x < n && threadIdx.x < 16) d[tail0 + threadIdx.x] = s[tail0 + threadIdx.x];
    }
}

// ---------------------------------------------------------------------------------------------------------------
// Start-up self-test of what these kernels assume about the LDS (density_hip_selftest / acquire_ctx):
//  (1) ds_mskor_rtn_b32 services the lanes of one instruction in ascending lane order — same half-dword, alternating halves of
//      one dword, mask-0 readers between writers, back-to-back instructions;
//  (2) a plain ds_write_b32 issued behind a wave's exchanges is not visible before them (the token hand-off), checked by 16
//      waves rotating like the kernels do, all hammering the same few dictionary slots;
//  (3) the lane-reversed ds_write_b16 restores a block (rollback).
// ---------------------------------------------------------------------------------------------------------------
namespace {

// (the self-test rotates rounds of 8 blocks over 16 waves, with an exchange statement of its own: answers and addresses in separate
// registers, and the token behind the exchanges or — bit 0 of DENSITY_HIP_TUNE, debug build — behind their answers)
constexpr uint32_t kRotWaves = 16, kRotThreads = kRotWaves * 64;
constexpr uint32_t kR = 8;                                   // blocks per round
#define DENSITY_ROT_XCHG8                                   \
    "ds_mskor_rtn_b32 %0, %8, %16, %24\n\t"                 \
    "ds_mskor_rtn_b32 %1, %9, %17, %25\n\t"                 \
    "ds_mskor_rtn_b32 %2, %10, %18, %26\n\t"                \
    "ds_mskor_rtn_b32 %3, %11, %19, %27\n\t"                \
    "ds_mskor_rtn_b32 %4, %12, %20, %28\n\t"                \
    "ds_mskor_rtn_b32 %5, %13, %21, %29\n\t"                \
    "ds_mskor_rtn_b32 %6, %14, %22, %30\n\t"                \
    "ds_mskor_rtn_b32 %7, %15, %23, %31\n\t"
#define DENSITY_ROT_OPERANDS(ret, addr, mask, val, tokaddr, tokval)                                                                     \
    : "=&v"(ret[0]), "=&v"(ret[1]), "=&v"(ret[2]), "=&v"(ret[3]), "=&v"(ret[4]), "=&v"(ret[5]), "=&v"(ret[6]), "=&v"(ret[7])              \
    : "v"(addr[0]), "v"(addr[1]), "v"(addr[2]), "v"(addr[3]), "v"(addr[4]), "v"(addr[5]), "v"(addr[6]), "v"(addr[7]),                     \
      "v"(mask[0]), "v"(mask[1]), "v"(mask[2]), "v"(mask[3]), "v"(mask[4]), "v"(mask[5]), "v"(mask[6]), "v"(mask[7]),                     \
      "v"(val[0]), "v"(val[1]), "v"(val[2]), "v"(val[3]), "v"(val[4]), "v"(val[5]), "v"(val[6]), "v"(val[7]), "v"(tokaddr), "v"(tokval)  \
    : "memory"
__device__ __forceinline__ void exchange_round(uint32_t (&ret)[kR], const uint32_t (&addr)[kR], const uint32_t (&mask)[kR], const uint32_t (&val)[kR],
                                               uint32_t tokaddr, uint32_t tokval, bool token_after_answers) {
    if (!token_after_answers) {
        asm volatile(DENSITY_ROT_XCHG8 "ds_write_b32 %32, %33\n\ts_waitcnt lgkmcnt(0)" DENSITY_ROT_OPERANDS(ret, addr, mask, val, tokaddr, tokval));
    } else {   // tuning / fall-back form: the token leaves only after the last answer is back
        asm volatile(DENSITY_ROT_XCHG8 "s_waitcnt lgkmcnt(0)\n\tds_write_b32 %32, %33" DENSITY_ROT_OPERANDS(ret, addr, mask, val, tokaddr, tokval));
    }
}

}  // namespace
__global__ __launch_bounds__(kRotThreads) void rotor_selftest_kernel(uint32_t* __restrict__ fail, uint32_t tune) {
    __shared__ __attribute__((aligned(16))) uint32_t cell[64];
    __shared__ __attribute__((aligned(16))) uint32_t syn[kSyBytes / 4];
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t wave = rfl(threadIdx.x >> 6);
    uint32_t bad = 0;
    if (threadIdx.x < 64) cell[threadIdx.x] = 0;
    if (threadIdx.x == 0) { syn[kSyD / 4] = 0; syn[kSyD / 4 + 1] = kNone; }
    __syncthreads();
    const uint32_t c0 = lds_addr(cell), sy = lds_addr(syn);
    if (wave == 0) {
        // (1a) all lanes, one half-dword, two instructions back to back: lane l must get lane l-1's entry
        uint32_t r0, r1, r2, r3;
        const uint32_t e0 = (lane + 1u) << 16, e1 = (lane + 101u) << 16;
        asm volatile("ds_mskor_rtn_b32 %0, %2, %3, %4\n\tds_mskor_rtn_b32 %1, %2, %3, %5\n\ts_waitcnt lgkmcnt(0)"
                     : "=&v"(r0), "=&v"(r1) : "v"(c0), "v"(0xffff0000u), "v"(e0), "v"(e1) : "memory");
        if ((r0 >> 16) != lane) bad |= 1u;
        if ((r1 >> 16) != (lane == 0 ? 64u : lane + 100u)) bad |= 2u;
        // (1b) alternating halves of one dword: even lanes the low half, odd lanes the high half; each half is its own chain
        const uint32_t sh = (lane & 1u) << 4;
        asm volatile("ds_mskor_rtn_b32 %0, %1, %2, %3\n\ts_waitcnt lgkmcnt(0)" : "=&v"(r2) : "v"(c0 + 4u), "v"(0xffffu << sh), "v"((lane + 1u) << sh) : "memory");
        if (((r2 >> sh) & 0xffffu) != (lane < 2 ? 0u : lane - 1u)) bad |= 4u;
        // (1c) mask-0 readers between writers: lanes = 3 (mod 4) write, the others read what the last writer below them left
        const bool wr = (lane & 3u) == 3u;
        asm volatile("ds_mskor_rtn_b32 %0, %1, %2, %3\n\ts_waitcnt lgkmcnt(0)" : "=&v"(r3) : "v"(c0 + 8u), "v"(wr ? 0xffffu : 0u), "v"(wr ? lane + 1u : 0u) : "memory");
        if ((r3 & 0xffffu) != (lane < 4 ? 0u : (lane & ~3u))) bad |= 8u;
        // (3) rollback of (1a)'s second instruction, then of its first: the cell must read 0 again
        uint32_t back;
        dict_store(bperm(63u - lane, c0 + 2u), bperm(63u - lane, r1 >> 16));
        dict_store(bperm(63u - lane, c0 + 2u), bperm(63u - lane, r0 >> 16));
        asm volatile("ds_read_b32 %0, %1\n\ts_waitcnt lgkmcnt(0)" : "=&v"(back) : "v"(c0) : "memory");
        if (back != 0) bad |= 16u;
    }
    __syncthreads();
    // (2) token rotation: round r (wave r % 16) appends to four chains (two dwords x two halves); the value a lane gets back
    // must be the entry of its predecessor in that chain: previous lane of the chain, previous block, previous round
    {
        const uint32_t chain = lane & 3u;                                         // dword (chain >> 1), half (chain & 1)
        const uint32_t a = c0 + 16u + 4u * (chain >> 1), sh = (chain & 1u) << 4;
        uint32_t addr[kR], mask[kR], val[kR], ret[kR];
        constexpr uint32_t kRounds = 192;
        for (uint32_t r = wave; r < kRounds; r += kRotWaves) {
#pragma unroll
            for (uint32_t j = 0; j < kR; ++j) {
                addr[j] = a; mask[j] = 0xffffu << sh;
                val[j] = ((((r * kR + j) * 16u + (lane >> 2)) + 1u) & 0xffffu) << sh;   // position in the chain + 1 (mod 2^16)
            }
            for (uint32_t spins = 0;; ++spins) {
                const uint32_t D = rfl(lds_peek2(sy + kSyD).x);
                if (D == r) break;
                if (D == kPoison) wave_exit();
                if (spins > kSpinLimit) { if (lane == 0) { atomicOr(fail, 64u << 8); lds_poke(sy + kSyD, kPoison); } wave_exit(); }
            }
            exchange_round(ret, addr, mask, val, lane == 0 ? sy + kSyD : sy + kSySink + 4u * lane, r + 1u, (tune & 1u) != 0);
#pragma unroll
            for (uint32_t j = 0; j < kR; ++j) {
                const uint32_t want = ((r * kR + j) * 16u + (lane >> 2)) & 0xffffu;
                if (((ret[j] >> sh) & 0xffffu) != want) bad |= 32u;
            }
        }
    }
    if (bad) atomicOr(fail, bad << 8);                                           // (bits 0..7 belong to container.hip's selftest_kernel)
}

// ---------------------------------------------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------------------------------------------
// DENSITY_HIP_PROF=1: per-wave, per-phase cycle accounting of work-group 0, printed to stderr after every launch (synchronises)
static constexpr size_t kProfWords = 128 + 5 * kProfRounds + 8;
uint64_t* rot_prof_buffer() {
    static uint64_t* buf = nullptr;
    if (!debug_env("DENSITY_HIP_PROF")) return nullptr;
    if (!buf && hipMalloc((void**)&buf, kProfWords * sizeof(uint64_t)) != hipSuccess) buf = nullptr;
    if (buf) { (void)hipDeviceSynchronize(); (void)hipMemset(buf, 0, kProfWords * sizeof(uint64_t)); (void)hipDeviceSynchronize(); }
    return buf;
}
void rot_prof_report(const char* what, const char* phases, uint64_t* buf, hipStream_t stream, uint32_t waves) {
    if (!buf) return;
    static uint64_t h[kProfWords];
    if (hipStreamSynchronize(stream) != hipSuccess || hipMemcpy(h, buf, sizeof(h), hipMemcpyDeviceToHost) != hipSuccess) return;
    if (const char* dump = debug_env("DENSITY_HIP_PROF_DUMP")) {                     // raw buffer, for offline analysis: <prefix>.<encode|decode>.bin
        char path[512];
        snprintf(path, sizeof(path), "%s.%s.bin", dump, what);
        if (FILE* f = fopen(path, "wb")) { fwrite(h, sizeof(uint64_t), kProfWords, f); fclose(f); }
    }
    fprintf(stderr, "[density_hip prof] %s work-group 0, kcycles per wave by phase (%s)\n", what, phases);
    {
        const uint64_t* c = h + 128 + 5 * kProfRounds;
        fprintf(stderr, "[density_hip prof]   events: fast rounds %llu, ordered rounds held %llu (%llu of them ran ahead) / taken back %llu, rounds walked in order %llu, aborts raised %llu\n",
                (unsigned long long)c[0], (unsigned long long)c[1], (unsigned long long)c[5], (unsigned long long)c[2], (unsigned long long)c[3], (unsigned long long)c[4]);
        fprintf(stderr, "[density_hip prof]   memo of predictions: %llu found in the early copy, %llu on a second look\n", (unsigned long long)c[6], (unsigned long long)c[7]);
    }
    for (int w = 0; w < 16; ++w) {
        uint64_t tot = 0;
        for (int k = 0; k < 8; ++k) tot += h[8 * w + k];
        fprintf(stderr, "[density_hip prof]   w%-2d", w);
        for (int k = 0; k < 8; ++k) fprintf(stderr, " %7.1f", (double)h[8 * w + k] / 1e3);
        fprintf(stderr, "  | total %8.1f\n", (double)tot / 1e3);
    }
    // D chain: hop = token seen (round r) - token seen (round r-1); critical = exchanges + token; detect = seen - max(previous token done, own arrival)
    const uint64_t* ts = h + 128;
    uint32_t n = 0, late = 0;
    double hop = 0, crit = 0, det = 0, lateness = 0;
    uint64_t hop_max = 0;
    uint32_t hist[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    for (uint32_t r = 17; r < kProfRounds; ++r) {
        if (!ts[4 * r + 1] || !ts[4 * r + 2] || !ts[4 * (r - 1) + 1] || !ts[4 * (r - 1) + 2]) continue;
        const uint64_t seen = ts[4 * r + 1], prev_seen = ts[4 * (r - 1) + 1], prev_done = ts[4 * (r - 1) + 2], arrive = ts[4 * r];
        if (seen < prev_seen) continue;
        const uint64_t hp = seen - prev_seen;
        hop += (double)hp; crit += (double)(ts[4 * r + 2] - seen);
        hop_max = hp > hop_max ? hp : hop_max;
        const uint64_t ready = arrive > prev_done ? arrive : prev_done;
        det += seen > ready ? (double)(seen - ready) : 0.0;
        if (arrive > prev_done) { ++late; lateness += (double)(arrive - prev_done); }
        uint32_t b = 0; for (uint64_t v = hp / 128; v && b < 7; v >>= 1) ++b;
        ++hist[b];
        ++n;
    }
    if (n) {
        fprintf(stderr, "[density_hip prof]   D chain over %u rounds: hop %.0f (max %llu) cycles = critical section %.0f + detect %.0f; owner arrived late in %u rounds (avg lateness %.0f)\n",
                n, hop / n, (unsigned long long)hop_max, crit / n, det / n, late, late ? lateness / late : 0.0);
        fprintf(stderr, "[density_hip prof]   hop histogram (<128, <256, <512, <1k, <2k, <4k, <8k, more):");
        for (int b = 0; b < 8; ++b) fprintf(stderr, " %u", hist[b]);
        fprintf(stderr, "\n");
        // why owners are late: a wave's own iteration = arrival(r) - exchanges done(r - waves), split by what its previous round was
        const uint64_t* notes = h + 128 + 4 * kProfRounds;
        double it_plain = 0, it_zero = 0, tail_plain = 0, tail_zero = 0;
        uint32_t n_plain = 0, n_zero = 0, late_after_zero = 0, late_total = 0, zero_rounds = 0;
        for (uint32_t r = 17 + waves; r < kProfRounds; ++r) {
            if (!ts[4 * r] || !ts[4 * (r - waves) + 2] || !ts[4 * (r - waves) + 3] || !ts[4 * (r - 1) + 2]) continue;
            const bool z = (notes[r - waves] & 1u) != 0;
            const double it = (double)(ts[4 * r] - ts[4 * (r - waves) + 2]), tail = (double)(ts[4 * (r - waves) + 3] - ts[4 * (r - waves) + 2]);
            if (z) { it_zero += it; tail_zero += tail; ++n_zero; } else { it_plain += it; tail_plain += tail; ++n_plain; }
            if (ts[4 * r] > ts[4 * (r - 1) + 2]) { ++late_total; if (z) ++late_after_zero; }
            if (notes[r] & 1u) ++zero_rounds;
        }
        fprintf(stderr, "[density_hip prof]   a wave between its exchanges and its next arrival: %.0f cycles (%.0f of them up to the end of the round) after a plain round (%u), "
                        "%.0f (%.0f) after a zero-entry round (%u); %u of %u late arrivals follow a zero-entry round; %u zero-entry rounds\n",
                n_plain ? it_plain / n_plain : 0.0, n_plain ? tail_plain / n_plain : 0.0, n_plain, n_zero ? it_zero / n_zero : 0.0, n_zero ? tail_zero / n_zero : 0.0, n_zero,
                late_after_zero, late_total, zero_rounds);
    }
}
// DENSITY_HIP_TUNE (debug build), read once: bit 0 = the self-test passes its token behind the answers
static uint32_t rot_tune() {
    static const uint32_t t = debug_env("DENSITY_HIP_TUNE") ? (uint32_t)atoi(debug_env("DENSITY_HIP_TUNE")) : 0u;
    return t;
}

hipError_t launch_rotor_selftest(uint32_t* d_fail, hipStream_t stream) {
    hipLaunchKernelGGL(rotor_selftest_kernel, dim3(1), dim3(kRotThreads), 0, stream, d_fail, rot_tune());
    return hipGetLastError();
}
hipError_t launch_scan_offsets(const uint64_t* d_sizes, uint32_t first, uint32_t count, uint64_t* d_carry, uint64_t* d_offsets, hipStream_t stream) {
    if (count == 0) return hipSuccess;
    hipLaunchKernelGGL(scan_offsets_kernel, dim3(1), dim3(64), 0, stream, d_sizes, first, count, d_carry, d_offsets);
    return hipGetLastError();
}
hipError_t launch_compact_bytes(const uint8_t* d_src, uint64_t src_stride, const uint64_t* d_sizes, const uint64_t* d_offsets, uint32_t n_chunks,
                                uint8_t* d_dst, hipStream_t stream) {
    if (n_chunks == 0) return hipSuccess;
    hipLaunchKernelGGL(compact_bytes_kernel, dim3(16, n_chunks), dim3(256), 0, stream, d_src, src_stride, d_sizes, d_offsets, d_dst);
    return hipGetLastError();
}

}  // namespace density

// The encoder and the decoder are files of their own, compiled HERE, as part of this translation unit: compiled on their own the encoder
// instances come out with a different register allocation and schedule (the default encoder: 5714 instead of 5712 instructions) although
// no line of them changes — the compiler's choices depend on what else is in the module —, and the measured kernels are the ones of the
// single module.
#include "rotor_encode.hip"
#include "rotor_decode.hip"
