// decode_passes.hip — Cheetah container DECODING in passes (gfx950): everything that is parallel inside a chunk runs as ordered LDS
// exchange passes over the whole chunk, and what is not — one chain of dependent 16-bit look-ups per chunk (decode_walk.hip) — runs alone, in LDS.
//
// The reference decodes a chunk quad by quad through three tables (cheetah.rs:68-103,154-163).  Taken apart:
//
//   records    A stream has no framing: a record's length follows from its signature, raw-copy blocks from the blow-up protection over
//              the lengths before them (codec.rs:88-123, protection_state.rs).  `parse`: one wave per chunk chases the records through
//              an LDS window of the stream (one LDS round trip per record) and leaves every record's position and kind.
//   flags      `prepare`: one lane per quad reads its flag and item (io/read_signature.rs:9-15): PLAIN quads go straight to the output,
//              every quad gets a descriptor {slot, flag}.
//   dictionary chunk_map[h] = {a, b} is touched by the non-predicted quads only, at slots the STREAM names (the hash of a PLAIN quad, the
//              item of a MAP quad): nothing in it depends on a predicted quad.  PLAIN: (a, b) <- (q, a); MAP_A reads a; MAP_B reads b and
//              swaps (cheetah.rs:76-93).  With two cells X, Y per slot and an order bit o (a = o ? Y : X, b = o ? X : Y) this is:
//              PLAIN writes the cell b sits in and toggles o; MAP_B toggles o; MAP_A changes nothing.  So an ordered XOR per slot gives
//              every quad the o it meets, and then X and Y are plain last-writer cells: an ordered exchange per cell (mask 0 = read),
//              exactly what the encoder's stages do (exchange_stages.hip).  `dictionary` (round 6: one kernel, a quarter of the slots per
//              work-group, the taking-part quads of a trip packed into whole blocks first) does both; every MAP quad is then known,
//              without a single dependent look-up.
//   contexts   prediction_map[last_hash] is read by predicted quads and written by the others (:72,81,90,98).  Its SLOT is the hash of the
//              quad before — for a quad behind a predicted one the hash of a value that has to be looked up first: a chain of dependent
//              reads through the data being produced.  This is the only sequential part, and it needs hashes, not quads: H[c] = hash of
//              what follows context c is a table of 64 Ki x 16 bits = 128 KiB of LDS.  `walk`: per chunk a team of four waves takes 128
//              quads a turn — speculative reads of H ahead of the turn, ONE ordered pass over H and its verification under a token
//              (round 6; rounds 3-5: one wave, a dependent LDS round trip per predicted quad) — and leaves every quad's context.
//   values     With the contexts known the prediction table is one more ordered exchange pass: predicted quads read T[c], the others write
//              their quad (`values`); the answers are the predicted quads.
//
// The output buffer itself holds the quads between the passes (PLAIN from `prepare`, MAP from `cells`, predicted from `values`).
// Bit-exact for ANY input: tables start as the reference's zeroed tables and hold full 32-bit quads; a stream the reference would panic
// on (truncated, output too small) raises the error word.  Lion keeps its one-wave decoder: its five-deep prediction rows would need
// 640 KiB of hashes for the walk (lion.rs:29-48), four CUs' worth of LDS.
#include "common.hpp"
#include "kernels.hpp"

#include <cstdlib>
#include <type_traits>

namespace density {

extern __shared__ __attribute__((aligned(16))) uint8_t pass_lds[];
bool g_force_serial_decode = false;   // density_hip_set_kernel_variant(128): Cheetah containers on the one-wave decoder instead
bool g_serial_parse = false;          // density_hip_set_kernel_variant(1024): the records of a chunk found by the one-wave walk alone (no window kernels)

namespace {

constexpr uint32_t kRecBytes = 128, kRecQuads = 32, kSigBytes = 8;        // cheetah.rs:188-196
constexpr uint32_t kRaw = 0x80000000u;                                    // rec[]: the block is a raw copy (codec.rs:89-91)
constexpr uint32_t kFlagPlain = 0, kFlagMapA = 1, kFlagPred = 3;                      // (2: MAP_B)   // cheetah.rs:17-23
// descriptor of a quad: slot [0,16) | flag [16,18) | takes no part (raw block, beyond the end) [19] | a MAP quad that read a never-written 0 [20]
constexpr uint32_t kDescNone = 1u << 19, kDescZero = 1u << 20;   // kDescZero: a MAP quad that read 0 (see the walk)
constexpr uint32_t kErrFormat = 1u, kErrWatchdog = 16u;
constexpr uint32_t kSpinLimit = 1u << 22, kPoison = 0xfffffffeu;

__device__ __forceinline__ uint32_t hash16(uint32_t q) { return (q * kHashMul) >> 16; }
// vec[lane] = val (both wave-uniform scalars): a compare and a select — v_writelane_b32 would want its lane select in M0 (an SGPR value and an SGPR
// lane select together break gfx9's one-scalar-operand rule), and M0 is the compiler's, not an asm statement's, to write
__device__ __forceinline__ uint32_t writelane(uint32_t vec, uint32_t val, uint32_t lane) {
    return lane_id() == lane ? val : vec;
}

// per chunk, left by `parse`: blocks, decoded bytes, quads and raw tail bytes of a ragged last record, where those bytes sit in the stream
struct ChunkInfo { uint32_t blocks, produced, last_quads, tail_bytes, tail_at, bad, ragged, pad1; };   // ragged: the last block is a partial record of last_quads quads + tail_bytes raw bytes

struct PassArgs {
    const uint8_t* in; const uint64_t* offsets; const uint64_t* sizes; uint32_t n_chunks;
    uint8_t* out; uint64_t out_stride, out_total;
    uint32_t* rec; uint32_t* desc; uint16_t* ctx; ChunkInfo* info; uint32_t* err;
};
__device__ __forceinline__ uint64_t chunk_cap(const PassArgs& a, uint64_t chunk) {
    const uint64_t room = a.out_total - chunk * a.out_stride;
    return room < a.out_stride ? room : a.out_stride;
}

// ---------------------------------------------------------------------------------------------------------------
// parse, in parallel (round 4): where the records of a CALM chunk stream start, without walking the stream from its first byte.
// A record's length is in its signature (8 + 128 - 2 per MAP flag - 4 per predicted one: cheetah.rs:17-23), so every even offset p is a candidate
// record start with a known successor, whether or not a record starts there; and as long as never two records in a row are incompressible
// (protection_state.rs:38-47) there are no raw copies and the FSM stays at rest.  The chain of real record starts enters each window of 2 KiB at one
// of 68 even offsets (a record is 8 .. 136 bytes long):
//   head      the one-wave walk below, with the real FSM, over the chunk's first records — a fresh dictionary makes them incompressible, raw copies
//             follow — until the FSM is at rest behind a record that was not incompressible: the windows count from there;
//   windows   per window, a lane per entry: from entry e the chain leaves the window at offset x of the next one after n records (or stops: fewer
//             than 136 bytes are left, the one-wave walk below takes over there), and whether it saw two incompressible records in a row;
//   walk      per chunk, the one-wave walk below with the windows' tables in LDS: wherever it stands at a window's entry with the FSM at rest, the
//             table says no pair lies ahead in this window and the record in front does not make one with its first, the window is taken in one step
//             (its entry and first block number noted); everything else — the windows with raw copies in them, the last records, the ragged end,
//             the checks — record by record as before;
//   emit      per window that was taken in one step, from its entry: rec[] of its blocks.
// (A chunk whose stream the tables have no room for, or that has no calm head, is walked whole.)  SURVEY.md §8: codec/codec.rs:82-126.
// ---------------------------------------------------------------------------------------------------------------
constexpr uint32_t kPW = 2048, kPE = 68, kPStop = 127, kPNone = 255, kHeadMark = 0x5eed0002u, kHeadMaxBlocks = 512;
constexpr uint32_t kPWinLds = kPW + 144;                                  // a window and what a record that starts in it may reach into the next
__device__ __forceinline__ uint32_t record_bytes(const uint8_t* lds_at) {  // item bytes behind the signature at a 2-byte aligned LDS address
    const uint16_t* h = reinterpret_cast<const uint16_t*>(lds_at);
    const uint32_t s0 = (uint32_t)h[0] | ((uint32_t)h[1] << 16), s1 = (uint32_t)h[2] | ((uint32_t)h[3] << 16);
    const uint32_t lo0 = s0 & 0x55555555u, hi0 = (s0 >> 1) & 0x55555555u, lo1 = s1 & 0x55555555u, hi1 = (s1 >> 1) & 0x55555555u;
    return 4u * kRecQuads - 2u * (uint32_t)(__builtin_popcount(lo0 | hi0) + __builtin_popcount(lo1 | hi1)) - 2u * (uint32_t)(__builtin_popcount(lo0 & hi0) + __builtin_popcount(lo1 & hi1));
}
__device__ __forceinline__ void stage_window(uint8_t* win, const uint8_t* src, uint32_t wstart, uint32_t elen, uint32_t tid, uint32_t threads) {
    typedef uint4 uint4_u __attribute__((aligned(1)));
    for (uint32_t v = tid; v < kPWinLds / 16; v += threads) {
        const uint32_t p = wstart + 16u * v;
        uint4 x = make_uint4(0, 0, 0, 0);
        if (p + 16u <= elen) { const uint4_u* sp = reinterpret_cast<const uint4_u*>(src + p); x = make_uint4(sp->x, sp->y, sp->z, sp->w); }
        else if (p < elen) {
            uint8_t t[16] = {};
            for (uint32_t i = 0; i < 16 && p + i < elen; ++i) t[i] = src[p + i];
            x = *reinterpret_cast<const uint4*>(t);
        }
        *reinterpret_cast<uint4*>(win + 16u * v) = x;
    }
    __syncthreads();
}
// T[(chunk * wpc + w) * kPE + e]: exit [0,7) (kPStop: the chain stopped inside the window) | records [7,17) | where it stopped, from the window's start [17,29)
// | first record incompressible [29] | last one [30] | two in a row [31]
__global__ __launch_bounds__(128) void cheetah_parse_windows(PassArgs a, uint32_t wpc, uint32_t* __restrict__ T, uint8_t* __restrict__ went) {
    __shared__ __attribute__((aligned(16))) uint8_t win[kPWinLds];
    const uint32_t e = threadIdx.x, w = blockIdx.x;                           // (two waves: the second one's four lanes take entries 64 .. 67)
    const uint64_t chunk = blockIdx.y;
    if (e == 0) went[chunk * wpc + w] = (uint8_t)kPNone;
    const uint64_t elen64 = a.sizes[chunk];
    if (elen64 >= 0x7fffff00ull) return;
    const ChunkInfo head = a.info[chunk];
    if (head.pad1 != kHeadMark) return;                                       // (no calm head: the one-wave walk takes the whole chunk)
    const uint32_t elen = (uint32_t)elen64;
    const uint64_t wstart64 = (uint64_t)head.produced + (uint64_t)w * kPW;    // windows count from where the head walk stopped
    if (wstart64 >= elen) return;
    const uint32_t wstart = (uint32_t)wstart64;
    const uint32_t hot_end = elen >= kSigBytes + kRecBytes ? elen - (kSigBytes + kRecBytes) + 1u : 0u;   // record starts below this have a whole record's room behind them (codec.rs:88)
    stage_window(win, a.in + a.offsets[chunk], wstart, elen, e, 128);
    if (e >= kPE) return;
    uint32_t pos = 2u * e, cnt = 0, first = 0, last = 0, pair = 0, stop = 0;
    while (pos < kPW) {
        if (wstart + pos >= hot_end) { stop = 1; break; }
        const uint32_t bytes = record_bytes(win + pos);
        const uint32_t inc = kSigBytes + bytes >= kRecBytes ? 1u : 0u;           // codec.rs:98
        if (cnt == 0) first = inc; else pair |= inc & last;
        last = inc; ++cnt;
        pos += kSigBytes + bytes;
    }
    T[(chunk * wpc + w) * kPE + e] = (stop ? kPStop : (pos - kPW) / 2u) | (cnt << 7) | ((stop ? pos : 0u) << 17) | (first << 29) | (last << 30) | (pair << 31);
}
__global__ __launch_bounds__(64) void cheetah_parse_emit(PassArgs a, uint32_t wpc, const uint8_t* __restrict__ went, const uint32_t* __restrict__ wbase) {
    __shared__ __attribute__((aligned(16))) uint8_t win[kPWinLds];
    const uint32_t lane = threadIdx.x, w = blockIdx.x;
    const uint64_t chunk = blockIdx.y;
    const uint32_t entry = went[chunk * wpc + w];
    if (entry == kPNone) return;                                              // (walked record by record, or not at all)
    const uint32_t elen = (uint32_t)a.sizes[chunk], wstart = a.info[chunk].pad1 + w * kPW;   // (pad1: where the chunk's windows count from, left by the walk)
    stage_window(win, a.in + a.offsets[chunk], wstart, elen, lane, 64);
    if (lane != 0) return;
    uint32_t* rec = a.rec + chunk * (a.out_stride / kRecBytes);
    uint32_t b = wbase[chunk * wpc + w], pos = 2u * entry;
    while (pos < kPW) {                                                       // (a window that is taken in one step holds whole records only, and its chain leaves it)
        rec[b++] = wstart + pos;
        pos += kSigBytes + record_bytes(win + pos);
    }
}

// ---------------------------------------------------------------------------------------------------------------
// parse: Codec::decode's walk over the records (codec/codec.rs:82-126) without decoding them
// ---------------------------------------------------------------------------------------------------------------
constexpr uint32_t kWin = 8192, kWinStride = kWin - 64;                   // bytes of stream per LDS window; windows overlap by 64 bytes (a signature + slack)
// mode 0: the whole chunk | 1: from the head on with the windows' tables (the whole chunk where there are none) | 2: the head alone
__global__ __launch_bounds__(64) void cheetah_parse(PassArgs a, uint32_t mode, uint32_t wpc, uint32_t table_lds, const uint32_t* __restrict__ T, uint8_t* __restrict__ went,
                                                    uint32_t* __restrict__ wbase) {
    __shared__ __attribute__((aligned(16))) uint8_t win[2][kWin];
    const uint32_t lane = threadIdx.x;
    const uint64_t chunk = blockIdx.x;
    const uint8_t* src = a.in + a.offsets[chunk];
    const uint64_t elen64 = a.sizes[chunk];
    const uint64_t cap = chunk_cap(a, chunk);
    uint32_t* rec = a.rec + chunk * (a.out_stride / kRecBytes);
    const uint32_t max_blocks = (uint32_t)((cap + kRecBytes - 1) / kRecBytes);
    ChunkInfo ci{};
    if (elen64 >= 0x7fffff00ull) { ci.bad = 1; }                           // 31-bit stream positions (a chunk stream: the launcher bounds it)
    const uint32_t elen = (uint32_t)elen64;
    Guard g;
    uint32_t ip = 0, op = 0, b = 0;
    const uint32_t misalign = (uint32_t)(reinterpret_cast<uintptr_t>(src) & 15u);   // (windows are loaded from 16-byte aligned addresses)
    const uint8_t* base0 = src - misalign;
    const uint32_t have = elen + misalign;                                // bytes from base0 to the stream's end
    // window k = bytes [k * kWinStride, k * kWinStride + kWin) from base0, in win[k & 1]; window k + 1 is in flight (registers) while k is walked
    uint4 pf[kWin / 1024];
    auto fetch = [&](uint32_t k) {
#pragma unroll
        for (uint32_t j = 0; j < kWin / 1024; ++j) {
            const uint32_t i = k * kWinStride + (j * 64u + lane) * 16u;
            pf[j] = i < have ? *reinterpret_cast<const uint4*>(base0 + i) : make_uint4(0, 0, 0, 0);   // (at most 15 bytes past the end, inside its 16-byte line)
        }
    };
    auto land = [&](uint32_t k) {
#pragma unroll
        for (uint32_t j = 0; j < kWin / 1024; ++j) *reinterpret_cast<uint4*>(&win[k & 1u][(j * 64u + lane) * 16u]) = pf[j];
        __syncthreads();
    };
    uint32_t wk = 0;                                                      // the window being walked
    fetch(0); land(0); fetch(1);
    // record positions are collected 64 at a time in a register (lane b % 64) and stored together
    uint32_t recv = 0;
    bool tables = false;
    uint32_t p0 = 0, nwin = 0;
    const uint32_t* Ts = reinterpret_cast<const uint32_t*>(pass_lds);
    if (mode == 1 && !ci.bad) {                                           // the head walk and the window kernels have been over this chunk
        const ChunkInfo head = a.info[chunk];
        if (head.pad1 == kHeadMark && head.produced < elen) {
            p0 = head.produced;
            nwin = (elen - p0 + kPW - 1) / kPW;
            tables = nwin <= wpc && (uint64_t)nwin * kPE * 4 <= table_lds;
        }
        if (tables) {
            uint32_t* Tw = reinterpret_cast<uint32_t*>(pass_lds);
            for (uint32_t i = lane; i < nwin * kPE; i += 64) Tw[i] = T[chunk * wpc * kPE + i];
            __syncthreads();
            b = head.blocks; ip = p0; op = b * kRecBytes;
            g.counter = b;                                                // at rest (no penalty, start 1) behind a record that was not incompressible
            if ((b & 63u) != 0 && lane < (b & 63u)) recv = rec[(b & ~63u) + lane];   // the positions of the group that is being filled
        }
    }
    auto put = [&](uint32_t blk, uint32_t value) {
        recv = writelane(recv, value, blk & 63u);
        if ((blk & 63u) == 63u && (blk & ~63u) + lane < max_blocks) rec[(blk & ~63u) + lane] = recv;   // (never into the next chunk's positions)
    };
    auto window_for = [&](uint32_t pos) {                                  // the window that holds the 12 bytes at stream offset pos
        const uint32_t want = (pos + misalign) / kWinStride;
        if (want != wk) {
            if (want != wk + 1u) fetch(want);                             // (never: a record is far shorter than a window)
            land(want);
            wk = want;
            fetch(want + 1u);
        }
    };
    auto signature_at = [&](uint32_t pos) -> uint64_t {                   // 8 bytes at a 2-byte aligned stream offset, as a scalar
        const uint32_t at = pos + misalign - wk * kWinStride;
        const uint32_t* wd = reinterpret_cast<const uint32_t*>(&win[wk & 1u][at & ~3u]);
        const uint32_t d0 = rfl(wd[0]), d1 = rfl(wd[1]), d2 = rfl(wd[2]);
        return (at & 2u) ? (((uint64_t)((d1 >> 16) | (d2 << 16)) << 32) | ((d0 >> 16) | (d1 << 16))) : (((uint64_t)d1 << 32) | d0);
    };
    const uint32_t full_blocks = (uint32_t)(cap / kRecBytes);             // blocks of 128 decoded bytes the output has room for
    bool head_ok = false;
    while (!ci.bad && ip < elen) {
        if (mode == 2) {                                                  // the head: until the FSM is at rest behind a record that was not incompressible
            if (b >= 2 && g.penalty == 0 && g.start == 1 && g.prev == 0) { head_ok = true; break; }
            if (b >= kHeadMaxBlocks) break;
        }
        if (tables && g.penalty == 0 && g.start == 1 && ip >= p0) {       // at a window's entry with the FSM at rest: the whole window in one step?
            const uint32_t rel = ip - p0, w = rel / kPW, off = rel - w * kPW;
            if (off < 2u * kPE && w < nwin) {
                const uint32_t t = rfl(Ts[w * kPE + off / 2u]), cnt = (t >> 7) & 0x3ffu, ex = t & 127u;
                if (cnt != 0 && ex != kPStop && (t >> 31) == 0 && (g.prev & (t >> 29) & 1u) == 0 && b + cnt <= full_blocks) {
                    if ((b & 63u) != 0 && lane < (b & 63u)) rec[(b & ~63u) + lane] = recv;   // what has been collected of the group so far (`emit` fills in behind it)
                    if (lane == 0) { went[chunk * wpc + w] = (uint8_t)(off / 2u); wbase[chunk * wpc + w] = b; }
                    b += cnt; op += cnt * kRecBytes; g.counter += cnt;
                    ip = p0 + (w + 1u) * kPW + 2u * ex;
                    g.prev = (t >> 30) & 1u;
                    continue;
                }
            }
        }
        window_for(ip);
        if (mode == 0 || (mode == 1 && !tables)) {   // The common case in as few (scalar) instructions as it takes — a lone wave issues one instruction every 4-5 cycles: records that
            // are whole (codec.rs:88: 136 bytes are left), whose signature lies in this window, with the blow-up protection at rest (no
            // penalty, penalty start 1: protection_state.rs:19-27 then only counts) and room in the output.
            const uint32_t wend = (wk + 1u) * kWinStride - misalign;       // stream offsets below this have their 12 bytes in the window
            const uint32_t whole_end = elen >= kSigBytes + kRecBytes ? elen - (kSigBytes + kRecBytes) + 1u : 0u;
            const uint32_t hot_end = wend < whole_end ? wend : whole_end;
            while (ip < hot_end && g.penalty == 0 && g.start == 1 && b < full_blocks) {
                const uint64_t sig = signature_at(ip);
                const uint64_t lo = sig & 0x5555555555555555ull, hi = (sig >> 1) & 0x5555555555555555ull;
                // 4 bytes per PLAIN quad, 2 per MAP quad, none per predicted one (cheetah.rs:17-23): 128 - 2 * (flags with a bit set) - 2 * (flags with both)
                const uint32_t bytes = 4u * kRecQuads - 2u * (uint32_t)__builtin_popcountll(lo | hi) - 2u * (uint32_t)__builtin_popcountll(lo & hi);
                put(b, ip);
                ++b; ip += kSigBytes + bytes; op += kRecBytes;
                ++g.counter;
                const uint32_t inc = kSigBytes + bytes >= kRecBytes ? 1u : 0u;   // codec.rs:98
                if (inc & g.prev) g.penalty = g.start;                    // protection_state.rs:38-47
                g.prev = inc;
            }
            if (ip >= elen) break;
            window_for(ip);
        }
        const uint32_t left = elen - ip;
        const bool fast = left >= kSigBytes + kRecBytes;                  // codec.rs:88: a whole record is certainly there
        if (g.block_is_copy()) {                                         // codec.rs:89-91,103-110
            const uint32_t take = left > kRecBytes ? kRecBytes : left;
            if (b >= max_blocks || (uint64_t)op + take > cap) { ci.bad = 1; break; }
            put(b, ip | kRaw);
            ++b; ip += take; op += take;
            if (!fast && ip == elen) break;                               // :107-109: no decay behind the last raw block
            g.decay();
            continue;
        }
        if (left < kSigBytes) { ci.bad = 1; break; }                      // reference: read_u64_le panics
        const uint64_t sig = signature_at(ip);
        const uint64_t lo = sig & 0x5555555555555555ull, hi = (sig >> 1) & 0x5555555555555555ull;
        if (fast) {
            const uint32_t nplain = kRecQuads - (uint32_t)__builtin_popcountll(lo | hi), npred = (uint32_t)__builtin_popcountll(lo & hi);
            const uint32_t bytes = 4u * nplain + 2u * (kRecQuads - nplain - npred);
            if (b >= max_blocks || (uint64_t)op + kRecBytes > cap) { ci.bad = 1; break; }
            put(b, ip);
            ++b; ip += kSigBytes + bytes; op += kRecBytes;
            g.update(kSigBytes + bytes >= kRecBytes);                     // codec.rs:98
            continue;
        }
        // tail loop (codec.rs:102-123 with cheetah.rs:165-185): lane k looks at quad k of the record
        const uint32_t k = lane & 31u;
        const uint32_t f = (uint32_t)(sig >> (2u * k)) & 3u;
        const uint64_t below = (1ull << (2u * k)) - 1ull;
        const uint32_t pl_b = k - (uint32_t)__builtin_popcountll((lo | hi) & below), pr_b = (uint32_t)__builtin_popcountll(lo & hi & below);
        const uint32_t before = 4u * pl_b + 2u * (k - pl_b - pr_b);       // item bytes in front of mine
        const uint32_t rem = left - kSigBytes;
        const uint32_t mine = f == kFlagPlain ? 4u : f == kFlagPred ? 0u : 2u;
        const bool gone = before > rem;                                   // (cannot be reached without an earlier stop or error)
        const bool stop = !gone && f == kFlagPlain && rem - before < 4u;  // :169-176: implicit PLAIN at the end of the data
        const bool fail = !gone && !stop && rem - before < mine;          // reference: slice panic
        const uint64_t stops = ballot64(lane < 32 && (stop || gone)), fails = ballot64(lane < 32 && fail);
        const uint32_t ks = stops ? (uint32_t)__builtin_ctzll(stops) : 32u;
        if (fails && (uint32_t)__builtin_ctzll(fails) < ks) { ci.bad = 1; break; }
        if (ks < 32u) {
            const uint32_t at_stop = rfl(bperm(ks, before));
            const uint32_t tail = rem - at_stop;                          // 0..3 raw bytes
            if (ks == 0 && tail == 0) { ip = elen; break; }               // a signature with nothing behind it that yields a byte: the reference stops here, having written nothing (:169-170)
            if (b >= max_blocks || (uint64_t)op + 4u * ks + tail > cap) { ci.bad = 1; break; }
            put(b, ip);
            ++b;
            ci.ragged = 1; ci.last_quads = ks; ci.tail_bytes = tail; ci.tail_at = ip + kSigBytes + at_stop;
            op += 4u * ks + tail; ip = elen;
            break;
        }
        // a whole (short) record after all
        const uint32_t nplain = kRecQuads - (uint32_t)__builtin_popcountll(lo | hi), npred = (uint32_t)__builtin_popcountll(lo & hi);
        const uint32_t bytes = 4u * nplain + 2u * (kRecQuads - nplain - npred);
        if (b >= max_blocks || (uint64_t)op + kRecBytes > cap) { ci.bad = 1; break; }
        put(b, ip);
        ++b; ip += kSigBytes + bytes; op += kRecBytes;
        g.update(kSigBytes + bytes >= kRecBytes);
    }
    if ((b & 63u) != 0 && lane < (b & 63u)) rec[(b & ~63u) + lane] = recv;   // the positions not yet stored
    if (mode == 2) {                                                      // (what is wrong with a chunk is the last walk's to say)
        ChunkInfo h{};
        h.blocks = b; h.produced = ip; h.pad1 = head_ok ? kHeadMark : 0u;
        if (lane == 0) a.info[chunk] = h;
        return;
    }
    ci.blocks = b; ci.produced = op; ci.pad1 = p0;
    if (lane == 0) {
        a.info[chunk] = ci;
        if (ci.bad) atomicOr(a.err, kErrFormat);
    }
}

// ---------------------------------------------------------------------------------------------------------------
// prepare: flags and items of every quad (one lane per quad, two records per wave)
// ---------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void cheetah_prepare(PassArgs a, uint32_t blocks_per_chunk) {
    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t pair = (uint64_t)blockIdx.x * 4u + (threadIdx.x >> 6);   // 64 quads = two records
    const uint64_t pairs_per_chunk = blocks_per_chunk / 2;
    const uint64_t chunk = pair / pairs_per_chunk;
    if (chunk >= a.n_chunks) return;
    const uint32_t pb = (uint32_t)(pair % pairs_per_chunk) * 2u + (lane >> 5);   // my record's block in the chunk
    const uint32_t k = lane & 31u;
    const ChunkInfo ci = a.info[chunk];
    const uint64_t step = chunk * (a.out_stride / 4) + (uint64_t)pb * kRecQuads + k;
    uint32_t d = kDescNone;
    if (!ci.bad && pb < ci.blocks) {
        const uint8_t* src = a.in + a.offsets[chunk];
        uint8_t* dst = a.out + chunk * a.out_stride + (uint64_t)pb * kRecBytes;
        const uint32_t r = a.rec[chunk * (a.out_stride / kRecBytes) + pb];
        const bool last = pb + 1 == ci.blocks;
        const uint32_t block_len = last ? ci.produced - pb * kRecBytes : kRecBytes;   // decoded bytes of this block
        if (r & kRaw) {
            const uint8_t* p = src + (r & ~kRaw);
            if (4u * k + 4u <= block_len) st32u(dst + 4u * k, ld32u(p + 4u * k));
            else for (uint32_t i = 4u * k; i < block_len; ++i) dst[i] = p[i];
        } else {
            const uint8_t* p = src + r;
            const uint64_t sig = (uint64_t)ld32u(p) | ((uint64_t)ld32u(p + 4) << 32);
            const uint32_t nq = (last && ci.ragged) ? ci.last_quads : kRecQuads;
            if (k < nq) {
                const uint32_t f = (uint32_t)(sig >> (2u * k)) & 3u;
                const uint64_t lo = sig & 0x5555555555555555ull, hi = (sig >> 1) & 0x5555555555555555ull, below = (1ull << (2u * k)) - 1ull;
                const uint32_t pl_b = k - (uint32_t)__builtin_popcountll((lo | hi) & below), pr_b = (uint32_t)__builtin_popcountll(lo & hi & below);
                const uint8_t* item = p + kSigBytes + 4u * pl_b + 2u * (k - pl_b - pr_b);
                uint32_t slot = 0;
                if (f == kFlagPlain) { const uint32_t q = ld32u(item); slot = hash16(q); *reinterpret_cast<uint32_t*>(dst + 4u * k) = q; }   // cheetah.rs:69-70
                else if (f != kFlagPred) slot = ld16u(item);                                                                           // :79,86
                d = slot | (f << 16);
            }
            if (last && ci.ragged && k < ci.tail_bytes) dst[4u * nq + k] = src[ci.tail_at + k];   // cheetah.rs:171-174
        }
    }
    a.desc[step] = d;
}

// ---------------------------------------------------------------------------------------------------------------
// ordered passes: one table (a part of its slots) per work-group, the quads of the chunk in stream order behind LDS tokens
// ---------------------------------------------------------------------------------------------------------------
constexpr uint32_t kHalfSlots = 32768, kQuarterSlots = 16384, kTable = kHalfSlots * 4, kAhead = 16, kPassWaves = 8;
constexpr uint32_t kOrderBytes = kQuarterSlots / 8;                         // the order bits of a quarter of the slots
constexpr uint32_t kDenseCap = 384;                                         // quads of a trip (of 1024) that the dictionary pass packs into whole blocks: six blocks' worth
constexpr uint32_t kPassBase = kTable + kPassWaves * 64 * 4 + 16 + kOrderBytes;
constexpr uint32_t pass_lds_bytes(int pass) { return kPassBase + (pass == 1 ? kPassWaves * kDenseCap * 8u : 0u); }

#define DENSITY_PASS_X16(OP, ra, m, v, tokaddr, tokval)                                                                            \
    asm volatile(                                                                                                                 \
        OP " %0, %0, %16, %32\n\t" OP " %1, %1, %17, %33\n\t" OP " %2, %2, %18, %34\n\t" OP " %3, %3, %19, %35\n\t"                   \
        OP " %4, %4, %20, %36\n\t" OP " %5, %5, %21, %37\n\t" OP " %6, %6, %22, %38\n\t" OP " %7, %7, %23, %39\n\t"                   \
        OP " %8, %8, %24, %40\n\t" OP " %9, %9, %25, %41\n\t" OP " %10, %10, %26, %42\n\t" OP " %11, %11, %27, %43\n\t"               \
        OP " %12, %12, %28, %44\n\t" OP " %13, %13, %29, %45\n\t" OP " %14, %14, %30, %46\n\t" OP " %15, %15, %31, %47\n\t"           \
        "ds_write_b32 %48, %49\n\t"                                                                                               \
        "s_waitcnt lgkmcnt(0)"                                                                                                    \
        : "+v"(ra[0]), "+v"(ra[1]), "+v"(ra[2]), "+v"(ra[3]), "+v"(ra[4]), "+v"(ra[5]), "+v"(ra[6]), "+v"(ra[7]),                 \
          "+v"(ra[8]), "+v"(ra[9]), "+v"(ra[10]), "+v"(ra[11]), "+v"(ra[12]), "+v"(ra[13]), "+v"(ra[14]), "+v"(ra[15])            \
        : "v"(m[0]), "v"(m[1]), "v"(m[2]), "v"(m[3]), "v"(m[4]), "v"(m[5]), "v"(m[6]), "v"(m[7]),                                 \
          "v"(m[8]), "v"(m[9]), "v"(m[10]), "v"(m[11]), "v"(m[12]), "v"(m[13]), "v"(m[14]), "v"(m[15]),                           \
          "v"(v[0]), "v"(v[1]), "v"(v[2]), "v"(v[3]), "v"(v[4]), "v"(v[5]), "v"(v[6]), "v"(v[7]),                                 \
          "v"(v[8]), "v"(v[9]), "v"(v[10]), "v"(v[11]), "v"(v[12]), "v"(v[13]), "v"(v[14]), "v"(v[15]),                           \
          "v"(tokaddr), "v"(tokval)                                                                                               \
        : "memory")
// (the XOR form takes no mask: ds_xor_rtn_b32 vdst, addr, data)
#define DENSITY_PASS_XOR16(ra, v, tokaddr, tokval)                                                                                 \
    asm volatile(                                                                                                                 \
        "ds_xor_rtn_b32 %0, %0, %16\n\t" "ds_xor_rtn_b32 %1, %1, %17\n\t" "ds_xor_rtn_b32 %2, %2, %18\n\t" "ds_xor_rtn_b32 %3, %3, %19\n\t"         \
        "ds_xor_rtn_b32 %4, %4, %20\n\t" "ds_xor_rtn_b32 %5, %5, %21\n\t" "ds_xor_rtn_b32 %6, %6, %22\n\t" "ds_xor_rtn_b32 %7, %7, %23\n\t"         \
        "ds_xor_rtn_b32 %8, %8, %24\n\t" "ds_xor_rtn_b32 %9, %9, %25\n\t" "ds_xor_rtn_b32 %10, %10, %26\n\t" "ds_xor_rtn_b32 %11, %11, %27\n\t"     \
        "ds_xor_rtn_b32 %12, %12, %28\n\t" "ds_xor_rtn_b32 %13, %13, %29\n\t" "ds_xor_rtn_b32 %14, %14, %30\n\t" "ds_xor_rtn_b32 %15, %15, %31\n\t" \
        "ds_write_b32 %32, %33\n\t"                                                                                               \
        "s_waitcnt lgkmcnt(0)"                                                                                                    \
        : "+v"(ra[0]), "+v"(ra[1]), "+v"(ra[2]), "+v"(ra[3]), "+v"(ra[4]), "+v"(ra[5]), "+v"(ra[6]), "+v"(ra[7]),                 \
          "+v"(ra[8]), "+v"(ra[9]), "+v"(ra[10]), "+v"(ra[11]), "+v"(ra[12]), "+v"(ra[13]), "+v"(ra[14]), "+v"(ra[15])            \
        : "v"(v[0]), "v"(v[1]), "v"(v[2]), "v"(v[3]), "v"(v[4]), "v"(v[5]), "v"(v[6]), "v"(v[7]),                                 \
          "v"(v[8]), "v"(v[9]), "v"(v[10]), "v"(v[11]), "v"(v[12]), "v"(v[13]), "v"(v[14]), "v"(v[15]),                           \
          "v"(tokaddr), "v"(tokval)                                                                                               \
        : "memory")

// K ordered operations and the token behind them in ONE statement (the dense form of the dictionary pass: K = 3 or 6 whole blocks per trip)
template <uint32_t K>
__device__ __forceinline__ void lds_xor_token(uint32_t (&ra)[K], const uint32_t (&x)[K], uint32_t tokaddr, uint32_t tokval) {
    static_assert(K == 3 || K == 6, "three or six blocks");
    if constexpr (K == 3)
        asm volatile("ds_xor_rtn_b32 %0, %0, %3\n\tds_xor_rtn_b32 %1, %1, %4\n\tds_xor_rtn_b32 %2, %2, %5\n\tds_write_b32 %6, %7\n\ts_waitcnt lgkmcnt(0)"
                     : "+v"(ra[0]), "+v"(ra[1]), "+v"(ra[2]) : "v"(x[0]), "v"(x[1]), "v"(x[2]), "v"(tokaddr), "v"(tokval) : "memory");
    else
        asm volatile("ds_xor_rtn_b32 %0, %0, %6\n\tds_xor_rtn_b32 %1, %1, %7\n\tds_xor_rtn_b32 %2, %2, %8\n\tds_xor_rtn_b32 %3, %3, %9\n\tds_xor_rtn_b32 %4, %4, %10\n\tds_xor_rtn_b32 %5, %5, %11\n\t"
                     "ds_write_b32 %12, %13\n\ts_waitcnt lgkmcnt(0)"
                     : "+v"(ra[0]), "+v"(ra[1]), "+v"(ra[2]), "+v"(ra[3]), "+v"(ra[4]), "+v"(ra[5])
                     : "v"(x[0]), "v"(x[1]), "v"(x[2]), "v"(x[3]), "v"(x[4]), "v"(x[5]), "v"(tokaddr), "v"(tokval) : "memory");
}
template <uint32_t K>
__device__ __forceinline__ void lds_mskor_token(uint32_t (&ra)[K], const uint32_t (&mk)[K], const uint32_t (&vl)[K], uint32_t tokaddr, uint32_t tokval) {
    static_assert(K == 3 || K == 6, "three or six blocks");
    if constexpr (K == 3)
        asm volatile("ds_mskor_rtn_b32 %0, %0, %3, %6\n\tds_mskor_rtn_b32 %1, %1, %4, %7\n\tds_mskor_rtn_b32 %2, %2, %5, %8\n\tds_write_b32 %9, %10\n\ts_waitcnt lgkmcnt(0)"
                     : "+v"(ra[0]), "+v"(ra[1]), "+v"(ra[2])
                     : "v"(mk[0]), "v"(mk[1]), "v"(mk[2]), "v"(vl[0]), "v"(vl[1]), "v"(vl[2]), "v"(tokaddr), "v"(tokval) : "memory");
    else
        asm volatile("ds_mskor_rtn_b32 %0, %0, %6, %12\n\tds_mskor_rtn_b32 %1, %1, %7, %13\n\tds_mskor_rtn_b32 %2, %2, %8, %14\n\tds_mskor_rtn_b32 %3, %3, %9, %15\n\t"
                     "ds_mskor_rtn_b32 %4, %4, %10, %16\n\tds_mskor_rtn_b32 %5, %5, %11, %17\n\tds_write_b32 %18, %19\n\ts_waitcnt lgkmcnt(0)"
                     : "+v"(ra[0]), "+v"(ra[1]), "+v"(ra[2]), "+v"(ra[3]), "+v"(ra[4]), "+v"(ra[5])
                     : "v"(mk[0]), "v"(mk[1]), "v"(mk[2]), "v"(mk[3]), "v"(mk[4]), "v"(mk[5]), "v"(vl[0]), "v"(vl[1]), "v"(vl[2]), "v"(vl[3]), "v"(vl[4]), "v"(vl[5]),
                       "v"(tokaddr), "v"(tokval) : "memory");
}

// PASS 1 `dictionary` (round 6: `order` and `cells` in one kernel): a work-group owns a QUARTER of the slots, both cells X, Y of each (16 Ki x 2 dwords) and
//        their order bits (16 Ki bits).  Per trip two ordered groups of LDS operations, each behind a token of its own:
//        A  an ordered XOR on the slot's order bit — PLAIN and MAP_B toggle it, MAP_A reads it (cheetah.rs:71-72,87-89); what comes back is the o the quad meets;
//        B  an ordered exchange on the cell the quad touches — a sits in cell o, b in cell 1 - o: PLAIN writes its quad to b's cell, MAP_A / MAP_B read a's / b's.
//        (Up to round 5 two kernels: `order` — two work-groups per chunk on dword-wide order bits, o written back into the descriptors — and `cells` — four
//        per chunk, (cell, half of the slots) — every one of them streaming the chunk's descriptors: 0.17 + 0.42 ms per 100 MB.)
// PASS 2 `values`: slot = the quad's context (a half of them per work-group); predicted quads read, the others write their quad (cheetah.rs:72,81,90,98)
// The 8 waves take the trips of 16 blocks of 64 quads in rotation (exchange_stages.hip); a wave asks for its NEXT trip's descriptors, quads and contexts
// before it waits for its turn (round 6: until then a trip began with its loads, and a wave's iteration was two memory round trips long — 2,600 cycles per
// trip and work-group where the exchanges and the hand-off take 700).
template <int PASS>
__global__ __launch_bounds__(kPassWaves * 64) void cheetah_pass(PassArgs a) {
    static_assert(PASS == 1 || PASS == 2, "dictionary or values");
    constexpr uint32_t W = kPassWaves;
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t wave = rfl(threadIdx.x >> 6);
    constexpr uint32_t parts = PASS == 1 ? 4u : 2u;
    const uint64_t chunk = blockIdx.x / parts;
    const uint32_t mypart = blockIdx.x % parts;
    const ChunkInfo ci = a.info[chunk];
    if (ci.bad) return;
    const uint32_t nsteps = ci.blocks * kRecQuads;                                 // (quads of a ragged last record beyond its end carry kDescNone)
    const uint32_t trips = (nsteps + kAhead * 64u - 1u) / (kAhead * 64u);
    const uint64_t s0 = chunk * (a.out_stride / 4);
    uint32_t* w = reinterpret_cast<uint32_t*>(pass_lds);
    for (uint32_t k = threadIdx.x; k < kPassBase / 4u; k += W * 64u) w[k] = 0u;   // the reference's zeroed tables; sinks; the tokens; the order bits
    __syncthreads();
    uint32_t* __restrict__ desc = a.desc + s0;
    const uint16_t* __restrict__ ctx = a.ctx + s0;
    uint32_t* __restrict__ val = reinterpret_cast<uint32_t*>(a.out + chunk * a.out_stride);
    const uint32_t lds0 = lds_addr(pass_lds);
    const uint32_t sink = lds0 + kTable + threadIdx.x * 4u;
    const uint32_t token_a = lds0 + kTable + W * 256u, token_b = token_a + 4u;
    const uint32_t obits = token_a + 16u;
    const uint64_t cap = chunk_cap(a, chunk);
    const uint32_t limit = (uint32_t)((cap + 3) / 4), whole = (uint32_t)(cap / 4);   // dwords of this chunk's output that exist / that exist whole
    uint32_t nd[kAhead], nv[kAhead], nk[kAhead];
    auto fetch = [&](uint32_t t) {
#pragma unroll
        for (uint32_t j = 0; j < kAhead; ++j) {
            const uint32_t i = (t * kAhead + j) * 64u + lane;
            nd[j] = i < nsteps ? desc[i] : kDescNone;
            nv[j] = i < whole ? val[i] : 0u;                                       // (a writer's quad, left there by `prepare` / `cells`; anything for the others)
            nk[j] = (PASS == 2 && i < nsteps) ? ctx[i] : 0u;
        }
    };
    // my turn on a token: every earlier trip's operations of that group are queued
    auto await = [&](uint32_t token, uint32_t t) -> bool {
        for (uint32_t spins = 0;; ++spins) {
            uint32_t seen;
            asm volatile("ds_read_b32 %0, %1\n\ts_waitcnt lgkmcnt(0)" : "=v"(seen) : "v"(token) : "memory");
            seen = rfl(seen);
            if (seen == t) return true;
            if (seen == kPoison || spins > kSpinLimit) {
                if (seen != kPoison && lane == 0) { atomicOr(a.err, kErrWatchdog); w[(token_a - lds0) / 4u] = kPoison; w[(token_b - lds0) / 4u] = kPoison; }
                return false;
            }
        }
    };
    if (wave < trips) fetch(wave);
    // The dictionary pass in DENSE form (round 6): a quarter of the slots means one lane in six takes part in a block's operations, and an ordered LDS
    // instruction costs its 23+ cycles whatever its exec mask.  So a wave packs the taking-part quads of its trip, in stream order, into whole blocks first —
    // {slot | flag | place in the trip, quad} through a staging area of its own in LDS (ballot, count of the lanes below, one 8-byte write per block; a wave's LDS
    // operations execute in order: no barrier) — and both ordered groups run on 3 (up to 192 quads) or 6 (up to 384) blocks instead of 16; a trip with more
    // (one slot over and over) keeps the sixteen-block form below.  Results go back to the quads' places by the place each entry carries.
    auto dense_trip = [&](auto kc, uint32_t t, uint32_t cnt, uint32_t stg) -> bool {
        constexpr uint32_t K = decltype(kc)::value, kOff = 1u << 31;
        uint32_t lo[K], ra[K], x[K], m[K], v[K];
#pragma unroll
        for (uint32_t b = 0; b < K; ++b) {
            uint64_t e;
            asm volatile("ds_read_b64 %0, %1\n\ts_waitcnt lgkmcnt(0)" : "=v"(e) : "v"(stg + (b * 64u + lane) * 8u) : "memory");
            const bool on = b * 64u + lane < cnt;
            lo[b] = on ? (uint32_t)e : kOff;                                  // (an entry's low word: slot [0,16) | flag [16,18) | place in the trip [18,28))
            v[b] = (uint32_t)(e >> 32);
            const uint32_t sq = lo[b] & (kQuarterSlots - 1u), f = (lo[b] >> 16) & 3u;
            ra[b] = on ? obits + (sq >> 5) * 4u : sink;
            x[b] = (on && f != kFlagMapA) ? 1u << (sq & 31u) : 0u;                 // toggles
        }
#pragma unroll
        for (uint32_t b = 0; b < K; ++b) asm volatile("" : "+v"(ra[b]), "+v"(x[b]));   // (made ahead of the wait, not behind it)
        if (!await(token_a, t)) return false;
        const uint32_t tokval = t + 1u;
        lds_xor_token<K>(ra, x, lane == 0 ? token_a : sink, tokval);
#pragma unroll
        for (uint32_t b = 0; b < K; ++b) {
            const bool on = !(lo[b] & kOff);
            const uint32_t sq = lo[b] & (kQuarterSlots - 1u), f = (lo[b] >> 16) & 3u, o = (ra[b] >> (sq & 31u)) & 1u;
            const uint32_t mycell = f == kFlagMapA ? o : 1u - o;
            const bool write = f == kFlagPlain;
            ra[b] = on ? lds0 + ((sq * 2u + mycell) * 4u) : sink;
            m[b] = (on && write) ? 0xffffffffu : 0u;
            v[b] = (on && write) ? v[b] : 0u;
        }
#pragma unroll
        for (uint32_t b = 0; b < K; ++b) asm volatile("" : "+v"(ra[b]), "+v"(m[b]), "+v"(v[b]));
        if (!await(token_b, t)) return false;
        lds_mskor_token<K>(ra, m, v, lane == 0 ? token_b : sink, tokval);
#pragma unroll
        for (uint32_t b = 0; b < K; ++b) {
            const bool rd = !(lo[b] & kOff) && ((lo[b] >> 16) & 3u) != kFlagPlain;
            const uint32_t i = t * (kAhead * 64u) + ((lo[b] >> 18) & 1023u);
            if (rd && i < limit) {
                val[i] = ra[b];
                if (ra[b] == 0u) desc[i] = (lo[b] & 0x3ffffu) | kDescZero;           // (see below)
            }
        }
        return true;
    };
    const uint32_t stage0 = lds0 + kPassBase + wave * (kDenseCap * 8u);
    // the sixteen-block form of a trip, from descriptors / quads / contexts in registers (the values pass; the dictionary pass's trips that do not pack)
    auto wide_trip = [&](uint32_t t, const uint32_t (&xd)[kAhead], const uint32_t (&xv)[kAhead], const uint32_t (&xk)[kAhead], bool fetch_next) -> bool {
        uint32_t ra[kAhead], m[kAhead], v[kAhead];
        uint32_t dd[kAhead], sh[kAhead];
        uint32_t minebits = 0, rdbits = 0;                                         // per lane, bit j: block j's quad is this work-group's / reads (in a vector register: 32 lane masks spill the scalar file)
#pragma unroll
        for (uint32_t j = 0; j < kAhead; ++j) {
            const uint32_t d = xd[j];
            dd[j] = d;
            const uint32_t f = (d >> 16) & 3u;
            const bool none = (d & kDescNone) != 0;
            if (PASS == 1) {
                const uint32_t key = d & 0xffffu, sq = key & (kQuarterSlots - 1u);
                const bool mine = !none && f != kFlagPred && (key >> 14) == mypart;
                minebits |= (mine ? 1u : 0u) << j;
                sh[j] = sq & 31u;
                ra[j] = mine ? obits + (sq >> 5) * 4u : sink;
                m[j] = (mine && f != kFlagMapA) ? 1u << sh[j] : 0u;                // toggles
                v[j] = xv[j];
            } else {
                const uint32_t key = xk[j];
                const bool write = f != kFlagPred;
                const bool mine = !none && (key >> 15) == mypart;
                ra[j] = mine ? lds0 + (key & (kHalfSlots - 1u)) * 4u : sink;
                m[j] = (mine && write) ? 0xffffffffu : 0u;
                v[j] = (mine && write) ? xv[j] : 0u;
                rdbits |= ((mine && !write) ? 1u : 0u) << j;
            }
        }
        if (fetch_next && t + W < trips) fetch(t + W);                             // in flight across the waits below
        // (the operands are made HERE, ahead of the wait: left to itself the compiler sinks their 230 instructions behind the poll loop — into the critical
        // section, where every later trip of the work-group waits for them)
#pragma unroll
        for (uint32_t j = 0; j < kAhead; ++j) asm volatile("" : "+v"(ra[j]), "+v"(m[j]), "+v"(v[j]));
        if (!await(token_a, t)) return false;
        if (PASS == 1) {
            const uint32_t tokaddr = lane == 0 ? token_a : sink, tokval = t + 1u;
            DENSITY_PASS_XOR16(ra, m, tokaddr, tokval);
#pragma unroll
            for (uint32_t j = 0; j < kAhead; ++j) {
                const uint32_t f = (dd[j] >> 16) & 3u, o = (ra[j] >> sh[j]) & 1u;
                // a sits in cell o, b in cell 1 - o (X = 0, Y = 1): PLAIN writes b's cell, MAP_A reads a's, MAP_B reads b's
                const uint32_t mycell = f == kFlagMapA ? o : 1u - o;
                const bool write = f == kFlagPlain, mine = (minebits >> j) & 1u;
                ra[j] = mine ? lds0 + (((dd[j] & (kQuarterSlots - 1u)) * 2u + mycell) * 4u) : sink;
                m[j] = (mine && write) ? 0xffffffffu : 0u;
                v[j] = (mine && write) ? v[j] : 0u;
                rdbits |= ((mine && !write) ? 1u : 0u) << j;
            }
#pragma unroll
            for (uint32_t j = 0; j < kAhead; ++j) asm volatile("" : "+v"(ra[j]), "+v"(m[j]), "+v"(v[j]));
            if (!await(token_b, t)) return false;
            const uint32_t tokaddr_b = lane == 0 ? token_b : sink;
            DENSITY_PASS_X16("ds_mskor_rtn_b32", ra, m, v, tokaddr_b, tokval);
        } else {
            const uint32_t tokaddr = lane == 0 ? token_a : sink, tokval = t + 1u;
            DENSITY_PASS_X16("ds_mskor_rtn_b32", ra, m, v, tokaddr, tokval);
        }
#pragma unroll
        for (uint32_t j = 0; j < kAhead; ++j) {
            const uint32_t i = (t * kAhead + j) * 64u + lane;
            if (((rdbits >> j) & 1u) && i < limit) {
                val[i] = ra[j];                                                    // cheetah.rs:80,87 / :96: the quad
                // A MAP quad's NEXT context is its item (cheetah.rs:78-83,85-92: the hash returned is the one read from the stream), but what a
                // later predicted quad in ITS context hashes to is the hash of the VALUE (:97-102).  The two agree whenever the cell holds a quad
                // some PLAIN quad put there — its slot is its hash — and differ only for a cell nothing has written yet: 0, whose hash is 0.  No
                // encoder produces that (a MAP of a never-written slot), a corrupt stream can: the walk needs to know (never taken otherwise).
                if (PASS == 1 && ra[j] == 0u) desc[i] = dd[j] | kDescZero;
            }
        }
        return true;
    };
    if (PASS == 2) {
        for (uint32_t t = wave; t < trips; t += W)
            if (!wide_trip(t, nd, nv, nk, true)) break;
        return;
    }
    // the dictionary pass: trip t packed in the staging area, trip t + W's descriptors and quads in flight in registers
    auto pack = [&]() -> uint32_t {
        uint32_t cnt = 0;
#pragma unroll
        for (uint32_t j = 0; j < kAhead; ++j) {
            const uint32_t d = nd[j], f = (d >> 16) & 3u;
            const bool mine = !(d & kDescNone) && f != kFlagPred && ((d & 0xffffu) >> 14) == mypart;
            const uint64_t bm = ballot64(mine);
            const uint32_t pos = cnt + mbcnt64(bm);
            if (mine && pos < kDenseCap) {
                const uint64_t e = (uint64_t)((d & 0x3ffffu) | ((j * 64u + lane) << 18)) | ((uint64_t)nv[j] << 32);
                asm volatile("ds_write_b64 %0, %1" ::"v"(stage0 + pos * 8u), "v"(e) : "memory");
            }
            cnt += (uint32_t)__builtin_popcountll(bm);
        }
        return cnt;
    };
    uint32_t cnt = 0;
    if (wave < trips) { cnt = pack(); if (wave + W < trips) fetch(wave + W); }
    for (uint32_t t = wave; t < trips; t += W) {
        bool ok;
        if (cnt <= 192u) ok = dense_trip(std::integral_constant<uint32_t, 3>{}, t, cnt, stage0);
        else if (cnt <= kDenseCap) ok = dense_trip(std::integral_constant<uint32_t, 6>{}, t, cnt, stage0);
        else {                                                                     // (rare: the trip's own descriptors and quads again, nothing in flight for it)
            uint32_t fd[kAhead], fv[kAhead], fk[kAhead];
#pragma unroll
            for (uint32_t j = 0; j < kAhead; ++j) {
                const uint32_t i = (t * kAhead + j) * 64u + lane;
                fd[j] = i < nsteps ? desc[i] : kDescNone;
                fv[j] = i < whole ? val[i] : 0u;
                fk[j] = 0u;
            }
            ok = wide_trip(t, fd, fv, fk, false);
        }
        if (!ok) break;
        if (t + W < trips) { cnt = pack(); if (t + 2u * W < trips) fetch(t + 2u * W); }
    }
}

}  // namespace
}  // namespace density

// The walk is a file of its own, compiled HERE, as part of this translation unit (what it needs of the above it names as it stands; a unit of its
// own would be free to allocate the passes' and the walk's registers differently: see rotor.hip on its kernel files).
#include "decode_walk.hip"

namespace density {

// ---------------------------------------------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------------------------------------------
// scratch: rec (a dword per 128-byte block) | desc (a dword per quad) | ctx (16 bits per quad) | chunk info
uint64_t decode_pass_scratch_bytes(uint64_t out_stride, uint32_t n_chunks) {
    const uint64_t span = (uint64_t)n_chunks * out_stride;                         // (arrays are indexed chunk * stride + ...)
    return ((span / kRecBytes * 4 + 255) & ~255ull) + ((span + 255) & ~255ull) + ((span / 2 + 255) & ~255ull) + (((uint64_t)n_chunks * sizeof(ChunkInfo) + 255) & ~255ull) + 256;
}
bool decode_pass_eligible(int algo, const uint8_t* d_in, const uint8_t* d_out, uint32_t n_chunks, uint64_t out_stride, uint64_t out_total) {
    if (algo != DENSITY_HIP_CHEETAH || g_force_serial_decode || g_force_lane_codec || g_force_wave_codec || g_rotor_unsafe) return false;
    if (n_chunks == 0 || (uintptr_t)d_out % 4 != 0) return false;
    // the head walk reads a signature as whole 16-bit halves of its window (signature_at: stream positions are even, and so must be the
    // window's `misalign`); chunk payloads start at 16-byte offsets from d_in, so an odd d_in is the one-wave decoder's
    if ((uintptr_t)d_in % 2 != 0) return false;
    // one chunk (a stream): the output capacity is the stride; chunks: whole pairs of records
    if (n_chunks > 1 && out_stride % 256 != 0) return false;
    // Where the passes win: from 64 KiB chunks on (measured, 100 MB of prose, decode ms passes / one wave per stream: 64 KiB 3.2 / 3.6,
    // 128 KiB 3.3 / 4.2, 256 KiB 4.4 / 6.2, 512 KiB 5.2 / 10.5, 1 MiB 9.8 / 20.2); shorter chunks have less to parse than the passes have to
    // set up.  DENSITY_HIP_PASS_MIN (bytes; tuning runs) moves the threshold.
    static const uint64_t min_chunk = debug_env("DENSITY_HIP_PASS_MIN") ? (uint64_t)atoll(debug_env("DENSITY_HIP_PASS_MIN")) : 64ull * 1024;
    const uint64_t per_chunk = n_chunks == 1 ? out_total : out_stride;
    return per_chunk >= min_chunk && per_chunk >= 65536 && per_chunk < (1ull << 31);
}
hipError_t launch_decode_passes(int algo, const uint8_t* d_in, const uint64_t* d_offsets, const uint64_t* d_sizes, uint32_t n_chunks, uint8_t* d_out,
                                uint64_t out_stride, uint64_t out_total, bool exact, uint64_t* d_produced, uint32_t* d_err, uint8_t* d_scratch,
                                hipStream_t stream);

namespace {
__global__ __launch_bounds__(256) void cheetah_finish(PassArgs a, uint32_t exact, uint64_t* __restrict__ produced) {
    const uint32_t chunk = blockIdx.x * 256u + threadIdx.x;
    if (chunk >= a.n_chunks) return;
    const ChunkInfo ci = a.info[chunk];
    produced[chunk] = ci.bad ? 0 : ci.produced;
    if (!ci.bad && exact && ci.produced != chunk_cap(a, chunk)) atomicOr(a.err, kErrFormat);
}
}  // namespace

hipError_t launch_decode_passes(int algo, const uint8_t* d_in, const uint64_t* d_offsets, const uint64_t* d_sizes, uint32_t n_chunks, uint8_t* d_out,
                                uint64_t out_stride, uint64_t out_total, bool exact, uint64_t* d_produced, uint32_t* d_err, uint8_t* d_scratch,
                                hipStream_t stream) {
    (void)algo;
    if (n_chunks == 1) out_stride = (out_total + 255) & ~255ull;                    // a single stream: its chunk is the whole output
    PassArgs a{};
    a.in = d_in; a.offsets = d_offsets; a.sizes = d_sizes; a.n_chunks = n_chunks; a.out = d_out; a.out_stride = out_stride; a.out_total = out_total;
    const uint64_t span = (uint64_t)n_chunks * out_stride;
    uint8_t* p = d_scratch;
    a.rec = reinterpret_cast<uint32_t*>(p); p += (span / kRecBytes * 4 + 255) & ~255ull;
    a.desc = reinterpret_cast<uint32_t*>(p); p += (span + 255) & ~255ull;
    a.ctx = reinterpret_cast<uint16_t*>(p); p += (span / 2 + 255) & ~255ull;
    a.info = reinterpret_cast<ChunkInfo*>(p);
    a.err = d_err;
    const uint32_t blocks_per_chunk = (uint32_t)(out_stride / kRecBytes);
    hipError_t e = hipFuncSetAttribute((const void*)cheetah_pass<1>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)pass_lds_bytes(1));
    if (e == hipSuccess) e = hipFuncSetAttribute((const void*)cheetah_pass<2>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)pass_lds_bytes(2));
    if (e == hipSuccess) e = hipFuncSetAttribute((const void*)cheetah_walk_team, hipFuncAttributeMaxDynamicSharedMemorySize, (int)kTeamLds);
    if (e != hipSuccess) return e;
    // the records of calm stretches are found by the window kernels (their tables live where the descriptors and contexts will: nothing else is in use yet)
    const uint64_t slot_bound = out_stride + out_stride / kRecBytes * kSigBytes + kSigBytes;
    const uint32_t wpc = (uint32_t)((slot_bound + kPW - 1) / kPW);
    // (the window kernels put the chunk on the grid's y axis: at most 65535 chunks — 4 GiB and more in 64 KiB chunks take the one-wave parse)
    const bool windows = !g_serial_parse && n_chunks <= 65535u && out_stride >= (64u << 10) && (uint64_t)wpc * kPE * 4 <= out_stride && (uint64_t)wpc * 8 <= out_stride / 2;
    if (windows) {
        uint32_t* T = a.desc;
        uint32_t* wbase = reinterpret_cast<uint32_t*>(a.ctx);
        uint8_t* went = reinterpret_cast<uint8_t*>(wbase + (uint64_t)n_chunks * wpc);
        const uint32_t table_lds = (uint32_t)std::min<uint64_t>((uint64_t)wpc * kPE * 4, 140u * 1024);   // (+ the walk's own 16 KiB of stream windows)
        e = hipFuncSetAttribute((const void*)cheetah_parse, hipFuncAttributeMaxDynamicSharedMemorySize, (int)table_lds);
        if (e != hipSuccess) return e;
        hipLaunchKernelGGL(cheetah_parse, dim3(n_chunks), dim3(64), 0, stream, a, 2u, 0u, 0u, (const uint32_t*)nullptr, (uint8_t*)nullptr, (uint32_t*)nullptr);
        hipLaunchKernelGGL(cheetah_parse_windows, dim3(wpc, n_chunks), dim3(128), 0, stream, a, wpc, T, went);
        if ((e = hipGetLastError()) != hipSuccess) return e;                      // (the walk below reads what these kernels wrote)
        hipLaunchKernelGGL(cheetah_parse, dim3(n_chunks), dim3(64), table_lds, stream, a, 1u, wpc, table_lds, (const uint32_t*)T, went, wbase);
        hipLaunchKernelGGL(cheetah_parse_emit, dim3(wpc, n_chunks), dim3(64), 0, stream, a, wpc, (const uint8_t*)went, (const uint32_t*)wbase);
    } else {
        hipLaunchKernelGGL(cheetah_parse, dim3(n_chunks), dim3(64), 0, stream, a, 0u, 0u, 0u, (const uint32_t*)nullptr, (uint8_t*)nullptr, (uint32_t*)nullptr);
    }
    const uint64_t pairs = (uint64_t)n_chunks * (blocks_per_chunk / 2);
    hipLaunchKernelGGL(cheetah_prepare, dim3((uint32_t)((pairs + 3) / 4)), dim3(256), 0, stream, a, blocks_per_chunk);
    hipLaunchKernelGGL(cheetah_pass<1>, dim3(4 * n_chunks), dim3(kPassWaves * 64), pass_lds_bytes(1), stream, a);
    hipLaunchKernelGGL(cheetah_walk_team, dim3(n_chunks), dim3(kTeam * 64), kTeamLds, stream, a);
    hipLaunchKernelGGL(cheetah_pass<2>, dim3(2 * n_chunks), dim3(kPassWaves * 64), pass_lds_bytes(2), stream, a);
    hipLaunchKernelGGL(cheetah_finish, dim3((n_chunks + 255) / 256), dim3(256), 0, stream, a, exact ? 1u : 0u, d_produced);
    return hipGetLastError();
}

}  // namespace density
