// rotor_decode.hip — the Chameleon wave-rotation DECODER for gfx950, index-fed (design notes: rotor.hip; shared device code:
// rotor_dev.hpp), and its launchers.
#include <cstdio>

#include "rotor_dev.hpp"

namespace density {

// ---------------------------------------------------------------------------------------------------------------
// decode (index-fed): Codec::decode (codec/codec.rs:82-126), Chameleon::decode_plain / decode_map (chameleon.rs:56-68)
// ---------------------------------------------------------------------------------------------------------------
// The raw-copy bits of a chunk's block index against the blow-up protection (protection_state.rs:19-47, codec.rs:89-91), WITHOUT walking
// the FSM over the chunk: called for block i only where it is raw or incompressible (a coded record of 256 bytes or more: at most 4 MAP
// flags), it checks what the FSM implies locally —
//   * a run of raw blocks starts right behind a TRIGGER: an incompressible coded block whose nearest earlier coded block (looking through
//     a raw run) was incompressible too (:38-47: `update` is not called for raw blocks, `prev` survives them);
//   * every trigger is followed by a raw block (unless the chunk ends there);
//   * the run is `copy_penalty_start` blocks long (or cut by the chunk's end).  That value is 1 at the chunk's start, grows by one at the end of
//     every run (:30-35) and is halved at every 16th block while above 1 (:19-27) — so it follows from the PREVIOUS run alone (whose
//     length is its own value when it was triggered, checked by that run's thread), and is back at 1 if no run ended within the last 8
//     sixteen-block boundaries (a u8 halves to 1 in at most 8 steps).
// Every thread checks its own blocks against the index copy in LDS; all of them passing is equivalent to the FSM walk
// (tests/test_index_fsm_model.py holds the same rules, in numpy, against the oracle's FSM).  A chunk starts with a fresh FSM.
__device__ __forceinline__ bool index_fsm_consistent(const uint8_t* ix, uint32_t i, uint32_t nblk) {
    auto raw = [&](uint32_t b) -> bool { return (ix[b] & kIdxCopy) != 0; };
    auto inc = [&](uint32_t b) -> bool { return ix[b] <= 4u; };                   // coded, at most 4 MAP flags (a ragged block says 0x7f)
    auto mult16 = [](uint32_t lo, uint32_t hi) -> uint32_t { return hi / 16u + 1u - (lo + 15u) / 16u; };   // multiples of 16 in [lo, hi], lo <= hi + 1
    auto halve = [](uint32_t s, uint32_t k) -> uint32_t { const uint32_t h = k < 32u ? s >> k : 0u; return s > 1u ? (h ? h : 1u) : s; };
    if (!raw(i)) {
        // an incompressible coded block: a trigger iff the coded block before it was incompressible as well
        uint32_t u = i;
        while (u > 0 && raw(u - 1)) --u;                                          // (u - 1: the nearest earlier coded block, if any)
        const bool trigger = u > 0 && inc(u - 1);
        return !trigger || i + 1 >= nblk || raw(i + 1);
    }
    if (i > 0 && raw(i - 1)) return true;                                         // inside a run: the run's first block answers for it
    if (i == 0 || !inc(i - 1)) return false;                                      // a run must start behind an incompressible coded block ...
    const uint32_t t = i - 1;
    uint32_t u = t;
    while (u > 0 && raw(u - 1)) --u;
    if (u == 0 || !inc(u - 1)) return false;                                      // ... whose coded predecessor was incompressible too
    uint32_t L = 1;
    while (i + L < nblk && raw(i + L)) ++L;
    // copy_penalty_start when t triggered: from the previous run, if one ended within reach
    uint32_t s = 1;
    const uint32_t reach = t > 143u ? t - 143u : 0u;
    uint32_t e = t;                                                               // (search (reach, t) backwards for a raw block: the previous run's last)
    while (e > reach && !raw(e - 1)) --e;
    if (e > reach) {
        const uint32_t last = e - 1;
        uint32_t a = last;
        while (a > 0 && raw(a - 1) && last - a < 255u) --a;                       // its first block; its trigger is a - 1
        const uint32_t Lp = last - a + 1u;
        const uint32_t s_end = (halve(Lp, a <= last ? mult16(a, last) : 0u) + 1u) & 0xffu;   // halvings at the run's own blocks, then + 1 at its end
        s = halve(s_end, mult16(last + 1u, t));
    }
    return L == s || (L < s && i + L == nblk);
}

// <kProf: cycle accounting (debug build), PAGED: the streams live in the pages of a paged container>
// (`zmap_words`: not used — rounds of 12 keep the zero-entry map in LDS; the launchers' interface still carries the scratch words)
template <bool kProf, bool PAGED = false>
__global__ __launch_bounds__(kDecWaves * 64) void chameleon_decode_rot(
    const uint8_t* __restrict__ in, const uint64_t* __restrict__ offsets, const uint64_t* __restrict__ sizes, uint8_t* __restrict__ out,
    uint64_t out_stride, uint64_t out_total, uint32_t flags, const uint8_t* __restrict__ index, uint32_t* __restrict__ zmap_words,
    uint64_t* __restrict__ produced, uint32_t* __restrict__ err, SegArgs seg, uint64_t* __restrict__ prof) {
    constexpr int R = kDecRound, W = kDecWaves;                                   // records per round; waves a round rotates over
    constexpr uint32_t kThreads = W * 64, kScanThreads = 512, kPerThread = kRotMaxBlocks / kScanThreads;   // position scan: 32 index entries per thread
    // flags: bit 0 = the output length is known exactly (container decode); bits 8..11 / 16..19 = how long a wave sleeps per hand-off still to
    // come / once it has seen the token reach its predecessor, in units of 64 cycles (the launcher's choice: decode_naps)
    const uint32_t exact = flags & 1u, nap_far = (flags >> 8) & 15u, nap_near = (flags >> 16) & 15u;
    auto nap = [](uint32_t n) {                                                   // s_sleep takes an immediate: 64 cycles per unit, in binary
        if (n & 8u) __builtin_amdgcn_s_sleep(8);
        if (n & 4u) __builtin_amdgcn_s_sleep(4);
        if (n & 2u) __builtin_amdgcn_s_sleep(2);
        if (n & 1u) __builtin_amdgcn_s_sleep(1);
    };

    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t wave = rfl(threadIdx.x >> 6);
    const uint64_t chunk = blockIdx.x;
    PhaseClock<kProf> clk(blockIdx.x == 0 ? prof : nullptr);   // phases: 0 stage A, 1 stage B, 2 operands, 3 D wait, 4 exchange, 5 quads, 6 zero-entry map, 7 stores + rotate
    const uint8_t* src = in + offsets[chunk];
    const uint8_t* idx = index + chunk * (out_stride / kBlock);                 // this chunk's slice of the block index (4-byte aligned: launcher)
    const uint64_t elen64 = sizes[chunk];
    uint8_t* dst = out + chunk * out_stride;
    const uint64_t room_all = out_total - chunk * out_stride;
    const uint64_t cap = room_all < out_stride ? room_all : out_stride;
    const uint32_t elen = elen64 > 0xfff00000ull ? 0xfff00000u : (uint32_t)elen64;   // 32-bit stream offsets in the pipeline; the in-order loop finishes longer streams
    const uint32_t nblk = (uint32_t)((cap + kBlock - 1) / kBlock);               // <= kRotMaxBlocks (launcher)
    constexpr uint32_t dSync = kDecSync;
    const ZmapLds zmap{kDecZmap};
    // the table sits at LDS address 0 (this kernel has no static LDS): slot addresses need no base
    const uint32_t sy = dSync;

    {   // fresh dictionary, this chunk's zero-entry map, the block index into LDS (a segment of a longer stream — SegArgs — starts from
        // the dictionary image it is given instead)
        uint4* p = reinterpret_cast<uint4*>(smem);
        const uint4 z = make_uint4(0, 0, 0, 0);
        const uint4* image = seg.init_images ? reinterpret_cast<const uint4*>(seg.init_images + chunk * kSegImageBytes) : nullptr;
        for (uint32_t i = threadIdx.x; i < kTableBytes / 16; i += kThreads) p[i] = image ? image[i] : z;
        for (uint32_t i = threadIdx.x; i < kZmapBytes / 16; i += kThreads) reinterpret_cast<uint4*>(smem + kDecZmap)[i] = image ? image[kTableBytes / 16 + i] : z;
        const uint32_t* iw = reinterpret_cast<const uint32_t*>(idx);
        uint32_t* lw = reinterpret_cast<uint32_t*>(smem + kDecIdx);
        for (uint32_t i = threadIdx.x; i < kRotMaxBlocks / 4; i += kThreads) lw[i] = i < (nblk + 3u) / 4u ? iw[i] : 0x7f7f7f7fu;   // beyond the chunk: "ragged" = stop
        if (threadIdx.x == 0) {
            *reinterpret_cast<uint4*>(smem + dSync + kSyD) = make_uint4(0u, kNone, 0u, 0u);
            *reinterpret_cast<uint64_t*>(smem + dSync + kSyEnd) = ~0ull;
            if (lds_addr(smem) != 0) atomicOr(err, kErrWatchdog);                 // (cannot happen: see above)
        }
        if (threadIdx.x < W) { *reinterpret_cast<uint32_t*>(smem + dSync + kSyZdone + 4u * threadIdx.x) = 0u; *reinterpret_cast<uint32_t*>(smem + dSync + kSyZset + 4u * threadIdx.x) = 0u; }
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");                         // (nothing of the set-up still in flight at the barrier)
    }
    __syncthreads();

    uint32_t bad_index = 0;
    // ---- record positions of the whole chunk: one prefix sum over the index (consecutive entries per thread).  A record is
    // pipelined only if it is complete and followed by at least 2 more stream bytes (a MAP item is fetched as a dword); the first
    // one that is not (ragged block, end of the stream, end of the output, an index that disagrees with the stream length) and
    // everything behind it is finished by the in-order loop (codec.rs:102-123).
    {
        uint32_t* wave_sums = reinterpret_cast<uint32_t*>(smem + dSync + kSyWsum);
        const bool scans = threadIdx.x < kScanThreads;                            // (the first 8 of the 12 waves do the scan)
        const uint32_t first = threadIdx.x * kPerThread;
        auto rec_len = [&](uint32_t ent) -> uint32_t { return (ent & kIdxCopy) ? kBlock : kSig + kBlock - 2u * (ent & 0x7fu); };
        uint32_t mine = 0;
        if (scans) {
#pragma unroll
            for (uint32_t k = 0; k < kPerThread; ++k) mine += rec_len(smem[kDecIdx + first + k]);
        }
        uint32_t incl = mine;
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const uint32_t o = bperm(lane >= (uint32_t)d ? lane - d : lane, incl);
            if (lane >= (uint32_t)d) incl += o;
        }
        if (lane == 63 && scans) wave_sums[wave] = incl;
        __syncthreads();
        if (scans) {
            uint32_t pos = incl - mine;
            for (uint32_t w = 0; w < wave; ++w) pos += wave_sums[w];
            uint64_t stop_key = ~0ull;
#pragma unroll
            for (uint32_t k = 0; k < kPerThread; ++k) {
                const uint32_t i = first + k, ent = smem[kDecIdx + i], l = rec_len(ent);
                // the raw-copy flags must be what the blow-up protection would have decided (below): looked at only where a block is raw or incompressible
                if (exact && i < nblk && __builtin_expect((ent & kIdxCopy) != 0 || ent <= 4u, 0) && !index_fsm_consistent(smem + kDecIdx, i, nblk)) bad_index = 1;
                if (i % R == 0) *reinterpret_cast<uint32_t*>(smem + kDecPos + (i / R) * 4u) = pos;
                const bool stop = (ent & 0x7fu) == kIdxRagged || i >= nblk || ((uint64_t)i + 1) * kBlock > cap || pos >= elen || elen - pos < l + 2u;
                if (stop && stop_key == ~0ull) stop_key = ((uint64_t)i << 33) | ((uint64_t)((ent & kIdxCopy) && i < nblk ? 1u : 0u) << 32) | pos;
                pos += l;
            }
            if (threadIdx.x == kScanThreads - 1 && stop_key == ~0ull) stop_key = ((uint64_t)kRotMaxBlocks << 33) | pos;
            if (stop_key != ~0ull) atomicMin(reinterpret_cast<unsigned long long*>(smem + dSync + kSyEnd), (unsigned long long)stop_key);
        }
    }
    __syncthreads();
    // ---- PAGED (round 5): the stream lives in pages (include/density_hip.h); positions so far are positions in the STREAM.  The chunk's directory is
    // checked against them — a page starts at a multiple of 16 blocks, pages follow one another in block order, the stream position of a page's first
    // block is the bytes of the pages before it, no page holds more than a page, every page lies inside the container — and then every round's
    // position is turned into an offset from page 0; bit 0 (record positions are even) marks the rounds a page change falls into. ----
    uint32_t* pg_first = reinterpret_cast<uint32_t*>(smem + kDecPages);
    uint32_t* pg_delta = pg_first + kDecMaxPages;
    uint32_t n_pages = 0;
    if constexpr (PAGED) {
        const uint32_t* dirp = seg.page_dir + chunk * seg.page_dir_words;
        n_pages = rfl(dirp[0]);
        const bool dir_ok = n_pages >= 1 && n_pages <= kDecMaxPages && 4u * (n_pages + 1u) <= seg.page_dir_words;
        if (!dir_ok) n_pages = 0;
        uint32_t used = 0, page = 0, first = 0;
        if (threadIdx.x < n_pages) {
            const uint4 e = *reinterpret_cast<const uint4*>(dirp + 4u * (threadIdx.x + 1u));
            page = e.x; first = e.y; used = e.z;
            pg_first[threadIdx.x] = first; pg_delta[threadIdx.x] = used;
        }
        if (threadIdx.x == 0) *reinterpret_cast<uint32_t*>(smem + dSync + kSyEnd + 8) = 0u;   // (the verdict word)
        __syncthreads();
        uint32_t before = 0;
        if (threadIdx.x < n_pages) {
            const uint32_t k = threadIdx.x;
            for (uint32_t m = 0; m < k; ++m) before += pg_delta[m];               // bytes of stream in the pages before this one
            bool ok = page < seg.page_limit && used <= kPageBytes && first % 16u == 0 && first < nblk && (k == 0 ? first == 0 : first > pg_first[k - 1]);
            if (ok) {
                // the stream position of block `first`: the position of its round and the index entries in front of it inside the round
                uint32_t at = *reinterpret_cast<const uint32_t*>(smem + kDecPos + (first / R) * 4u);
                for (uint32_t b = first / R * R; b < first; ++b) { const uint32_t ent = smem[kDecIdx + b]; at += (ent & kIdxCopy) ? kBlock : kSig + kBlock - 2u * (ent & 0x7fu); }
                ok = at == before;
            }
            // the pages hold the chunk's stream and nothing else: the last page ends where the size table says the stream ends — which also keeps
            // every stream position below `elen` inside a page of the directory (no read through a directory that is shorter than its stream)
            if (k + 1u == n_pages && (uint64_t)before + used != elen64) ok = false;
            if (!ok) bad_index = 1;
        }
        if (!dir_ok) bad_index = 1;
        if (bad_index) atomicOr(reinterpret_cast<uint32_t*>(smem + dSync + kSyEnd + 8), 1u);
        __syncthreads();
        if (threadIdx.x < n_pages) pg_delta[threadIdx.x] = (page << kPageShift) - before;
        const bool dead = *reinterpret_cast<const uint32_t*>(smem + dSync + kSyEnd + 8) != 0;   // a directory (or index) that lies: nothing is read through it
        __syncthreads();
        for (uint32_t x = threadIdx.x; x <= kRotMaxBlocks / R; x += kThreads) {
            const uint32_t b = x * R;
            uint32_t lo = 0, hi = n_pages ? n_pages - 1u : 0u;                     // the last page whose first block is <= b
            while (lo < hi) { const uint32_t mid = (lo + hi + 1u) >> 1; if (pg_first[mid] <= b) lo = mid; else hi = mid - 1u; }
            uint32_t* slot = reinterpret_cast<uint32_t*>(smem + kDecPos + x * 4u);
            const bool change = lo + 1u < n_pages && pg_first[lo + 1u] < b + R;
            *slot = dead ? 0u : (*slot + pg_delta[lo]) | (change ? 1u : 0u);
        }
        if (dead) { if (threadIdx.x == 0) { atomicOr(err, 8u); *reinterpret_cast<uint64_t*>(smem + dSync + kSyEnd) = 0; } }   // no record is followed: the in-order tail reports the rest
        __syncthreads();
    }
    const uint64_t end_key = *reinterpret_cast<const uint64_t*>(smem + dSync + kSyEnd);
    const uint32_t nvalid = rfl((uint32_t)(end_key >> 33));                      // records [0, nvalid) are complete and followed by more data
    const uint32_t npr = nvalid / R;                                              // whole rounds: these rotate; the rest (< R records + the ragged end) is the epilogue

    // ---- three-stage software pipeline per wave: A(x + 2W) signature loads | B(x + W) item loads | C(x) dictionary + stores ----
    // Per round in flight: lane j < R holds record j's position and (one 8-byte load) its signature; after stage B every lane
    // holds its R items and its R MAP/PLAIN flags (bit j of `hits`).  All rounds are whole, so every stage is straight-line code:
    // the loads of a stage leave back to back and nothing waits for a store.
    struct Meta { uint32_t posv, cnt; u32x2 sgv; uint32_t copy_mask; };
    // (Rounds past the end are clamped to the last one instead of skipped — a few redundant loads at the end of a chunk — so that the
    // number and order of memory operations per iteration is fixed and the compiler's waits count exactly.)
    auto stage_a = [&](uint32_t xr, Meta& m) {                                   // positions of round x; signatures requested
        const uint32_t x = xr < npr ? xr : npr - 1u;
        const uint32_t e = smem[kDecIdx + x * R + (lane < R ? lane : 0u)];        // lane j < R: entry of record j
        uint32_t base = rfl(lds_peek1(kDecPos + x * 4u));
        const uint32_t mylen = (e & kIdxCopy) ? kBlock : kSig + kBlock - 2u * (e & 0x7fu);
        uint32_t hop = 0;                                                         // PAGED: what the records behind a page change inside this round are further on
        if constexpr (PAGED) {
            if (__builtin_expect(base & 1u, 0)) {                                 // (a page change falls into this round: some forty times per 4 MiB chunk)
                uint32_t k = 0;
                while (k + 1u < n_pages && pg_first[k + 1u] <= x * R) ++k;        // the page of the round's first record; the next one starts inside the round
                const uint32_t j0 = pg_first[k + 1u] - x * R;
                hop = lane >= j0 ? pg_delta[k + 1u] - pg_delta[k] : 0u;
                base &= ~1u;
            }
        }
        uint32_t incl = mylen;                                                    // prefix within rows of 16 lanes
        incl += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)incl, 0x111, 0xf, 0xf, true);   // row_shr:1
        incl += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)incl, 0x112, 0xf, 0xf, true);   // row_shr:2
        incl += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)incl, 0x114, 0xf, 0xf, true);   // row_shr:4
        incl += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)incl, 0x118, 0xf, 0xf, true);   // row_shr:8
        m.posv = base + incl - mylen + hop;
        m.copy_mask = (uint32_t)ballot64((e & kIdxCopy) != 0 && lane < R);
        m.sgv = *reinterpret_cast<const u32x2_u*>(src + ((lane < R && !(e & kIdxCopy)) ? m.posv : base));   // codec.rs:28-31 (idle lanes: any valid address)
        m.cnt = e & 0x7fu;                                                        // the entry's MAP count: checked against the signature in stage B
    };
    const uint32_t minus_2lane = 0u - 2u * lane;
    auto stage_b = [&](const Meta& m, uint32_t& hits, uint32_t (&item)[R]) {    // signatures -> MAP/PLAIN flags, item loads
        // the index must agree with the stream it describes: a record's MAP count is its signature's popcount (lane j < R: record j)
        bad_index |= (lane < R && !((m.copy_mask >> lane) & 1u) && (uint32_t)(__builtin_popcount(m.sgv.x) + __builtin_popcount(m.sgv.y)) != m.cnt) ? 1u : 0u;
        hits = 0;
        // (lane j < R prepares record j for all lanes at once — a raw record has no signature: no MAP flags, its 256 bytes are its "items" —
        // so that the loop below is three lane reads per record and no scalar arithmetic)
        const uint32_t codedv = ((m.copy_mask >> lane) & 1u) ? 0u : ~0u;             // all ones, or 0 for 256 raw bytes without a signature (codec.rs:89-91)
        const uint32_t sxv = m.sgv.x & codedv, syv = m.sgv.y & codedv, pbv = m.posv + (codedv & kSig);
#pragma unroll
        for (uint32_t j = 0; j < R; ++j) {                                        // (straight-line: selects, no branches)
            const uint32_t slo = rlane_u(sxv, (int)j), shi = rlane_u(syv, (int)j), pos = rlane_u(pbv, (int)j);
            uint32_t bit;                                                         // this lane's flag: one select on the signature as a lane mask
            asm("v_cndmask_b32_e64 %0, 0, 1, %1" : "=v"(bit) : "s"(((uint64_t)shi << 32) | slo));
            hits |= bit << j;
            // this lane's item sits 4 bytes further per PLAIN lane below it and 2 per MAP lane: 4*lane - 2*(MAP lanes below), from the record's items on
            const uint32_t t = __builtin_amdgcn_mbcnt_hi(shi, __builtin_amdgcn_mbcnt_lo(slo, minus_2lane));   // MAP lanes below - 2*lane
            // (one multiply-add — left to the compiler: a shift pair and a subtract; the stream's base is the load's scalar operand)
            uint32_t off;
            asm("v_mad_i32_i24 %0, %1, -2, %2" : "=v"(off) : "v"(t), "s"(pos));
            item[j] = ld32u(src + off);
        }
    };

    Meta ma, mb, mc;
    ma.posv = mb.posv = mc.posv = 0; ma.cnt = mb.cnt = mc.cnt = 0; ma.copy_mask = mb.copy_mask = mc.copy_mask = 0;
    ma.sgv = mb.sgv = mc.sgv = u32x2{0u, 0u};
    uint32_t itemb[R], itemc[R], hitsb = 0, hitsc = 0;
#pragma unroll
    for (uint32_t j = 0; j < R; ++j) { itemb[j] = 0; itemc[j] = 0; }
    // prologue: B(w) needs A(w); A(w + W) goes out behind it
    if (npr) {
        stage_a(wave, mb);
        stage_b(mb, hitsc, itemc);
        mc = mb;
        stage_a(wave + W, mb);
        // Everything asked for so far is waited for HERE, once, visibly to the compiler: with nothing pending at the top of the loop the
        // waits it places inside count from the loop's own order of loads and stores (a signature load is followed by the round's 12
        // record stores, so the next round's stage B waits for "all but the last 12"); with loads still pending from out here it would
        // settle for the common bound of both ways in — zero — and every round would begin by waiting for its predecessor's stores.
        asm volatile("" : : "v"(mb.sgv.x), "v"(mb.sgv.y), "v"(mb.posv), "v"(mc.sgv.x), "v"(mc.sgv.y));
#pragma unroll
        for (uint32_t j = 0; j < R; ++j) asm volatile("" : : "v"(itemc[j]));
    }

    uint32_t ra[R], mask[R], val[R];
    for (uint32_t x = wave; x < npr; x += W) {
        clk.start();
        __builtin_amdgcn_s_setprio(1);                                   // (priorities: see the encoder's exchange)
        // (B first: what it waits for — the signatures requested one iteration ago — is older than anything issued since, so the
        // wait does not cover a load that has just left)
        stage_b(mb, hitsb, itemb);
        clk.mark(1);
        stage_a(x + 2 * W, ma);
        clk.mark(0);

        // ---- C: operands of the dictionary step ----
        // (Instruction count is this kernel's time: a wave whose iteration is longer than W hand-offs arrives late for its turn, and every
        // late arrival stalls the chain — six instructions per record less made the kernel 17 % faster.  Hence: the loop below treats every
        // record as coded and a rare branch behind it takes the raw-copy records' operands back (a chunk's cold start; incompressible
        // data), and the rare zero-entry candidates cost one compare per record each way, their lanes collected in scalar registers.)
        const uint32_t coded_mask = ((1u << R) - 1u) & ~mc.copy_mask;             // records that go through the dictionary
        const uint32_t hit_mask = seg.lastwriters_only ? 0u : hitsc;              // MAP quads that are looked up (raw records have no hit bits: stage B)
        // zplain: lanes with a zero-entry CANDIDATE that writes — a PLAIN quad whose stored entry is 0 (those that read 0: zm[] below)
        uint64_t zplain = 0;
#pragma unroll
        for (uint32_t j = 0; j < R; ++j) {
            const uint32_t qv = itemc[j];
            const uint32_t P = qv * kHashMul;
            // MAP: the item is the slot (chameleon.rs:64-68); PLAIN: the upper half of the hash product — one select with a half-word pick per
            // side; `em`: 0xffff for the lanes that write (PLAIN: chameleon.rs:56-61), 0 for those that only read (MAP); `mm`: the MAP lanes
            uint32_t h, em;
            uint64_t mm;
            asm("v_and_b32 %0, %5, %3\n\t"
                "v_cmp_ne_u32 vcc, 0, %0\n\t"
                "v_cndmask_b32_sdwa %0, %4, %6, vcc dst_sel:DWORD dst_unused:UNUSED_PAD src0_sel:WORD_1 src1_sel:WORD_0\n\t"
                "v_cndmask_b32 %1, %7, 0, vcc\n\t"
                "s_mov_b64 %2, vcc"
                : "=&v"(h), "=&v"(em), "=s"(mm) : "v"(hitsc), "v"(P), "n"(1u << j), "v"(qv), "v"(0xffffu) : "vcc");
            const uint32_t sh = h << 4;                                           // (a shift takes the low five bits of its count: (h & 1) << 4)
            // stored_entry(qv, P) for the lanes that write, 0 for a MAP lane (`em` is 0xffff or 0: the salt needs no mask of its own)
            const uint32_t e = (((P & 0xfffeu) | (qv >> 31)) ^ __umul24(P >> 16, kSaltMul)) & em;
            ra[j] = (h >> 1) << 2;
            mask[j] = em << sh;
            val[j] = e << sh;
            zplain |= ballot64(e == 0) & ~mm;                                     // a PLAIN quad whose stored entry is 0 (one compare; the rest is scalar)
        }
        // A round that will MARK the zero-entry map (a PLAIN quad whose entry is 0: about four per 4 MiB of text) says so before its exchanges:
        // rounds behind it that only LOOK a slot up in the map (every recurrence of such a quad: one round in 25) then wait for nothing but
        // earlier rounds that have said so — almost never — instead of for every earlier round to finish.
        // (round 5) ... unless it is the ZERO quad, whose entry 0 in slot 0 is no candidate (a 0 there IS the zero quad, written or not): the first
        // zero quad behind anything else that hashed to slot 0 — once per incompressible patch of mixed data — used to announce a mark, and a
        // marking round waits for every earlier round to be through.  Looked at exactly, in a rare branch (a last-writers pass does mark slot 0:
        // there the mark says "written").
        uint64_t zreal = zplain;
        if (__builtin_expect(zplain != 0, 0) && !seg.lastwriters_only) {
            zreal = 0;
#pragma nounroll
            for (uint32_t j = 0; j < R; ++j) {                                    // (rolled, over select chains, like every rare path of this kernel)
                const uint32_t it = pick<R>(itemc, j), P = it * kHashMul;
                zreal |= ballot64(!((hitsc >> j) & 1u) && ((coded_mask >> j) & 1u) && (P >> 16) != 0 && stored_entry(it, P) == 0);
            }
        }
        const bool marks = zreal != 0;
        if (__builtin_expect(marks, 0)) { if (lane == 0) lds_poke(sy + kSyZset + 4u * wave, x + 1u); }
        if (__builtin_expect(mc.copy_mask != 0, 0)) {
            // raw-copy records (codec.rs:89-91) touch no state: their lanes read a harmless conflict-free word instead
#pragma unroll
            for (uint32_t j = 0; j < R; ++j) {
                const bool raw = (mc.copy_mask >> j) & 1u;
                ra[j] = raw ? 4u * lane : ra[j];
                mask[j] = raw ? 0u : mask[j];
                val[j] = raw ? 0u : val[j];
            }
        }
        const uint32_t tokaddr = lane == 0 ? sy + kSyD : sy + kSySink + 4u * lane;
        uint32_t tokval = x + 1u;                                                 // (in its register before the wait: nothing but the priority change between the token and the exchanges)
        asm volatile("" : "+v"(tokval));
        pin_operands<R>(ra, mask, val);                                           // complete before the wait for the token
        clk.mark(2);
        clk.stamp(x, 0, lane);
        __builtin_amdgcn_s_setprio(2);
        // ---- D chain ----
        // (Every poll is an LDS instruction in the queue the token holder's exchanges go through.  A wave two or more turns away sleeps for most
        // of the hand-offs still to come — one takes 600 cycles and more —, the next in line polls; when it has SEEN the token reach its
        // predecessor it sleeps through the first part of that critical section too.)
        for (uint32_t spins = 0, seen = ~0u;;) {
            const uint32_t D = rfl(lds_peek1(sy + kSyD));
            if (D == x) break;
            if (D == kPoison) wave_exit();
            const uint32_t dist = x - D;
            // (a hand-off is ~480 cycles + ~19 per record — profiles/r04_*: 690 for rounds of 12, 780 for 16; the sleeps cover about half of one)
            if (dist >= 2) { for (uint32_t k = 1; k < dist && k < 6; ++k) nap(nap_far); }   // 320 cycles (rounds of 12) per hand-off to come
            else {
                if (seen != ~0u && seen != D) nap(nap_near);                      // 192 cycles of a critical section of 450 and more (12 records)
                if (poll_word(sy + kSyD, x, 8)) break;
            }
            seen = D;
            watchdog(spins, sy, err, lane);
        }
        clk.mark(3);
        clk.stamp(x, 1, lane);
        __builtin_amdgcn_s_setprio(3);
        exchange_tied12(ra, mask, val, tokaddr, tokval);
        __builtin_amdgcn_s_setprio(0);
        clk.mark(4);
        clk.stamp(x, 2, lane);

        // ---- what each slot holds at this lane's turn -> quads (in place of the answers) ----
        // (a MAP quad that read 0 — never written, or a genuine zero entry? — is a lane of zm[j]: the compare costs what the running minimum
        // it replaces cost, its answer lands in scalar registers, and the rare path below knows record and lanes without working them out again)
        uint64_t zany = 0;
        uint32_t zrec = 0;                                                        // the records that have such a lane: one scalar bit per record (a lane mask per record was 2 R scalar registers)
#pragma unroll
        for (uint32_t j = 0; j < R; ++j) {
            const bool maps = (hit_mask >> j) & 1u;
            const uint32_t h = itemc[j] & 0xffffu;
            const uint32_t cur = __builtin_amdgcn_ubfe(ra[j], itemc[j] << 4, 16);  // the slot's half of the word ((h & 1) << 4: a bit-field offset is five bits)
            const uint64_t mm = ballot64(maps);                                   // the MAP lanes as a lane mask: for the select below and, in scalar registers, for
            const uint64_t zj = ballot64(cur == 0) & mm;                          // "MAP of a slot holding 0": never written, or a genuine zero entry?
            zany |= zj;
            zrec |= (zj != 0 ? 1u : 0u) << j;
            const uint32_t mq = entry_to_quad(h, cur);                            // (for every lane, then one select: cheaper than an exec mask around it)
            asm("v_cndmask_b32_e64 %0, %1, %2, %3" : "=v"(ra[j]) : "v"(itemc[j]), "v"(mq), "s"(mm));
        }
        clk.mark(5);
        // ---- zero-entry map, in stream order (rare: stored entries are salted).  A round with no such quad only reports "done"; one that
        // has any first waits until every earlier round has reported (wave w' owns the rounds = w' mod W). ----
        if (__builtin_expect(marks || zany != 0, 0)) {
          if (!marks) {
            // (round 5) Slot 0 needs no map: its entry 0 IS the zero quad, written or not (chameleon.rs:41,88-100) — and the zero quad is the
            // commonest quad of real data (zero pages, padding).  Its MAP lanes read 0 like a candidate's, so all-zero input took every record
            // of every round through the select chains below, low-entropy data every other round.  Here, still in the rare branch (rounds
            // without any 0 read never get here), the candidates are made exact again: a MAP lane that read 0 — its quad is the one an entry of
            // 0 stands for in its slot, entry -> quad being one-to-one per slot — in a slot other than 0.
            uint32_t real = 0;
            for (uint32_t zb = zrec; zb; zb &= zb - 1u) {                         // (rolled, over select chains)
                const uint32_t j = (uint32_t)__builtin_ctz(zb);
                const uint32_t h = pick<R>(itemc, j) & 0xffffu;
                real |= (ballot64(((hit_mask >> j) & 1u) != 0 && h != 0 && pick<R>(ra, j) == entry_to_quad(h, 0)) != 0 ? 1u : 0u) << j;
            }
            zrec &= real;
            if (zrec == 0) zany = 0;
          }
          if (marks || zany != 0) {
            clk.note(x, 1, lane);
            for (uint32_t spins = 0;;) {
                const uint32_t wv = lane % W;
                if (marks) {
                    // marks must not be seen by look-ups of earlier rounds: every earlier round has finished its zero-entry phase
                    const uint32_t d = (wave + W - wv) % W;                       // wave wv's last round before x is x - d
                    const uint32_t done = lds_peek1(sy + kSyZdone + 4u * wv);    // (rounds finished: last round + 1)
                    if (ballot64(d != 0 && x >= d && done < x - d + 1u) == 0) break;
                } else {
                    // look-ups only: the marks of earlier rounds must be in — those rounds said so before their exchanges, i.e. before ours
                    const uint32_t pending = lds_peek1(sy + kSyZset + 4u * wv);  // (round + 1, 0: none)
                    if (ballot64(pending != 0 && pending - 1u < x) == 0) break;
                }
                if (rfl(lds_peek1(sy + kSyD)) == kPoison) wave_exit();
                watchdog(spins, sy, err, lane);
            }
            if (!marks) {
                // Look-ups only (about one round in 25 on repetitive text: every recurrence of a quad whose entry is 0): nothing in this round
                // changes the map, so its look-ups need no order among themselves — all lanes of a record at once, usually one lane of one record
                // The records concerned — usually one — one by one, in a ROLLED loop over select chains.  (Round 4: every rare path of this kernel
                // is rolled now.  Unrolled, their per-record temporaries were all live at once and set the kernel's register need — 160 for rounds
                // of 12, spills for anything longer — although the common path needs ~120; rolled, rounds of 16 and 20 fit 12 waves' 168.)  Which of
                // the record's lanes read 0 is worked out again: the quad such a lane holds is the one an entry of 0 stands for in its slot, and
                // entry -> quad is one-to-one per slot.
                for (uint32_t zb = zrec; zb; zb &= zb - 1u) {
                    const uint32_t j = (uint32_t)__builtin_ctz(zb);
                    const uint32_t it = pick<R>(itemc, j), an = pick<R>(ra, j);
                    const uint32_t h = it & 0xffffu;
                    const bool t = ((hit_mask >> j) & 1u) && an == entry_to_quad(h, 0) && h != 0;   // (slot 0: "never written" and its zero entry both stand for the zero quad)
                    uint32_t bit = 1;
                    if (t) bit = zmap.test(h);
                    const uint32_t outv = (t && !bit) ? 0u : an;                  // chameleon.rs:64-68 on a never-written (zero) word
#pragma unroll
                    for (uint32_t k = 0; k < R; ++k) {
                        uint32_t jj = j;
                        asm volatile("" : "+s"(jj));                              // (opaque, as in pick)
                        ra[k] = jj == k ? outv : ra[k];
                    }
                }
            } else {
            // which records have such a quad — from what is still in registers, a few instructions per record — then those records one by one, usually one
            uint32_t zblocks = 0;
#pragma nounroll
            for (uint32_t j = 0; j < R; ++j) {                                    // (rolled, over select chains: see above)
                // a PLAIN quad with stored entry 0 (from the item again: the exchange operands are dead by now, and keeping them alive for this path
                // cost the common one registers), or a MAP quad whose slot gave the quad that an entry of 0 stands for
                const uint32_t it = pick<R>(itemc, j), an = pick<R>(ra, j);
                const bool wrote0 = !((hitsc >> j) & 1u) && ((coded_mask >> j) & 1u) && stored_entry(it, it * kHashMul) == 0;
                const bool read0 = ((hit_mask >> j) & 1u) && an == entry_to_quad(it & 0xffffu, 0);
                zblocks |= (ballot64(wrote0 || read0) != 0 ? 1u : 0u) << j;
            }
            zblocks &= coded_mask;
            for (uint32_t zb = zblocks; zb; zb &= zb - 1u) {
                const uint32_t j = (uint32_t)__builtin_ctz(zb);
                const bool coded = (coded_mask >> j) & 1u;
                const bool hit = (hitsc >> j) & 1u;
                const uint32_t qv = pick<R>(itemc, j), cur = pick<R>(ra, j);
                const uint32_t P = qv * kHashMul;
                const uint32_t h = hit ? (qv & 0xffffu) : (P >> 16);
                const bool zset = coded && !hit && stored_entry(qv, P) == 0 && (h != 0 || seg.lastwriters_only);
                const bool ztest = coded && hit && h != 0 && cur == entry_to_quad(h, 0) && !seg.lastwriters_only;
                uint64_t todo = ballot64(zset || ztest);
                uint32_t out = cur;
                while (todo) {                                                    // ascending lane == stream order
                    const uint32_t l = (uint32_t)__builtin_ctzll(todo);
                    todo &= todo - 1;
                    if (lane == l) {
                        if (zset) zmap.set(h);
                        else if (!zmap.test(h)) out = 0;                          // chameleon.rs:64-68 on a never-written (zero) word
                    }
                }
#pragma unroll
                for (uint32_t k = 0; k < R; ++k) {
                    uint32_t jj = j;
                    asm volatile("" : "+s"(jj));                                  // (opaque, as in pick)
                    ra[k] = jj == k ? out : ra[k];
                }
            }
            }
          }
        }
        if (lane == 0) {
            if (marks) { asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); lds_poke(sy + kSyZset + 4u * wave, 0u); }   // (behind the marks: LDS operations of a wave execute in order)
            lds_poke(sy + kSyZdone + 4u * wave, x + 1u);
        }
        clk.mark(6);

        // ---- stores: 256 coalesced bytes per record ----
        uint8_t* base = dst + (uint64_t)x * R * kBlock;
#pragma unroll
        for (uint32_t j = 0; j < R; ++j) *reinterpret_cast<uint32_t*>(base + j * kBlock + 4u * lane) = ra[j];   // (a last-writers pass stores too: a branch here would cost stage B its exact waits)
        // ---- rotate the pipeline ----
        mc = mb; mb = ma; hitsc = hitsb;
#pragma unroll
        for (uint32_t j = 0; j < R; ++j) itemc[j] = itemb[j];
        clk.mark(7);
        clk.stamp(x, 3, lane);
    }
    clk.flush(wave, lane);

    if (ballot64(bad_index != 0) != 0 && lane == 0) atomicOr(err, 8u);             // (lane j < R holds record j's verdict: any lane's counts)
    wg_barrier();
    // ---- epilogue on one wave, in order: the records of the last, partial round — one call per record, the block's raw-copy flag
    // from the index standing in for the FSM — then the ragged end of the stream (codec.rs:102-123) ----
    if (wave == 0) {
        Guard g;
        // (PAGED: no page starts inside this tail — the encoder keeps room for it in the last round's page —, so one offset turns its stream positions
        // into offsets from page 0; a directory that says otherwise is malformed)
        uint32_t tail_delta = 0;
        bool bad = false;
        if constexpr (PAGED) {
            if (n_pages == 0 || *reinterpret_cast<const uint32_t*>(smem + dSync + kSyEnd + 8) != 0 || pg_first[n_pages - 1u] > npr * R) bad = true;
            else tail_delta = pg_delta[n_pages - 1u];
        }
        const uint32_t end_at = (uint32_t)end_key + tail_delta;
        // (32-bit arithmetic like every page offset: the last page may lie BELOW the stream bytes in front of it — a producer may number its pages in any
        // order; this library's encoder never does, its counter only grows —, and the sum must wrap like the offsets it is compared with)
        const uint64_t elen_at = (uint32_t)((uint32_t)elen64 + tail_delta);
        uint64_t ip = npr * R < nvalid ? (rfl(lds_peek1(kDecPos + npr * 4u)) & (PAGED ? ~1u : ~0u)) : end_at, op = (uint64_t)npr * R * kBlock;
        for (uint32_t i = npr * R; i < nvalid && !bad; ++i) {
            const uint32_t ent = smem[kDecIdx + i];
            const uint64_t rec_end = ip + ((ent & kIdxCopy) ? kBlock : kSig + kBlock - 2u * (ent & 0x7fu));
            g.penalty = (ent & kIdxCopy) ? 1u : 0u; g.start = 1; g.prev = 0; g.counter = 1;
            // The record's signature must say what the index says (as the rotating rounds check it): lengths alone do not — a corrupted signature with MORE
            // MAP flags makes the record 8 or more bytes shorter than the index has it, and the bytes left over pass for a signature with no items behind it
            // (codec.rs:102-123 on an exhausted buffer), where the reference reads the next record from the wrong place (tools/gpu_fuzz_tail.py, round 6).
            if (!(ent & kIdxCopy)) {
                if (rec_end > elen_at || ip + kSig > rec_end) bad = true;
                else {
                    const uint64_t sig = (uint64_t)rfl(ld32u(src + ip)) | ((uint64_t)rfl(ld32u(src + ip + 4)) << 32);
                    if ((uint32_t)__builtin_popcountll(sig) != (ent & 0x7fu)) bad = true;
                }
                if (bad) break;
            }
            bad = !decode_in_order(src, rec_end, dst, cap, g, ip, op, 0u, zmap, lane, seg.lastwriters_only != 0) || ip != rec_end;
        }
        g.penalty = (uint32_t)(end_key >> 32) & 1u; g.start = 1; g.prev = 0; g.counter = 1;    // the stopping block's raw-copy flag is all that is left of the FSM
        if (!bad && (ip != end_at || op != (uint64_t)nvalid * kBlock)) bad = true;
        if (!bad) bad = !decode_in_order(src, elen_at, dst, cap, g, ip, op, 0u, zmap, lane, seg.lastwriters_only != 0);
        if (exact && !bad && op != cap) bad = true;
        if (lane == 0) {
            produced[chunk] = op;
            if (bad) atomicOr(err, 1u);
        }
    }
    if (seg.final_images) {                                                        // the dictionary as this chunk leaves it
        __threadfence();
        wg_barrier();
        uint4* image = reinterpret_cast<uint4*>(seg.final_images + chunk * kSegImageBytes);
        const uint4* p = reinterpret_cast<const uint4*>(smem);
        for (uint32_t i = threadIdx.x; i < kTableBytes / 16; i += kThreads) image[i] = p[i];
        for (uint32_t i = threadIdx.x; i < kZmapBytes / 16; i += kThreads) image[kTableBytes / 16 + i] = reinterpret_cast<const uint4*>(smem + kDecZmap)[i];
    }
}

// ---- host launchers ----
namespace {
// how long the decoder's waiting waves sleep (units of 64 cycles): per hand-off still to come (bits 8..11 of the kernel's flags) and once the
// token has reached the predecessor (bits 16..19); DENSITY_HIP_NAP="far,near" overrides (tuning runs, debug build)
uint32_t decode_naps() {
    static const char* env = debug_env("DENSITY_HIP_NAP");
    uint32_t far_ = 5u, near_ = 3u;
    if (env) { unsigned a = 0, b = 0; if (sscanf(env, "%u,%u", &a, &b) == 2) { far_ = a & 15u; near_ = b & 15u; } }
    return (far_ << 8) | (near_ << 16);
}
constexpr uint32_t kDecThreads = kDecWaves * 64;
}  // namespace

bool rotor_decode_eligible(const uint8_t* d_out, uint32_t n_chunks, uint64_t out_stride, uint64_t out_total, const uint8_t* d_index, const uint32_t* d_zmap) {
    if (!d_index || !d_zmap || n_chunks > kMaxPipelinedChunks) return false;
    const uint64_t per_chunk = n_chunks == 1 ? (out_total < out_stride ? out_total : out_stride) : out_stride;
    if ((per_chunk + kBlock - 1) / kBlock > kRotMaxBlocks) return false;
    if ((uintptr_t)d_index % 4 != 0 || (n_chunks > 1 && (out_stride / kBlock) % 4 != 0)) return false;
    return (uintptr_t)d_out % 4 == 0 && (n_chunks == 1 || out_stride % 4 == 0);
}
hipError_t launch_rotor_decode(const uint8_t* d_in, const uint64_t* d_offsets, const uint64_t* d_sizes, uint32_t n_chunks, uint8_t* d_out,
                               uint64_t out_stride, uint64_t out_total, bool exact, const uint8_t* d_index, uint32_t* d_zmap,
                               uint64_t* d_produced, uint32_t* d_err, hipStream_t stream) {
    uint64_t* prof = rot_prof_buffer();
    // rounds of 12 records on 12 waves (168 registers each): the longest round that does not spill, i.e. the shortest chain per record.  What
    // was measured against it — 8 on 16, 16 and 20 on 12, 12 and 16 on 16, one set of item registers — is in DESIGN.md 4.3.
    auto kernel = prof ? chameleon_decode_rot<true> : chameleon_decode_rot<false>;
    hipError_t e = hipFuncSetAttribute((const void*)kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)kDecLds);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(kernel, dim3(n_chunks), dim3(kDecThreads), kDecLds, stream, d_in, d_offsets, d_sizes, d_out, out_stride, out_total,
                       (exact ? 1u : 0u) | decode_naps(), d_index, d_zmap, d_produced, d_err, SegArgs{}, prof);
    rot_prof_report("decode", "stage A | stage B | operands | D wait | exchange | quads | Z chain | stores", prof, stream, kDecWaves);
    return hipGetLastError();
}
hipError_t launch_rotor_decode_paged(const uint8_t* d_pages, const uint64_t* d_offsets, const uint64_t* d_sizes, uint32_t n_chunks, uint8_t* d_out, uint64_t out_stride,
                                     uint64_t out_total, const uint8_t* d_index, const uint32_t* d_dir, uint32_t dir_words, uint32_t n_pages, uint32_t* d_zmap,
                                     uint64_t* d_produced, uint32_t* d_err, hipStream_t stream) {
    auto kernel = chameleon_decode_rot<false, true>;
    hipError_t e = hipFuncSetAttribute((const void*)kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)kDecLdsPaged);
    if (e != hipSuccess) return e;
    SegArgs pg;
    pg.page_dir = const_cast<uint32_t*>(d_dir); pg.page_dir_words = dir_words; pg.page_limit = n_pages;
    hipLaunchKernelGGL(kernel, dim3(n_chunks), dim3(kDecThreads), kDecLdsPaged, stream, d_pages, d_offsets, d_sizes, d_out, out_stride, out_total,
                       1u | decode_naps(), d_index, d_zmap, d_produced, d_err, pg, (uint64_t*)nullptr);
    return hipGetLastError();
}
hipError_t launch_rotor_decode_seg(const uint8_t* d_in, const uint64_t* d_offsets, const uint64_t* d_sizes, uint32_t n_chunks, uint8_t* d_out,
                                   uint64_t out_stride, uint64_t out_total, const uint8_t* d_index, uint32_t* d_zmap, uint64_t* d_produced, uint32_t* d_err,
                                   SegArgs seg, hipStream_t stream) {
    auto kernel = chameleon_decode_rot<false>;
    hipError_t e = hipFuncSetAttribute((const void*)kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)kDecLds);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(kernel, dim3(n_chunks), dim3(kDecThreads), kDecLds, stream, d_in, d_offsets, d_sizes, d_out, out_stride, out_total, decode_naps(),
                       d_index, d_zmap, d_produced, d_err, seg, (uint64_t*)nullptr);
    return hipGetLastError();
}

}  // namespace density
