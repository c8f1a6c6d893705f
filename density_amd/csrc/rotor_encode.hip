// rotor_encode.hip — the Chameleon wave-rotation ENCODER for gfx950 (design notes: rotor.hip; shared device code: rotor_dev.hpp), the
// last-writers kernel and the image merge of the segmented whole-stream encode, and their launchers.
#include "rotor_dev.hpp"

namespace density {

namespace {

#define DENSITY_ROT_PF16 \
    "global_load_dword v240, %0, off offset:0\n\t" \
    "global_load_dword v241, %0, off offset:256\n\t" \
    "global_load_dword v242, %0, off offset:512\n\t" \
    "global_load_dword v243, %0, off offset:768\n\t" \
    "global_load_dword v244, %0, off offset:1024\n\t" \
    "global_load_dword v245, %0, off offset:1280\n\t" \
    "global_load_dword v246, %0, off offset:1536\n\t" \
    "global_load_dword v247, %0, off offset:1792\n\t" \
    "global_load_dword v248, %0, off offset:2048\n\t" \
    "global_load_dword v249, %0, off offset:2304\n\t" \
    "global_load_dword v250, %0, off offset:2560\n\t" \
    "global_load_dword v251, %0, off offset:2816\n\t" \
    "global_load_dword v252, %0, off offset:3072\n\t" \
    "global_load_dword v253, %0, off offset:3328\n\t" \
    "global_load_dword v254, %0, off offset:3584\n\t" \
    "global_load_dword v255, %0, off offset:3840\n\t"
#define DENSITY_ROT_MV16 \
    "v_mov_b32 %0, v240\n\t" \
    "v_mov_b32 %1, v241\n\t" \
    "v_mov_b32 %2, v242\n\t" \
    "v_mov_b32 %3, v243\n\t" \
    "v_mov_b32 %4, v244\n\t" \
    "v_mov_b32 %5, v245\n\t" \
    "v_mov_b32 %6, v246\n\t" \
    "v_mov_b32 %7, v247\n\t" \
    "v_mov_b32 %8, v248\n\t" \
    "v_mov_b32 %9, v249\n\t" \
    "v_mov_b32 %10, v250\n\t" \
    "v_mov_b32 %11, v251\n\t" \
    "v_mov_b32 %12, v252\n\t" \
    "v_mov_b32 %13, v253\n\t" \
    "v_mov_b32 %14, v254\n\t" \
    "v_mov_b32 %15, v255\n\t"
#define DENSITY_ROT_STAGE16 "v240", "v241", "v242", "v243", "v244", "v245", "v246", "v247", "v248", "v249", "v250", "v251", "v252", "v253", "v254", "v255"
// Next round's quads, fetched by hand: 16 dword loads (one 256-byte block each) the compiler does not see as memory operations, so
// it places no wait of its own between them and the stores that follow.  They land in the 16 highest registers of the wave
// (v240..v255, named in the statements and declared clobbered), which the compiler, allocating upwards from v0, never reaches in
// these kernels (tools/check_isa.py checks that no other instruction names them), so nothing can read or move them early.  (The
// accumulation registers would be the natural staging area, but a kernel that names one has its register file split in halves.)
// `quads_landed` waits — for everything (kDrained), or for all but the 16 younger memory operations the caller guarantees to have
// issued since (vmcnt counts a wave's loads and stores in order) — and reads them into `q`.
__device__ __forceinline__ void prefetch_quads(const uint8_t* p) { asm volatile(DENSITY_ROT_PF16 : : "v"(p) : "memory", DENSITY_ROT_STAGE16); }
template <bool kDrained>
__device__ __forceinline__ void quads_landed(uint32_t (&q)[16]) {
    if constexpr (kDrained) asm volatile("s_waitcnt vmcnt(0)\n\t" DENSITY_ROT_MV16 : DENSITY_ROT_EACH16("=v", q) : : DENSITY_ROT_STAGE16);
    else asm volatile("s_waitcnt vmcnt(16)\n\t" DENSITY_ROT_MV16 : DENSITY_ROT_EACH16("=v", q) : : DENSITY_ROT_STAGE16);
}

}  // namespace

// ---------------------------------------------------------------------------------------------------------------
// encode: Codec::encode / encode_block (codec/codec.rs:34-80), Chameleon::encode_quad (chameleon.rs:88-100)
// ---------------------------------------------------------------------------------------------------------------
// <kProf: cycle accounting (debug build), PAGED: the output is a paged container, SPLIT: 8 chain + 8 emit waves instead of 8 that do both>
template <bool kProf, bool PAGED = false, bool SPLIT = false>
__global__ __launch_bounds__(SPLIT ? 2 * kEncWaves * 64 : kEncWaves * 64) void chameleon_encode_rot(
    const uint8_t* __restrict__ in, uint64_t total, uint64_t chunk_bytes, uint8_t* __restrict__ out, uint64_t out_stride,
    uint64_t* __restrict__ sizes, uint8_t* __restrict__ index, uint32_t* __restrict__ err, SegArgs seg, uint64_t* __restrict__ prof) {
    constexpr int R = kEncRound, W = kEncWaves;                                   // blocks per round; waves a round rotates over (split: chain waves)
    constexpr uint32_t kThreads = SPLIT ? 2u * W * 64u : W * 64u;
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t wave = rfl(threadIdx.x >> 6);
    const uint64_t chunk = blockIdx.x;
    PhaseClock<kProf> clk(blockIdx.x == 0 ? prof : nullptr);   // phases: 0 hash, 1 D wait, 2 exchange, 3 signatures, 4 O wait + commit, 5 load wait, 6 emit, 7 in-order rounds
    const uint8_t* src = in + chunk * chunk_bytes;
    const uint64_t len = (total - chunk * chunk_bytes) < chunk_bytes ? (total - chunk * chunk_bytes) : chunk_bytes;
    // PAGED (round 5): no slot per chunk — `out` is page 0 of the container, stream positions are absolute offsets from it, and the stream moves to
    // a fresh page (one shared counter) whenever a round's records would not fit the rest of its page (below: page_place)
    uint8_t* dst = PAGED ? out : out + chunk * out_stride;
    uint8_t* idx = index ? index + chunk * (chunk_bytes / kBlock) : nullptr;     // this chunk's slice of the block index
    const uint32_t nfull = (uint32_t)(len / kBlock);                              // whole blocks (the launcher bounds len)
    const uint32_t nrounds = nfull / R;                                           // whole rounds: these rotate; the rest (< R blocks + a ragged one) is the epilogue
    uint32_t* dir = PAGED ? seg.page_dir + chunk * seg.page_dir_words : nullptr;   // this chunk's page directory
    // the table sits at LDS address 0 (this kernel has no static LDS): slot addresses need no base
    const uint32_t sy = kEncSync;
    const ZmapLds zmap{kEncZmap};

    {   // fresh state per chunk (chameleon.rs:45-48): zero table, zero-entry map, tokens: round 0 in slow mode, nothing committed
        // (a segment of a longer stream — SegArgs — starts from the dictionary image and FSM state it is given instead, and in
        // speculation mode if its predecessor ended calm)
        uint4* p = reinterpret_cast<uint4*>(smem);
        const uint4 z = make_uint4(0, 0, 0, 0);
        const uint4* image = seg.init_images ? reinterpret_cast<const uint4*>(seg.init_images + chunk * kSegImageBytes) : nullptr;
        for (uint32_t i = threadIdx.x; i < (kTableBytes + kZmapBytes) / 16; i += kThreads) p[i] = image ? image[i] : z;
        if (threadIdx.x == 0) {
            const uint32_t g0 = seg.init_guard ? seg.init_guard[chunk] : pack_guard(Guard{});
            uint32_t pos0 = 0;
            if (PAGED) {                                                          // this chunk's first page and its spare: {page base, stream bytes in earlier pages, spare page, pages so far}
                const uint32_t pg = atomicAdd(seg.page_counter, 2u);
                if (pg + 2u > seg.page_limit && err) atomicOr(err, 2u);           // (cannot happen: the launcher's bound is every chunk's worst case)
                pos0 = pg << kPageShift;
                *reinterpret_cast<uint4*>(smem + kEncSync + kSyPage) = make_uint4(pos0, 0u, pg + 1u, 1u);
                *reinterpret_cast<uint4*>(dir + 4) = make_uint4(pg, 0u, 0u, 0u);
            }
            *reinterpret_cast<uint4*>(smem + kEncSync + kSyD) = make_uint4((g0 >> 31) ? 0u : 1u, kNone, 0u, 0u);
            *reinterpret_cast<uint4*>(smem + kEncSync + kSyO) = make_uint4(0u, kNone, pos0, g0 & 0x7fffffffu);
            if (lds_addr(smem) != 0 && err) atomicOr(err, kErrWatchdog);           // (cannot happen: see above)
        }
        if (threadIdx.x < kMemoEntries) *reinterpret_cast<uint4*>(smem + kEncSync + kSyMemo + 16u * threadIdx.x) = make_uint4(kNone, 0u, 0u, 0u);
        if (SPLIT) {                                                              // ring words and mail boxes: nothing filled, nothing drained, nothing posted, nothing taken
            if (threadIdx.x < 2) *reinterpret_cast<uint4*>(smem + kEncRingSync + 16u * threadIdx.x) = z;
            if (threadIdx.x >= 64 && threadIdx.x < 64 + 16) *reinterpret_cast<uint4*>(smem + kEncMbox + kMboxBytes * ((threadIdx.x - 64) >> 1) + 128u + 16u * (threadIdx.x & 1u)) = z;
        }
    }
    __syncthreads();

    // 8 waves have 256 registers each: the quads stay in registers across the waits and the next round's are fetched a round ahead.
    // (split: a chain wave takes its quads from the ring and keeps them only up to the exchange operands — the rare paths that want them
    // again load them from L2 —, and the hash product is made again for the emit)
    uint32_t cur_round = 0;                                                       // (split: the round whose quads such a path loads)
    uint32_t q[R], hp[R];                                                         // hp: the quads' hash products (kept with them)
#pragma unroll
    for (uint32_t j = 0; j < R; ++j) hp[j] = 0;
    auto load_round = [&](uint32_t (&d)[R], uint32_t r) {
        if (r < nrounds) {
            const uint8_t* p = src + (uint64_t)r * (R * kBlock);
#pragma unroll
            for (uint32_t j = 0; j < R; ++j) d[j] = *reinterpret_cast<const uint32_t*>(p + j * kBlock + 4u * lane);
        }
    };
    // (split, rare paths of a chain wave: the round's quads again, unconditionally — a guarded load would keep the old values alive across the common path)
    // Every such path loads into an array of ITS OWN (one merged with `q` would have the compiler keep two sets of quads alive in the common path).
    auto reload_quads = [&](uint32_t (&t)[R], uint32_t r) {
        const uint8_t* p = src + (uint64_t)r * (R * kBlock);
#pragma unroll
        for (uint32_t j = 0; j < R; ++j) t[j] = *reinterpret_cast<const uint32_t*>(p + j * kBlock + 4u * lane);
    };
    // quad -> exchange operands {dword address, half mask, entry << 16*half} (chameleon.rs:89, chameleon_dev.hpp)
    auto operands = [&](uint32_t qv, uint32_t& a, uint32_t& m, uint32_t& v, uint32_t* keep = nullptr) {
        const uint32_t P = qv * kHashMul;
        if (keep) *keep = P;
        const uint32_t sh = (P >> 12) & 16u;                                      // (h & 1) << 4
        a = (P >> 15) & 0x1fffcu;                                                 // (h >> 1) << 2
        m = 0xffffu << sh;
        v = stored_entry(qv, P) << sh;
    };
    // one record (codec.rs:39-67, io/write_buffer.rs) or raw block (codec.rs:35-37) to its place in the stream
    auto emit_block = [&](uint8_t* rec, uint32_t qv, uint64_t sg, bool raw) {
        if (raw) {
            st32u(rec + 4u * lane, qv);
        } else {
            const uint32_t off = kSig + 4u * lane - 2u * mbcnt64(sg);
            if (lane < 2) st32u(rec + 4u * lane, lane ? (uint32_t)(sg >> 32) : (uint32_t)sg);   // codec.rs:24-26
            if ((sg >> lane) & 1ull) st16u(rec + off, (qv * kHashMul) >> 16); else st32u(rec + off, qv);
        }
    };
    // one block in order: FSM, then either a raw copy or the dictionary step with the zero-entry map (slow rounds, epilogue)
    // a register array parked in the staging area (array 0 or 1), and element j (wave-uniform, not a compile-time constant) of it:
    // what the rolled loops of the rare paths index instead of registers (a dynamically indexed register array would live in scratch
    // memory, whose loads the compiler waits for at the top of every round, common path included)
    auto park = [&](uint32_t which, const uint32_t (&a)[R]) {
        uint32_t base = kEncStage + which * 4096u + 4u * lane;
        asm volatile("" : "+v"(base));                                            // (made here, on the rare path: not an invariant of the round loop)
#pragma unroll
        for (uint32_t j = 0; j < R; ++j) DENSITY_LDS_POKE_AT(base, j * 256u, a[j]);
    };
    auto parked = [&](uint32_t which, uint32_t j) -> uint32_t { return lds_peek1(kEncStage + which * 4096u + j * 256u + 4u * lane); };
    auto block_in_order = [&](Guard& g, uint32_t qv, uint32_t& a, uint32_t m, uint32_t v, uint64_t& sg, bool& raw) {
        sg = 0;
        raw = g.block_is_copy();                                                  // codec.rs:35
        if (raw) { g.decay(); return; }
        const uint32_t old = exchange_block(a, m, v);
        a = old;                                                                  // (like the fast path: the answer replaces the address)
        const bool susp = v == 0 && qv != 0;                                       // stored entry 0 outside slot 0 (entry 0 in slot 0 is the zero quad)
        const uint32_t zbit = zmap_claim_in_order(zmap, susp, (qv * kHashMul) >> 16, lane);
        sg = ballot64(((old ^ v) & m) == 0 && (!susp || zbit));                    // chameleon.rs:90-99
        g.update((uint32_t)__builtin_popcountll(sg) <= 4u);                        // codec.rs:68: 8 + 256 - 2*hits >= 256
    };

    uint32_t ra[R], mask[R], val[R];                                              // per block: address, then (after the exchange) the answer; half mask; entry
#pragma unroll
    for (uint32_t j = 0; j < R; ++j) { q[j] = 0; ra[j] = 0; mask[j] = 0; val[j] = 0; }
    // The records of a round without raw blocks, straight-line: the signatures and the index bytes leave from lanes 0..R-1 in one
    // store each (lane j: record j, offsets by a DPP prefix over the record lengths); per block the MAP lanes store the 2-byte slot
    // index (the upper half of the hash product), the PLAIN lanes the quad, through an SGPR base (io/write_buffer.rs:13-27).
    const uint32_t minus_2lane = 0u - 2u * lane;
    auto emit_round_coded = [&](const uint32_t (&qq)[R], uint32_t pos0, uint8_t* idxp, uint32_t slo, uint32_t shi) {
        const uint32_t nhv = (uint32_t)(__builtin_popcount(slo) + __builtin_popcount(shi));
        const uint32_t lenv = kSig + kBlock - 2u * nhv;
        uint32_t incl = lenv;                                                                 // prefix within a row of 16 lanes
        incl += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)incl, 0x111, 0xf, 0xf, true);   // row_shr:1
        incl += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)incl, 0x112, 0xf, 0xf, true);   // row_shr:2
        incl += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)incl, 0x114, 0xf, 0xf, true);   // row_shr:4
        incl += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)incl, 0x118, 0xf, 0xf, true);   // row_shr:8
        const uint32_t posv = pos0 + incl - lenv;                                                 // lane j: where record j starts
        if (lane < R) {
            *reinterpret_cast<u32x2_u*>(dst + posv) = u32x2{slo, shi};                             // codec.rs:24-26
            if (idxp) idxp[lane] = (uint8_t)nhv;
        }
        const uint32_t itemsv = posv + kSig;                                                      // lane j: where record j's items start
        // ONE store per record: every lane writes four bytes at its item's place — a PLAIN lane its quad, a MAP lane its 16-bit hash and, behind
        // it, the two bytes that FOLLOW its item in the stream: the first two of the next lane's item, or (lane 63) of the next record's
        // signature.  Neighbours then write the same bytes twice, with the same values.  (A second, 2-byte store for the MAP lanes cost the
        // texture path as much as the first: the encoder was 13 % faster without it.)  Only the round's last record, whose successor is
        // another wave's, keeps two masked stores.
#pragma unroll
        for (uint32_t j = 0; j < R; ++j) {
            const uint64_t sg = ((uint64_t)rlane_u(shi, (int)j) << 32) | rlane_u(slo, (int)j);
            const uint64_t plain = ~sg;
            const uint32_t pos = rlane_u(itemsv, (int)j);                         // (one read instead of a scalar running sum: popcount, shift, subtract, add)
            // the item's place: 4*lane - 2*(MAP lanes below) from the record's items on — the signature itself is the mask that is counted (no
            // complement to make), the count seeded with -2*lane, times -2 and added in one instruction
            const uint32_t P = !SPLIT ? hp[j] : qq[j] * kHashMul;              // (the hash is the MAP item: chameleon.rs:92)
            if (j + 1 < R) {
                const uint32_t nsig = rlane_u(slo, (int)j + 1);                    // the next record's first bytes: its signature's low word
                uint32_t val, off;
                asm volatile(
                    "s_mov_b64 vcc, %[sg]\n\t"
                    // an item's first two bytes: MAP the hash, PLAIN the quad's low half
                    "v_cndmask_b32_sdwa %[v], %[q], %[P], vcc dst_sel:DWORD dst_unused:UNUSED_PAD src0_sel:WORD_0 src1_sel:WORD_1\n\t"
                    "v_mbcnt_lo_u32_b32 %[o], %[sl], %[ln]\n\t"                        // MAP lanes below - 2 * lane (the count seeded with -2 * lane) ...
                    "v_mbcnt_hi_u32_b32 %[o], %[sh], %[o]\n\t"                        // (two instructions between the select and the lane shift that reads it: the wait states a DPP source needs)
                    "v_mov_b32_dpp %[v], %[v] wave_shl:1 row_mask:0xf bank_mask:0xf\n\t"   // ... of the NEXT lane's item (lane 63: replaced below)
                    "v_mad_i32_i24 %[o], %[o], -2, %[pos]\n\t"                        // ... times -2, from the record's items on: 4 * lane - 2 * (MAP lanes below)
                    "v_writelane_b32 %[v], %[ns], 63\n\t"
                    "v_perm_b32 %[v], %[v], %[P], %[sel]\n\t"                         // hash | following bytes << 16
                    "v_cndmask_b32 %[v], %[q], %[v], vcc\n\t"                         // PLAIN lanes: the quad
                    "global_store_dword %[o], %[v], %[dst]"
                    : [v] "=&v"(val), [o] "=&v"(off)
                    : [P] "v"(P), [q] "v"(qq[j]), [sg] "s"(sg), [sl] "s"((uint32_t)sg), [sh] "s"((uint32_t)(sg >> 32)), [ln] "v"(minus_2lane), [pos] "s"(pos),
                      [ns] "s"(nsig), [sel] "s"(0x05040302u), [dst] "s"(dst)
                    : "memory", "vcc");
            } else {
                const uint32_t off = pos + 2u * __builtin_amdgcn_mbcnt_hi((uint32_t)(plain >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)plain, lane));
                asm volatile(
                    // (an SGPR a VALU instruction has just written — the compiler reloading a spilled base — needs 5 wait states
                    // before a memory instruction reads it: its own code sees to that, an asm statement must)
                    "s_nop 4\n\t"
                    "s_mov_b64 exec, %4\n\t"
                    "global_store_dword %0, %2, %3\n\t"
                    "s_not_b64 exec, exec\n\t"
                    "global_store_short_d16_hi %0, %1, %3\n\t"
                    "s_mov_b64 exec, -1"
                    ::"v"(off), "v"(P), "v"(qq[j]), "s"(dst), "s"(plain) : "memory", "scc");
            }
            __builtin_amdgcn_sched_barrier(0);
        }
    };

    // undo the exchanges of this wave's round, last block first: the lowest lane of a slot holds the pre-block entry, so the
    // answers go back lane-reversed in ONE ds_write_b16 per block (ascending lane service order: the highest physical lane =
    // the lowest original lane wins)
    // (`skip`: blocks of the round that exchanged nothing — the raw copies an ordered round predicted, below)
    auto rollback_round = [&](uint32_t skip = 0u) {
        if constexpr (SPLIT) { uint32_t t[R]; reload_quads(t, cur_round); park(0, t); } else park(0, q);
        park(1, ra);                                                  // (a rolled loop: this path is rare, its code must not weigh on the common one)
#pragma nounroll
        for (int j = (int)R - 1; j >= 0; --j) {
            if ((skip >> j) & 1u) continue;
            const uint32_t P = parked(0, (uint32_t)j) * kHashMul, srj = parked(1, (uint32_t)j);
            const uint32_t hi = (P >> 16) & 1u;                                    // 1: the slot is the upper half of its dword
            const uint32_t a16 = ((P >> 15) & 0x1fffcu) + 2u * hi;
            const uint32_t prev = hi ? (srj >> 16) : (srj & 0xffffu);
            const uint32_t ar = bperm(63u - lane, a16), pr = bperm(63u - lane, prev);
            dict_store(ar, pr);
        }
    };
    // Abort protocol (all 16 waves; `holding`: this wave has exchanged `hold_round` and not committed it).  After the first
    // barrier nobody is inside a critical section, D says how far the dictionary got (rounds < d exchanged), A which round
    // failed; rounds d-1 .. A are rolled back one per barrier step by their owners, then the chain restarts at A in slow mode.
    uint32_t hold_skip = 0;                                                       // blocks of the round this wave holds that exchanged nothing (a run-ahead round's predicted raw copies)
    auto abort_sync = [&](bool holding, uint32_t hold_round) {
        wg_barrier();
        const u32x2 v = lds_peek2(sy + kSyD);
        const uint32_t d = rfl(v.x) >> 1, a = rfl(v.y);
        for (uint32_t x = d; x-- > a;) {
            if (holding && hold_round == x) rollback_round(hold_skip);
            wg_barrier();
        }
        if (wave == a % W && lane == 0) {
            lds_poke(sy + kSyD + 12, 0u);                                         // (no run-ahead behind an abort: the restarted round waits for its payload)
            lds_poke(sy + kSyD, (a << 1) | 1u);
            lds_poke(sy + kSyD + 4, kNone);
            lds_poke(sy + kSyO + 4, kNone);
        }
        wg_barrier();
    };

    // PAGED: where a round of `need` bytes goes whose turn it is at stream position `pos` — there, if it ends INSIDE the page (strictly: a position on
    // a page boundary is then always a fresh page's start), else at the start of the spare page, which becomes the stream's page (io/write_buffer.rs:
    // 29-31's running total moves on in the directory instead: bytes used per page).  Called by the holder of the commit token only; `refill`: the
    // spare was taken, a new one is fetched once the tokens have been passed on.
    bool refill = false;
    auto page_place = [&](uint32_t pos, uint32_t need, uint32_t first_block) -> uint32_t {
        if (__builtin_expect((pos & (kPageBytes - 1u)) + need < kPageBytes, 1)) return pos;
        const u32x4 st = lds_peek4(sy + kSyPage);
        const uint32_t base = rfl(st.x), before = rfl(st.y), count = rfl(st.w);
        uint32_t spare = rfl(st.z);
        if (spare == kNone) spare = rfl(lane == 0 ? atomicAdd(seg.page_counter, 1u) : 0u);          // (the refill has not come back yet: rare)
        if (spare >= seg.page_limit) { if (err && lane == 0) atomicOr(err, 2u); spare = seg.page_limit - 1u; }   // (cannot happen, see above; never write past the output)
        if (lane == 0) {
            dir[4u * count + 2u] = pos - base;                                    // bytes of stream in the page that is left
            *reinterpret_cast<uint4*>(dir + 4u * (count + 1u)) = make_uint4(spare, first_block, 0u, 0u);
            const u32x4 v = {spare << kPageShift, before + (pos - base), kNone, count + 1u};
            asm volatile("ds_write_b128 %0, %1" ::"v"(sy + kSyPage), "v"(v) : "memory");
        }
        // a new spare only if the stream is LIKELY to outgrow this page: what is left of the chunk at the bytes per block the stream has had so far, and
        // an eighth on top.  The last page of a chunk mostly needs none, and a spare nobody uses is 64 KiB of the container (one per chunk until round 6:
        // 2.4 % of the headline blob).  If the guess is wrong the next change of pages takes its page from the counter itself (above: spare == kNone).
        refill = (uint64_t)(nfull - first_block + 1u) * (before + (pos - base)) * 9u >= (uint64_t)first_block * (8u * kPageBytes);
        return spare << kPageShift;
    };
    auto page_refill = [&]() {
        if (lane == 0) { const uint32_t pg = atomicAdd(seg.page_counter, 1u); lds_poke(sy + kSyPage + 8u, pg); }
        refill = false;
    };
    // (the last whole round also keeps room for what follows it on one wave: the blocks of the partial round and the ragged block — so that no page
    // starts inside the decoder's in-order tail)
    const uint32_t tail_need = PAGED ? (nfull - nrounds * R + 1u) * (kSig + kBlock) : 0u;
    // ---- SPLIT: the ring and the mail boxes (constants above) ----
    // Every spin of either role looks for a raised abort — the work-group barrier of the protocol counts all sixteen waves; an emit wave never holds an
    // uncommitted round, a chain wave none at these places — and for the watchdog's poison.
    auto join_abort = [&]() {
        const u32x2 v = lds_peek2(sy + kSyD);
        const uint32_t A = rfl(v.y);
        if (__builtin_expect(A != kNone, 0)) { if (A == kPoison) wave_exit(); abort_sync(false, 0); }
    };
    // chain wave: round r's quads out of the ring (its LDS reads execute in issue order: whoever sees the `freed` word may overwrite the slot)
    auto ring_take = [&](uint32_t (&d)[R], uint32_t r) {
        const uint32_t slot = r % kRingSlots;
        for (uint32_t spins = 0; !poll_word(kEncRingSync + 4u * slot, r + 1u, 4);) { join_abort(); __builtin_amdgcn_s_sleep(1); watchdog(spins, sy, err, lane); }
        clk.mark(5);
        const uint32_t at = kEncRing + slot * kSlotBytes + 4u * lane;
        // (one statement, issue to wait: an answer of an asynchronous LDS read exists for the compiler only when the statement ends)
        asm volatile("ds_read_b32 %0, %16 offset:0\n\t"
                     "ds_read_b32 %1, %16 offset:256\n\t"
                     "ds_read_b32 %2, %16 offset:512\n\t"
                     "ds_read_b32 %3, %16 offset:768\n\t"
                     "ds_read_b32 %4, %16 offset:1024\n\t"
                     "ds_read_b32 %5, %16 offset:1280\n\t"
                     "ds_read_b32 %6, %16 offset:1536\n\t"
                     "ds_read_b32 %7, %16 offset:1792\n\t"
                     "ds_read_b32 %8, %16 offset:2048\n\t"
                     "ds_read_b32 %9, %16 offset:2304\n\t"
                     "ds_read_b32 %10, %16 offset:2560\n\t"
                     "ds_read_b32 %11, %16 offset:2816\n\t"
                     "ds_read_b32 %12, %16 offset:3072\n\t"
                     "ds_read_b32 %13, %16 offset:3328\n\t"
                     "ds_read_b32 %14, %16 offset:3584\n\t"
                     "ds_read_b32 %15, %16 offset:3840\n\t"
                     "s_waitcnt lgkmcnt(0)"
                     : DENSITY_ROT_EACH16("=&v", d)
                     : "v"(at) : "memory");
        if (lane == 0) lds_poke(kEncRingSync + 16u + 4u * slot, r + 1u);
    };
    // emit wave: round r's quads into the ring, once the chain wave of round r - kRingSlots has drained the slot
    auto ring_put = [&](const uint32_t (&d)[R], uint32_t r) {
        const uint32_t slot = r % kRingSlots;
        // (this wave is idle most of a round — it waits here for about five hand-offs of the chain —: long naps at the lowest priority, so that its
        // polls take neither LDS cycles from the exchanges nor issue slots from the waves it waits for)
        if (r >= kRingSlots) {
            __builtin_amdgcn_s_setprio(0);
            for (uint32_t spins = 0; !poll_word(kEncRingSync + 16u + 4u * slot, r + 1u - kRingSlots, 1);) { join_abort(); __builtin_amdgcn_s_sleep(12); watchdog(spins, sy, err, lane); }
            __builtin_amdgcn_s_setprio(1);
        }
        const uint32_t base = kEncRing + slot * kSlotBytes + 4u * lane;
#pragma unroll
        for (uint32_t j = 0; j < R; ++j) DENSITY_LDS_POKE_AT(base, j * 256u, d[j]);
        if (lane == 0) lds_poke(kEncRingSync + 4u * slot, r + 1u);
    };
    // chain wave `wave`, round r committed: its signatures and stream position to the partner (`skip`: the chain wave wrote the round out itself —
    // rounds with raw-copy blocks); the box is free once the partner has taken the pair's previous round
    auto mbox_post = [&](uint32_t r, uint32_t pos, uint32_t lo, uint32_t hi, uint32_t skip) {
        const uint32_t mb = kEncMbox + kMboxBytes * wave;
        if (r >= (uint32_t)W)
            for (uint32_t spins = 0; !poll_word(mb + 144u, r + 1u - W, 2);) { join_abort(); __builtin_amdgcn_s_sleep(1); watchdog(spins, sy, err, lane); }
        if (lane < R) lds_poke2(mb + 8u * lane, lo, hi);
        if (lane == 0) { lds_poke(mb + 132u, pos); lds_poke(mb + 128u, ((r + 1u) << 1) | skip); }
    };
    auto mbox_wait = [&](uint32_t e, uint32_t r, uint32_t& pos, uint32_t& lo, uint32_t& hi) -> bool {
        const uint32_t mb = kEncMbox + kMboxBytes * e;
        uint32_t seq;
        __builtin_amdgcn_s_setprio(0);
        for (uint32_t spins = 0;;) {
            seq = rfl(lds_peek1(mb + 128u));
            if ((seq >> 1) == r + 1u) break;
            join_abort(); __builtin_amdgcn_s_sleep(6); watchdog(spins, sy, err, lane);
        }
        __builtin_amdgcn_s_setprio(1);
        pos = rfl(lds_peek1(mb + 132u));
        const u32x2 sg = lds_peek2(mb + 8u * (lane < R ? lane : 0u));
        lo = lane < R ? sg.x : 0u; hi = lane < R ? sg.y : 0u;
        if (lane == 0) lds_poke(mb + 144u, r + 1u);
        return (seq & 1u) != 0;
    };
    if (SPLIT && wave >= (uint32_t)W) {
        // ---- emit wave e: loads the rounds e, e + 8, ..., hands their quads to the chain wave e through the ring — a round ahead of the one it is
        // about to write out — and writes a round's records once the chain wave has committed it (mail box).  Three register sets: the round waiting
        // for its commit, the next one (on its way into the ring) and the one after that, whose loads are issued BEFORE the wait for the commit and
        // the emit, so that their latency lies under both.
        // The memory queue and the compiler: its bookkeeping cannot see the record stores (issued inside asm statements) and is conservative across
        // the loop's edge, so a wait it places for a LOAD also waits for stores it does not know of.  Inside the emit that was ruinous (measured:
        // 4600 instead of 2600 cycles per round — from the ninth record on, every record waited for the acknowledgement of an older record's store),
        // so the quads are "laundered" once they have landed: an empty statement that redefines them, after which the compiler attaches no pending
        // load to them and the emit runs without a wait.  What is left is one over-long wait per round, in front of the ring transfer (the loads it
        // waits for were issued before the last emit's stores: it sits that emit's stores out too), where this wave has slack.  (Loads issued by hand,
        // out of the compiler's sight, were tried: it copies the "defined" registers at the loop's edge before they have landed — tools/check_isa.py
        // finds such copies.)
        // Priority 1 like a chain wave that hashes: below the chain's critical steps (2, 3), above the waves that only poll for this one's work (0).
        __builtin_amdgcn_s_setprio(1);
        const uint32_t e = wave - W;
        auto launder = [&](uint32_t (&d)[R]) {
#pragma unroll
            for (uint32_t j = 0; j < R; ++j) asm volatile("" : "+v"(d[j]));
        };
        uint32_t qa[R], qb[R], qc[R];
#pragma unroll
        for (uint32_t j = 0; j < R; ++j) { qa[j] = 0; qb[j] = 0; qc[j] = 0; }
        load_round(qa, e);
        if (e < nrounds) ring_put(qa, e);
        launder(qa);
        load_round(qb, e + W);
        auto step = [&](uint32_t (&cur)[R], uint32_t (&nxt)[R], uint32_t (&fut)[R], uint32_t r) {
            clk.start();
            if (r + W < nrounds) ring_put(nxt, r + W);
            launder(nxt);
            clk.mark(1);
            load_round(fut, r + 2u * W);
            uint32_t pos, lo, hi;
            const bool skip = mbox_wait(e, r, pos, lo, hi);
            clk.mark(4);
            if (!skip) emit_round_coded(cur, pos, idx ? idx + (uint64_t)r * R : nullptr, lo, hi);
            clk.mark(6);
        };
        for (uint32_t r = e; r < nrounds; r += 3u * W) {
            step(qa, qb, qc, r);
            if (r + W < nrounds) step(qb, qc, qa, r + W);
            if (r + 2u * W < nrounds) step(qc, qa, qb, r + 2u * W);
        }
    } else {
    if constexpr (!SPLIT) {
        // (by hand like every later fetch: a load the compiler can see ahead of the loop would make it wait, at the top of every
        // iteration, until all but a few of the previous round's record stores have been acknowledged)
        if (wave < nrounds) { prefetch_quads(src + (uint64_t)wave * (R * kBlock) + 4u * lane); quads_landed<true>(q); }
    }
    uint32_t poll_tries = 16;                                                     // polls for the FAST token before a look at the whole D line: few while this wave's rounds are ordered ones
    for (uint32_t r = wave; r < nrounds; r += W) {
        clk.start();
        __builtin_amdgcn_s_setprio(1);                                   // (see the priorities note at the exchange)
        if (SPLIT) { cur_round = r; ring_take(q, r); clk.mark(7); }
        uint32_t slo = 0, shi = 0;                                                // lane j: the signature of block j (codec.rs:24-26)
        uint32_t copy_mask = 0, opos = 0;
        bool fast_commit = false, prefetched = false;
        // an ORDERED round (below): its commit payload, and how far it is final — blocks below it_j0, the FSM state in front of it_j0, the raw-copy
        // blocks (final below it_j0, predicted from there on), the prediction and the state behind the round if it holds
        uint32_t P0 = 0, P1 = 0, it_j0 = kNone, it_state = 0, it_raw = 0, it_mode = 0, it_end = 0;
        bool have_turn = false, ahead = false;
        hold_skip = 0;
      // (re-entered after an abort, and by an ordered round whose prediction failed: the answers have replaced the addresses, so the
      // operands are made again)
      for (bool reentered = false;; reentered = true) {
        uint32_t zblocks = 0, zq = 0;
        bool zsusp = false;
        auto prepare = [&](const uint32_t (&qq)[R]) {
        uint32_t zmin = 0xffffffffu;
#pragma unroll
        for (uint32_t j = 0; j < R; ++j) {
            operands(qq[j], ra[j], mask[j], val[j], !SPLIT ? &hp[j] : nullptr);
            zmin = val[j] < zmin ? val[j] : zmin;
            __builtin_amdgcn_sched_barrier(0);                                    // block by block: short live ranges, not maximal overlap
        }
        // Blocks with a quad that needs the zero-entry map (about one quad in 64 Ki): found here, ahead of the waits, together with the
        // first such block's quads, so that the commit — which holds up every later round — has next to nothing left to look up.
        if (__builtin_expect(ballot64(zmin == 0) != 0, 0)) {                      // a stored entry 0: the zero quad (harmless) or one outside slot 0
            asm volatile("");                                                     // (nothing of this block is worth computing ahead of the test: sixteen compares of the common path otherwise)
#pragma unroll
            for (uint32_t j = 0; j < R; ++j) zblocks |= (ballot64(val[j] == 0 && qq[j] != 0) != 0 ? 1u : 0u) << j;
            if (zblocks) {
                const uint32_t j0 = (uint32_t)__builtin_ctz(zblocks);
                zq = pick<R>(qq, j0);
                zsusp = pick<R>(val, j0) == 0 && zq != 0;
            }
        }
        };
        if (SPLIT && reentered) reload_quads(q, r);
        prepare(q);
        const bool zero_round = zblocks != 0;
        uint32_t tokaddr = lane == 0 ? sy + kSyD : sy + kSySink + 4u * lane;
        uint32_t tokval = (r + 1u) << 1;                                          // (in its register before the wait, like the operands)
        asm volatile("" : "+v"(tokval));
        pin_operands<R>(ra, mask, val);                                           // complete before the wait for the token

        clk.mark(0);
        clk.stamp(r, 0, lane);
        __builtin_amdgcn_s_setprio(2);
        {
            // ---- D chain: wait for this round's turn ----
            uint32_t slow = 1, dS = 0, dF = 0;                                    // dS, dF: the D line's run-ahead words (below: ordered rounds that run ahead)
            bool got_payload = false;
            // (the memo of FSM predictions as it stands now, read AHEAD of the wait: inside a stretch its entries are stable, and the look-up behind the
            // token is then a compare instead of an LDS round trip — 200 cycles of every run-ahead hop; a miss reads it again)
            u32x4 memo_early = {kNone, 0u, 0u, 0u};
            if (poll_tries != 16 && !have_turn) memo_early = lds_peek4(sy + kSyMemo + 16u * (lane & (kMemoEntries - 1u)));
            if (!have_turn)
            for (uint32_t spins = 0;;) {
                if (poll_tries != 16) {
                    // this wave's last round was an ordered one: most likely this one is too, and then it needs the commit payload as well —
                    // the D line and the O line in one look instead of one after the other (behind a few tight polls for this round's slow token:
                    // a round that runs ahead is handed over like a fast one, and the two-line look alone found it 775 cycles late)
                    // (first a few tight polls of the D line for this round's slow token — a round that runs ahead is handed over like a fast one, every
                    // LDS round trip on the way is 200 cycles of the hop: the line's run-ahead words come with the token)
                    {
                        u32x4 dl1;
                        if (poll_line(sy + kSyD, (r << 1) | 1u, 8, dl1) && rfl(dl1.y) == kNone) { slow = 1; dS = rfl(dl1.z); dF = rfl(dl1.w); break; }
                    }
                    u32x4 dl, ol;
                    lds_peek4x2(sy + kSyD, dl, ol);
                    const uint32_t D = rfl(dl.x), A = rfl(dl.y);
                    if (__builtin_expect(A != kNone, 0)) { if (A == kPoison) wave_exit(); abort_sync(false, 0); continue; }
                    if ((D >> 1) == r) {
                        slow = D & 1u; dS = rfl(dl.z); dF = rfl(dl.w);
                        if (slow && rfl(ol.x) == r) { P0 = rfl(ol.z); P1 = rfl(ol.w); got_payload = true; }
                        break;
                    }
                    if (D & 1u) backoff_ordered(r - (D >> 1)); else backoff(r - (D >> 1));
                    watchdog(spins, sy, err, lane);
                    continue;
                }
                if (poll_word(sy + kSyD, r << 1, 16)) { slow = 0; break; }         // the common hand-off: fast token for this round
                const u32x4 v = lds_peek4(sy + kSyD);
                const uint32_t D = rfl(v.x), A = rfl(v.y);
                if (__builtin_expect(A != kNone, 0)) { if (A == kPoison) wave_exit(); abort_sync(false, 0); continue; }
                if ((D >> 1) == r) { slow = D & 1u; dS = rfl(v.z); dF = rfl(v.w); break; }
                backoff(r - (D >> 1));
                watchdog(spins, sy, err, lane);
            }
            clk.mark(1);
            clk.stamp(r, 1, lane);
            if (__builtin_expect(!slow, 1)) {
                // ---- fast round: R speculative exchanges, token passed behind them ----
                // Priorities: the SIMD's arbiter prefers, at equal priority, the wave that was launched first, which leaves the last-launched
                // wave of each SIMD short of issue slots and late for its turns.  So a wave's priority follows its deadline instead: 3
                // inside the exchanges, 2 on the way to the commit and while it waits for a token, 1 while it prepares its next round, 0
                // while it writes records out (nobody waits for those).
                __builtin_amdgcn_s_setprio(3);
                exchange_tied16(ra, mask, val, tokaddr, tokval);
                __builtin_amdgcn_s_setprio(2);
                clk.mark(2);
                clk.stamp(r, 2, lane);
                // the next round's quads are asked for HERE, a signature pass and a commit wait earlier than behind the commit (their latency
                // under load is of the order of a whole emit; 2 % faster than behind it); once per round, whatever becomes of it (an abort
                // re-enters the loop)
                if constexpr (!SPLIT)
                    if (!prefetched && r + W < nrounds) { prefetch_quads(src + (uint64_t)(r + W) * (R * kBlock) + 4u * lane); prefetched = true; }
                // The signatures (chameleon.rs:90-99: MAP flag = 1 iff the slot held this quad), block j's into lane j of slo / shi.  gfx950: an SGPR
                // written by a VALU instruction — the compare — needs 2 wait states before a VALU instruction — the lane write — reads it, which the
                // compiler sees to in its own code but not inside an asm statement: so block j's two lane writes go out behind block j + 1's compare
                // (and block j's own: three instructions in between), four instructions per block with no idle one.
                uint64_t sgp;
                {
                    const uint32_t x0 = (ra[0] ^ val[0]) & mask[0];
                    asm volatile("v_cmp_eq_u32_e64 %0, 0, %1" : "=s"(sgp) : "v"(x0));
                }
#pragma unroll
                for (uint32_t j = 1; j < R; ++j) {
                    const uint32_t xj = (ra[j] ^ val[j]) & mask[j];
                    uint64_t sgn;
                    if (j == 1) {                                                 // (block 0's compare has no lane writes behind it: one idle state)
                        asm volatile("v_cmp_eq_u32_e64 %2, 0, %3\n\ts_nop 0\n\tv_writelane_b32 %0, %4, %6\n\tv_writelane_b32 %1, %5, %6"
                                     : "+v"(slo), "+v"(shi), "=&s"(sgn) : "v"(xj), "s"((uint32_t)sgp), "s"((uint32_t)(sgp >> 32)), "n"(0));
                    } else {
                        asm volatile("v_cmp_eq_u32_e64 %2, 0, %3\n\tv_writelane_b32 %0, %4, %6\n\tv_writelane_b32 %1, %5, %6"
                                     : "+v"(slo), "+v"(shi), "=&s"(sgn) : "v"(xj), "s"((uint32_t)sgp), "s"((uint32_t)(sgp >> 32)), "n"(j - 1));
                    }
                    sgp = sgn;
                }
                asm volatile("s_nop 1\n\tv_writelane_b32 %0, %2, %4\n\tv_writelane_b32 %1, %3, %4" : "+v"(slo), "+v"(shi) : "s"((uint32_t)sgp), "s"((uint32_t)(sgp >> 32)), "n"(R - 1));
                // everything the commit needs that does not depend on the token: incompressible records (codec.rs:68: 8 + 256 - 2*hits >= 256) and the
                // bytes of the round — a sum over the lanes' record lengths instead of a scalar count and add per block
                const uint32_t nhv = (uint32_t)(__builtin_popcount(slo) + __builtin_popcount(shi));
                uint32_t inc = (uint32_t)ballot64(lane < R && nhv <= 4u);
                uint32_t sum;
                {
                    uint32_t acc = kSig + kBlock - 2u * nhv;                                              // (lanes >= R hold no signature: their slo / shi are 0, and they are not summed)
                    acc += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)acc, 0x111, 0xf, 0xf, true);     // row_shr:1
                    acc += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)acc, 0x112, 0xf, 0xf, true);     // row_shr:2
                    acc += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)acc, 0x114, 0xf, 0xf, true);     // row_shr:4
                    acc += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)acc, 0x118, 0xf, 0xf, true);             // row_shr:8
                    sum = rlane_u(acc, (int)R - 1);
                }
                uint32_t hits = 0;                                                                        // (only the rare zero-entry path below wants the count itself)
                // computed HERE: left to itself the compiler sinks both — and the 16 signatures they need — below the token wait,
                // into the commit
                asm volatile("" : "+s"(inc), "+s"(sum));
                clk.mark(3);
                // ---- O chain: commit ----
                bool aborted = false;
                for (uint32_t spins = 0;;) {
                    u32x4 v = lds_peek4(sy + kSyO);
                    for (uint32_t i = 0; i < 16 && rfl(v.x) != r; ++i) v = lds_peek4(sy + kSyO);   // token and payload in one read
                    const uint32_t O = rfl(v.x), A = rfl(v.y);
                    if (O == r) { P0 = rfl(v.z); P1 = rfl(v.w); break; }
                    if (__builtin_expect(A != kNone, 0)) { if (A == kPoison) wave_exit(); abort_sync(true, r); aborted = true; break; }
                    backoff(r - O);
                    watchdog(spins, sy, err, lane);
                }
                if (aborted) continue;
                // Zero-entry map, in stream order (this wave holds the commit token): every quad whose stored entry is 0 outside slot 0 marks
                // its slot; its MAP flag — the slot read 0 — stands only if the slot had been marked before, i.e. really held this entry
                // and not just never anything.  `flipped`: the marks this round set itself (taken back if the round is rolled back).
                uint32_t flipped = 0;
                if (__builtin_expect(zero_round, 0)) {
                    uint32_t qz_[R];
                    if constexpr (SPLIT) reload_quads(qz_, r);
                    const uint32_t (&qz)[R] = *(SPLIT ? &qz_ : &q);
                    clk.note(r, 1, lane);
                    hits = (R * (kSig + kBlock) - sum) >> 1;
                    bool first = true;
                    for (uint32_t zb = zblocks; zb; zb &= zb - 1u, first = false) {
                        const uint32_t j = (uint32_t)__builtin_ctz(zb);
                        const uint32_t qv = first ? zq : pick<R>(qz, j);
                        const bool susp = first ? zsusp : (pick<R>(val, j) == 0 && qv != 0);
                        const uint32_t zbit = zmap_claim_in_order(zmap, susp, (qv * kHashMul) >> 16, lane);
                        flipped |= (susp && !zbit ? 1u : 0u) << j;
                        const uint64_t sg = ((uint64_t)rlane(shi, j) << 32) | rlane(slo, j);
                        const uint64_t lost = ballot64(susp && !zbit) & sg;
                        slo = lane == j ? (uint32_t)(sg & ~lost) : slo;
                        shi = lane == j ? (uint32_t)((sg & ~lost) >> 32) : shi;
                        hits -= (uint32_t)__builtin_popcountll(lost);
                    }
                    inc = (uint32_t)ballot64(lane < R && (uint32_t)(__builtin_popcount(slo) + __builtin_popcount(shi)) <= 4u);
                    sum = R * (kSig + kBlock) - 2u * hits;
                }
                // which blocks the FSM would have turned into raw copies: block j+1 iff inc[j] && prev[j] (protection_state.rs:38-47)
                const uint32_t t = inc & ((inc << 1) | ((P1 >> 16) & 1u));
                if (__builtin_expect((P1 & 0xffu) != 0 || (t & ((1u << (R - 1)) - 1u)) != 0, 0)) {
                    if (ballot64(flipped != 0)) {
                        uint32_t qz_[R];
                        if constexpr (SPLIT) reload_quads(qz_, r);
                        const uint32_t (&qz)[R] = *(SPLIT ? &qz_ : &q);
                        for (uint32_t zb = zblocks; zb; zb &= zb - 1u) {
                            const uint32_t j = (uint32_t)__builtin_ctz(zb);
                            if ((flipped >> j) & 1u) zmap.clear((pick<R>(qz, j) * kHashMul) >> 16);
                        }
                    }
                    // (the chunk's abort count, for the ordered rounds' patience: this wave holds the commit token, the payload is its to amend)
                    if (lane == 0) { lds_poke(sy + kSyO + 12, ((P1 >> 24) & 3u) < 3u ? P1 + 0x01000000u : P1); lds_poke(sy + kSyD + 4, r); lds_poke(sy + kSyO + 4, r); }
                    clk.count(4, lane);
                    abort_sync(true, r);
                    continue;
                }
                uint32_t g_out;
                if (__builtin_expect((P1 & 0x1ffffu) == 0 && inc == 0, 1)) {
                    // calm, start == 1: only the block counter moves (and no incompressible stretch is running: its count, bits
                    // 26..28, goes)
                    g_out = (P1 & 0xe3e1ffffu) | ((((P1 >> 17) + R) & 15u) << 17);
                } else {
                    Guard g = unpack_guard(P1);
#pragma unroll
                    for (uint32_t j = 0; j < R; ++j) (void)g.block_is_copy();        // no block was a copy: bookkeeping only (:19-27)
                    g.penalty = ((t >> (R - 1)) & 1u) ? g.start : 0u;
                    g.prev = (inc >> (R - 1)) & 1u;
                    g_out = pack_guard(g) | (P1 & 0x03000000u);
                }
                opos = PAGED ? page_place(P0, sum + (r + 1u == nrounds ? tail_need : 0u), r * R) : P0;
                if (lane == 0) {
                    lds_poke2(sy + kSyO + 8, opos + sum, g_out);
                    lds_poke(sy + kSyO, r + 1u);
                }
                copy_mask = 0;
                __builtin_amdgcn_s_setprio(0);
                fast_commit = true;
                if (PAGED && refill) page_refill();
                // (next round's quads, unless asked for already: in flight behind the commit, landed by the end of the emit)
                if constexpr (!SPLIT) if (!prefetched && r + W < nrounds) prefetch_quads(src + (uint64_t)(r + W) * (R * kBlock) + 4u * lane);
                clk.mark(4);
                clk.count(0, lane);
                poll_tries = 16;
                break;
            }
            // ---- ordered round (round 5): everything before it is final first, then the round in batches ----
            // A round behind an abort or behind unrest does not speculate ACROSS rounds: it waits for its commit payload, so the FSM state at its
            // first block is known.  INSIDE the round the raw-copy blocks are predicted — calm state: none; inside an incompressible stretch
            // (penalty running, or the last coded block incompressible): every coded block incompressible, which makes the FSM a function of its
            // state alone (protection_state.rs:19-47) —, the blocks predicted coded exchange in one go like a fast round's, and the FSM walked over
            // the signatures they produce must arrive at the predicted raw blocks: by induction, block by block, the round is then exactly the
            // sequential one.  Where it does not — block jm — everything below jm IS final; this wave takes back its exchanges from jm on (nobody
            // has seen them: the dictionary token leaves only with the commit), predicts again from the exact state at jm — the other way round:
            // a raw copy where none was expected starts an incompressible stretch, a coded block where a copy was expected ends one — and
            // exchanges the rest of the round again; jm only grows.  No barrier, no other wave involved: data that flips between compressible and
            // incompressible every few KiB costs a round a second batch, not an abort of the work-group per flip; incompressible data runs in
            // batches too.
            bool ordered = false;
            {
                if (!have_turn) {
                    bool aborted = false;
                    // RUN-AHEAD (round 5): inside a long incompressible stretch — random input, data that is compressed already — the state behind a
                    // round is its prediction round after round (every coded block incompressible: the FSM is a function of its state alone), so the
                    // dictionary token need not wait for the commit: the predecessor passed it on right behind its exchanges, with the state it
                    // PREDICTS for this round (D line, words 2 and 3).  This round predicts from that, exchanges, passes the token on the same way,
                    // and only then waits for its commit payload — which must show the state it assumed, and its own signatures the stretch going on;
                    // if not, the abort protocol takes back what ran ahead, as for a fast round, and the chain restarts here without run-ahead.
                    // An ordinary ordered round starts it after kStormRounds rounds of an unbroken stretch (payload bits 26..28).
                    ahead = dF == 1u && !zero_round && (dS & 0x100ffu) != 0;
                    if (!got_payload && !ahead)
                    for (uint32_t spins = 0;;) {
                        const u32x4 v = lds_peek4(sy + kSyO);
                        const uint32_t O = rfl(v.x), A = rfl(v.y);
                        if (O == r) { P0 = rfl(v.z); P1 = rfl(v.w); break; }
                        if (A != kNone) { if (A == kPoison) wave_exit(); abort_sync(false, 0); aborted = true; break; }
                        backoff(r - O);
                        watchdog(spins, sy, err, lane);
                    }
                    if (aborted) continue;
                    have_turn = true;
                    // (a fresh chunk's first round is the cold start — raw copies for certain, nothing to predict —, and the rare zero-entry quads
                    // are settled block by block: those rounds are walked in order, below)
                    if (!zero_round && !(r == 0 && !seg.init_images)) {
                        it_j0 = 0; it_state = ahead ? dS & 0x1fffffu : P1 & 0x1fffffu; it_raw = 0;
                        it_end = (it_state & ~0x1e0000u) | ((((it_state >> 17) + R) & 15u) << 17);   // (calm, start == 1, no incompressible block: only the counter moves)
                        it_mode = (it_state & 0x100ffu) != 0 ? 1u : 0u;              // penalty running or the last coded block incompressible
                        if ((it_state & 0x1ffffu) != 0) {                                // (calm, start == 1: no raw copy while no block is incompressible, only the counter moves: the check below)
                            // Inside an incompressible stretch the state in front of a round repeats with a period of a few rounds (the counter moves
                            // by R = 16 a round, penalty and start go round a short cycle), and the prediction is a function of that state alone: a
                            // memo of eight in the sync block, touched only by the holder of the commit token, saves the walk — a few hundred scalar
                            // instructions in the one place where every later round waits.
                            u32x4 e = memo_early;                                    // lane l: entry l mod 8; the round's number picks the one to replace
                            uint64_t found = ballot64(e.x == it_state);
                            if (it_mode && found) clk.count(6, lane);
                            if (!(it_mode && found)) { e = lds_peek4(sy + kSyMemo + 16u * (lane & (kMemoEntries - 1u))); found = ballot64(e.x == it_state); if (it_mode && found) clk.count(7, lane); }
                            if (it_mode && found) {
                                const uint32_t l0 = (uint32_t)__builtin_ctzll(found);
                                it_raw = rlane(e.y, l0); it_end = rlane(e.z, l0);
                            } else {
                                fsm_predict(it_state, 0u, it_mode, 0u, it_raw, it_end);
                                if (it_mode && lane == 0) {
                                    const u32x4 v = {it_state, it_raw, it_end, 0u};
                                    asm volatile("ds_write_b128 %0, %1" ::"v"(sy + kSyMemo + 16u * (r & (kMemoEntries - 1u))), "v"(v) : "memory");
                                }
                            }
                        }
                    }
                }
                ordered = it_j0 != kNone;
            }
            bool batched = false;
            uint32_t osum = 0, ounrest = 0;
            Guard og;
            if (ordered) {
                // only the blocks from it_j0 on that are predicted coded exchange (final blocks and raw copies — codec.rs:35-37 — touch no state); no
                // token behind them: it leaves with the commit
                const uint32_t keep_lo = slo, keep_hi = shi;                       // (final blocks keep their signatures)
                if (ahead) {                                                      // the token behind the exchanges (LDS order), with the state predicted for the next round
                    exchange_some_ahead(ra, mask, val, rfl(it_raw), sy + kSyD, it_end, ((r + 1u) << 1) | 1u);
                    hold_skip = it_raw;
                    clk.stamp(r, 2, lane);
                } else
                exchange_some(ra, mask, val, rfl(it_raw | ((1u << it_j0) - 1u)));
#pragma unroll
                for (uint32_t j = 0; j < R; ++j) {                                // chameleon.rs:90-99 (an idle block's "signature" is never looked at)
                    const uint64_t sg = ballot64(((ra[j] ^ val[j]) & mask[j]) == 0);
                    slo = lane == j ? (uint32_t)sg : slo;
                    shi = lane == j ? (uint32_t)(sg >> 32) : shi;
                }
                // ---- do the signatures lead the FSM to the predicted raw copies? ----
                {
                    const uint32_t below = (1u << it_j0) - 1u, all = (1u << R) - 1u;
                    slo = lane < it_j0 ? keep_lo : slo;                            // (final blocks keep their signatures; theirs of this pass are of idle lanes)
                    shi = lane < it_j0 ? keep_hi : shi;
                    const uint32_t nh2 = (uint32_t)(__builtin_popcount(slo) + __builtin_popcount(shi));
                    const uint32_t inc_all = (uint32_t)ballot64(lane < R && nh2 <= 4u) & ~it_raw;   // codec.rs:68, coded blocks
                    const uint32_t coded_new = all & ~it_raw & ~below;
                    bool done = ((inc_all ^ (it_mode ? all : 0u)) & coded_new) == 0;   // every block behaved as predicted: the prediction's end state stands
                    if (ahead) {
                        // the commit turn: only now is the state in front of this round known — it must be the one that was assumed
                        bool aborted = false;
                        for (uint32_t spins = 0;;) {
                            const u32x4 v = lds_peek4(sy + kSyO);
                            const uint32_t O = rfl(v.x), A = rfl(v.y);
                            if (O == r) { P0 = rfl(v.z); P1 = rfl(v.w); break; }
                            if (A != kNone) { if (A == kPoison) wave_exit(); abort_sync(true, r); aborted = true; break; }
                            backoff_ordered(r - O);
                            watchdog(spins, sy, err, lane);
                        }
                        if (!aborted && (!done || (P1 & 0x1fffffu) != it_state)) {
                            if (lane == 0) { lds_poke(sy + kSyO + 12, ((P1 >> 24) & 3u) < 3u ? P1 + 0x01000000u : P1); lds_poke(sy + kSyD + 4, r); lds_poke(sy + kSyO + 4, r); }
                            clk.count(4, lane);
                            abort_sync(true, r);
                            aborted = true;
                        }
                        if (aborted) { ahead = false; have_turn = false; it_j0 = kNone; hold_skip = 0; continue; }
                    } else
                    if (!done) {
                        uint32_t sm, mm;
                        const uint32_t jm = fsm_verify(it_state, it_j0, inc_all, it_raw, sm, mm);
                        if (jm == (uint32_t)R) { done = true; it_end = sm; }          // (single incompressible blocks in a calm round: no raw copy came of them)
                        else {
                            clk.count(2, lane);
                            rollback_round(it_raw | ((1u << jm) - 1u));             // the exchanges from jm on, last block first
                            uint32_t raw_new;
                            fsm_predict(sm, jm, mm, it_raw, raw_new, it_end);
                            it_raw = raw_new; it_j0 = jm; it_state = sm; it_mode = mm;
                            continue;
                        }
                    }
                    batched = true;
                    clk.count(1, lane);
                    og = unpack_guard(it_end);
                    uint32_t acc = ((it_raw >> lane) & 1u) ? kBlock : kSig + kBlock - 2u * nh2;              // lane j < R: bytes of block j
                    acc = lane < R ? acc : 0u;
                    acc += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)acc, 0x111, 0xf, 0xf, true);     // row_shr:1
                    acc += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)acc, 0x112, 0xf, 0xf, true);     // row_shr:2
                    acc += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)acc, 0x114, 0xf, 0xf, true);     // row_shr:4
                    acc += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)acc, 0x118, 0xf, 0xf, true);     // row_shr:8
                    osum = rlane_u(acc, 15);
                    ounrest = inc_all != 0 ? 1u : 0u;
                }
            }
            // ---- in-order round: everything before it is final (the wait above); walk the blocks with the FSM ----
            Guard g = batched ? og : unpack_guard(P1);
            uint32_t sum = osum, unrest = ounrest;
            copy_mask = batched ? it_raw : 0u;
            if (!batched) {
                clk.count(3, lane);
                slo = 0; shi = 0;
                if constexpr (SPLIT) { uint32_t t[R]; reload_quads(t, r); park(0, t); } else park(0, q);   // (a rolled loop, as in rollback_round)
#pragma nounroll
                for (uint32_t j = 0; j < R; ++j) {
                    const uint32_t qv = parked(0, j);
                    uint32_t a, m, v;
                    operands(qv, a, m, v);
                    bool raw;
                    uint64_t sg;
                    block_in_order(g, qv, a, m, v, sg, raw);
                    slo = lane == j ? (uint32_t)sg : slo;
                    shi = lane == j ? (uint32_t)(sg >> 32) : shi;
                    copy_mask |= (raw ? 1u : 0u) << j;
                    unrest |= g.prev;
                    sum += raw ? kBlock : kSig + kBlock - 2u * (uint32_t)__builtin_popcountll(sg);
                }
            }
            opos = PAGED ? page_place(P0, sum + (r + 1u == nrounds ? tail_need : 0u), r * R) : P0;
            if (seg.raw_blocks && copy_mask && lane == 0) atomicAdd(seg.raw_blocks + chunk, (uint32_t)__builtin_popcount(copy_mask));
            // back to speculation ACROSS rounds only after quiet_rounds() rounds in a row without an incompressible or raw block (the count rides in
            // bits 21..23 of the commit payload): a mis-speculated fast round costs a work-group barrier and the roll-back of every round that ran
            // ahead — dozens of ordered rounds' worth
            const uint32_t streak = (g.penalty | copy_mask | unrest) != 0 ? 0u : (((P1 >> 21) & 7u) < 7u ? ((P1 >> 21) & 7u) + 1u : 7u);
            const uint32_t stay_slow = streak < quiet_rounds(P1) ? 1u : 0u;
            // (rounds in a row that were one incompressible stretch, as predicted from their first block on: run-ahead starts behind kStormRounds of them)
            const uint32_t storm = batched && it_mode && it_j0 == 0 ? (((P1 >> 26) & 7u) < 7u ? ((P1 >> 26) & 7u) + 1u : 7u) : 0u;
            if (lane == 0) {
                lds_poke2(sy + kSyO + 8, opos + sum, pack_guard(g) | (streak << 21) | (P1 & 0x03000000u) | (storm << 26));
                lds_poke(sy + kSyO, r + 1u);
                if (!ahead) {                                                     // (a round that ran ahead passed the dictionary token on behind its exchanges)
                    lds_poke2(sy + kSyD + 8, pack_guard(g), storm >= kStormRounds && stay_slow ? 1u : 0u);
                    lds_poke(sy + kSyD, ((r + 1u) << 1) | stay_slow);
                }
            }
            hold_skip = 0;
            if (ahead) clk.count(5, lane);
            if constexpr (!SPLIT) if (!prefetched && r + W < nrounds) prefetch_quads(src + (uint64_t)(r + W) * (R * kBlock) + 4u * lane);   // (as behind a fast commit)
            poll_tries = 2;
            if (PAGED && refill) page_refill();
            clk.mark(7);
            break;
        }
      }

        clk.mark(5);

        // ---- emit: records of this round and their block-index bytes ----
        if (SPLIT && copy_mask == 0) {
            __builtin_amdgcn_s_setprio(1);
            mbox_post(r, opos, slo, shi, 0u);                                     // the partner writes the records (it has the quads)
        } else if (__builtin_expect(copy_mask == 0, 1)) {
            emit_round_coded(q, opos, idx ? idx + (uint64_t)r * R : nullptr, slo, shi);
        } else {
            // (unrolled since round 5 — ordered rounds made incompressible data a common case: the rolled loop picked every block's quads out of
            // the registers by a chain of selects, ten thousand cycles a round)
            uint8_t* rec = dst + opos;
            uint32_t qe_[R];
            if constexpr (SPLIT) reload_quads(qe_, r);
            const uint32_t (&qe)[R] = *(SPLIT ? &qe_ : &q);
            if (idx && lane < R) idx[(uint64_t)r * R + lane] = (uint8_t)(((copy_mask >> lane) & 1u) ? kIdxCopy : (uint32_t)(__builtin_popcount(slo) + __builtin_popcount(shi)));
#pragma unroll
            for (uint32_t j = 0; j < R; ++j) {
                const bool raw = (copy_mask >> j) & 1u;
                const uint64_t sg = ((uint64_t)rlane_u(shi, (int)j) << 32) | rlane_u(slo, (int)j);
                emit_block(rec, qe[j], sg, raw);
                rec += raw ? kBlock : kSig + kBlock - 2u * (uint32_t)__builtin_popcountll(sg);
            }
            if (SPLIT) mbox_post(r, opos, slo, shi, 1u);                          // (the partner drops its copy of the round)
        }
        // (split: the next round's quads come out of the ring at the top of the loop; else both ways out of the round have asked for them)
        if constexpr (!SPLIT) {
            if (r + W < nrounds) {
                // behind a fast commit at least R stores are younger than the R loads (emit_round_coded: one store per record, one or two for the
                // last — a store none of whose lanes is active is not counted — and the signatures go out in one more)
                if (fast_commit) quads_landed<false>(q); else quads_landed<true>(q);
            }
        }
        clk.mark(6);
        clk.stamp(r, 3, lane);
    }
    }
    clk.flush(wave, lane);

    // ---- end of the chunk: every round committed (no abort can follow) ----
    for (uint32_t spins = 0;;) {
        const u32x4 v = lds_peek4(sy + kSyO);
        if (rfl(v.x) == nrounds) break;
        if (rfl(v.y) == kPoison) wave_exit();
        if (rfl(v.y) != kNone) abort_sync(false, 0); else __builtin_amdgcn_s_sleep(4);
        watchdog(spins, sy, err, lane);
    }
    wg_barrier();
    // ---- epilogue on one wave: the blocks of the last, partial round in order, then the ragged block (codec.rs:51-63) ----
    if (wave == 0) {
        const u32x4 v = lds_peek4(sy + kSyO);
        Guard g = unpack_guard(rfl(v.w));
        uint64_t opos = rfl(v.z);
        for (uint32_t b = nrounds * R; b < nfull; ++b) {
            const uint32_t qv = *reinterpret_cast<const uint32_t*>(src + (uint64_t)b * kBlock + 4u * lane);
            uint32_t a, m, vv;
            operands(qv, a, m, vv);
            uint64_t sg;
            bool raw;
            block_in_order(g, qv, a, m, vv, sg, raw);
            emit_block(dst + opos, qv, sg, raw);
            const uint32_t nh = (uint32_t)__builtin_popcountll(sg);
            if (idx && lane == 0) idx[b] = (uint8_t)(raw ? kIdxCopy : nh);
            if (seg.raw_blocks && raw && lane == 0) atomicAdd(seg.raw_blocks + chunk, 1u);
            opos += raw ? kBlock : kSig + kBlock - 2u * nh;
        }
        // (a segment that is not the stream's last ends on a whole block; bit 31: the next one may start speculating)
        if (seg.final_guard && lane == 0) seg.final_guard[chunk] = pack_guard(g) | (g.penalty == 0 ? 0x80000000u : 0u);
        const uint64_t end = encode_ragged_block(src, len, nfull, dst, opos, g, idx, 0u, zmap, lane);
        if (PAGED) {                                                              // the stream's length is the bytes used over its pages; the last page's share and the count go into the directory
            const u32x4 st = lds_peek4(sy + kSyPage);
            const uint32_t base = rfl(st.x), before = rfl(st.y), count = rfl(st.w);
            if (lane == 0) {
                dir[4u * count + 2u] = (uint32_t)end - base;
                *reinterpret_cast<uint4*>(dir) = make_uint4(count, 0u, 0u, 0u);
                sizes[chunk] = (uint64_t)before + ((uint32_t)end - base);
            }
        } else
        if (lane == 0) sizes[chunk] = end;
    }
    if (seg.final_images) {                                                        // the dictionary as this chunk leaves it
        wg_barrier();
        uint4* image = reinterpret_cast<uint4*>(seg.final_images + chunk * kSegImageBytes);
        const uint4* p = reinterpret_cast<const uint4*>(smem);
        for (uint32_t i = threadIdx.x; i < (kTableBytes + kZmapBytes) / 16; i += kThreads) image[i] = p[i];
    }
}

// ---------------------------------------------------------------------------------------------------------------
// Segments of one long stream (whole-stream-exact parallel encode, api.hip::run_stream_encode_segmented)
// ---------------------------------------------------------------------------------------------------------------
// "Last writers": the dictionary image a FRESH table has after every block of a chunk went through it (no raw-copy blocks: what
// the segmented encode speculates for every segment but the first).  The D chain of the encoder and nothing else: rounds of 16
// blocks rotate over 16 waves, each wave issues its round's ordered exchanges behind the token and drops the answers; zero-entry
// quads mark their slot (the marks need no order: a stale mark under a non-zero entry is never consulted).  Whole rounds only.
__global__ __launch_bounds__(1024) void chameleon_lastwriters_rot(const uint8_t* __restrict__ in, uint64_t chunk_bytes, uint8_t* __restrict__ images,
                                                                   uint32_t* __restrict__ err) {
    constexpr int R = 16, W = 16;
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t wave = rfl(threadIdx.x >> 6);
    const uint64_t chunk = blockIdx.x;
    const uint8_t* src = in + chunk * chunk_bytes;
    const uint32_t nrounds = (uint32_t)(chunk_bytes / (R * kBlock));
    const uint32_t sy = kEncSync;
    const ZmapLds zmap{kEncZmap};
    {
        uint4* p = reinterpret_cast<uint4*>(smem);
        const uint4 z = make_uint4(0, 0, 0, 0);
        for (uint32_t i = threadIdx.x; i < (kTableBytes + kZmapBytes) / 16; i += W * 64) p[i] = z;
        if (threadIdx.x == 0) *reinterpret_cast<uint4*>(smem + kEncSync + kSyD) = make_uint4(0u, kNone, 0u, 0u);
    }
    __syncthreads();
    uint32_t q[R], ra[R], mask[R], val[R];
    for (uint32_t r = wave; r < nrounds; r += W) {
        const uint8_t* p = src + (uint64_t)r * (R * kBlock);
        bool zero_entry = false;
#pragma unroll
        for (uint32_t j = 0; j < R; ++j) q[j] = *reinterpret_cast<const uint32_t*>(p + j * kBlock + 4u * lane);
#pragma unroll
        for (uint32_t j = 0; j < R; ++j) {
            const uint32_t P = q[j] * kHashMul;
            const uint32_t sh = (P >> 12) & 16u;
            ra[j] = (P >> 15) & 0x1fffcu;
            mask[j] = 0xffffu << sh;
            val[j] = stored_entry(q[j], P) << sh;
            zero_entry |= val[j] == 0;
        }
        const uint32_t tokaddr = lane == 0 ? sy + kSyD : sy + kSySink + 4u * lane;
        pin_operands<R>(ra, mask, val);
        for (uint32_t spins = 0;;) {
            if (poll_word(sy + kSyD, r, 16)) break;
            const uint32_t D = rfl(lds_peek1(sy + kSyD));
            if (D == r) break;
            if (D == kPoison) wave_exit();
            backoff(r - D);
            watchdog(spins, sy, err, lane);
        }
        __builtin_amdgcn_s_setprio(3);
        exchange_tied16(ra, mask, val, tokaddr, r + 1u);
        __builtin_amdgcn_s_setprio(0);
        if (__builtin_expect(ballot64(zero_entry) != 0, 0)) {
#pragma unroll
            // (the zero quad in slot 0 included: here the mark also says "this chunk wrote the slot", which an entry of 0 alone does not;
            // nothing ever consults slot 0's mark)
            for (uint32_t j = 0; j < R; ++j) if (val[j] == 0) (void)zmap.test_and_set((q[j] * kHashMul) >> 16);
        }
    }
    wg_barrier();
    uint4* image = reinterpret_cast<uint4*>(images + chunk * kSegImageBytes);
    const uint4* lp = reinterpret_cast<const uint4*>(smem);
    for (uint32_t i = threadIdx.x; i < (kTableBytes + kZmapBytes) / 16; i += W * 64) image[i] = lp[i];
}

// Start images: slot by slot, the base image with the last-writer images of the following chunks laid over it one after the other
// (a slot counts as written by a chunk if its entry is non-zero or its zero-entry mark is set).  One thread per slot; the output
// marks are OR-ed into pre-zeroed words.
__global__ __launch_bounds__(256) void merge_images_kernel(const uint8_t* __restrict__ base, const uint8_t* __restrict__ lastwriters,
                                                           uint8_t* __restrict__ start, uint32_t count) {
    const uint32_t slot = blockIdx.x * blockDim.x + threadIdx.x;                  // 0 .. 65535
    uint32_t e = reinterpret_cast<const uint16_t*>(base)[slot];
    uint32_t z = (reinterpret_cast<const uint32_t*>(base + kTableBytes)[slot >> 5] >> (slot & 31u)) & 1u;
    for (uint32_t k = 0; k < count; ++k) {
        uint8_t* out = start + (uint64_t)k * kSegImageBytes;
        reinterpret_cast<uint16_t*>(out)[slot] = (uint16_t)e;
        if (z) atomicOr(reinterpret_cast<uint32_t*>(out + kTableBytes) + (slot >> 5), 1u << (slot & 31u));
        if (k + 1 == count) break;                                                // (the last chunk has no successor: its last writers were never computed)
        const uint8_t* lw = lastwriters + (uint64_t)k * kSegImageBytes;
        const uint32_t le = reinterpret_cast<const uint16_t*>(lw)[slot];
        const uint32_t lz = (reinterpret_cast<const uint32_t*>(lw + kTableBytes)[slot >> 5] >> (slot & 31u)) & 1u;
        if (le != 0 || lz) { e = le; z = lz; }
    }
}

// ---------------------------------------------------------------------------------------------------------------
// host launchers
// ---------------------------------------------------------------------------------------------------------------
bool g_rotor_split = kRotorSplitDefault;
bool rotor_encode_eligible(const uint8_t* d_in, uint64_t total, uint64_t chunk_bytes, uint32_t n_chunks) {
    const bool aligned = ((uintptr_t)d_in % 4 == 0) && (n_chunks == 1 || chunk_bytes % 4 == 0);
    return aligned && (n_chunks == 1 ? total : chunk_bytes) < (1ull << 31);   // 32-bit stream positions
}
namespace {
// work-group and LDS of the encoder that is selected: 8 waves that do everything, or the split encoder (round 5: 8 chain + 8 emit waves,
// the quads handed over through an LDS ring; kernel variant bit 11 selects the one that is not kRotorSplitDefault)
uint32_t enc_threads() { return (g_rotor_split ? 2u : 1u) * kEncWaves * 64u; }
uint32_t enc_lds() { return g_rotor_split ? kEncLdsSplit : kEncLds; }
}  // namespace
// (rounds of 16 blocks on 8 waves: the longer round amortises the hand-off, and 8 waves have the registers to keep their quads.  What was
// measured against it — 8 blocks on 16 waves, 16 on 12, the prefetch behind the commit — is in DESIGN.md 4.3.)
hipError_t launch_rotor_encode(const uint8_t* d_in, uint64_t total, uint64_t chunk_bytes, uint32_t n_chunks, uint8_t* d_out, uint64_t out_stride,
                               uint64_t* d_sizes, uint8_t* d_index, uint32_t* d_err, hipStream_t stream) {
    uint64_t* prof = rot_prof_buffer();
    const bool split = g_rotor_split;
    auto kernel = split ? (prof ? chameleon_encode_rot<true, false, true> : chameleon_encode_rot<false, false, true>)
                        : (prof ? chameleon_encode_rot<true> : chameleon_encode_rot<false>);
    hipError_t e = hipFuncSetAttribute((const void*)kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)enc_lds());
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(kernel, dim3(n_chunks), dim3(enc_threads()), enc_lds(), stream, d_in, total, chunk_bytes, d_out, out_stride, d_sizes, d_index,
                       d_err, SegArgs{}, prof);
    if (split)
        rot_prof_report("encode (split)",
                        "chain waves 0-7: hash | D wait | exchange | signatures | O wait+commit | ring: wait for the quads | post | ring: the reads "
                        "(+ in-order rounds);  emit waves 8-15: - | ring transfer incl. the wait for the slot | - | - | mail box wait | - | emit | -",
                        prof, stream, 2 * kEncWaves);
    else
        rot_prof_report("encode", "hash | D wait | exchange | signatures | O wait+commit | load wait | emit | in-order rounds", prof, stream, kEncWaves);
    return hipGetLastError();
}
hipError_t launch_rotor_encode_paged(const uint8_t* d_in, uint64_t total, uint64_t chunk_bytes, uint32_t n_chunks, uint8_t* d_pages, uint32_t page_limit,
                                     uint32_t* d_page_counter, uint32_t* d_dir, uint32_t dir_words, uint64_t* d_sizes, uint8_t* d_index, uint32_t* d_err,
                                     hipStream_t stream) {
    auto kernel = g_rotor_split ? chameleon_encode_rot<false, true, true> : chameleon_encode_rot<false, true>;
    hipError_t e = hipFuncSetAttribute((const void*)kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)enc_lds());
    if (e != hipSuccess) return e;
    SegArgs pg;
    pg.page_counter = d_page_counter; pg.page_dir = d_dir; pg.page_dir_words = dir_words; pg.page_limit = page_limit;
    hipLaunchKernelGGL(kernel, dim3(n_chunks), dim3(enc_threads()), enc_lds(), stream, d_in, total, chunk_bytes, d_pages, (uint64_t)0, d_sizes, d_index,
                       d_err, pg, (uint64_t*)nullptr);
    return hipGetLastError();
}
hipError_t launch_rotor_encode_seg(const uint8_t* d_in, uint64_t total, uint64_t chunk_bytes, uint32_t n_chunks, uint8_t* d_out, uint64_t out_stride,
                                   uint64_t* d_sizes, uint32_t* d_err, SegArgs seg, hipStream_t stream) {
    auto kernel = g_rotor_split ? chameleon_encode_rot<false, false, true> : chameleon_encode_rot<false>;
    hipError_t e = hipFuncSetAttribute((const void*)kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)enc_lds());
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(kernel, dim3(n_chunks), dim3(enc_threads()), enc_lds(), stream, d_in, total, chunk_bytes, d_out, out_stride, d_sizes,
                       (uint8_t*)nullptr, d_err, seg, (uint64_t*)nullptr);
    return hipGetLastError();
}
hipError_t launch_rotor_lastwriters(const uint8_t* d_in, uint64_t chunk_bytes, uint32_t n_chunks, uint8_t* d_images, uint32_t* d_err, hipStream_t stream) {
    if (n_chunks == 0) return hipSuccess;
    hipError_t e = hipFuncSetAttribute((const void*)chameleon_lastwriters_rot, hipFuncAttributeMaxDynamicSharedMemorySize, (int)kEncLds);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(chameleon_lastwriters_rot, dim3(n_chunks), dim3(1024), kEncLds, stream, d_in, chunk_bytes, d_images, d_err);
    return hipGetLastError();
}
hipError_t launch_merge_images(const uint8_t* d_base, const uint8_t* d_lastwriters, uint8_t* d_start, uint32_t count, hipStream_t stream) {
    if (count == 0) return hipSuccess;
    // the marks are OR-ed in: clear them first (one strided fill)
    hipError_t e = hipMemset2DAsync(d_start + kTableBytes, kSegImageBytes, 0, kZmapBytes, count, stream);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(merge_images_kernel, dim3(65536 / 256), dim3(256), 0, stream, d_base, d_lastwriters, d_start, count);
    return hipGetLastError();
}

}  // namespace density
