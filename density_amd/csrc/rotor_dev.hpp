// rotor_dev.hpp — device-side pieces shared by the Chameleon wave-rotation kernels (rotor_encode.hip, rotor_decode.hip, rotor.hip):
// the geometry, the LDS layouts, token peeks and pokes, the ordered exchanges of a round, the packed FSM state and its closed forms,
// the watchdog, the phase clock of the profiling instances and the token polls.  See rotor.hip for the design notes.
#pragma once
#include "chameleon_dev.hpp"
#include "kernels.hpp"

namespace density {

namespace {

// The geometry.  Encoder: rounds of 16 blocks on 8 waves (256 registers a wave: the quads of a round stay in registers from the hash to
// the emit); the split encoder runs the same rounds on 8 chain + 8 emit waves.  Decoder: rounds of 12 records on 12 waves (168 registers
// a wave: the longest round that does not spill).  The geometries that were measured against these and lost: DESIGN.md 4.3.
constexpr int kEncRound = 16, kEncWaves = 8;
constexpr int kDecRound = 12, kDecWaves = 12;

constexpr uint32_t kNone = 0xffffffffu;
// sync block (bytes from its base): D line {D, A}; O line {O, A', P0, P1}; a 256-byte sink for the idle lanes of a token write;
// 16 words "rounds whose zero-entry-map phase this wave has finished" (decoder); 16 words "the round of this wave that is about to
// mark the map" (decoder)
constexpr uint32_t kSyD = 0, kSyO = 16, kSyZ = 32, kSyEnd = 48, kSySink = 64, kSyZdone = 64 + 256, kSyWsum = 64 + 256 + 64,
                   kSyZset = 64 + 256 + 64 + 64, kSyBytes = 64 + 256 + 64 + 64 + 64;
// (encoder: the words of the decoder's zero-entry chain hold the memo of FSM predictions instead — 8 entries of {state, raw-copy blocks,
// end state, -})
constexpr uint32_t kSyMemo = kSyZdone, kMemoEntries = 8;
constexpr uint32_t kSyPage = kSyZ;                                             // (PAGED encoder: 16 bytes of page state, the commit token's holder's)
static_assert(kSyMemo + 16u * kMemoEntries <= kSyBytes, "memo inside the sync block");
// encoder LDS: table | zero-entry map | sync
constexpr uint32_t kEncZmap = kTableBytes, kEncSync = kTableBytes + kZmapBytes, kEncStage = kEncSync + kSyBytes;
// (encoder staging: two arrays of 16 blocks x 64 lanes for the rolled loops of the rare paths — rollback, in-order rounds, zero-entry
// quads at commit — which exclude one another in time, so the whole work-group shares one copy)
constexpr uint32_t kEncStageBytes = 2u * kEncRound * 256u, kEncLds = kEncStage + kEncStageBytes;
// decoder LDS: table | block-index copy | round positions | zero-entry map | sync
// (rounds of 12 leave room for the map in LDS: a look-up in global memory is a memory round trip of microseconds, and one round in 25
// has one on repetitive text)
constexpr uint32_t kRotMaxBlocks = 16384;                    // blocks per chunk the decoder keeps an index copy for (4 MiB chunks)
constexpr uint32_t kDecIdx = kTableBytes, kDecPos = kDecIdx + kRotMaxBlocks;
constexpr uint32_t kDecPosBytes = ((kRotMaxBlocks / kDecRound + 1u) * 4u + 15u) & ~15u;
constexpr uint32_t kDecZmap = kDecPos + kDecPosBytes, kDecSync = kDecZmap + kZmapBytes, kDecLds = kDecSync + kSyBytes;
// PAGED decoder: behind the sync block, per page of the chunk its first block and what turns a stream position into an offset from page 0
constexpr uint32_t kDecMaxPages = kPagedMaxPages;
static_assert(kPagedMaxChunk == (uint64_t)kRotMaxBlocks * 256u, "the paged form ends where the index-fed decoder does");
constexpr uint32_t kDecPages = kDecLds, kDecLdsPaged = kDecLds + 8u * kDecMaxPages;
// SPLIT encoder (round 5): eight CHAIN waves (hash, exchange, signatures, commit) and eight EMIT waves.  Behind the
// staging area: the quad ring — three rounds of 16 blocks x 64 lanes, filled by the emit waves (which load the input and keep the quads
// for the emit), drained by the chain waves —, its words {ready[3], -, freed[3], -}, and one mail box per pair of waves: the signatures
// of a committed round (lane j's 8 bytes), then {sequence word, stream position, -, -}, then {taken, -, -, -}
constexpr uint32_t kRingSlots = 3, kSlotBytes = kEncRound * 256u;
constexpr uint32_t kEncRing = kEncLds, kEncRingSync = kEncRing + kRingSlots * kSlotBytes, kEncMbox = kEncRingSync + 32u, kMboxBytes = 160u;
constexpr uint32_t kEncLdsSplit = kEncMbox + 8u * kMboxBytes;
static_assert(kEncLdsSplit <= 160u * 1024u && kEncRing % 16u == 0, "LDS budget of the split encoder");
static_assert(kEncLds <= 160u * 1024u && kDecLdsPaged <= 160u * 1024u, "LDS budget");


typedef uint32_t u32x2 __attribute__((ext_vector_type(2)));
typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
typedef u32x2 u32x2_u __attribute__((aligned(1)));

// token polls: every lane reads the same address (broadcast), the caller takes lane 0's copy
__device__ __forceinline__ u32x2 lds_peek2(uint32_t addr) {
    u32x2 v;
    asm volatile("ds_read_b64 %0, %1\n\ts_waitcnt lgkmcnt(0)" : "=&v"(v) : "v"(addr) : "memory");
    return v;
}
__device__ __forceinline__ u32x4 lds_peek4(uint32_t addr) {
    u32x4 v;
    asm volatile("ds_read_b128 %0, %1\n\ts_waitcnt lgkmcnt(0)" : "=&v"(v) : "v"(addr) : "memory");
    return v;
}
// two consecutive 16-byte lines in one round trip (the D line and the O line of the sync block)
__device__ __forceinline__ void lds_peek4x2(uint32_t addr, u32x4& a, u32x4& b) {
    asm volatile("ds_read_b128 %0, %2\n\tds_read_b128 %1, %2 offset:16\n\ts_waitcnt lgkmcnt(0)" : "=&v"(a), "=&v"(b) : "v"(addr) : "memory");
}
__device__ __forceinline__ uint32_t lds_peek1(uint32_t addr) {
    uint32_t v;
    asm volatile("ds_read_b32 %0, %1\n\ts_waitcnt lgkmcnt(0)" : "=&v"(v) : "v"(addr) : "memory");
    return v;
}
__device__ __forceinline__ uint32_t rlane_u(uint32_t v, int l) { return (uint32_t)__builtin_amdgcn_readlane((int)v, l); }
__device__ __forceinline__ uint32_t rlane(uint32_t v, uint32_t l) { return (uint32_t)__builtin_amdgcn_readlane((int)v, (int)l); }
__device__ __forceinline__ void lds_poke(uint32_t addr, uint32_t v) { asm volatile("ds_write_b32 %0, %1" ::"v"(addr), "v"(v) : "memory"); }
// the same at a compile-time offset from a base register (16-bit field): R addresses from ONE register — per-lane addresses that differ by constants would
// otherwise be hoisted out of the round loop one register each, rare paths included, and sit on the common path's register budget
#define DENSITY_LDS_POKE_AT(base, off, v) asm volatile("ds_write_b32 %0, %1 offset:%2" ::"v"(base), "v"(v), "n"(off) : "memory")
__device__ __forceinline__ void lds_poke2(uint32_t addr, uint32_t a, uint32_t b) {
    const u32x2 v = {a, b};
    asm volatile("ds_write_b64 %0, %1" ::"v"(addr), "v"(v) : "memory");
}
// the work-group barrier of the (rare) abort protocol and of the kernel's end: own LDS traffic retired first
__device__ __forceinline__ void wg_barrier() { asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory"); }

// The critical section of a round: its ordered exchanges (ds_mskor_rtn_b32, chameleon_dev.hpp) from prepared registers, the answer
// returned in place of the address, then the token for the next round written behind them (lane 0 writes the token word, the other
// lanes a sink, so the store has no bank conflict), then the answers.  One asm statement: the answers are valid when it ends, nothing
// the compiler does can touch a register still in flight.  16 blocks: the encoder and the last-writers kernel; 12 records: the decoder.
// (operand lists of 12 / 16 array elements, constraint `c` each)
#define DENSITY_ROT_EACH12(c, a) c(a[0]), c(a[1]), c(a[2]), c(a[3]), c(a[4]), c(a[5]), c(a[6]), c(a[7]), c(a[8]), c(a[9]), c(a[10]), c(a[11])
#define DENSITY_ROT_EACH16(c, a) DENSITY_ROT_EACH12(c, a), c(a[12]), c(a[13]), c(a[14]), c(a[15])
#define DENSITY_ROT_X16 \
    "ds_mskor_rtn_b32 %0, %0, %16, %32\n\t" \
    "ds_mskor_rtn_b32 %1, %1, %17, %33\n\t" \
    "ds_mskor_rtn_b32 %2, %2, %18, %34\n\t" \
    "ds_mskor_rtn_b32 %3, %3, %19, %35\n\t" \
    "ds_mskor_rtn_b32 %4, %4, %20, %36\n\t" \
    "ds_mskor_rtn_b32 %5, %5, %21, %37\n\t" \
    "ds_mskor_rtn_b32 %6, %6, %22, %38\n\t" \
    "ds_mskor_rtn_b32 %7, %7, %23, %39\n\t" \
    "ds_mskor_rtn_b32 %8, %8, %24, %40\n\t" \
    "ds_mskor_rtn_b32 %9, %9, %25, %41\n\t" \
    "ds_mskor_rtn_b32 %10, %10, %26, %42\n\t" \
    "ds_mskor_rtn_b32 %11, %11, %27, %43\n\t" \
    "ds_mskor_rtn_b32 %12, %12, %28, %44\n\t" \
    "ds_mskor_rtn_b32 %13, %13, %29, %45\n\t" \
    "ds_mskor_rtn_b32 %14, %14, %30, %46\n\t" \
    "ds_mskor_rtn_b32 %15, %15, %31, %47\n\t"
#define DENSITY_ROT_X12 \
    "ds_mskor_rtn_b32 %0, %0, %12, %24\n\t" \
    "ds_mskor_rtn_b32 %1, %1, %13, %25\n\t" \
    "ds_mskor_rtn_b32 %2, %2, %14, %26\n\t" \
    "ds_mskor_rtn_b32 %3, %3, %15, %27\n\t" \
    "ds_mskor_rtn_b32 %4, %4, %16, %28\n\t" \
    "ds_mskor_rtn_b32 %5, %5, %17, %29\n\t" \
    "ds_mskor_rtn_b32 %6, %6, %18, %30\n\t" \
    "ds_mskor_rtn_b32 %7, %7, %19, %31\n\t" \
    "ds_mskor_rtn_b32 %8, %8, %20, %32\n\t" \
    "ds_mskor_rtn_b32 %9, %9, %21, %33\n\t" \
    "ds_mskor_rtn_b32 %10, %10, %22, %34\n\t" \
    "ds_mskor_rtn_b32 %11, %11, %23, %35\n\t"
__device__ __forceinline__ void exchange_tied16(uint32_t (&ra)[16], const uint32_t (&mask)[16], const uint32_t (&val)[16], uint32_t tokaddr, uint32_t tokval) {
    asm volatile(DENSITY_ROT_X16 "ds_write_b32 %48, %49\n\ts_waitcnt lgkmcnt(0)"
                 : DENSITY_ROT_EACH16("+v", ra)
                 : DENSITY_ROT_EACH16("v", mask), DENSITY_ROT_EACH16("v", val), "v"(tokaddr), "v"(tokval)
                 : "memory");
}
__device__ __forceinline__ void exchange_tied12(uint32_t (&ra)[12], const uint32_t (&mask)[12], const uint32_t (&val)[12], uint32_t tokaddr, uint32_t tokval) {
    asm volatile(DENSITY_ROT_X12 "ds_write_b32 %36, %37\n\ts_waitcnt lgkmcnt(0)"
                 : DENSITY_ROT_EACH12("+v", ra)
                 : DENSITY_ROT_EACH12("v", mask), DENSITY_ROT_EACH12("v", val), "v"(tokaddr), "v"(tokval)
                 : "memory");
}
// The exchanges of an ORDERED round (encoder) in one statement: block j's is skipped if bit j of `idle` is set (a final block, a
// predicted raw copy); no token behind them.
#define DENSITY_ROT_XC16 \
    "s_bitcmp1_b32 %[idle], 0\n\ts_cbranch_scc1 .Lskip0_%=\n\tds_mskor_rtn_b32 %0, %0, %16, %32\n.Lskip0_%=:\n\t" \
    "s_bitcmp1_b32 %[idle], 1\n\ts_cbranch_scc1 .Lskip1_%=\n\tds_mskor_rtn_b32 %1, %1, %17, %33\n.Lskip1_%=:\n\t" \
    "s_bitcmp1_b32 %[idle], 2\n\ts_cbranch_scc1 .Lskip2_%=\n\tds_mskor_rtn_b32 %2, %2, %18, %34\n.Lskip2_%=:\n\t" \
    "s_bitcmp1_b32 %[idle], 3\n\ts_cbranch_scc1 .Lskip3_%=\n\tds_mskor_rtn_b32 %3, %3, %19, %35\n.Lskip3_%=:\n\t" \
    "s_bitcmp1_b32 %[idle], 4\n\ts_cbranch_scc1 .Lskip4_%=\n\tds_mskor_rtn_b32 %4, %4, %20, %36\n.Lskip4_%=:\n\t" \
    "s_bitcmp1_b32 %[idle], 5\n\ts_cbranch_scc1 .Lskip5_%=\n\tds_mskor_rtn_b32 %5, %5, %21, %37\n.Lskip5_%=:\n\t" \
    "s_bitcmp1_b32 %[idle], 6\n\ts_cbranch_scc1 .Lskip6_%=\n\tds_mskor_rtn_b32 %6, %6, %22, %38\n.Lskip6_%=:\n\t" \
    "s_bitcmp1_b32 %[idle], 7\n\ts_cbranch_scc1 .Lskip7_%=\n\tds_mskor_rtn_b32 %7, %7, %23, %39\n.Lskip7_%=:\n\t" \
    "s_bitcmp1_b32 %[idle], 8\n\ts_cbranch_scc1 .Lskip8_%=\n\tds_mskor_rtn_b32 %8, %8, %24, %40\n.Lskip8_%=:\n\t" \
    "s_bitcmp1_b32 %[idle], 9\n\ts_cbranch_scc1 .Lskip9_%=\n\tds_mskor_rtn_b32 %9, %9, %25, %41\n.Lskip9_%=:\n\t" \
    "s_bitcmp1_b32 %[idle], 10\n\ts_cbranch_scc1 .Lskip10_%=\n\tds_mskor_rtn_b32 %10, %10, %26, %42\n.Lskip10_%=:\n\t" \
    "s_bitcmp1_b32 %[idle], 11\n\ts_cbranch_scc1 .Lskip11_%=\n\tds_mskor_rtn_b32 %11, %11, %27, %43\n.Lskip11_%=:\n\t" \
    "s_bitcmp1_b32 %[idle], 12\n\ts_cbranch_scc1 .Lskip12_%=\n\tds_mskor_rtn_b32 %12, %12, %28, %44\n.Lskip12_%=:\n\t" \
    "s_bitcmp1_b32 %[idle], 13\n\ts_cbranch_scc1 .Lskip13_%=\n\tds_mskor_rtn_b32 %13, %13, %29, %45\n.Lskip13_%=:\n\t" \
    "s_bitcmp1_b32 %[idle], 14\n\ts_cbranch_scc1 .Lskip14_%=\n\tds_mskor_rtn_b32 %14, %14, %30, %46\n.Lskip14_%=:\n\t" \
    "s_bitcmp1_b32 %[idle], 15\n\ts_cbranch_scc1 .Lskip15_%=\n\tds_mskor_rtn_b32 %15, %15, %31, %47\n.Lskip15_%=:\n\t"
__device__ __forceinline__ void exchange_some(uint32_t (&ra)[16], const uint32_t (&mask)[16], const uint32_t (&val)[16], uint32_t idle) {
    asm volatile(DENSITY_ROT_XC16 "s_waitcnt lgkmcnt(0)"
                 : DENSITY_ROT_EACH16("+v", ra)
                 : DENSITY_ROT_EACH16("v", mask), DENSITY_ROT_EACH16("v", val), [idle] "s"(idle)
                 : "memory", "scc");
}
// the same for a round that RUNS AHEAD (rotor_encode.hip): the dictionary token — its run-ahead words {state predicted for the next
// round, 1}, then the token word — is written behind the exchanges in the same statement, by lane 0 alone, before their answers are
// waited for
__device__ __forceinline__ void exchange_some_ahead(uint32_t (&ra)[16], const uint32_t (&mask)[16], const uint32_t (&val)[16], uint32_t idle,
                                                    uint32_t dline, uint32_t state, uint32_t token) {
    const u32x2 words = {state, 1u};
    const uint32_t dline2 = dline + 8u;
    asm volatile(DENSITY_ROT_XC16
                 "s_mov_b64 exec, 1\n\t"
                 "ds_write_b64 %[d2], %[w]\n\t"
                 "ds_write_b32 %[d], %[t]\n\t"
                 "s_mov_b64 exec, -1\n\t"
                 "s_waitcnt lgkmcnt(0)"
                 : DENSITY_ROT_EACH16("+v", ra)
                 : DENSITY_ROT_EACH16("v", mask), DENSITY_ROT_EACH16("v", val), [idle] "s"(idle),
                   [d2] "v"(dline2), [w] "v"(words), [d] "v"(dline), [t] "v"(token)
                 : "memory", "scc");
}
// element j (wave-uniform, not a compile-time constant) of a register array, for the rolled loops of the rare paths: a chain of
// selects, so the array stays in registers (a dynamically indexed copy would live in scratch memory, and the compiler's waits for
// its loads would also hold the common path at the top of every round)
template <int R>
__device__ __forceinline__ uint32_t pick(const uint32_t (&a)[R], uint32_t j) {
    uint32_t v = a[0];
#pragma unroll
    for (uint32_t k = 1; k < (uint32_t)R; ++k) {
        uint32_t jj = j;
        asm volatile("" : "+s"(jj));                                              // (opaque: or the compiler turns the chain back into a table in scratch)
        v = jj == k ? a[k] : v;
    }
    return v;
}
// (keeps a set of operands from being scheduled past this point, i.e. into the critical section behind the token wait)
template <int R>
__device__ __forceinline__ void pin_operands(uint32_t (&ra)[R], uint32_t (&mask)[R], uint32_t (&val)[R]) {
#pragma unroll
    for (int j = 0; j < R; ++j) asm volatile("" : "+v"(ra[j]), "+v"(mask[j]), "+v"(val[j]));
}
__device__ __forceinline__ uint32_t exchange_block(uint32_t addr, uint32_t mask, uint32_t val) {
    uint32_t ret;
    asm volatile("ds_mskor_rtn_b32 %0, %1, %2, %3\n\ts_waitcnt lgkmcnt(0)" : "=&v"(ret) : "v"(addr), "v"(mask), "v"(val) : "memory");
    return ret;
}

// Commit payload {stream position (32 bits: the launcher bounds the chunk), FSM state}: penalty [0,8) | start-1 [8,16) | prev [16] | counter&15 [17,21)
// (protection_state.rs: copy_penalty, copy_penalty_start are u8, only counter & 0xf is ever tested).  Calm state with start == 1: low 17 bits 0.
__device__ __forceinline__ uint32_t pack_guard(const Guard& g) { return (g.penalty & 0xffu) | (((g.start - 1u) & 0xffu) << 8) | ((g.prev & 1u) << 16) | ((g.counter & 15u) << 17); }
__device__ __forceinline__ Guard unpack_guard(uint32_t w) {
    Guard g;
    g.penalty = w & 0xffu; g.start = ((w >> 8) & 0xffu) + 1u; g.prev = (w >> 16) & 1u; g.counter = (w >> 17) & 15u;
    return g;
}

// The FSM of an ORDERED round of the encoder (R = 16 blocks), protection_state.rs:19-47 on packed states (pack_guard), wave-uniform (scalar registers).
// fsm_verify: blocks j0..R-1 from the state `st` in front of block j0; every block's raw-copy status must be bit j of `raw_old` (what the last
// exchange assumed), a coded block is incompressible iff bit j of `inc` (its signature).  Returns the first block that is not what was assumed
// (R: none; then `state` is the state behind the round), the state in front of it and whether it is a raw copy — a raw copy where none was
// expected starts an incompressible stretch, a coded block where a copy was expected ends one.
__device__ __forceinline__ uint32_t fsm_verify(uint32_t st, uint32_t j0, uint32_t inc, uint32_t raw_old, uint32_t& state, uint32_t& is_copy) {
    constexpr uint32_t R = kEncRound;
    Guard g = unpack_guard(st);
    is_copy = 0;
    uint32_t j = j0;
#pragma nounroll
    for (; j < R; ++j) {
        const uint32_t copy = g.penalty != 0 ? 1u : 0u;                            // (what block_is_copy will say: the halving in it does not change that)
        if (copy != ((raw_old >> j) & 1u)) { is_copy = copy; break; }
        (void)g.block_is_copy();                                                   // codec.rs:35
        if (copy) g.decay();                                                       // codec.rs:36-37
        else g.update((inc >> j) & 1u);                                            // codec.rs:68
    }
    state = pack_guard(g);
    return j;
}
// fsm_predict: the raw-copy blocks among j0..R-1 (`raw`: bits below j0 as given) and the state behind the round if every coded block from j0
// on is incompressible (`storm`) or none is — the FSM is then a function of its state alone, taken run by run instead of block by block:
// a run of raw copies (penalty blocks, protection_state.rs:30-35), one coded block that triggers the next (:38-47), ...; `start` is halved at
// the one block of the stretch whose counter is a multiple of 16 (:19-27: before that block's own decay or trigger).
__device__ __forceinline__ void fsm_predict(uint32_t st, uint32_t j0, uint32_t storm, uint32_t raw_below, uint32_t& raw, uint32_t& end_state) {
    constexpr uint32_t R = kEncRound;
    uint32_t p = st & 0xffu, s = ((st >> 8) & 0xffu) + 1u, v = (st >> 16) & 1u, c = (st >> 17) & 15u;
    uint32_t j = j0;
    raw = raw_below & ((1u << j0) - 1u);
#pragma nounroll
    while (j < R) {
        const uint32_t kh = (16u - c) & 15u;                                       // blocks in front of the next halving point
        if (p) {                                                                   // a run of raw copies
            uint32_t L = R - j;
            L = p < L ? p : L;
            raw |= ((1u << L) - 1u) << j;
            if (kh < L && s > 1u) s >>= 1;
            c = (c + L) & 15u; p -= L; j += L;
            if (p == 0) s = (s + 1u) & 0xffu;
        } else if (storm) {                                                        // one coded, incompressible block
            if (kh == 0 && s > 1u) s >>= 1;
            c = (c + 1u) & 15u; ++j;
            if (v) p = s;
            v = 1;
        } else {                                                                   // coded blocks to the round's end, none of them incompressible
            const uint32_t n = R - j;
            if (kh < n && s > 1u) s >>= 1;
            c = (c + n) & 15u; j = R; v = 0;
        }
    }
    end_state = (p & 0xffu) | (((s - 1u) & 0xffu) << 8) | (v << 16) | (c << 17);
}

// ordered rounds without unrest before the encoder speculates ACROSS rounds again: 2, and 2 more (at most 7) with every abort the chunk has seen —
// its count, up to 3, rides in bits 24..25 of the commit payload.  (Same box, round 5: leaving after 2 quiet rounds is as fast as round 4's library
// on text at 1 GiB and 6 % faster at 10 MB — the cold start of every 64 KiB chunk is ordered rounds now, not block-by-block walks —, waiting for
// 6 always costs text 1.3 % / 10 % / 13 % at 1 GiB / 100 MB / 10 MB; data that flips every few KiB aborts a work-group per flip when it leaves early.)
__device__ __forceinline__ uint32_t quiet_rounds(uint32_t P1) { const uint32_t q = 2u + 2u * ((P1 >> 24) & 3u); return q > 7u ? 7u : q; }
constexpr uint32_t kStormRounds = 3;                                              // ordered rounds of one unbroken incompressible stretch before the dictionary token runs ahead of the commit
constexpr uint32_t kSpinLimit = 1u << 22, kPoison = 0xfffffffeu, kErrWatchdog = 16u;
__device__ __forceinline__ void wave_exit() { asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)\n\ts_endpgm" ::: "memory"); }
__device__ __forceinline__ void watchdog(uint32_t& spins, uint32_t sync_base, uint32_t* err, uint32_t lane) {
    if (__builtin_expect(++spins > kSpinLimit, 0)) {
        if (lane == 0) {
            if (err) atomicOr(err, kErrWatchdog);
            lds_poke(sync_base + kSyD, kPoison); lds_poke(sync_base + kSyD + 4, kPoison);
            lds_poke(sync_base + kSyO, kPoison); lds_poke(sync_base + kSyO + 4, kPoison);
            lds_poke(sync_base + kSyZ, kPoison);
        }
        wave_exit();
    }
}

// optional cycle accounting (DENSITY_HIP_PROF=1): work-group 0 reports, per wave, the cycles spent in each phase of its iterations
constexpr uint32_t kProfRounds = 2048;
template <bool ON>
struct PhaseClock;
template <>
struct PhaseClock<false> {
    __device__ __forceinline__ explicit PhaseClock(uint64_t*) {}
    __device__ __forceinline__ void start() {}
    __device__ __forceinline__ void mark(int) {}
    __device__ __forceinline__ void stamp(uint32_t, uint32_t, uint32_t) {}
    __device__ __forceinline__ void note(uint32_t, uint32_t, uint32_t) {}
    __device__ __forceinline__ void flush(uint32_t, uint32_t) {}
    __device__ __forceinline__ void count(int, uint32_t) {}
};
template <>
struct PhaseClock<true> {
    uint64_t* out; uint64_t t0 = 0; uint32_t ph[8] = {0, 0, 0, 0, 0, 0, 0, 0};   // (32-bit sums: the profiling instances are as short of registers as the shipped ones)
    __device__ __forceinline__ explicit PhaseClock(uint64_t* o) : out(o) {}
    __device__ __forceinline__ void start() { if (out) t0 = __builtin_readcyclecounter(); }
    __device__ __forceinline__ void mark(int k) { if (out) { const uint64_t t = __builtin_readcyclecounter(); ph[k] += (uint32_t)(t - t0); t0 = t; } }
    // per-round time stamps of the D chain (rounds < kProfRounds): 0 = started polling, 1 = token seen, 2 = exchanges + token done, 3 = round finished
    __device__ __forceinline__ void stamp(uint32_t r, uint32_t what, uint32_t lane) {
        if (out && r < kProfRounds && lane == 0) out[128 + 4 * r + what] = __builtin_readcyclecounter();
    }
    // a mark on a round (bit 0: it went through the zero-entry path)
    __device__ __forceinline__ void note(uint32_t r, uint32_t v, uint32_t lane) {
        if (out && r < kProfRounds && lane == 0) out[128 + 4 * kProfRounds + r] = v;
    }
    __device__ __forceinline__ void flush(uint32_t wave, uint32_t lane) { if (out && lane == 0) for (int k = 0; k < 8; ++k) out[8 * wave + k] = ph[k]; }
    // event counters of work-group 0 (encoder: 0 fast rounds committed, 1 ordered rounds that held, 2 ordered rounds taken back, 3 rounds
    // walked in order, 4 aborts raised, 5 ordered rounds that ran ahead)
    __device__ __forceinline__ void count(int k, uint32_t lane) { if (out && lane == 0) atomicAdd(reinterpret_cast<unsigned long long*>(out + 128 + 5 * kProfRounds + k), 1ull); }
};

// Waiting for a token.  The wave whose turn is next (or next but one) polls in a loop of five instructions; waves further away sleep
// for most of the distance first (a round hand-off takes a few hundred cycles), so that the LDS and the issue slots stay with
// the waves that work.
__device__ __forceinline__ void backoff(uint32_t dist) {
    if (dist <= 2) return;
    if (dist > 8) __builtin_amdgcn_s_sleep(24);
    else if (dist > 4) __builtin_amdgcn_s_sleep(8);
    else __builtin_amdgcn_s_sleep(3);
}
// the same between ORDERED rounds, whose hand-offs take a thousand cycles and more: only the next wave polls, the others nap for most of their distance
// (seven waves polling two 16-byte lines each kept the LDS busy enough to triple the round trip of the holder's own look-ups)
__device__ __forceinline__ void backoff_ordered(uint32_t dist) {
    if (dist <= 1) return;
    if (dist > 4) __builtin_amdgcn_s_sleep(40);
    else if (dist > 2) __builtin_amdgcn_s_sleep(20);
    else __builtin_amdgcn_s_sleep(8);
}
// up to `tries` back-to-back polls of one token word for one value
// (Written out: the compiled loop kept its counter in a vector register and took ten instructions per poll — every one of them between
// "the token is there" and the first exchange of the new holder.  Five here: read, wait, lane 0's copy, compare, branch; the count-down is
// issued while the read is in flight.)
__device__ __forceinline__ bool poll_word(uint32_t addr, uint32_t want, uint32_t tries) {
    uint32_t v, seen;
    asm volatile(
        "1:\n\t"
        "ds_read_b32 %[v], %[a]\n\t"
        "s_sub_u32 %[n], %[n], 1\n\t"
        "s_waitcnt lgkmcnt(0)\n\t"
        "v_readfirstlane_b32 %[s], %[v]\n\t"
        "s_cmp_eq_u32 %[s], %[w]\n\t"
        "s_cbranch_scc1 2f\n\t"
        "s_cmp_lg_u32 %[n], 0\n\t"
        "s_cbranch_scc1 1b\n"
        "2:"
        : [v] "=&v"(v), [s] "=&s"(seen), [n] "+s"(tries)
        : [a] "v"(addr), [w] "s"(want)
        : "scc", "memory");
    return seen == want;
}

// the same on a whole 16-byte line whose first word is the token: the line as it was when the token matched, or as last seen (four one-word reads in
// one round trip: a tuple register cannot be named word by word in an asm statement)
__device__ __forceinline__ bool poll_line(uint32_t addr, uint32_t want, uint32_t tries, u32x4& line) {
    uint32_t seen, w0, w1, w2, w3;
    asm volatile(
        "1:\n\t"
        "ds_read_b32 %[w0], %[a]\n\t"
        "ds_read_b32 %[w1], %[a] offset:4\n\t"
        "ds_read_b32 %[w2], %[a] offset:8\n\t"
        "ds_read_b32 %[w3], %[a] offset:12\n\t"
        "s_sub_u32 %[n], %[n], 1\n\t"
        "s_waitcnt lgkmcnt(0)\n\t"
        "v_readfirstlane_b32 %[s], %[w0]\n\t"
        "s_cmp_eq_u32 %[s], %[w]\n\t"
        "s_cbranch_scc1 2f\n\t"
        "s_cmp_lg_u32 %[n], 0\n\t"
        "s_cbranch_scc1 1b\n"
        "2:"
        : [w0] "=&v"(w0), [w1] "=&v"(w1), [w2] "=&v"(w2), [w3] "=&v"(w3), [s] "=&s"(seen), [n] "+s"(tries)
        : [a] "v"(addr), [w] "s"(want)
        : "scc", "memory");
    line = u32x4{w0, w1, w2, w3};
    return seen == want;
}

}  // namespace

// ---- host side, rotor.hip: the cycle accounting of a DENSITY_HIP_PROF=1 run (debug build; nullptr / nothing in the shipped library) ----
#define DENSITY_ROT_LOCAL __attribute__((visibility("hidden")))   // shared by the rotation files, not part of the library's interface
DENSITY_ROT_LOCAL uint64_t* rot_prof_buffer();
DENSITY_ROT_LOCAL void rot_prof_report(const char* what, const char* phases, uint64_t* buf, hipStream_t stream, uint32_t waves);

}  // namespace density
