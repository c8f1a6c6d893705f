// decode_walk.hip — the contexts of Cheetah's decode passes (gfx950): the one chain of the decoder, walked on 16-bit hashes in LDS.
// Compiled as part of decode_passes.hip (the overall design, PassArgs, the descriptors and the error words are there).
//
// prediction_map[last_hash] is read by predicted quads and written by the others (cheetah.rs:72,81,90,97-102,161: last_hash).  A quad's context is the
// hash of the quad before it: a MAP quad's hash is its item, a PLAIN quad's the hash of its value — in the descriptor either way —, a predicted quad's
// comes out of H[context], which holds per context the hash of the VALUE last left there (for a MAP quad that read a never-written 0, kDescZero, that is
// 0 and not its item).  The chain is only as long as its DEPENDENT links: a predicted quad's context is in the descriptors unless the quad before it was
// predicted too — in 100 MB of prose four of five predicted quads follow a quad that was not.  So per block of 64 quads (a quad per lane):
//   speculate  the contexts of the lanes behind predicted quads by plain READS of H as it stands, level by level (a lane's level = the predicted lanes
//              right in front of it: one LDS round trip per level for all 64 lanes, where a run-by-run walk pays one per run and quad);
//   execute    ALL 64 table operations in one ordered instruction (ds_mskor_rtn_b32 on the 16-bit halves: gfx950 serves the lanes of one LDS
//              instruction in ascending order — §4.2 of DESIGN.md, verified at start-up —, a predicted lane reads, the others write H[context]);
//   verify     a predicted lane must have read in the ordered pass what its successors' contexts were derived from.  If every one did, the contexts
//              ARE the sequential ones (induction over the lanes: lane 0's context is the running one; if lanes 0..i hold the right contexts the
//              ordered pass did to H exactly what cheetah.rs:72,81,90,97-102 do up to quad i, so what lane i read is right, and with it lane i+1's
//              context).  If lane i0 is the first that read something else (a context written earlier in the SAME block: "the " twice within 256
//              bytes with two followers), lanes 0..i0 stand, the lanes behind it take their writes back — old halves, highest lane first: the lane-
//              reversed store of rotor.hip — and go again from what lane i0 really read.
// kTeamBlocks blocks (128 quads, a register per block and lane) go through speculate / execute / verify TOGETHER: the levels' reads of all of them are
// in flight at once and the ordered pass is kTeamBlocks instructions back to back (a wave's LDS instructions execute in issue order: block 0's lanes,
// then block 1's), so they share the LDS round trips; a wrong speculation costs one more pass over the chain behind it.
//
// A TEAM of waves (round 6).  One wave spends its time ISSUING: ~380 instructions per 128 quads at one instruction per five cycles — classification, the
// speculative reads level by level, the bookkeeping — and only ~500 cycles of those 2,500 in what must happen in stream order (the ordered pass over H
// and its verification).  So kTeam waves of one work-group share the chunk's H: wave w takes the groups g = w (mod kTeam) of 128 quads, does everything
// that needs no order AHEAD of its turn — its descriptors come straight from memory into registers one iteration of its own ahead, the speculative reads see H
// as it stands, groups of other waves not yet applied: speculation may be as stale as it likes, the verification does not care how a context was
// guessed — and then, holding the token (an LDS word: the group whose turn it is; the running context travels beside it):
//   patch      lane 0's context, if the quad before the group was predicted (its hash is the predecessor's to tell);
//   execute    the ordered pass, verify, take back and go again from the first wrong read until every lane stands;
//   hand on    the running context and the token; the contexts are stored behind that.
// Groups this form does not take — a raw-copy block, the chunk's end, a run of eight and more predicted quads (periodic input, zeros: a level costs what
// a link does) — are walked block by block under the token, run by run.  A wave's LDS operations execute in issue order and the token is written behind
// them: whoever sees it sees H after them (§4.2).
namespace density {
namespace {

// Geometry (fixed in round 6; the builds it was chosen from — other team sizes, 1 and 4 blocks a turn, reads further ahead — and their times: DESIGN.md,
// "Geometry A/B on one box"): waves of a team, blocks of 64 quads a turn, how many turns ahead of its own a wave starts its speculative reads.
constexpr uint32_t kTeam = 4, kTeamBlocks = 2, kTeamAhead = 1;
constexpr uint32_t kWalkTable = 65536u * 2u, kTeamLds = kWalkTable + 64;      // H | {the group whose turn it is, the running context}

// lane-mask select: mask[lane] ? a : b with the mask in a scalar register pair (one VALU instruction; the compiler's own form of "(m >> lane) & 1" is three)
__device__ __forceinline__ uint32_t msel(uint64_t m, uint32_t ifset, uint32_t ifclear) {
    uint32_t r;
    asm("v_cndmask_b32_e64 %0, %1, %2, %3" : "=v"(r) : "v"(ifclear), "v"(ifset), "s"(m));
    return r;
}
// the group's LDS operations issued back to back and waited for inside ONE statement (an answer in flight lives in a register the compiler believes
// written: nothing but the wait may stand between issue and use)
static_assert(kTeamBlocks == 2, "the group helpers and the block-by-block arm are written out for two blocks");
__device__ __forceinline__ void lds_read_u16_group(uint32_t (&r)[kTeamBlocks], const uint32_t (&addr)[kTeamBlocks]) {
    asm volatile("ds_read_u16 %0, %2\n\tds_read_u16 %1, %3\n\ts_waitcnt lgkmcnt(0)" : "=&v"(r[0]), "=&v"(r[1]) : "v"(addr[0]), "v"(addr[1]) : "memory");
}
__device__ __forceinline__ void lds_mskor_group(uint32_t (&r)[kTeamBlocks], const uint32_t (&addr)[kTeamBlocks], const uint32_t (&mk)[kTeamBlocks], const uint32_t (&vl)[kTeamBlocks]) {
    asm volatile("ds_mskor_rtn_b32 %0, %2, %4, %6\n\tds_mskor_rtn_b32 %1, %3, %5, %7\n\ts_waitcnt lgkmcnt(0)"
                 : "=&v"(r[0]), "=&v"(r[1]) : "v"(addr[0]), "v"(addr[1]), "v"(mk[0]), "v"(mk[1]), "v"(vl[0]), "v"(vl[1]) : "memory");
}
// One block of 64 quads that all take part, some of them predicted (not all): the chain run by run, hand-written — a lone wave issues one instruction
// every 4-5 cycles, and under the token the team is one wave, so the instruction count IS the walk's time (the compiled form of the scalar loop in the
// kernel's block-by-block arm spends ~110 instructions per run, this one ~29).  Per run of quads that are not predicted ONE ordered 16-bit store under
// an exec mask (each writes H[its context] = its hash, cheetah.rs:72,81,90; the first one's context is the running one, patched into its lane), per
// predicted quad one LDS round trip (:97-102).
// (v_writelane takes its lane from M0: an SGPR value and an SGPR lane select in one instruction break gfx9's one-scalar rule)
// State in the loop: `c2` = LDS address of H[running context]; `av` = per lane the LDS address of H[its context] (2 * hash of the quad before it,
// patched where the context is the running one) — the store's address operand and, shifted back, the context to report.
// c: the running context in, out; hw: what H takes for the lane's quad; returns every lane's context.
__device__ __forceinline__ uint32_t walk_chain_block(uint32_t lds0, uint32_t& c, uint32_t hprev, uint32_t h, uint32_t hw, uint64_t Pin) {
    const uint64_t P = ((uint64_t)rfl((uint32_t)(Pin >> 32)) << 32) | rfl((uint32_t)Pin);   // (wave-uniform by construction: said so to the register allocator)
    uint32_t av = lds0 + 2u * hprev;
    const uint32_t h2 = lds0 + 2u * h;                                      // what the running context becomes behind a quad that is not predicted
    uint64_t prem = P;
    uint32_t c2 = rfl(lds0 + 2u * c);
    uint32_t s_pos, s_p, s_r, v_t, v_u, s_m0;
    uint64_t s_m;
    asm volatile(
        "s_mov_b32 %[m0s], m0\n\t"                                            // (M0 is the compiler's: handed back as found)
        "s_mov_b32 %[pos], 0\n"
        "1:\n\t"                                                             // ---- next run of quads that are not predicted: [pos, p)
        "s_ff1_i32_b64 %[p], %[prem]\n\t"
        "s_min_u32 %[p], %[p], 64\n\t"                                       // (no predicted quad left: -1 -> 64)
        "s_sub_u32 %[r], %[p], %[pos]\n\t"
        "s_cmp_eq_u32 %[r], 0\n\t"
        "s_cbranch_scc1 2f\n\t"
        "s_bfm_b64 %[m], %[r], %[pos]\n\t"                                   // r bits from pos on (r < 64: some quad is predicted)
        "s_mov_b32 m0, %[pos]\n\t"
        "s_add_u32 %[r], %[p], -1\n\t"
        "v_writelane_b32 %[av], %[c2], m0\n\t"
        "s_mov_b64 exec, %[m]\n\t"
        "ds_write_b16 %[av], %[h]\n\t"
        "s_mov_b64 exec, -1\n\t"
        "v_readlane_b32 %[c2], %[h2], %[r]\n"
        "2:\n\t"
        "s_cmp_ge_u32 %[p], 64\n\t"
        "s_cbranch_scc1 4f\n\t"
        "v_mov_b32 %[t], %[c2]\n"
        // ---- a predicted quad at lane p: c <- H[c] (cheetah.rs:97-102).  Round 4: the chain is the read, one add and the branch — ~85 cycles
        // instead of ~105.  The address of H[c] (`t`, the same in every lane) goes into lane p's `av` by a select under a one-lane mask, the
        // bookkeeping and the test "is the next quad predicted too" are issued while the read is in flight (its answer lands in `u`, so `t`
        // stays readable), and the scalar copy of the context is taken once per run instead of once per quad.
        "3:\n\t"
        "ds_read_u16 %[u], %[t]\n\t"
        "s_bfm_b64 %[m], 1, %[p]\n\t"
        "s_bitset0_b64 %[prem], %[p]\n\t"
        "s_add_u32 %[p], %[p], 1\n\t"
        "v_cndmask_b32_e64 %[av], %[av], %[t], %[m]\n\t"
        "s_bitcmp1_b64 %[prem], %[p]\n\t"                                    // (p == 64 tests bit 0, which is clear by now: lane 0 was either not predicted or has been taken)
        "s_waitcnt lgkmcnt(0)\n\t"
        "v_lshl_add_u32 %[t], %[u], 1, %[lds0]\n\t"
        "s_cbranch_scc1 3b\n\t"
        "s_nop 0\n\t"
        "v_readfirstlane_b32 %[c2], %[t]\n\t"
        "s_cmp_ge_u32 %[p], 64\n\t"
        "s_cbranch_scc1 4f\n\t"
        "s_mov_b32 %[pos], %[p]\n\t"
        "s_branch 1b\n"
        "4:\n\t"
        "s_mov_b32 m0, %[m0s]\n\t"
        : [av] "+v"(av), [c2] "+s"(c2), [prem] "+s"(prem), [pos] "=&s"(s_pos), [p] "=&s"(s_p), [r] "=&s"(s_r), [m] "=&s"(s_m), [t] "=&v"(v_t), [u] "=&v"(v_u), [m0s] "=&s"(s_m0)
        : [h] "v"(hw), [h2] "v"(h2), [lds0] "s"(lds0)
        : "memory", "scc");
    c = (c2 - lds0) >> 1;
    return (av - lds0) >> 1;
}

__global__ __launch_bounds__(kTeam * 64) void cheetah_walk_team(PassArgs a) {
    constexpr uint32_t G = kTeamBlocks;                                             // (every per-block loop below is unrolled over it)
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t wave = rfl(threadIdx.x >> 6);
    const uint64_t chunk = blockIdx.x;
    const ChunkInfo ci = a.info[chunk];
    if (ci.bad) return;
    const uint32_t nsteps = ci.blocks * kRecQuads;
    const uint32_t nblk = (nsteps + 63u) / 64u;
    const uint32_t ngroups = (nblk + G - 1u) / G;
    const uint64_t s0 = chunk * (a.out_stride / 4);
    const uint32_t* __restrict__ desc = a.desc + s0;
    uint16_t* __restrict__ ctx = a.ctx + s0;
    {   // H starts as the hash of the reference's zeroed prediction table: hash(0) = 0; token 0, running context 0 (cheetah.rs:52)
        uint4* p = reinterpret_cast<uint4*>(pass_lds);
        for (uint32_t i = threadIdx.x; i < kTeamLds / 16; i += kTeam * 64) p[i] = make_uint4(0, 0, 0, 0);
        __syncthreads();
    }
    const uint32_t lds0 = lds_addr(pass_lds);
    const uint32_t token = lds0 + kWalkTable;                                       // {the group whose turn it is, the running context in front of it}: one 8-byte word
    uint32_t nd[G], nprev = 0;
    auto fetch = [&](uint32_t g) {
#pragma unroll
        for (uint32_t b = 0; b < G; ++b) {
            const uint32_t i = (g * G + b) * 64u + lane;
            nd[b] = i < nsteps ? desc[i] : kDescNone;
        }
        nprev = g ? desc[g * G * 64u - 1u] : 0u;                                      // the quad in front of the group
    };
    if (wave < ngroups) fetch(wave);
    for (uint32_t g = wave; g < ngroups; g += kTeam) {
        const uint32_t blk = g * G;
        uint32_t dv[G], hv[G], hwv[G], cvv[G], rsv[G], rfv[G], r2v[G], shv[G];
        uint64_t Pm[G], Nm[G], K0m[G], known[G], fin[G], rdone[G];
        const uint32_t dprev = rfl(nprev);
        bool ok = blk + G <= nblk;
#pragma unroll
        for (uint32_t b = 0; b < G; ++b) {
            dv[b] = nd[b];
            hv[b] = dv[b] & 0xffffu;
            hwv[b] = (dv[b] & kDescZero) ? 0u : hv[b];
            const bool none = (dv[b] & kDescNone) != 0, pred = ((dv[b] >> 16) & 3u) == kFlagPred;
            Pm[b] = ballot64(!none && pred); Nm[b] = ballot64(!none && !pred);
            uint64_t lr = Pm[b] & (Pm[b] >> 1); lr &= lr >> 2; lr &= lr >> 4;
            ok = ok && (Pm[b] | Nm[b]) == ~0ull && lr == 0;
        }
        if (g + kTeam < ngroups) fetch(g + kTeam);                                    // in flight across this turn
        // the context in front of the group, where the descriptors tell it: the hash of a quad that took part and was not predicted
        const bool c_known = g == 0 || (!(dprev & kDescNone) && ((dprev >> 16) & 3u) != kFlagPred);
        const uint32_t c_spec = g == 0 ? 0u : (dprev & 0xffffu);
        // speculate: every level's reads of all G blocks in flight together (lanes whose context is known and who have not read yet)
        auto speculate = [&]() __attribute__((always_inline)) {
            for (;;) {
                uint64_t R[G], any = 0;
#pragma unroll
                for (uint32_t b = 0; b < G; ++b) { R[b] = Pm[b] & known[b] & ~rdone[b]; any |= R[b]; }
                if (!any) break;
                uint32_t r[G], ad[G];
#pragma unroll
                for (uint32_t b = 0; b < G; ++b) ad[b] = lds0 + 2u * cvv[b];
                lds_read_u16_group(r, ad);                                             // (every block reads, whether or not one of its lanes needs it: a stale context is a valid address)
#pragma unroll
                for (uint32_t b = 0; b < G; ++b) {
                    const uint64_t in = (R[b] << 1) | (b == 0 ? 0ull : (R[b ? b - 1 : 0] >> 63));   // the lanes that learn their context this round
                    if (R[b]) rsv[b] = msel(R[b], r[b], rsv[b]);
                    if (in) {
                        uint32_t up = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)r[b], 0x138, 0xf, 0xf, false);   // wave_shr:1
                        if (b != 0 && (in & 1ull)) { const uint32_t carry = (uint32_t)__builtin_amdgcn_readlane((int)r[b ? b - 1 : 0], 63); up = lane == 0 ? carry : up; }
                        cvv[b] = msel(in, up, cvv[b]);
                    }
                    known[b] |= in; rdone[b] |= R[b];
                }
            }
        };
        // the ordered pass's operands: made AHEAD of the turn too (only a patched lane 0 or a wrong read makes them again)
        uint32_t xa[G], xm[G], xv[G];
        auto prepare_exec = [&]() __attribute__((always_inline)) {
#pragma unroll
            for (uint32_t b = 0; b < G; ++b) {
                shv[b] = (cvv[b] & 1u) * 16u;
                const uint64_t w = Nm[b] & ~fin[b];
                xa[b] = lds0 + ((2u * cvv[b]) & ~3u);
                xm[b] = msel(w, 0xffffu << shv[b], 0u); xv[b] = msel(w, hwv[b] << shv[b], 0u);
            }
        };
        if (ok) {
#pragma unroll
            for (uint32_t b = 0; b < G; ++b) {
                const uint32_t hp = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)hv[b], 0x138, 0xf, 0xf, false);   // wave_shr:1
                const uint32_t first = b == 0 ? c_spec : (uint32_t)__builtin_amdgcn_readlane((int)hv[b ? b - 1 : 0], 63);   // (meaningful only where the quad before was not predicted)
                cvv[b] = lane == 0 ? first : hp;
                K0m[b] = (Nm[b] << 1) | (b == 0 ? (c_known ? 1ull : 0ull) : (Nm[b ? b - 1 : 0] >> 63));
                known[b] = K0m[b]; fin[b] = 0; rsv[b] = 0; rfv[b] = 0; rdone[b] = 0;
            }
            if (g >= kTeamAhead) {                                                    // not before my turn is kTeamAhead turns away: what is read earlier is stale more often than not
                for (uint32_t spins = 0; spins < kSpinLimit; ++spins) {
                    uint32_t seen;
                    asm volatile("ds_read_b32 %0, %1\n\ts_waitcnt lgkmcnt(0)" : "=v"(seen) : "v"(token) : "memory");
                    seen = rfl(seen);
                    if (seen + kTeamAhead >= g) break;
                }
            }
            speculate();                                                              // AHEAD of my turn: H as it stands
            prepare_exec();
        }
        // ---- my turn ----
        uint32_t c;
        {
            bool poisoned = false;
            for (uint32_t spins = 0;; ++spins) {
                uint64_t tc;
                asm volatile("ds_read_b64 %0, %1\n\ts_waitcnt lgkmcnt(0)" : "=v"(tc) : "v"(token) : "memory");
                const uint32_t seen = rfl((uint32_t)tc);
                if (seen == g) { c = rfl((uint32_t)(tc >> 32)); break; }
                if (seen == kPoison || spins > kSpinLimit) {
                    if (seen != kPoison && lane == 0) { atomicOr(a.err, kErrWatchdog); *reinterpret_cast<volatile uint32_t*>(pass_lds + kWalkTable) = kPoison; }
                    poisoned = true;
                    break;
                }
            }
            if (poisoned) break;
        }
        if (ok) {
            if (!c_known) {                                                          // the predecessor's last quad was predicted (or took no part): its hash is what the predecessor says
                cvv[0] = lane == 0 ? c : cvv[0];
                K0m[0] |= 1ull; known[0] |= 1ull;
                speculate();                                                          // (what lane 0's context sets free)
                prepare_exec();
            }
            for (;;) {
                // execute: the lanes that do not stand yet, block after block, each in lane order
                uint32_t ret[G];
                lds_mskor_group(ret, xa, xm, xv);
                // verify
                uint64_t bad[G], anybad = 0;
#pragma unroll
                for (uint32_t b = 0; b < G; ++b) {
                    r2v[b] = (ret[b] >> shv[b]) & 0xffffu;
                    // a predicted lane that has not read at all yet (its context never became known: cannot happen once lane 0's is) counts as wrong
                    bad[b] = (ballot64(r2v[b] != rsv[b]) | ~rdone[b]) & Pm[b] & ~fin[b];
                    anybad |= bad[b];
                }
                if (__builtin_expect(anybad == 0, 1)) {
#pragma unroll
                    for (uint32_t b = 0; b < G; ++b) rfv[b] = msel(~fin[b], r2v[b], rfv[b]);
                    break;
                }
                uint32_t b0 = 0;
#pragma unroll
                for (uint32_t b = G; b-- > 0;) if (bad[b]) b0 = b;
                uint64_t badb = bad[0];
#pragma unroll
                for (uint32_t b = 1; b < G; ++b) badb = b0 == b ? bad[b] : badb;
                const uint32_t i0 = (uint32_t)__builtin_ctzll(badb);
                const uint64_t upto = (2ull << i0) - 1ull;                           // lanes 0 .. i0 of block b0 (i0 == 63: all of them)
                uint64_t stands[G];
#pragma unroll
                for (uint32_t b = 0; b < G; ++b) stands[b] = b < b0 ? ~0ull : b == b0 ? upto : 0ull;
                // the writes behind the first wrong read are taken back: old halves, the latest write first (blocks from the last to b0, lanes reversed)
#pragma unroll
                for (uint32_t b = G; b-- > 0;) {
                    const uint64_t undo = Nm[b] & ~stands[b] & ~fin[b];
                    if (undo) {
                        const uint32_t ar = bperm(63u - lane, lds0 + 2u * cvv[b]), old = bperm(63u - lane, r2v[b]);
                        if ((undo >> (63u - lane)) & 1ull) asm volatile("ds_write_b16 %0, %1" ::"v"(ar), "v"(old) : "memory");
                    }
                }
                // (r2v[b0], in the spelling the measured kernel was compiled from: "b0 == 0 ? r2v[0] : r2v[1]" gives the same instructions on other registers)
                const uint32_t truth = (uint32_t)__builtin_amdgcn_readlane((int)(b0 == 0 ? r2v[0] : b0 == 1 ? r2v[G > 1 ? 1 : 0] : b0 == 2 ? r2v[G > 2 ? 2 : 0] : r2v[G > 3 ? 3 : 0]), (int)i0);
                bool all = true;
                uint64_t nextm[G];
#pragma unroll
                for (uint32_t b = 0; b < G; ++b) {
                    rfv[b] = msel(stands[b] & ~fin[b], r2v[b], rfv[b]);
                    fin[b] = stands[b];
                    all = all && fin[b] == ~0ull;
                    // the lane behind (b0, i0) now knows its context; everything else behind it is as unknown as before the first round
                    const uint64_t next = b == b0 ? (i0 == 63u ? 0ull : (2ull << i0) & ~upto) : (b == b0 + 1u && i0 == 63u ? 1ull : 0ull);
                    if (next) cvv[b] = msel(next, truth, cvv[b]);
                    nextm[b] = next;
                }
                if (all) break;
                // What has to be guessed again is the CHAIN behind the wrong read — the lane that now knows its context, the run of predicted lanes it starts
                // and the lane behind that run —, not the block: every other lane's context and speculative read are as good a guess as they were, and the
                // next verification holds all of them to the ordered pass again.  (A chain that runs on into the next block: everything behind the wrong read, as before.)
                const uint32_t cb = i0 == 63u ? b0 + 1u : b0, start = i0 == 63u ? 0u : i0 + 1u;
                uint64_t pcb = Pm[0];
#pragma unroll
                for (uint32_t b = 1; b < G; ++b) pcb = cb == b ? Pm[b] : pcb;
                const uint64_t inv = ~(pcb >> start);
                const uint32_t end = start + (inv ? (uint32_t)__builtin_ctzll(inv) : 64u);   // the lane behind the run (the chain's last)
                if (end <= 63u) {
                    const uint64_t A = ((2ull << end) - 1ull) & ~((1ull << start) - 1ull);
#pragma unroll
                    for (uint32_t b = 0; b < G; ++b)
                        if (b == cb) { known[b] = (known[b] & ~A) | nextm[b]; rdone[b] &= ~A; }
                } else {
#pragma unroll
                    for (uint32_t b = 0; b < G; ++b) { known[b] = fin[b] | nextm[b] | K0m[b]; rdone[b] = fin[b]; }
                }
                speculate();
                prepare_exec();
            }
            const uint32_t last = msel(Pm[G - 1], rfv[G - 1], hv[G - 1]);
            c = (uint32_t)__builtin_amdgcn_readlane((int)last, 63);
        } else {
            // block by block, run by run (cheetah.rs:97-102).  A block with quads that take no part (a raw-copy block's, the chunk's end) goes through the
            // scalar loop below, stepping over them: the context passes through (codec.rs:89-91: a raw block touches no state); so does a block whose
            // quads are all predicted or all not.
            // (one_block is written out per block: left as a loop over b the compiler keeps it rolled and the masks in vector registers)
            auto one_block = [&](auto bc) __attribute__((always_inline)) {
                constexpr uint32_t b = decltype(bc)::value;
                if (blk + b >= nblk) { cvv[b] = 0; return; }
                const uint32_t h = hv[b], hw = hwv[b];
                const uint64_t P = Pm[b], N = Nm[b], active = P | N;
                const uint32_t hprev = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)h, 0x138, 0xf, 0xf, false);   // wave_shr:1
                if (active == ~0ull && P != 0 && P != ~0ull) {                        // every quad takes part, some are predicted: the hand-written chain
                    cvv[b] = walk_chain_block(lds0, c, hprev, h, hw, P);
                    return;
                }
                uint32_t cv = 0, pos = 0;
                while (pos < 64u) {
                    const uint64_t rest = active >> pos;
                    if (!rest) break;
                    pos += (uint32_t)__builtin_ctzll(rest);
                    if ((N >> pos) & 1ull) {
                        const uint64_t inv = ~(N >> pos);
                        const uint32_t r = inv ? (uint32_t)__builtin_ctzll(inv) : 64u - pos;
                        const bool in = lane >= pos && lane < pos + r;
                        const uint32_t mine = lane == pos ? c : hprev;
                        if (in) {
                            cv = mine;
                            asm volatile("ds_write_b16 %0, %1" ::"v"(lds0 + 2u * mine), "v"(hw) : "memory");
                        }
                        c = (uint32_t)__builtin_amdgcn_readlane((int)h, (int)(pos + r - 1u));
                        pos += r;
                    } else {
                        const uint64_t inv = ~(P >> pos);
                        const uint32_t r = inv ? (uint32_t)__builtin_ctzll(inv) : 64u - pos;
                        for (uint32_t t = 0; t < r; ++t) {
                            if (lane == pos + t) cv = c;
                            uint32_t nx;
                            asm volatile("ds_read_u16 %0, %1\n\ts_waitcnt lgkmcnt(0)" : "=v"(nx) : "v"(lds0 + 2u * c) : "memory");
                            nx = rfl(nx);
                            if (nx == c) {                                             // a fixed point: the table does not change inside a run
                                if (lane > pos + t && lane < pos + r) cv = c;
                                break;
                            }
                            c = nx;
                        }
                        pos += r;
                    }
                }
                cvv[b] = cv;
            };
            one_block(std::integral_constant<uint32_t, 0>{});
            one_block(std::integral_constant<uint32_t, 1>{});
        }
        // hand on: the token and the running context in one 8-byte write, behind everything this turn did to H (a wave's LDS operations execute as issued)
        {
            const uint64_t tc = (uint64_t)(g + 1u) | ((uint64_t)c << 32);
            asm volatile("ds_write_b64 %0, %1" ::"v"(token), "v"(tc) : "memory");
        }
#pragma unroll
        for (uint32_t b = 0; b < G; ++b) { const uint32_t i = (blk + b) * 64u + lane; if (i < nsteps) ctx[i] = (uint16_t)cvv[b]; }
    }
}

}  // namespace
}  // namespace density
