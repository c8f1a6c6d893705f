// api_internal.hpp — what the three units of the C ABI share.  api.hip: per-device context, workspace plans, the container's device-side
// drivers (pack, unpage and slice are one: run_slice_container), the device-pointer and bookkeeping entry points.  api_stream.hip: ONE reference stream — the reference's nine symbols and their
// device-pointer forms, long Chameleon streams in parallel segments, staged or pipelined from host pointers.  api_host.hip: the host-pointer
// container calls, staged or pipelined in slices.  Here: geometry of the formats, the context, the kernel-variant bits, the workspace plans with
// their typed views, and the steps every driver repeats (workspace resolution, read-back, drain, slice arithmetic).  Internal to libdensity_hip.so.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdio>
#include <cstring>
#include <initializer_list>
#include <mutex>
#include <string>
#include <vector>

#include "../../include/density_hip.h"
#include "common.hpp"
#include "kernels.hpp"

namespace density {
namespace api {

constexpr int kMaxDevices = 16;
constexpr size_t kAlign = 256;
constexpr size_t kMaxChunk = 1u << 30;   // u32 size table: a chunk stream must stay below 4 GiB

extern thread_local std::string g_last_error;
extern int g_profiling;
extern int g_variant;                 // density_hip_set_kernel_variant
extern uint64_t g_pass_decodes;       // density_hip_decode_pass_count: Cheetah decodes served by the decode passes
extern uint64_t g_stream_stats[4];    // density_hip_stream_stats: long streams encoded in segments | encode passes | decoded in segments | long streams decoded sequentially
void set_error(const char* what, hipError_t e = hipSuccess);

// the bits of density_hip_set_kernel_variant, a test hook: include/density_hip.h says what each one selects (payload bytes are identical in every variant)
enum Variant : int {
    kVarSimple = 1, kVarNoIndex = 2, kVarRolePipeline = 4, kVarBatchedStitch = 8, kVarLaneCodec = 16, kVarWaveCodec = 32, kVarStageAudit = 64, kVarSerialDecode = 128,
    kVarPipeAlways = 256, kVarPipeNever = 512, kVarSerialParse = 1024, kVarRotorOtherSplit = 2048,   // (4096, 8192, 16384: reserved)
    kVarLionOneWave = 32768,
    kVarNoRotor = kVarSimple | kVarRolePipeline,   // either way the wave-rotation kernels, and with them segments and pages, are out
};
inline bool variant(int bits) { return (g_variant & bits) != 0; }

inline size_t align_up(size_t v, size_t a) { return (v + a - 1) / a * a; }

inline bool valid_algo(int algo) { return algo >= DENSITY_HIP_CHAMELEON && algo <= DENSITY_HIP_LION; }
// chunk_size 0 = automatic: one chunk is one work-group on one CU, so an input should be cut into at least as many chunks as the device has
// CUs (256) where that is possible without dropping below 64 KiB (small chunks restart the dictionary and cost ratio), and no finer than that
// (every chunk start costs a table clear and a few in-order rounds): never above 4 MiB, the largest chunk the index-fed decoder takes.
// 10 MB -> 64 KiB (156 chunks), 100 MB -> 384 KiB (255), 256 MiB -> 1 MiB, 1 GiB -> 4 MiB, 1.5 GiB -> 3 MiB (512).
// Lion runs one WAVE per chunk stream and is bound by memory latency per stream, not by a CU's LDS (below).  Cheetah's decode passes (decode_passes.hip) walk one chunk per CU, in time proportional to the chunk: one
// chunk per CU exactly — the input over 256, up to whole 4 KiB trips of the encoder's passes — between 64 KiB and 1 MiB (100 MB -> 384 KiB:
// ratio 1.67 where 64 KiB chunks gave 1.34, and a faster round trip).
inline size_t auto_chunk(size_t n, int algo = DENSITY_HIP_CHAMELEON) {
    if (algo == DENSITY_HIP_CHEETAH) {
        size_t c = align_up((n + 255) / 256, 4096);
        if (c < (64u << 10)) c = 64u << 10;
        if (c > (1u << 20)) c = 1u << 20;
        return c;
    }
    if (algo == DENSITY_HIP_CHAMELEON) {
        // (round 4: not a power of two any more.  A chunk is a work-group is a CU, so what counts is WHOLE WAVES of 256 chunks: 100 MB in 382 chunks
        // of 256 KiB is two rounds of work-groups, the second half empty; in 255 chunks of 384 KiB it is one — a quarter less time, and a better
        // ratio.  The fewest whole waves of chunks of at most 4 MiB, the input spread evenly over them in whole rounds of 16 blocks.)
        if (n <= 256u * (size_t)(64u << 10)) return 64u << 10;
        const size_t waves = (n + 256u * (size_t)(4u << 20) - 1) / (256u * (size_t)(4u << 20));
        size_t c = align_up((n + 256 * waves - 1) / (256 * waves), 4096);
        if (c < (64u << 10)) c = 64u << 10;
        if (c > (4u << 20)) c = 4u << 20;
        return c;
    }
    // Lion: one wave per chunk stream, bound by memory latency per stream — the largest power of two that still gives the device 700 streams (about three per CU)
    // (round 4, with two records per step: 100 MB in 128 KiB chunks runs as fast as round 3's 64 KiB chunks did, at ratio 1.41 instead of 1.28)
    size_t c = 1u << 20;
    while (c > (64u << 10) && n / c < 700) c >>= 1;
    return c;
}
inline size_t normalise_chunk(size_t chunk, size_t n, int algo = DENSITY_HIP_CHAMELEON) { return chunk == 0 ? auto_chunk(n, algo) : chunk; }
inline bool valid_chunk(size_t chunk) { return chunk >= 256 && chunk % 256 == 0 && chunk <= kMaxChunk; }
// a call's algorithm and chunk size (0 = automatic: *chunk becomes what it stands for) are ones the library takes
inline bool take_geometry(int algo, size_t n, size_t* chunk) { *chunk = normalise_chunk(*chunk, n, algo); return valid_algo(algo) && valid_chunk(*chunk); }
inline size_t chunk_count(size_t n, size_t chunk) { return (n + chunk - 1) / chunk; }
inline size_t index_base(size_t n_chunks) { return align_up(sizeof(density_hip_header_t) + 4 * n_chunks, 16); }
inline size_t index_bytes(size_t total_len, bool with_index) { return with_index ? (total_len + 255) / 256 : 0; }
inline size_t payload_base(size_t n_chunks, size_t total_len, bool with_index) { return align_up(index_base(n_chunks) + index_bytes(total_len, with_index), 16); }
inline bool want_index(int algo) { return algo == DENSITY_HIP_CHAMELEON && !variant(kVarNoIndex); }
// paged container (DENSITY_HIP_FLAG_PAGED): behind the block index the page directory (per chunk: 16 bytes {n_pages}, then 16 bytes per page), then,
// on the next page-size boundary of the container, the pages
inline size_t paged_dir_base(size_t n_chunks, size_t total_len) { return payload_base(n_chunks, total_len, true); }
inline uint32_t paged_pages_per_chunk(size_t chunk) { return pages_per_chunk(safe_size(DENSITY_HIP_CHAMELEON, chunk)); }
inline size_t paged_dir_bytes(size_t n_chunks, size_t chunk) { return 4 * (size_t)page_dir_words(paged_pages_per_chunk(chunk)) * n_chunks; }
inline size_t paged_pages_base(size_t n_chunks, size_t total_len, size_t chunk) { return align_up(paged_dir_base(n_chunks, total_len) + paged_dir_bytes(n_chunks, chunk), kAlign); }
// what the paged form is for: Chameleon, chunks of 1 MiB and more (a chunk's last page is half empty on average: 3 % of a MiB of text), 32-bit positions
// — and of at most 4 MiB: only the index-fed rotation decoder reads pages in place (kPagedMaxChunk = its kRotMaxBlocks blocks, its directory copy holds
// kPagedMaxPages pages), and the library writes no container it cannot read
inline bool paged_eligible(int algo, size_t n, size_t chunk) {
    const size_t nc = chunk_count(n, chunk);
    return algo == DENSITY_HIP_CHAMELEON && want_index(algo) && nc > 1 && chunk >= (1u << 20) && chunk <= kPagedMaxChunk && paged_pages_per_chunk(chunk) <= kPagedMaxPages &&
           (uint64_t)nc * paged_pages_per_chunk(chunk) * kPageBytes < (1ull << 32);
}
size_t container_bound_paged(int algo, size_t n, size_t chunk);
inline size_t slot_stride(int algo, size_t chunk) { return align_up(safe_size(algo, chunk), kAlign); }
// sealed container (DENSITY_HIP_FLAG_CHECKSUM): the trailer of a word per chunk at the container's end, and what sealing can add to a bound (the gap in front of it too)
inline size_t trailer_bytes(size_t n_chunks) { return align_up(4 * n_chunks, 16); }
inline size_t header_trailer(const density_hip_header_t& h) { return (h.flags & DENSITY_HIP_FLAG_CHECKSUM) ? trailer_bytes(h.n_chunks) : 0; }
inline size_t seal_overhead(size_t n_chunks) { return 16 + trailer_bytes(n_chunks); }
// the parity blob "DHP1" of an input of n bytes cut every `chunk` (valid) bytes, `requested` groups asked for: its header (n_chunks must fit 32 bits), its size
// (version 1: the P rows; version 2: as many Q rows behind them), and the longest group — version 2 takes 255 members: 2 has order 255 in GF(2^8)
inline density_hip_parity_header_t make_parity_header(size_t n, size_t chunk, uint32_t requested, uint8_t version = 1) {
    const size_t n_chunks = chunk_count(n, chunk);
    return density_hip_parity_header_t{DENSITY_HIP_PARITY_MAGIC, version, 0, 0, (uint32_t)chunk, (uint32_t)n_chunks, n, (uint32_t)std::min<size_t>(requested, n_chunks),
                                       (uint32_t)align_up(std::min(n, chunk), 16)};
}
inline size_t parity_bytes(const density_hip_parity_header_t& ph) { return sizeof(ph) + (size_t)ph.version * ph.n_groups * ph.row_bytes; }
inline size_t parity_group_members(const density_hip_parity_header_t& ph) { return ph.n_groups ? ((size_t)ph.n_chunks + ph.n_groups - 1) / ph.n_groups : 0; }
constexpr size_t kParityQMembers = 255;
// the scratch of a seal in a workspace: the error word, the geometry the device reads from the container's header, a word per chunk (of which an
// input of n bytes has at most one per 256 bytes)
struct SealPlan {
    size_t total;
    uint32_t* err(uint8_t* ws) const { return reinterpret_cast<uint32_t*>(ws); }
    uint32_t* geom(uint8_t* ws) const { return reinterpret_cast<uint32_t*>(ws + 64); }
    uint32_t* acc(uint8_t* ws) const { return reinterpret_cast<uint32_t*>(ws + kAlign); }
};
inline SealPlan plan_seal(size_t n) { return SealPlan{kAlign + align_up(4 * ((n + 255) / 256) + 4, kAlign)}; }

struct Buffer {
    void* p = nullptr;
    size_t cap = 0;
    hipError_t ensure(size_t n) {
        if (n <= cap) return hipSuccess;
        if (p) { hipError_t e = hipFree(p); p = nullptr; cap = 0; if (e != hipSuccess) return e; }
        const size_t want = align_up(n + n / 8, 1 << 20);
        hipError_t e = hipMalloc(&p, want);
        if (e != hipSuccess) { p = nullptr; return e; }
        cap = want;
        return hipSuccess;
    }
};

// pinned host memory of the context (the device's copies to and from it are asynchronous); grows like Buffer
struct PinnedBuffer {
    uint8_t* p = nullptr;
    size_t cap = 0;
    hipError_t ensure(size_t n) {
        if (n <= cap) return hipSuccess;
        release();
        const size_t want = align_up(n + n / 2, 4096);
        const hipError_t e = hipHostMalloc((void**)&p, want, hipHostMallocDefault);
        if (e == hipSuccess) cap = want;
        return e;
    }
    void release() { if (p) (void)hipHostFree(p); p = nullptr; cap = 0; }
};

struct DeviceCtx {
    std::mutex mu;
    bool ready = false, selftest_ok = false;
    uint32_t selftest_bits = 0;
    hipStream_t stream = nullptr, stitch_stream = nullptr;   // stitch_stream: the compaction of one batch of chunks beside the encoding of the next
    hipEvent_t batch_done[8] = {}, stitch_done = nullptr;
    Buffer work, stage_in, stage_out, seg;   // seg: scratch of the segmented stream encode
    // the pipelined host-pointer container calls: an upload, a download and four kernel streams, events per slice, the slice sizes in pinned memory
    hipStream_t up = nullptr, down = nullptr, kern[4] = {};
    std::vector<hipEvent_t> pipe_events;
    PinnedBuffer pin_sizes;                  // the pipelined container encode: the running end of the container behind every slice
    PinnedBuffer pin_meta;                   // the pipelined stream calls: per segment sizes, offsets, states as the device reports them
    // profiling: event marks accumulated since the last density_hip_last_timings() (name == nullptr opens a call)
    std::vector<hipEvent_t> events;
    std::vector<const char*> names;
    size_t n_marks = 0;
};
constexpr size_t kMaxMarks = 8192;

extern DeviceCtx g_ctx[kMaxDevices];
// Returns the context of the current device with its internal stream created and the LDS self-test passed.
DeviceCtx* acquire_ctx();

struct Profiler {
    DeviceCtx* c;
    hipStream_t s;
    bool on;
    Profiler(DeviceCtx* ctx, hipStream_t stream) : c(ctx), s(stream), on(g_profiling != 0) { mark(nullptr); }
    void mark(const char* name) {
        if (!on) return;
        if (c->n_marks >= kMaxMarks) { on = false; return; }
        if (c->n_marks >= c->events.size()) {
            hipEvent_t ev;
            if (hipEventCreate(&ev) != hipSuccess) { on = false; return; }
            c->events.push_back(ev);
            c->names.push_back(nullptr);
        }
        c->names[c->n_marks] = name;
        (void)hipEventRecord(c->events[c->n_marks++], s);
    }
};

// A caller's buffer pinned in place for the duration of a call (hipHostRegister: microseconds on this platform, probes/host_register.hip), so that
// copies from and to it are asynchronous.  Where pinning fails (memory that is already registered, read-only mappings) the staged paths are taken.
// What a successful registration is worth: the runtime keeps pins of its own pageable copies in a cache, and a register over a larger extent of a
// buffer it has such a pin for can "succeed" with the cached pin's pages and no more — the pages behind them stay unmapped and the first access
// faults the GPU (round 4).  Round 5 looked for a check (probes/host_register_trap.hip, profiles/r05_probe_host_register_trap.txt): for a clean and
// for a suspect registration alike hipHostGetDevicePointer translates the first and the last byte, hipMemGetAddressRange reports base 0 and the
// full span, hipPointerGetAttributes the same type and pointers — nothing the API says tells them apart, and the minimal sequence (a pageable copy
// of part of a buffer, then the register) does not fault by itself.  So the defence stays where round 4 put it: THIS library never lets the runtime
// pin a caller's memory (copy_host_side_pinned below), and the translation of both ends is checked because it is free.  A caller whose OTHER
// libraries copy part of a buffer pageably and then hand us the whole of it can still meet the runtime's cache; bounce buffers of our own would
// close that at the price of a CPU copy of every byte (10 GB/s against the 40-50 the pipelined calls move).
struct PinnedInPlace {
    void* p = nullptr;
    PinnedInPlace(const void* q, size_t n) {
        if (!q || !n) return;
        void* host = const_cast<void*>(q);
        if (hipHostRegister(host, n, hipHostRegisterDefault) != hipSuccess) { (void)hipGetLastError(); return; }
        void *d0 = nullptr, *d1 = nullptr;
        const bool whole = hipHostGetDevicePointer(&d0, host, 0) == hipSuccess &&
                           hipHostGetDevicePointer(&d1, static_cast<uint8_t*>(host) + (n - 1), 0) == hipSuccess &&
                           static_cast<uint8_t*>(d1) - static_cast<uint8_t*>(d0) == (ptrdiff_t)(n - 1);
        if (whole) p = host;
        else { (void)hipGetLastError(); (void)hipHostUnregister(host); (void)hipGetLastError(); }
    }
    ~PinnedInPlace() { if (p) (void)hipHostUnregister(p); }
    PinnedInPlace(const PinnedInPlace&) = delete;
    PinnedInPlace& operator=(const PinnedInPlace&) = delete;
    explicit operator bool() const { return p != nullptr; }
};
// One copy between the caller's memory and the device on stream s, complete on return.  A megabyte and more: the caller's side is pinned in place for
// the copy's duration by US — never by the runtime's own pageable-copy path, which pins the caller's pages too and keeps the pin in a cache of its own
// (the last eight per queue) beyond the call.  A later hipHostRegister of the same buffer over a LARGER extent is then answered with the cached pin's
// pages and no more: the pages behind them are not mapped, and the first access faults the GPU (round 4: "memory access fault ... write access to a
// read-only page" on the last page of an output buffer — a staged decode had brought down a few bytes less into it than the pipelined call that
// followed registered; in a DENSITY_HIP_DEBUG build DENSITY_HIP_RAW_STAGED=1 brings the old copies back, tools/gpu_host_stream_sequence.py walks the sequence).
inline hipError_t copy_host_side_pinned(void* dst, const void* src, size_t n, hipMemcpyKind kind, hipStream_t s) {
    if (n == 0) return hipSuccess;
    const void* host = kind == hipMemcpyHostToDevice ? src : dst;
    // (the switch — debug builds only — is the round-4 fault's reproducer, tools/gpu_host_stream_sequence.py; a pin that fails leaves the copy pageable)
    const bool pin_it = n >= (1u << 20) && !debug_env("DENSITY_HIP_RAW_STAGED");
    PinnedInPlace pin(pin_it ? host : nullptr, n);
    const hipError_t e = hipMemcpyAsync(dst, src, n, kind, s), e2 = hipStreamSynchronize(s);
    return e != hipSuccess ? e : e2;
}
constexpr uint32_t kPipeMaxSlices = 48;
// the upload, download and kernel streams of the pipelined host-pointer calls and n_events events (api_host.hip)
bool pipe_streams(DeviceCtx* c, uint32_t n_events);
// The workspace of a device-pointer call: the caller's if it gave one — it must hold `need` — else the context's, grown to `own` (the container decode
// asks for the decode passes' scratch on top of `need`).  *ws_size, where wanted: what the workspace holds.
inline int resolve_workspace(DeviceCtx* c, void* d_workspace, size_t workspace_size, size_t need, size_t own, uint8_t** ws, size_t* ws_size = nullptr) {
    if (d_workspace && workspace_size < need) { set_error("workspace too small"); return DENSITY_HIP_ERR_CAPACITY; }
    const hipError_t e = d_workspace ? hipSuccess : c->work.ensure(own);
    if (e != hipSuccess) { set_error("workspace allocation", e); return DENSITY_HIP_ERR_RUNTIME; }
    *ws = (uint8_t*)(d_workspace ? d_workspace : c->work.p);
    if (ws_size) *ws_size = d_workspace ? workspace_size : c->work.cap;
    return DENSITY_HIP_OK;
}
// the staging buffers of a host-pointer call: its input and its output on the device, the context's workspace
inline hipError_t ensure_staging(DeviceCtx* c, size_t in_bytes, size_t out_bytes, size_t ws_bytes) {
    hipError_t e = c->stage_in.ensure(in_bytes);
    if (e == hipSuccess) e = c->stage_out.ensure(out_bytes);
    return e == hipSuccess ? c->work.ensure(ws_bytes) : e;
}
// The end of a pipelined call: every stream it used is synchronised whatever happened before — nothing may still be reading or writing the caller's
// buffers when they are unpinned — and the first error wins (`e`: the call's status so far).
inline hipError_t drain(hipError_t e, std::initializer_list<hipStream_t> streams) {
    for (hipStream_t q : streams) { const hipError_t x = hipStreamSynchronize(q); if (e == hipSuccess) e = x; }
    return e;
}
// slice k of a pipelined or batched call, `per` chunks to a slice: chunks [first, first + count) and their bytes [off, off + len) of the `total` plain bytes
struct Slice { uint32_t first, count; uint64_t off, len; };
inline Slice slice_of(uint32_t k, uint32_t per, size_t n_chunks, size_t chunk, size_t total) {
    const uint32_t first = k * per, count = first + per <= n_chunks ? per : (uint32_t)(n_chunks - first);
    const uint64_t off = (uint64_t)first * chunk;
    return {first, count, off, std::min<uint64_t>(total - off, (uint64_t)count * chunk)};
}
// The error word, and with it one more small object (a header, a size), back on the host: queued on s, complete on return.  What the bits of the
// word mean is the caller's business.
inline hipError_t read_back(hipStream_t s, const uint32_t* d_err, uint32_t* h_err, void* h_obj = nullptr, const void* d_obj = nullptr, size_t obj_bytes = 0) {
    hipError_t e = h_obj ? hipMemcpyAsync(h_obj, d_obj, obj_bytes, hipMemcpyDeviceToHost, s) : hipSuccess;
    if (e == hipSuccess) e = hipMemcpyAsync(h_err, d_err, sizeof(*h_err), hipMemcpyDeviceToHost, s);
    if (e == hipSuccess) e = hipStreamSynchronize(s);
    return e;
}

constexpr size_t kSerialSlots = 16384;   // concurrent chunk streams of the functional Cheetah/Lion kernels (one lane each; 12 / 28 GiB of tables when all are in use)
constexpr size_t kSerialTableBudget = 8ull << 30;   // ... but never more than 8 GiB of tables (the count comes from an untrusted header on decode): Cheetah 10922 streams, Lion 4681
inline size_t serial_slots(int algo, size_t n_chunks) {
    if (algo == DENSITY_HIP_CHAMELEON) return 0;
    const size_t by_memory = kSerialTableBudget / serial_table_bytes(algo);
    size_t cap = kSerialSlots < by_memory ? kSerialSlots : by_memory;
    if (const char* e = debug_env("DENSITY_HIP_SERIAL_SLOTS")) { const size_t v = (size_t)atoll(e); if (v >= 1 && v < cap) cap = v; }   // (debug builds: streams in flight, tools/gpu_lion_slots.py)
    return n_chunks < cap ? n_chunks : cap;
}
inline size_t serial_tables(int algo, size_t n_chunks) { return algo == DENSITY_HIP_CHAMELEON ? 0 : align_up(serial_slots(algo, n_chunks) * serial_table_bytes(algo), kAlign); }

inline size_t zmap_bytes(int algo, size_t n_chunks) { return (algo == DENSITY_HIP_CHAMELEON && n_chunks <= kMaxPipelinedChunks) ? align_up((n_chunks ? n_chunks : 1) * kZmapWordsPerChunk * 4, kAlign) : 0; }

// The plans: where everything lies in a workspace (the sizes the ABI reports follow from the offsets), and the workspace `ws` seen through them.
struct EncodePlan {
    size_t chunk, n_chunks, stride, off_err, off_sizes, off_offsets, off_slots, off_tables, off_zmap, off_stage, total;
    uint32_t* err(uint8_t* ws) const { return reinterpret_cast<uint32_t*>(ws + off_err); }
    uint32_t* page_counter(uint8_t* ws) const { return err(ws) + 4; }                  // (the paged form: pages handed out so far)
    uint64_t* sizes(uint8_t* ws) const { return reinterpret_cast<uint64_t*>(ws + off_sizes); }
    uint64_t* offsets(uint8_t* ws) const { return reinterpret_cast<uint64_t*>(ws + off_offsets); }
    uint64_t* carry(uint8_t* ws) const { return offsets(ws) + n_chunks; }               // (the extra entry of the offsets array: the running end)
    uint8_t* slots(uint8_t* ws) const { return ws + off_slots; }
    uint8_t* tables(uint8_t* ws) const { return ws + off_tables; }
    uint32_t* zmap(uint8_t* ws) const { return off_stage > off_zmap ? reinterpret_cast<uint32_t*>(ws + off_zmap) : nullptr; }   // nullptr: no zmap (zmap_bytes() == 0)
    uint8_t* stage(uint8_t* ws) const { return total > off_stage ? ws + off_stage : nullptr; }                                 // nullptr: the exchange passes will not run
};
EncodePlan plan_encode(int algo, size_t n, size_t chunk);
struct DecodePlan {
    size_t off_err, off_sizes, off_offsets, off_produced, off_tables, off_zmap, off_pass, total, total_with_passes;
    uint32_t* err(uint8_t* ws) const { return reinterpret_cast<uint32_t*>(ws + off_err); }
    uint32_t* damaged(uint8_t* ws) const { return err(ws) + 1; }                        // (a verdict decode: the number of damaged chunks)
    uint32_t* recovered(uint8_t* ws) const { return err(ws) + 2; }                      // (a recover decode: the number of chunks rebuilt)
    // (a recover decode, behind the verifying sum: that leaves its sums in the first word per chunk of `produced`; the second is free for a word per parity group:
    // parity.hip's plan word)
    uint32_t* victims(uint8_t* ws, uint32_t n_chunks) const { return reinterpret_cast<uint32_t*>(produced(ws)) + n_chunks; }
    uint64_t* sizes(uint8_t* ws) const { return reinterpret_cast<uint64_t*>(ws + off_sizes); }
    uint64_t* offsets(uint8_t* ws) const { return reinterpret_cast<uint64_t*>(ws + off_offsets); }
    uint64_t* produced(uint8_t* ws) const { return reinterpret_cast<uint64_t*>(ws + off_produced); }
    uint8_t* tables(uint8_t* ws) const { return ws + off_tables; }
    uint32_t* zmap(uint8_t* ws) const { return total > off_zmap ? reinterpret_cast<uint32_t*>(ws + off_zmap) : nullptr; }       // nullptr: no zmap (zmap_bytes() == 0)
    // nullptr: no decode passes for this container, or a (caller's smaller) workspace of ws_size bytes that does not hold their scratch: the one-wave decoder
    uint8_t* pass(uint8_t* ws, size_t ws_size) const { return (ws_size >= total_with_passes && total_with_passes > total) ? ws + off_pass : nullptr; }
};
// out_stride != 0 (the container's chunk size / a stream's output capacity): Cheetah's decode passes (decode_passes.hip) want a dword and
// a half per quad of scratch behind everything else; `total` is what the one-wave decoders need, `total_with_passes` what the passes need
DecodePlan plan_decode(int algo, size_t n_chunks, size_t out_stride = 0);

// algorithm dispatch
hipError_t codec_encode(int algo, const uint8_t* d_in, uint64_t total, uint64_t chunk_bytes, uint32_t n_chunks, uint8_t* d_out,
                        uint64_t out_stride, uint64_t* d_sizes, uint8_t* d_index, uint8_t* d_tables, uint32_t* d_zmap, uint8_t* d_stage, uint32_t* d_err, hipStream_t s);
hipError_t codec_decode(int algo, const uint8_t* d_in, const uint64_t* d_offsets, const uint64_t* d_sizes, uint32_t n_chunks, uint8_t* d_out,
                        uint64_t out_stride, uint64_t out_total, bool exact, const uint8_t* d_index, uint64_t* d_produced, uint32_t* d_err,
                        uint8_t* d_tables, uint32_t* d_zmap, hipStream_t s, uint8_t* d_pass = nullptr);
const char* encode_kernel_name(int algo);
const char* decode_kernel_name(int algo);
size_t container_bound(int algo, size_t n, size_t chunk);
size_t container_bound_slotted(int algo, size_t n, size_t chunk);
int check_header(const density_hip_header_t& h, size_t container_size);
// what check_header asks of a header before it looks at any length: magic, version, algorithm, chunk size and count, known flags, a paged form that exists
bool header_is_containers(const density_hip_header_t& h);
// the input bytes chunks [first, first + count) of a container cover, and density_hip_slice_bound(): 0 for a window that is not inside the container's chunks
inline size_t slice_len(const density_hip_header_t& h, uint32_t first, uint32_t count) {
    return (size_t)(std::min<uint64_t>(h.total_len, ((uint64_t)first + count) * h.chunk_size) - (uint64_t)first * h.chunk_size);
}
size_t slice_bound(const density_hip_header_t& h, uint32_t first, uint32_t count);

// a container's header as the encoders hand it to the layout kernels (container_len: theirs to fill in)
inline density_hip_header_t make_header(int algo, size_t chunk, size_t n_chunks, size_t total_len, uint32_t flags) {
    return density_hip_header_t{DENSITY_HIP_MAGIC, (uint8_t)algo, 1, (uint16_t)flags, (uint32_t)chunk, (uint32_t)n_chunks, total_len, 0};
}
enum class Form { Packed, Slotted, Paged };   // how a container's chunk streams lie: gathered | in worst-case slots | in pages
// One slice (slice_of) of a packed container's encode on stream s: its chunks into their worst-case slots, then — behind `predecessor`, the event
// of the slice in front where that ran on another stream — its place in the container from the running end *p.carry(ws); gather_slice brings the
// streams there.  The batched device encode and the pipelined host encode are these two per slice.  prof: the marks of the device call.
hipError_t encode_slice(const EncodePlan& p, uint8_t* ws, const uint8_t* d_in, const Slice& sl, bool is_first, bool is_last, const density_hip_header_t& hdr,
                        uint8_t* d_out, uint64_t cap, hipStream_t s, Profiler* prof, hipEvent_t predecessor);
hipError_t gather_slice(const EncodePlan& p, uint8_t* ws, const Slice& sl, bool is_last, uint8_t* d_out, hipStream_t s);

// device-side drivers of the container (api.hip; ctx already acquired; `ws` points at a workspace of sufficient size)
int run_encode_container(DeviceCtx* c, int algo, const uint8_t* d_in, size_t n, uint8_t* d_out, size_t cap, size_t chunk,
                         uint8_t* ws, hipStream_t s, density_hip_header_t* header_out, Form form = Form::Packed);
int run_decode_container(DeviceCtx* c, const uint8_t* d_in, size_t container_size, const density_hip_header_t& h, uint8_t* d_out,
                         size_t cap, uint8_t* ws, hipStream_t s, size_t* decoded_out, size_t ws_size = 0);
// run_decode_container on a SEALED container, then a verdict word per chunk in d_verdicts, the count in p.damaged(ws) and, with DENSITY_HIP_SALVAGE_BLANK in
// `flags`, zeros over the damaged chunks' output; damaged_out (host, nullable): synchronises and reports.  With `rec` (a recover decode) the chunks that are
// the only damaged ones of their parity groups — with Q rows: the only one or two — are rebuilt and verified again in between, their number goes to p.recovered(ws), and the code returned is
// DENSITY_HIP_OK wherever no chunk remains damaged; rec->recovered_out (host, nullable) synchronises as damaged_out does.
struct Recovery {
    const uint8_t* d_rows;            // the blob's rows on the device (behind its header), checked against the container by check_parity_header
    uint32_t n_groups, row_bytes;
    bool with_q;                      // a version-2 blob: n_groups Q rows behind the n_groups P rows
    uint32_t* recovered_out;
};
int run_decode_verdicts(DeviceCtx* c, const uint8_t* d_in, size_t container_size, const density_hip_header_t& h, uint8_t* d_out, size_t cap, uint8_t* ws,
                        hipStream_t s, size_t ws_size, uint32_t* d_verdicts, unsigned flags, uint32_t* damaged_out, const Recovery* rec = nullptr);
// a parity blob's header against the container it is to serve and the bytes there are of it: DENSITY_HIP_OK / _ERR_FORMAT / _ERR_ARGUMENT (include/density_hip.h)
int check_parity_header(const density_hip_parity_header_t& ph, const density_hip_header_t& h, size_t parity_size);
// a parity header that stands for itself — no container to hold it against —: magic, version, a valid chunk size, n_chunks, n_groups and row_bytes as the formulas
// give them for its total_len, version 2 with groups of at most 255
bool parity_header_is_blobs(const density_hip_parity_header_t& ph);
// a parity update (density_hip_parity_update_device): the blob's header and the bytes there are of it (DENSITY_HIP_ERR_FORMAT), then the edit through
// density_hip_parity_update_header (DENSITY_HIP_ERR_ARGUMENT); *after: the header behind the edit
int check_parity_update(const density_hip_parity_header_t& ph, size_t parity_size, uint64_t offset, size_t old_size, size_t new_size, density_hip_parity_header_t* after);
// density_hip_parity_size (version 1) and density_hip_parity2_size (version 2)
size_t parity_size_of(uint8_t version, size_t input_size, size_t chunk_size, uint32_t n_groups);
// the seal of the container just encoded for d_in (`ws`: plan_seal(n).total bytes); `header`: the caller's copy of its header, or nullptr
int run_seal_container(DeviceCtx* c, const uint8_t* d_in, size_t n, uint8_t* d_out, size_t cap, const density_hip_header_t* header, uint8_t* ws, hipStream_t s,
                       density_hip_header_t* header_out);
// chunks [first, first + count) of the container at d_in (header h: checked, the window inside it, cap >= slice_bound()) as a packed container at d_out.
// The one driver of density_hip_slice_device, density_hip_pack_device and density_hip_unpage_device: the last two are the window [0, h.n_chunks) — of no
// chunks for an empty container, cap >= container_bound() — and differ in what they ask of the header and in what WindowCaller holds: the two profiling
// marks, the call's name in the messages, and whether a SLOTTED source's streams are gathered by compact_kernel, the packed encode's gather, instead of
// run_gather_kernel.  The pack asks for that: on a whole slotted container of 1 GiB the run gather measured 5 % behind it (profiles/repack_rate.txt).
struct WindowCaller { const char *layout_mark, *gather_mark, *name; bool compact_slots; };
int run_slice_container(DeviceCtx* c, const uint8_t* d_in, const density_hip_header_t& h, uint32_t first, uint32_t count, uint8_t* d_out, size_t cap, uint8_t* ws,
                        hipStream_t s, density_hip_header_t* header_out, const WindowCaller& caller = {"slice_layout", "slice_gather", "slice", false});
// a join (density_hip_join_device): what its part list comes to — algorithm, chunk size and the flags the parts share, the output's chunks and input bytes, the
// parts that are not skipped — or why it is refused; the capacity it asks for; every live part's header against its container_size (DENSITY_HIP_ERR_FORMAT)
struct JoinGeometry { int algo; uint32_t chunk_size, flags, live; uint64_t n_chunks, total_len; };
const char* join_geometry(const density_hip_join_part_t* parts, uint32_t n_parts, JoinGeometry* g);
size_t join_bound(const JoinGeometry& g);
int check_join_parts(const density_hip_join_part_t* parts, uint32_t n_parts);
// the scratch of a join in a workspace: the error word and the run table, three words per output chunk (the part table travels with the launches
// and takes no room here)
struct JoinPlan {
    size_t n_chunks, total;
    uint32_t* err(uint8_t* ws) const { return reinterpret_cast<uint32_t*>(ws); }
    uint64_t* lens(uint8_t* ws) const { return reinterpret_cast<uint64_t*>(ws + kAlign); }
    uint64_t* src(uint8_t* ws) const { return lens(ws) + align_up(n_chunks, kAlign / 8); }
    uint64_t* dst_off(uint8_t* ws) const { return src(ws) + align_up(n_chunks, kAlign / 8); }
};
inline JoinPlan plan_join(size_t n_chunks) { return JoinPlan{n_chunks, kAlign + 3 * align_up(8 * n_chunks, kAlign)}; }
// the parts' windows (device pointers; join_geometry and check_join_parts passed, cap >= join_bound()) as one packed container at d_out; `ws`: plan_join().total bytes
int run_join_container(DeviceCtx* c, const density_hip_join_part_t* parts, uint32_t n_parts, const JoinGeometry& g, uint8_t* d_out, size_t cap, uint8_t* ws,
                       hipStream_t s, density_hip_header_t* header_out);
// ... of one reference stream (api_stream.hip)
int run_stream_encode(DeviceCtx* c, int algo, const uint8_t* d_in, size_t n, uint8_t* d_out, size_t cap, uint8_t* ws, hipStream_t s, size_t* size_out);
int run_stream_decode(DeviceCtx* c, int algo, const uint8_t* d_in, size_t n, uint8_t* d_out, size_t cap, uint8_t* ws, hipStream_t s, size_t* size_out);

}  // namespace api
}  // namespace density
