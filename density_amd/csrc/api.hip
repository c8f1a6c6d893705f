// api.hip — the C ABI of libdensity_hip.so (include/density_hip.h), first of three units: per-device context, workspace plans, the
// container's device-side drivers (encode in its three forms, decode, pack, unpage, slice, join) and the device-pointer / bookkeeping entry points.
// (api_stream.hip: one reference stream, from device and from host pointers; api_host.hip: the host-pointer container calls.)  No CPU
// codec lives here: every byte is produced by the gfx950 kernels, and every entry point fails (returns 0 / an error code) when no usable
// HIP device is present.  Pack, unpage and slice are ONE driver: the packed form of a container is its chunk window [0, n_chunks), and run_windows — the
// driver of the join — takes one part as it takes several.
#include "api_internal.hpp"

namespace density {
namespace api {

thread_local std::string g_last_error;
int g_profiling = 0;
int g_variant = 0;
uint64_t g_pass_decodes = 0;
uint64_t g_stream_stats[4] = {0, 0, 0, 0};
DeviceCtx g_ctx[kMaxDevices];

void set_error(const char* what, hipError_t e) {
    g_last_error = what;
    if (e != hipSuccess) { g_last_error += ": "; g_last_error += hipGetErrorString(e); }
}

DeviceCtx* acquire_ctx() {
    int dev = -1;
    hipError_t e = hipGetDevice(&dev);
    if (e != hipSuccess || dev < 0 || dev >= kMaxDevices) { set_error("no HIP device available", e); return nullptr; }
    DeviceCtx* c = &g_ctx[dev];
    std::lock_guard<std::mutex> lk(c->mu);
    if (!c->ready) {
        hipDeviceProp_t prop;
        e = hipGetDeviceProperties(&prop, dev);
        if (e != hipSuccess) { set_error("hipGetDeviceProperties", e); return nullptr; }
        if (std::strncmp(prop.gcnArchName, "gfx950", 6) != 0) { set_error("device is not gfx950 (MI355X); this library has no other code path"); return nullptr; }
        e = hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking);
        if (e == hipSuccess) e = hipStreamCreateWithFlags(&c->stitch_stream, hipStreamNonBlocking);
        for (int i = 0; i < 8 && e == hipSuccess; ++i) e = hipEventCreateWithFlags(&c->batch_done[i], hipEventDisableTiming);
        if (e == hipSuccess) e = hipEventCreateWithFlags(&c->stitch_done, hipEventDisableTiming);
        if (e != hipSuccess) { set_error("hipStreamCreate", e); return nullptr; }
        // kernels rely on ascending-lane service order of same-address LDS accesses: verify on this device
        uint32_t* d_fail = nullptr;
        uint32_t h_fail = 1;
        e = hipMalloc((void**)&d_fail, sizeof(uint32_t));
        if (e == hipSuccess) e = hipMemsetAsync(d_fail, 0, sizeof(uint32_t), c->stream);
        if (e == hipSuccess) e = launch_selftest(d_fail, c->stream);
        if (e == hipSuccess) e = launch_rotor_selftest(d_fail, c->stream);
        if (e == hipSuccess) e = hipMemcpyAsync(&h_fail, d_fail, sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream);
        if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
        if (d_fail) (void)hipFree(d_fail);
        if (e != hipSuccess) { set_error("LDS self-test launch", e); return nullptr; }
        // bits 0..7 (container.hip): plain 16-bit LDS writes in lane order — every kernel needs it; bits 8..11 (rotor.hip): lane order of the
        // ordered exchange ds_mskor_rtn_b32 — all but the one-wavefront kernels need it; bits 12, 13: lane-reversed rollback and the token
        // hand-off behind the exchanges — only the wave-rotation kernels need them.  A device that fails a later group runs on what is left.
        c->selftest_bits = h_fail;
        c->selftest_ok = (h_fail & 0xffu) == 0;
        density::g_exchange_unsafe = (h_fail & 0x0f00u) != 0;
        density::g_rotor_unsafe = (h_fail & 0xff00u) != 0;
        c->ready = true;
    }
    if (!c->selftest_ok) { set_error("LDS write-order self-test failed on this device; refusing to run"); return nullptr; }
    return c;
}

EncodePlan plan_encode(int algo, size_t n, size_t chunk) {
    EncodePlan p{};
    p.chunk = chunk;
    p.n_chunks = chunk_count(n, chunk);
    p.stride = slot_stride(algo, chunk);
    p.off_err = 0;
    p.off_sizes = kAlign;
    p.off_offsets = p.off_sizes + align_up(8 * p.n_chunks, kAlign);
    p.off_slots = p.off_offsets + align_up(8 * (p.n_chunks + 1), kAlign);
    p.off_tables = p.off_slots + (p.n_chunks > 1 ? p.n_chunks * p.stride : 0);   // one chunk encodes straight into the container
    p.off_zmap = p.off_tables + serial_tables(algo, p.n_chunks ? p.n_chunks : 1);
    p.off_stage = p.off_zmap + zmap_bytes(algo, p.n_chunks);
    // the exchange passes of Cheetah / Lion (exchange_stages.hip): a dword per quad, the per-block masks, the record offsets
    // — only where the passes will run: every condition of stage_encode_eligible but the input pointer's alignment is known here (chunk count
    // limits, head size, table budget, forced variants), and a caller sizing its own workspace should not pay 1.25-1.5 x the input for nothing
    const bool passes = algo != DENSITY_HIP_CHAMELEON && p.n_chunks <= 0xffffffffull && serial_slots(algo, p.n_chunks) == p.n_chunks &&   // (the passes keep a table slot per CHUNK)
                        stage_encode_eligible(algo, nullptr, n, chunk, (uint32_t)p.n_chunks);
    p.total = p.off_stage + (passes ? align_up(stage_scratch_bytes(algo, n, (uint32_t)p.n_chunks), kAlign) : 0);
    return p;
}
DecodePlan plan_decode(int algo, size_t n_chunks, size_t out_stride) {
    DecodePlan p{};
    p.off_err = 0;
    p.off_sizes = kAlign;
    p.off_offsets = p.off_sizes + align_up(8 * n_chunks, kAlign);
    p.off_produced = p.off_offsets + align_up(8 * (n_chunks + 1), kAlign);
    p.off_tables = p.off_produced + align_up(8 * (n_chunks ? n_chunks : 1), kAlign);
    p.off_zmap = p.off_tables + serial_tables(algo, n_chunks ? n_chunks : 1);
    p.total = p.off_zmap + zmap_bytes(algo, n_chunks);
    p.off_pass = p.total;
    p.total_with_passes = p.total;
    if (algo == DENSITY_HIP_CHEETAH && out_stride && n_chunks)
        p.total_with_passes = p.off_pass + align_up(decode_pass_scratch_bytes(n_chunks == 1 ? align_up(out_stride, 256) : out_stride, (uint32_t)n_chunks), kAlign);
    return p;
}

// algorithm dispatch: Chameleon has the LDS-resident pipelined kernels, Cheetah/Lion the functional one-lane-per-stream kernels
hipError_t codec_encode(int algo, const uint8_t* d_in, uint64_t total, uint64_t chunk_bytes, uint32_t n_chunks, uint8_t* d_out,
                        uint64_t out_stride, uint64_t* d_sizes, uint8_t* d_index, uint8_t* d_tables, uint32_t* d_zmap, uint8_t* d_stage, uint32_t* d_err, hipStream_t s) {
    if (algo == DENSITY_HIP_CHAMELEON) return launch_chameleon_encode(d_in, total, chunk_bytes, n_chunks, d_out, out_stride, d_sizes, d_index, d_zmap, d_err, s);
    if (d_stage && serial_slots(algo, n_chunks) == n_chunks && stage_encode_eligible(algo, d_in, total, chunk_bytes, n_chunks))   // Cheetah / Lion: passes of ordered LDS exchanges, the one-wave kernels for what they hand back
        return launch_stage_encode(algo, d_in, total, chunk_bytes, n_chunks, d_out, out_stride, d_sizes, d_tables, (uint32_t)serial_slots(algo, n_chunks), d_stage, d_err, s);
    return launch_serial_encode(algo, d_in, total, chunk_bytes, n_chunks, d_out, out_stride, d_sizes, d_tables, (uint32_t)serial_slots(algo, n_chunks), s);
}
hipError_t codec_decode(int algo, const uint8_t* d_in, const uint64_t* d_offsets, const uint64_t* d_sizes, uint32_t n_chunks, uint8_t* d_out,
                        uint64_t out_stride, uint64_t out_total, bool exact, const uint8_t* d_index, uint64_t* d_produced, uint32_t* d_err,
                        uint8_t* d_tables, uint32_t* d_zmap, hipStream_t s, uint8_t* d_pass) {
    if (algo == DENSITY_HIP_CHAMELEON) return launch_chameleon_decode(d_in, d_offsets, d_sizes, n_chunks, d_out, out_stride, out_total, exact, d_index, d_zmap, d_produced, d_err, s);
    if (d_pass && decode_pass_eligible(algo, d_in, d_out, n_chunks, out_stride, out_total) && ++g_pass_decodes)   // Cheetah: parallel inside the chunk but for the chain of contexts
        return launch_decode_passes(algo, d_in, d_offsets, d_sizes, n_chunks, d_out, out_stride, out_total, exact, d_produced, d_err, d_pass, s);
    return launch_serial_decode(algo, d_in, d_offsets, d_sizes, n_chunks, d_out, out_stride, out_total, exact, d_produced, d_err, d_tables, (uint32_t)serial_slots(algo, n_chunks), s);
}
const char* encode_kernel_name(int algo) { return algo == DENSITY_HIP_CHAMELEON ? "chameleon_encode_chunks" : algo == DENSITY_HIP_CHEETAH ? "cheetah_encode_chunks" : "lion_encode_chunks"; }
const char* decode_kernel_name(int algo) { return algo == DENSITY_HIP_CHAMELEON ? "chameleon_decode_chunks" : algo == DENSITY_HIP_CHEETAH ? "cheetah_decode_chunks" : "lion_decode_chunks"; }

// every payload but the last `stride` bytes from the next, the last one as long as its chunk can get
static size_t bound_at_stride(int algo, size_t n, size_t chunk, size_t stride) {
    const size_t nc = chunk_count(n, chunk);
    size_t bound = payload_base(nc, n, true);      // (with the block index: an upper bound for both flavours)
    if (nc) bound += (nc - 1) * stride + safe_size(algo, n - (nc - 1) * chunk);
    return bound;
}
size_t container_bound(int algo, size_t n, size_t chunk) { return bound_at_stride(algo, n, chunk, align_up(safe_size(algo, chunk), 16)); }
// a slotted container: every payload in its worst-case slot
size_t container_bound_slotted(int algo, size_t n, size_t chunk) { return bound_at_stride(algo, n, chunk, slot_stride(algo, chunk)); }

// a paged container: every chunk as many pages as its worst case needs (they are taken as the streams grow: a container of text ends far below this)
size_t container_bound_paged(int algo, size_t n, size_t chunk) {
    if (!paged_eligible(algo, n, chunk)) return container_bound_slotted(algo, n, chunk);
    const size_t nc = chunk_count(n, chunk);
    return paged_pages_base(nc, n, chunk) + nc * (size_t)paged_pages_per_chunk(chunk) * kPageBytes;
}

bool header_is_containers(const density_hip_header_t& h) {
    if (h.magic != DENSITY_HIP_MAGIC || h.version != 1 || !valid_algo(h.algo)) return false;
    if (!valid_chunk(h.chunk_size)) return false;
    if (h.n_chunks != chunk_count(h.total_len, h.chunk_size)) return false;
    if (h.flags & ~(DENSITY_HIP_FLAG_BLOCK_INDEX | DENSITY_HIP_FLAG_SLOTTED | DENSITY_HIP_FLAG_PAGED | DENSITY_HIP_FLAG_CHECKSUM)) return false;
    // pages: Chameleon with its block index
    if ((h.flags & DENSITY_HIP_FLAG_PAGED) && (h.algo != DENSITY_HIP_CHAMELEON || (h.flags & (DENSITY_HIP_FLAG_BLOCK_INDEX | DENSITY_HIP_FLAG_SLOTTED)) != DENSITY_HIP_FLAG_BLOCK_INDEX)) return false;
    return true;
}

int check_header(const density_hip_header_t& h, size_t container_size) {
    if (!header_is_containers(h)) return DENSITY_HIP_ERR_FORMAT;
    const size_t trailer = header_trailer(h);                                      // a sealed container ends in its trailer: the form's own rules hold for what lies in front of it
    if (h.flags & DENSITY_HIP_FLAG_PAGED) {                                        // whole pages behind the directory
        const size_t pb = paged_pages_base(h.n_chunks, h.total_len, h.chunk_size);
        if (h.container_len > container_size || h.container_len < pb + trailer) return DENSITY_HIP_ERR_FORMAT;
        if ((h.container_len - trailer - pb) % kPageBytes != 0 || h.container_len - trailer - pb >= (1ull << 32)) return DENSITY_HIP_ERR_FORMAT;
        return DENSITY_HIP_OK;
    }
    if (h.container_len > container_size || h.container_len < payload_base(h.n_chunks, h.total_len, h.flags & DENSITY_HIP_FLAG_BLOCK_INDEX) + trailer) return DENSITY_HIP_ERR_FORMAT;
    return DENSITY_HIP_OK;
}

size_t slice_bound(const density_hip_header_t& h, uint32_t first, uint32_t count) {
    if (!header_is_containers(h) || count == 0 || (uint64_t)first + count > h.n_chunks) return 0;
    const size_t len = slice_len(h, first, count);
    return container_bound(h.algo, len, h.chunk_size) + ((h.flags & DENSITY_HIP_FLAG_CHECKSUM) ? seal_overhead(count) : 0);
}

// ---- device-side drivers (ctx already acquired; `ws` points at a workspace of sufficient size) ----

hipError_t encode_slice(const EncodePlan& p, uint8_t* ws, const uint8_t* d_in, const Slice& sl, bool is_first, bool is_last, const density_hip_header_t& hdr,
                        uint8_t* d_out, uint64_t cap, hipStream_t s, Profiler* prof, hipEvent_t predecessor) {
    const bool with_index = hdr.flags & DENSITY_HIP_FLAG_BLOCK_INDEX;
    uint8_t* d_index = with_index ? d_out + index_base(p.n_chunks) : nullptr;
    uint32_t* d_zmap = p.zmap(ws);
    hipError_t e = codec_encode(hdr.algo, d_in + sl.off, sl.len, p.chunk, sl.count, p.slots(ws) + (uint64_t)sl.first * p.stride, p.stride, p.sizes(ws) + sl.first,
                                d_index ? d_index + sl.off / 256 : nullptr, p.tables(ws), d_zmap ? d_zmap + (uint64_t)sl.first * kZmapWordsPerChunk : nullptr, p.stage(ws), p.err(ws), s);
    if (prof) prof->mark(encode_kernel_name(hdr.algo));
    if (e == hipSuccess && predecessor) e = hipStreamWaitEvent(s, predecessor, 0);
    if (e == hipSuccess) e = launch_layout_encode_batch(p.sizes(ws), sl.first, sl.count, is_first, is_last, hdr, payload_base(p.n_chunks, hdr.total_len, with_index), d_out, cap,
                                                        p.offsets(ws), p.carry(ws), p.err(ws), s);
    if (prof) prof->mark("layout_encode");
    return e;
}
hipError_t gather_slice(const EncodePlan& p, uint8_t* ws, const Slice& sl, bool is_last, uint8_t* d_out, hipStream_t s) {
    return launch_compact(p.slots(ws) + (uint64_t)sl.first * p.stride, p.stride, p.sizes(ws) + sl.first, p.offsets(ws) + sl.first, sl.count, d_out, p.err(ws), s, !is_last);
}

namespace {
// The form a container is actually written in: what the paged form is not for goes to the slotted one, and one chunk encodes straight into place either way.
Form settle_form(Form want, int algo, const uint8_t* d_in, size_t n, size_t chunk, size_t n_chunks) {
    if (want == Form::Paged && !(paged_eligible(algo, n, chunk) && rotor_encode_eligible(d_in, n, chunk, (uint32_t)n_chunks) && !g_rotor_unsafe && !variant(kVarNoRotor))) want = Form::Slotted;
    if (want == Form::Slotted && n_chunks <= 1) want = Form::Packed;
    return want;
}
}  // namespace

int run_encode_container(DeviceCtx* c, int algo, const uint8_t* d_in, size_t n, uint8_t* d_out, size_t cap, size_t chunk,
                         uint8_t* ws, hipStream_t s, density_hip_header_t* header_out, Form form) {
    const EncodePlan p = plan_encode(algo, n, chunk);
    if (p.n_chunks > 0xffffffffull) { set_error("too many chunks"); return DENSITY_HIP_ERR_ARGUMENT; }
    form = settle_form(form, algo, d_in, n, chunk, p.n_chunks);
    const size_t bound = form == Form::Paged ? container_bound_paged(algo, n, chunk) : form == Form::Slotted ? container_bound_slotted(algo, n, chunk) : container_bound(algo, n, chunk);
    if (cap < bound) { set_error("output capacity below density_hip_container_bound()"); return DENSITY_HIP_ERR_CAPACITY; }
    const uint32_t nch = (uint32_t)p.n_chunks;
    uint32_t* d_err = p.err(ws);
    uint64_t* d_sizes = p.sizes(ws);
    const density_hip_header_t hdr = make_header(algo, chunk, nch, n, (want_index(algo) ? DENSITY_HIP_FLAG_BLOCK_INDEX : 0) |
                                                 (form == Form::Slotted ? DENSITY_HIP_FLAG_SLOTTED : form == Form::Paged ? DENSITY_HIP_FLAG_PAGED : 0));
    const bool with_index = hdr.flags & DENSITY_HIP_FLAG_BLOCK_INDEX;
    const uint64_t pbase = payload_base(nch, n, with_index);
    uint8_t* d_index = with_index ? d_out + index_base(nch) : nullptr;
    Profiler prof(c, s);
    hipError_t e = hipMemsetAsync(d_err, 0, sizeof(uint32_t), s);
    if (e != hipSuccess) { set_error("hipMemsetAsync", e); return DENSITY_HIP_ERR_RUNTIME; }
    if (form == Form::Paged) {
        // Paged container (round 5): the wire form WITHOUT a stitch.  The encode kernel places the streams itself, page by page (64 KiB, from one
        // counter, in the order the chunks ask for them): dense but for the unused tails of the pages, and a chunk's stream is its pages' used bytes
        // in directory order.  write_buffer.rs:29-31's running total lives in the directory.
        const uint64_t dir_base = paged_dir_base(nch, n), pages_base = paged_pages_base(nch, n, chunk);
        const uint32_t ppc = paged_pages_per_chunk(chunk);
        uint32_t* d_counter = p.page_counter(ws);
        e = hipMemsetAsync(d_counter, 0, sizeof(uint32_t), s);
        if (e == hipSuccess) e = launch_rotor_encode_paged(d_in, n, chunk, nch, d_out + pages_base, (uint32_t)std::min<uint64_t>((cap - pages_base) / kPageBytes, 0xffffu),
                                                         d_counter, reinterpret_cast<uint32_t*>(d_out + dir_base), page_dir_words(ppc), d_sizes, d_index, d_err, s);
        prof.mark(encode_kernel_name(algo));
        if (e == hipSuccess) e = launch_layout_encode_paged(d_sizes, nch, hdr, dir_base, dir_base + paged_dir_bytes(nch, chunk), pages_base, d_out, cap, d_counter, d_err, s);
        prof.mark("layout_encode");
    } else if (nch == 1 || form == Form::Slotted) {
        // The chunk streams stay where the encoder puts them, no stitch pass.  A single chunk: its stream goes straight to its final place.
        // Slotted container: worst-case slots INSIDE the container, at payload_base + i * slot_stride, and the size table says how much of each
        // slot is stream.  No gather: the decoder reads the slots through the same arithmetic; the packed wire form is made when the
        // container leaves the device (density_hip_pack_device: a copy happens there anyway).
        const uint64_t stride = nch == 1 ? 0 : p.stride;
        e = codec_encode(algo, d_in, n, chunk, nch, d_out + pbase, stride, d_sizes, d_index, p.tables(ws), p.zmap(ws), p.stage(ws), d_err, s);
        prof.mark(encode_kernel_name(algo));
        if (e == hipSuccess) e = launch_layout_encode(d_sizes, nch, hdr, pbase, d_out, cap, p.offsets(ws), d_err, s, stride);
        prof.mark("layout_encode");
    } else {
        // Chunk streams go to worst-case slots; their sizes are known only afterwards (write_buffer.rs:29-31 keeps a running total: in
        // parallel an exclusive scan), then the streams are gathered into the packed container.  Optional (kVarBatchedStitch, measured, not
        // the default): large inputs encoded in up to kStitchBatches batches of whole multiples of 256 chunks (one per CU) with the gather of
        // batch k on a second stream beside the encoding of batch k+1.  It hides the gather but the encoder — whose dictionary chain is
        // sensitive to load latency — slows down by as much (0.68 + 0.10 ms against 0.56 + 0.25 ms per GiB): DESIGN.md.
        constexpr uint32_t kStitchBatches = 4;
        uint32_t per = nch, batches = 1;
        if (algo == DENSITY_HIP_CHAMELEON && nch >= 512 && variant(kVarBatchedStitch)) {
            batches = nch / 256 < kStitchBatches ? nch / 256 : kStitchBatches;
            per = ((nch + batches - 1) / batches + 255) / 256 * 256;
            batches = (nch + per - 1) / per;
        }
        for (uint32_t k = 0; k < batches && e == hipSuccess; ++k) {
            const Slice sl = slice_of(k, per, nch, chunk, n);
            const bool is_last = k + 1 == batches;
            e = encode_slice(p, ws, d_in, sl, k == 0, is_last, hdr, d_out, cap, s, &prof, nullptr);
            if (e != hipSuccess) break;
            if (batches == 1) {
                e = gather_slice(p, ws, sl, is_last, d_out, s);
                prof.mark("compact");
            } else {
                e = hipEventRecord(c->batch_done[k], s);
                if (e == hipSuccess) e = hipStreamWaitEvent(c->stitch_stream, c->batch_done[k], 0);
                if (e == hipSuccess) e = gather_slice(p, ws, sl, is_last, d_out, c->stitch_stream);
            }
        }
        if (e == hipSuccess && batches > 1) {                               // the caller's stream continues when the last gather is done
            e = hipEventRecord(c->stitch_done, c->stitch_stream);
            if (e == hipSuccess) e = hipStreamWaitEvent(s, c->stitch_done, 0);
            prof.mark("stitch_tail");
        }
    }
    if (e != hipSuccess) { set_error("kernel launch (encode)", e); return DENSITY_HIP_ERR_RUNTIME; }
    if (header_out) {
        uint32_t h_err = 0;
        e = read_back(s, d_err, &h_err, header_out, d_out, sizeof(*header_out));
        if (e != hipSuccess) { set_error("encode (device)", e); return DENSITY_HIP_ERR_RUNTIME; }
        if (h_err & 16u) { set_error("encode: device-side watchdog"); return DENSITY_HIP_ERR_RUNTIME; }
        if (h_err) { set_error("container does not fit the output capacity"); return DENSITY_HIP_ERR_CAPACITY; }
    }
    return DENSITY_HIP_OK;
}

int run_decode_container(DeviceCtx* c, const uint8_t* d_in, size_t container_size, const density_hip_header_t& h, uint8_t* d_out,
                         size_t cap, uint8_t* ws, hipStream_t s, size_t* decoded_out, size_t ws_size) {
    if (cap < h.total_len) { set_error("output capacity below the container's total_len"); return DENSITY_HIP_ERR_CAPACITY; }
    const DecodePlan p = plan_decode(h.algo, h.n_chunks, h.chunk_size);
    uint32_t* d_err = p.err(ws);
    uint64_t *d_sizes = p.sizes(ws), *d_offsets = p.offsets(ws), *d_produced = p.produced(ws);
    uint32_t* d_zmap = p.zmap(ws);
    Profiler prof(c, s);
    hipError_t e = hipMemsetAsync(d_err, 0, sizeof(uint32_t), s);
    const bool with_index = h.flags & DENSITY_HIP_FLAG_BLOCK_INDEX;
    const uint8_t* d_index = with_index ? d_in + index_base(h.n_chunks) : nullptr;
    // a sealed container's trailer is not payload: the streams and pages end in front of it
    const size_t trailer = header_trailer(h), body_len = h.container_len - trailer;
    if (trailer) container_size = body_len;
    if (h.flags & DENSITY_HIP_FLAG_PAGED) {
        // the pages are read where they lie: the rotation decoder turns stream positions into page offsets through the chunk's directory
        const size_t dir_base = paged_dir_base(h.n_chunks, h.total_len), pages_base = paged_pages_base(h.n_chunks, h.total_len, h.chunk_size);
        if (g_rotor_unsafe || !rotor_decode_eligible(d_out, h.n_chunks, h.chunk_size, h.total_len, d_index, d_zmap) || (uintptr_t)(d_in + pages_base) % 4 != 0) {
            set_error("a paged container needs the rotation decoder (chunks of at most 4 MiB, 4-byte aligned buffers)"); return DENSITY_HIP_ERR_UNSUPPORTED;
        }
        if (e == hipSuccess) e = launch_layout_decode_paged(d_in, h.n_chunks, d_sizes, d_offsets, s);
        prof.mark("layout_decode");
        if (e == hipSuccess) e = launch_rotor_decode_paged(d_in + pages_base, d_offsets, d_sizes, h.n_chunks, d_out, h.chunk_size, h.total_len, d_index,
                                                         reinterpret_cast<const uint32_t*>(d_in + dir_base), page_dir_words(paged_pages_per_chunk(h.chunk_size)),
                                                         (uint32_t)((body_len - pages_base) / kPageBytes), d_zmap, d_produced, d_err, s);
        prof.mark(decode_kernel_name(h.algo));
    } else {
        if (e == hipSuccess) e = launch_layout_decode(d_in, container_size, h.n_chunks, payload_base(h.n_chunks, h.total_len, with_index), d_sizes, d_offsets, d_err, s,
                                                      (h.flags & DENSITY_HIP_FLAG_SLOTTED) ? slot_stride(h.algo, h.chunk_size) : 0);
        prof.mark("layout_decode");
        if (e == hipSuccess) e = codec_decode(h.algo, d_in, d_offsets, d_sizes, h.n_chunks, d_out, h.chunk_size, h.total_len, true, d_index, d_produced, d_err, p.tables(ws), d_zmap, s,
                                              p.pass(ws, ws_size));
        prof.mark(decode_kernel_name(h.algo));
    }
    if (trailer) {
        // sealed: the sum of what was just decoded against the trailer, on the device (the decoders' per-chunk counts are not needed any more: their
        // words hold the sums).  Whatever a damaged stream decoded to lies inside the output: the decoders write nothing past it.
        if (e == hipSuccess) e = launch_checksum(d_out, h.total_len, h.chunk_size, h.n_chunks, reinterpret_cast<uint32_t*>(d_produced), d_in + body_len, d_err, s);
        prof.mark("checksum_verify");
    }
    if (e != hipSuccess) { set_error("kernel launch (decode)", e); return DENSITY_HIP_ERR_RUNTIME; }
    if (decoded_out) {
        uint32_t h_err = 0;
        e = read_back(s, d_err, &h_err);
        if (e != hipSuccess) { set_error("decode (device)", e); return DENSITY_HIP_ERR_RUNTIME; }
        if (h_err & ~kErrChecksum) { set_error("malformed or truncated container payload"); *decoded_out = 0; return DENSITY_HIP_ERR_FORMAT; }
        if (h_err) { set_error("checksum mismatch: the container decodes, but not to the bytes that were sealed"); *decoded_out = 0; return DENSITY_HIP_ERR_CHECKSUM; }
        *decoded_out = h.total_len;
    }
    return DENSITY_HIP_OK;
}

// A verdict decode of a sealed container: run_decode_container as it stands (asynchronous: it reports nothing), then the sums it has just left in the
// workspace held against the trailer once more for a word per chunk and a count, then — with DENSITY_HIP_SALVAGE_BLANK — zeros over the damaged chunks.
// damaged_out (host, nullable): synchronises; it is written wherever the verdicts are valid, a format error included.
int run_decode_verdicts(DeviceCtx* c, const uint8_t* d_in, size_t container_size, const density_hip_header_t& h, uint8_t* d_out, size_t cap, uint8_t* ws,
                        hipStream_t s, size_t ws_size, uint32_t* d_verdicts, unsigned flags, uint32_t* damaged_out, const Recovery* rec) {
    if (const int rc = run_decode_container(c, d_in, container_size, h, d_out, cap, ws, s, nullptr, ws_size)) return rc;
    const DecodePlan p = plan_decode(h.algo, h.n_chunks, h.chunk_size);
    Profiler prof(c, s);
    uint32_t* d_acc = reinterpret_cast<uint32_t*>(p.produced(ws));
    const uint8_t* d_trailer = d_in + (h.container_len - header_trailer(h));
    hipError_t e = launch_chunk_verdicts(d_acc, h.total_len, h.chunk_size, h.n_chunks, d_trailer, d_verdicts, p.damaged(ws), p.err(ws), s);
    prof.mark("chunk_verdicts");
    if (rec) {
        // recovery: what the verdicts say can be rebuilt is rebuilt from the parity rows, summed again and held against the trailer once more
        uint32_t* d_victims = p.victims(ws, h.n_chunks);
        if (e == hipSuccess) e = launch_recover_rebuild(d_out, h.total_len, h.chunk_size, h.n_chunks, rec->d_rows, rec->n_groups, rec->row_bytes, rec->with_q, d_verdicts, d_victims, d_acc, s);
        prof.mark("recover_rebuild");
        if (e == hipSuccess) e = launch_recover_verify(d_out, h.total_len, h.chunk_size, h.n_chunks, rec->n_groups, rec->with_q, d_victims, d_acc, d_trailer, d_verdicts, p.damaged(ws), p.recovered(ws), s);
        prof.mark("recover_verify");
    }
    if (flags & DENSITY_HIP_SALVAGE_BLANK) {
        if (e == hipSuccess) e = launch_blank_chunks(d_out, h.total_len, h.chunk_size, h.n_chunks, d_verdicts, s);
        prof.mark("blank_chunks");
    }
    if (e != hipSuccess) { set_error("kernel launch (verdicts)", e); return DENSITY_HIP_ERR_RUNTIME; }
    if (damaged_out || (rec && rec->recovered_out)) {
        uint32_t h_err = 0, counts[2] = {0, 0};                                        // {damaged, recovered}: neighbours in the workspace
        e = read_back(s, p.err(ws), &h_err, counts, p.damaged(ws), rec ? sizeof(counts) : sizeof(counts[0]));
        if (e != hipSuccess) { set_error("decode (device)", e); return DENSITY_HIP_ERR_RUNTIME; }
        if (damaged_out) *damaged_out = counts[0];
        if (rec && rec->recovered_out) *rec->recovered_out = counts[1];
        if (h_err && !(rec && counts[0] == 0)) {                                       // (recovered whole: every chunk's content has been verified, whatever a decoder raised)
            const bool format = h_err & ~kErrChecksum;
            char msg[160];
            int at = std::snprintf(msg, sizeof(msg), "%s: %u of %u chunks damaged", format ? "malformed or truncated container payload" : "checksum mismatch", counts[0], h.n_chunks);
            if (rec) std::snprintf(msg + at, sizeof(msg) - at, ", %u recovered", counts[1]);
            set_error(msg);
            return format ? DENSITY_HIP_ERR_FORMAT : DENSITY_HIP_ERR_CHECKSUM;
        }
    }
    return DENSITY_HIP_OK;
}

int check_parity_header(const density_hip_parity_header_t& ph, const density_hip_header_t& h, size_t parity_size) {
    if (ph.magic != DENSITY_HIP_PARITY_MAGIC || (ph.version != 1 && ph.version != 2)) { set_error("bad parity header"); return DENSITY_HIP_ERR_FORMAT; }
    if (ph.chunk_size != h.chunk_size || ph.n_chunks != h.n_chunks || ph.total_len != h.total_len) { set_error("recover: the parity blob is not this container's (chunk size, chunks, length)"); return DENSITY_HIP_ERR_ARGUMENT; }
    const density_hip_parity_header_t want = make_parity_header(h.total_len, h.chunk_size, ph.n_groups);
    if ((h.n_chunks && !ph.n_groups) || ph.n_groups != want.n_groups || ph.row_bytes != want.row_bytes) { set_error("bad parity header (groups, row length)"); return DENSITY_HIP_ERR_FORMAT; }
    if (ph.version == 2 && parity_group_members(ph) > kParityQMembers) { set_error("bad parity header (version 2: a group of more than 255 chunks)"); return DENSITY_HIP_ERR_FORMAT; }
    if (parity_size < parity_bytes(ph)) { set_error("parity blob shorter than its header and rows"); return DENSITY_HIP_ERR_FORMAT; }
    return DENSITY_HIP_OK;
}

bool parity_header_is_blobs(const density_hip_parity_header_t& ph) {
    if (ph.magic != DENSITY_HIP_PARITY_MAGIC || (ph.version != 1 && ph.version != 2) || !valid_chunk(ph.chunk_size)) return false;
    const density_hip_parity_header_t want = make_parity_header(ph.total_len, ph.chunk_size, ph.n_groups, ph.version);
    if (chunk_count(ph.total_len, ph.chunk_size) != ph.n_chunks || (ph.n_chunks && !ph.n_groups) || ph.n_groups != want.n_groups || ph.row_bytes != want.row_bytes) return false;
    return ph.version != 2 || parity_group_members(ph) <= kParityQMembers;
}

int check_parity_update(const density_hip_parity_header_t& ph, size_t parity_size, uint64_t offset, size_t old_size, size_t new_size, density_hip_parity_header_t* after) {
    if (!parity_header_is_blobs(ph)) { set_error("bad parity header"); return DENSITY_HIP_ERR_FORMAT; }
    if (parity_size < parity_bytes(ph)) { set_error("parity blob shorter than its header and rows"); return DENSITY_HIP_ERR_FORMAT; }
    return density_hip_parity_update_header(&ph, offset, old_size, new_size, after);
}

size_t parity_size_of(uint8_t version, size_t input_size, size_t chunk_size, uint32_t n_groups) {
    if (!valid_chunk(chunk_size) || chunk_count(input_size, chunk_size) > 0xffffffffull || (input_size && !n_groups)) return 0;
    const density_hip_parity_header_t ph = make_parity_header(input_size, chunk_size, n_groups, version);
    return version == 2 && parity_group_members(ph) > kParityQMembers ? 0 : parity_bytes(ph);
}

// ---- join: chunk windows of several containers as one packed container ----

// what the host can say of a join before any byte moves: nullptr and *g, or why the part list is refused (include/density_hip.h: DENSITY_HIP_ERR_ARGUMENT)
const char* join_geometry(const density_hip_join_part_t* parts, uint32_t n_parts, JoinGeometry* g) {
    *g = JoinGeometry{};
    if (!parts || n_parts == 0 || n_parts > DENSITY_HIP_JOIN_MAX_PARTS) return "join: 1 to DENSITY_HIP_JOIN_MAX_PARTS parts";
    bool have = false, ragged = false;
    for (uint32_t p = 0; p < n_parts; ++p) {
        const density_hip_join_part_t& q = parts[p];
        if (q.chunk_count == 0) continue;                                              // skipped: nothing of it is read
        if (!q.container || !q.header || q.container_size < sizeof(density_hip_header_t)) return "join: a part without its container or without its header";
        const density_hip_header_t& h = *q.header;
        if (!header_is_containers(h)) return "join: not a container's header";
        if ((uint64_t)q.first_chunk + q.chunk_count > h.n_chunks) return "join: a window that is not inside its container's chunks";
        const uint32_t flags = h.flags & (DENSITY_HIP_FLAG_BLOCK_INDEX | DENSITY_HIP_FLAG_CHECKSUM);
        if (!have) { g->algo = h.algo; g->chunk_size = h.chunk_size; g->flags = flags; have = true; }
        else if (g->algo != h.algo || g->chunk_size != h.chunk_size || g->flags != flags) return "join: parts that differ in algorithm, chunk size, block index or seal";
        if (ragged) return "join: a ragged chunk anywhere but at the output's end";
        const uint64_t len = slice_len(h, q.first_chunk, q.chunk_count);
        ragged = len != (uint64_t)q.chunk_count * h.chunk_size;
        g->n_chunks += q.chunk_count;
        g->total_len += len;
        ++g->live;
    }
    if (!have) return "join: no chunks";
    if (g->n_chunks > 0xffffffffull) return "join: more chunks than a header counts";
    return nullptr;
}

size_t join_bound(const JoinGeometry& g) {
    return container_bound(g.algo, g.total_len, g.chunk_size) + ((g.flags & DENSITY_HIP_FLAG_CHECKSUM) ? seal_overhead(g.n_chunks) : 0);
}

int check_join_parts(const density_hip_join_part_t* parts, uint32_t n_parts) {
    for (uint32_t p = 0; p < n_parts; ++p)
        if (parts[p].chunk_count && check_header(*parts[p].header, parts[p].container_size) != DENSITY_HIP_OK) {
            set_error("join: bad container header (its length, or its trailer's, against container_size)");
            return DENSITY_HIP_ERR_FORMAT;
        }
    return DENSITY_HIP_OK;
}

// The parts' windows -> one packed container: everything the host can say of a part — where its size table, index bytes, trailer entries and (slotted) streams
// lie — goes into the part table, which travels with the launches; where a packed part's window lies the layout kernel finds out and leaves on the device.
// A paged part goes through the directory check and the unpage gather, handed offset pointers and its stretch of the run table.  What the caller brings
// (WindowCall): the scratch in its own workspace, and what WindowCaller says of it.
struct WindowCall {
    uint32_t* err;
    uint64_t *lens, *src, *dst_off;       // a word per output chunk each
    uint64_t* run;                         // not null: one word, and a single packed part moves as the one run the layout kernel leaves there (the kernel
                                           // leaves 0 there for more than one part: then as with null, a run per chunk)
    uint64_t longest_run;                  // what no stream of a part that is not paged exceeds: sizes the gather's tiles per run
    WindowCaller caller;
};
static int run_windows(DeviceCtx* c, const density_hip_join_part_t* parts, uint32_t n_parts, const JoinGeometry& g, uint8_t* d_out, size_t cap, const WindowCall& w,
                       hipStream_t s, density_hip_header_t* header_out) {
    uint32_t* const d_err = w.err;
    uint64_t *const d_lens = w.lens, *const d_src = w.src, *const d_dst_off = w.dst_off;
    const bool with_index = g.flags & DENSITY_HIP_FLAG_BLOCK_INDEX, sealed = g.flags & DENSITY_HIP_FLAG_CHECKSUM;
    const density_hip_header_t out_h = make_header(g.algo, g.chunk_size, g.n_chunks, g.total_len, g.flags & DENSITY_HIP_FLAG_BLOCK_INDEX);
    const uint64_t out_base = payload_base(g.n_chunks, g.total_len, with_index);
    const uint32_t ppc = paged_pages_per_chunk(g.chunk_size);
    const uint64_t dir_entry = 16ull * (ppc + 1u);
    JoinSources src{};
    TrailerRuns trailers{};
    Profiler prof(c, s);
    hipError_t e = hipMemsetAsync(d_err, 0, sizeof(uint32_t), s);
    uint32_t live = 0;
    bool any_unpaged = false;
    uint64_t K = 0, index_at = index_base(g.n_chunks);
    for (uint32_t i = 0; i < n_parts; ++i) {
        const density_hip_join_part_t& q = parts[i];
        if (q.chunk_count == 0) continue;
        const density_hip_header_t& h = *q.header;
        const uint8_t* d_in = (const uint8_t*)q.container;
        const bool paged = h.flags & DENSITY_HIP_FLAG_PAGED;
        const uint64_t stride = (h.flags & DENSITY_HIP_FLAG_SLOTTED) ? slot_stride(h.algo, h.chunk_size) : 0;
        const uint64_t pbase = payload_base(h.n_chunks, h.total_len, with_index);          // (paged: the directory's base)
        const size_t body_len = h.container_len - header_trailer(h), len = slice_len(h, q.first_chunk, q.chunk_count);   // the streams and pages end in front of a sealed container's trailer
        src.p[live] = JoinSource{d_in, body_len, h.total_len, pbase, paged ? kJoinPaged : stride, q.first_chunk, q.chunk_count};
        trailers.p[live] = TrailerRun{d_in + body_len + 4ull * q.first_chunk, (uint32_t)K, q.chunk_count};
        if (paged && e == hipSuccess) {
            // the directory check on the window's chunks alone: its chunk 0 is chunk `first` — the size table is read at d_in + 4 * first, the directory so
            // much further on — and the input ends where the container's does
            const uint64_t pages_base = paged_pages_base(h.n_chunks, h.total_len, h.chunk_size);
            e = launch_check_directory(d_in + 4ull * q.first_chunk, q.chunk_count, h.chunk_size, h.total_len - (uint64_t)q.first_chunk * h.chunk_size,
                                       pbase + (dir_entry - 4ull) * q.first_chunk, ppc, (uint32_t)((body_len - pages_base) / kPageBytes), d_lens + K, d_err, s);
        }
        if (with_index) {                                                                  // (chunks are whole blocks, and every part but the last covers whole chunks: whole index bytes)
            if (e == hipSuccess) e = hipMemcpyAsync(d_out + index_at, d_in + index_base(h.n_chunks) + (uint64_t)q.first_chunk * h.chunk_size / 256, index_bytes(len, true), hipMemcpyDeviceToDevice, s);
            index_at += index_bytes(len, true);
        }
        any_unpaged |= !paged;
        K += q.chunk_count;
        ++live;
    }
    if (e == hipSuccess) e = launch_window_layout(src, live, (uint32_t)g.algo, g.chunk_size, d_out, cap, out_h, out_base, d_lens, d_src, d_dst_off, w.run, d_err, s);
    prof.mark(w.caller.layout_mark);
    if (e == hipSuccess) {
        // one packed part of a caller that asked for it: ONE run, its streams lie as the output wants them, gaps included; one slotted part of a caller that asked
        // for that: the encoder's gather over its slots; else a run per chunk (none of a paged part's)
        if (w.run && live == 1 && src.p[0].slot_stride == 0) e = launch_run_gather(d_src, w.run, d_dst_off, 1, src.p[0].limit - src.p[0].src_base, d_out, d_err, s);
        else if (w.caller.compact_slots && live == 1 && src.p[0].slot_stride != kJoinPaged)
            e = launch_compact(src.p[0].in + src.p[0].src_base + src.p[0].first * src.p[0].slot_stride, src.p[0].slot_stride, d_lens, d_dst_off, (uint32_t)g.n_chunks, d_out, d_err, s);
        else if (any_unpaged) e = launch_run_gather(d_src, d_lens, d_dst_off, (uint32_t)g.n_chunks, w.longest_run, d_out, d_err, s);
    }
    K = 0;
    for (uint32_t i = 0; i < n_parts; ++i) {
        const density_hip_join_part_t& q = parts[i];
        if (q.chunk_count == 0) continue;
        const density_hip_header_t& h = *q.header;
        if ((h.flags & DENSITY_HIP_FLAG_PAGED) && e == hipSuccess)
            e = launch_unpage((const uint8_t*)q.container, q.chunk_count, payload_base(h.n_chunks, h.total_len, with_index) + dir_entry * q.first_chunk,
                              paged_pages_base(h.n_chunks, h.total_len, h.chunk_size), ppc, d_lens + K, d_dst_off + K, d_out, d_err, s);
        K += q.chunk_count;
    }
    prof.mark(w.caller.gather_mark);
    if (sealed) {
        if (e == hipSuccess) e = launch_place_trailer(trailers, live, d_out, cap, (uint32_t)g.n_chunks, d_err, s);
        prof.mark("move_trailer");
    }
    const auto named = [&w](const char* front, const char* back) { return std::string(front) + w.caller.name + back; };   // (a refusal's message: nothing is built where none is raised)
    if (e != hipSuccess) { set_error(named("kernel launch (", ")").c_str(), e); return DENSITY_HIP_ERR_RUNTIME; }
    if (header_out) {
        uint32_t h_err = 0;
        e = read_back(s, d_err, &h_err, header_out, d_out, sizeof(*header_out));
        if (e != hipSuccess) { set_error(named("", " (device)").c_str(), e); return DENSITY_HIP_ERR_RUNTIME; }
        if (h_err & 4u) { set_error(named("", ": a window the call cannot follow (size table, slots or page directory of its chunks)").c_str()); return DENSITY_HIP_ERR_FORMAT; }
        if (h_err) { set_error("container does not fit the output capacity"); return DENSITY_HIP_ERR_CAPACITY; }
    }
    return DENSITY_HIP_OK;
}

// A slice is a join of one part; its tables lie in plan_decode's arrays of the SOURCE (density_hip_decode_workspace_size), its packed window moves as one run.
// Pack and unpage are the slice [0, h.n_chunks) under marks and a name of their own (an empty container: a part that is skipped, and the front matter alone;
// it has no trailer, so it packs as an unsealed one).
int run_slice_container(DeviceCtx* c, const uint8_t* d_in, const density_hip_header_t& h, uint32_t first, uint32_t count, uint8_t* d_out, size_t cap, uint8_t* ws,
                        hipStream_t s, density_hip_header_t* header_out, const WindowCaller& caller) {
    const DecodePlan p = plan_decode(h.algo, h.n_chunks);
    const density_hip_join_part_t part{d_in, (size_t)h.container_len, &h, first, count};
    const uint32_t flags = (h.flags & DENSITY_HIP_FLAG_BLOCK_INDEX) | (header_trailer(h) ? DENSITY_HIP_FLAG_CHECKSUM : 0);
    const JoinGeometry g{h.algo, h.chunk_size, flags, 1, count, slice_len(h, first, count)};
    const WindowCall w{p.err(ws), p.produced(ws), p.offsets(ws), p.sizes(ws), p.offsets(ws) + h.n_chunks, (h.flags & DENSITY_HIP_FLAG_SLOTTED) ? slot_stride(h.algo, h.chunk_size) : safe_size(h.algo, h.chunk_size), caller};
    return run_windows(c, &part, 1, g, d_out, cap, w, s, header_out);
}

int run_join_container(DeviceCtx* c, const density_hip_join_part_t* parts, uint32_t n_parts, const JoinGeometry& g, uint8_t* d_out, size_t cap, uint8_t* ws,
                       hipStream_t s, density_hip_header_t* header_out) {
    const JoinPlan p = plan_join(g.n_chunks);
    const WindowCall w{p.err(ws), p.lens(ws), p.src(ws), p.dst_off(ws), nullptr, safe_size(g.algo, g.chunk_size), {"join_layout", "join_gather", "join", false}};
    return run_windows(c, parts, n_parts, g, d_out, cap, w, s, header_out);
}

// The seal of the container just written for d_in, in place: every chunk of the INPUT summed (checksum.hip), the trailer behind the container, the flag
// and the new length in its header.  Where the container ends, and how the input was cut, is read from the header on the device, so that nothing here
// waits for the encoder; the caller's copy of the header only lets the call refuse at once what the device would refuse.
int run_seal_container(DeviceCtx* c, const uint8_t* d_in, size_t n, uint8_t* d_out, size_t cap, const density_hip_header_t* header, uint8_t* ws, hipStream_t s,
                       density_hip_header_t* header_out) {
    if (header) {
        if (check_header(*header, cap) != DENSITY_HIP_OK) { set_error("seal: bad container header"); return DENSITY_HIP_ERR_ARGUMENT; }
        if (header->flags & DENSITY_HIP_FLAG_CHECKSUM) { set_error("seal: the container is sealed already"); return DENSITY_HIP_ERR_ARGUMENT; }
        if (header->total_len != n) { set_error("seal: input_size is not the container's total_len"); return DENSITY_HIP_ERR_ARGUMENT; }
        if (align_up(header->container_len, 16) + trailer_bytes(header->n_chunks) > cap) { set_error("seal: the capacity does not hold the trailer (density_hip_seal_overhead())"); return DENSITY_HIP_ERR_CAPACITY; }
    }
    const SealPlan p = plan_seal(n);
    Profiler prof(c, s);
    hipError_t e = hipMemsetAsync(p.err(ws), 0, sizeof(uint32_t), s);
    if (e == hipSuccess) e = launch_seal(d_in, n, d_out, cap, p.geom(ws), p.acc(ws), p.err(ws), s);
    prof.mark("checksum_seal");
    if (e != hipSuccess) { set_error("kernel launch (seal)", e); return DENSITY_HIP_ERR_RUNTIME; }
    if (header_out) {
        uint32_t h_err = 0;
        e = read_back(s, p.err(ws), &h_err, header_out, d_out, sizeof(*header_out));
        if (e != hipSuccess) { set_error("seal (device)", e); return DENSITY_HIP_ERR_RUNTIME; }
        if (h_err & 1u) { set_error("seal: not this input's unsealed container (sealed already, or input_size is not its total_len)"); return DENSITY_HIP_ERR_ARGUMENT; }
        if (h_err) { set_error("seal: the capacity does not hold the trailer (density_hip_seal_overhead())"); return DENSITY_HIP_ERR_CAPACITY; }
    }
    return DENSITY_HIP_OK;
}

namespace {
// the three density_hip_encode_device* symbols: they differ in the form asked for
int encode_device(Form form, int algo, const void* d_input, size_t input_size, void* d_output, size_t output_capacity, size_t chunk_size, void* d_workspace,
                  size_t workspace_size, void* stream, density_hip_header_t* header_out) {
    g_last_error.clear();
    if (!take_geometry(algo, input_size, &chunk_size) || (!d_input && input_size) || !d_output) { set_error("bad argument"); return DENSITY_HIP_ERR_ARGUMENT; }
    DeviceCtx* c = acquire_ctx();
    if (!c) return DENSITY_HIP_ERR_RUNTIME;
    std::lock_guard<std::mutex> lk(c->mu);
    const size_t need = plan_encode(algo, input_size, chunk_size).total;
    uint8_t* ws = nullptr;
    if (const int rc = resolve_workspace(c, d_workspace, workspace_size, need, need, &ws)) return rc;
    return run_encode_container(c, algo, (const uint8_t*)d_input, input_size, (uint8_t*)d_output, output_capacity, chunk_size, ws, stream ? (hipStream_t)stream : c->stream, header_out, form);
}
// the header of an object on the device: the caller's copy, or read back on s — ordered behind whatever produced the object on the caller's
// stream (streams here are non-blocking: a plain hipMemcpy is not).  Not judged here.
template <typename Header>
int fetch_header(const Header* header, const void* d_object, hipStream_t s, Header* h, const char* what) {
    if (header) { *h = *header; return DENSITY_HIP_OK; }
    hipError_t e = hipMemcpyAsync(h, d_object, sizeof(*h), hipMemcpyDeviceToHost, s);
    if (e == hipSuccess) e = hipStreamSynchronize(s);
    if (e != hipSuccess) { set_error(what, e); return DENSITY_HIP_ERR_RUNTIME; }
    return DENSITY_HIP_OK;
}
// a container's header, checked against the container's size
int container_header(const density_hip_header_t* header, const void* d_container, size_t container_size, hipStream_t s, density_hip_header_t* h) {
    if (const int rc = fetch_header(header, d_container, s, h, "header read-back")) return rc;
    if (check_header(*h, container_size) != DENSITY_HIP_OK) { set_error("bad container header"); return DENSITY_HIP_ERR_FORMAT; }
    return DENSITY_HIP_OK;
}
// a parity blob's header (at least sizeof(*ph) bytes of the blob are there); check_parity_header / check_parity_update judge it
int parity_header(const density_hip_parity_header_t* header, const void* d_parity, hipStream_t s, density_hip_parity_header_t* ph) {
    return fetch_header(header, d_parity, s, ph, "parity header read-back");
}
// The opening of the calls that repack ONE container (density_hip_pack_device, _unpage_device, _slice_device): the arguments all of them refuse, the context
// — locked while the Repack lives —, the stream and the container's header as fetch_header gives it.  What a call asks of the header, in which order and under
// which code, stands in the call; then the workspace (plan_decode's arrays of the source) and the driver, run_slice_container.
struct Repack {
    DeviceCtx* c = nullptr;
    std::unique_lock<std::mutex> lk;
    hipStream_t s = nullptr;
    density_hip_header_t h;
    uint8_t* ws = nullptr;
};
int open_repack(const void* d_container, size_t container_size, const density_hip_header_t* header, const void* d_output, void* stream, Repack* r) {
    g_last_error.clear();
    if (!d_container || container_size < sizeof(density_hip_header_t) || !d_output) { set_error("bad argument"); return DENSITY_HIP_ERR_ARGUMENT; }
    r->c = acquire_ctx();
    if (!r->c) return DENSITY_HIP_ERR_RUNTIME;
    r->lk = std::unique_lock<std::mutex>(r->c->mu);
    r->s = stream ? (hipStream_t)stream : r->c->stream;
    return fetch_header(header, d_container, r->s, &r->h, "header read-back");
}
int repack_workspace(Repack* r, void* d_workspace, size_t workspace_size) {
    const size_t need = plan_decode(r->h.algo, r->h.n_chunks).total;
    return resolve_workspace(r->c, d_workspace, workspace_size, need, need, &r->ws);
}
// what pack and unpage ask of the output: the packed bound of the whole container, and the seal's share where a trailer comes along
int whole_capacity(const density_hip_header_t& h, size_t cap) {
    const bool trailer = header_trailer(h) != 0;
    if (cap >= container_bound(h.algo, h.total_len, h.chunk_size) + (trailer ? seal_overhead(h.n_chunks) : 0)) return DENSITY_HIP_OK;
    set_error(trailer ? "output capacity below density_hip_container_bound() + density_hip_seal_overhead()" : "output capacity below density_hip_container_bound()");
    return DENSITY_HIP_ERR_CAPACITY;
}
// density_hip_parity_device and density_hip_parity2_device: they differ in the blob's version
int parity_device(uint8_t version, const void* d_input, size_t input_size, size_t chunk_size, uint32_t n_groups, void* d_parity, size_t parity_capacity, void* stream) {
    g_last_error.clear();
    const size_t need = parity_size_of(version, input_size, chunk_size, n_groups);
    if (!need || (!d_input && input_size) || !d_parity) { set_error("bad argument"); return DENSITY_HIP_ERR_ARGUMENT; }
    if (parity_capacity < need) { set_error("parity capacity below density_hip_parity_size() / density_hip_parity2_size()"); return DENSITY_HIP_ERR_CAPACITY; }
    DeviceCtx* c = acquire_ctx();
    if (!c) return DENSITY_HIP_ERR_RUNTIME;
    std::lock_guard<std::mutex> lk(c->mu);
    hipStream_t s = stream ? (hipStream_t)stream : c->stream;
    Profiler prof(c, s);
    const hipError_t e = launch_parity_rows((const uint8_t*)d_input, make_parity_header(input_size, chunk_size, n_groups, version), (uint8_t*)d_parity, s);
    prof.mark(version == 2 ? "parity2_rows" : "parity_rows");
    if (e != hipSuccess) { set_error("kernel launch (parity)", e); return DENSITY_HIP_ERR_RUNTIME; }
    return DENSITY_HIP_OK;
}
}  // namespace

}  // namespace api
}  // namespace density

using namespace density;
using namespace density::api;

extern "C" {

// ---- section 2: container + device API ----
size_t density_hip_container_bound(int algo, size_t input_size, size_t chunk_size) {
    return take_geometry(algo, input_size, &chunk_size) ? container_bound(algo, input_size, chunk_size) : 0;
}

size_t density_hip_encode_workspace_size(int algo, size_t input_size, size_t chunk_size) {
    return take_geometry(algo, input_size, &chunk_size) ? plan_encode(algo, input_size, chunk_size).total : 0;
}

size_t density_hip_decode_workspace_size(uint32_t n_chunks) {   // the largest of the three algorithms
    const size_t a = plan_decode(DENSITY_HIP_LION, n_chunks).total, b = plan_decode(DENSITY_HIP_CHAMELEON, n_chunks).total;
    return a > b ? a : b;
}

size_t density_hip_decode_workspace_size_for(int algo, size_t total_len, size_t chunk_size) {
    return take_geometry(algo, total_len, &chunk_size) ? plan_decode(algo, chunk_count(total_len, chunk_size), chunk_size).total_with_passes : 0;
}

int density_hip_encode_device(int algo, const void* d_input, size_t input_size, void* d_output, size_t output_capacity, size_t chunk_size,
                              void* d_workspace, size_t workspace_size, void* stream, density_hip_header_t* header_out) {
    return encode_device(Form::Packed, algo, d_input, input_size, d_output, output_capacity, chunk_size, d_workspace, workspace_size, stream, header_out);
}
int density_hip_encode_device_slotted(int algo, const void* d_input, size_t input_size, void* d_output, size_t output_capacity, size_t chunk_size,
                                      void* d_workspace, size_t workspace_size, void* stream, density_hip_header_t* header_out) {
    return encode_device(Form::Slotted, algo, d_input, input_size, d_output, output_capacity, chunk_size, d_workspace, workspace_size, stream, header_out);
}
int density_hip_encode_device_paged(int algo, const void* d_input, size_t input_size, void* d_output, size_t output_capacity, size_t chunk_size,
                                    void* d_workspace, size_t workspace_size, void* stream, density_hip_header_t* header_out) {
    return encode_device(Form::Paged, algo, d_input, input_size, d_output, output_capacity, chunk_size, d_workspace, workspace_size, stream, header_out);
}
size_t density_hip_paged_pages_per_chunk(size_t chunk_size) { return valid_chunk(chunk_size) ? paged_pages_per_chunk(chunk_size) : 0; }
size_t density_hip_container_bound_paged(int algo, size_t input_size, size_t chunk_size) {
    return take_geometry(algo, input_size, &chunk_size) ? container_bound_paged(algo, input_size, chunk_size) : 0;
}

size_t density_hip_container_bound_slotted(int algo, size_t input_size, size_t chunk_size) {
    if (!take_geometry(algo, input_size, &chunk_size)) return 0;
    const size_t a = container_bound_slotted(algo, input_size, chunk_size), b = container_bound(algo, input_size, chunk_size);
    return a > b ? a : b;
}

int density_hip_pack_device(const void* d_container, size_t container_size, const density_hip_header_t* header, void* d_output,
                            size_t output_capacity, void* d_workspace, size_t workspace_size, void* stream, density_hip_header_t* header_out) {
    Repack r;
    if (const int rc = open_repack(d_container, container_size, header, d_output, stream, &r)) return rc;
    if (check_header(r.h, container_size) != DENSITY_HIP_OK) { set_error("bad container header"); return DENSITY_HIP_ERR_FORMAT; }
    // a PAGED container is wire-ready as it stands, and its streams are not where the packed / slotted arithmetic looks for them
    if (r.h.flags & DENSITY_HIP_FLAG_PAGED) { set_error("density_hip_pack_device: a paged container is not packed (it is wire-ready; decode it or read its pages)"); return DENSITY_HIP_ERR_UNSUPPORTED; }
    if (const int rc = repack_workspace(&r, d_workspace, workspace_size)) return rc;
    if (const int rc = whole_capacity(r.h, output_capacity)) return rc;
    return run_slice_container(r.c, (const uint8_t*)d_container, r.h, 0, r.h.n_chunks, (uint8_t*)d_output, output_capacity, r.ws, r.s, header_out, {"layout_encode", "compact", "pack", true});
}

int density_hip_unpage_device(const void* d_container, size_t container_size, const density_hip_header_t* header, void* d_output,
                              size_t output_capacity, void* d_workspace, size_t workspace_size, void* stream, density_hip_header_t* header_out) {
    Repack r;
    if (const int rc = open_repack(d_container, container_size, header, d_output, stream, &r)) return rc;
    if (check_header(r.h, container_size) != DENSITY_HIP_OK) { set_error("bad container header"); return DENSITY_HIP_ERR_FORMAT; }
    if (!(r.h.flags & DENSITY_HIP_FLAG_PAGED)) { set_error("density_hip_unpage_device: not a paged container (density_hip_pack_device takes the packed and slotted forms)"); return DENSITY_HIP_ERR_ARGUMENT; }
    if (const int rc = repack_workspace(&r, d_workspace, workspace_size)) return rc;
    if (const int rc = whole_capacity(r.h, output_capacity)) return rc;
    return run_slice_container(r.c, (const uint8_t*)d_container, r.h, 0, r.h.n_chunks, (uint8_t*)d_output, output_capacity, r.ws, r.s, header_out, {"layout_encode", "unpage", "unpage", false});
}

int density_hip_chunk_range(const density_hip_header_t* header, uint64_t offset, uint64_t length, uint32_t* first_chunk, uint32_t* chunk_count, uint64_t* skip) {
    if (!header || !header_is_containers(*header) || !first_chunk || !chunk_count || !skip) return DENSITY_HIP_ERR_ARGUMENT;
    if (length == 0 || offset > header->total_len || length > header->total_len - offset) return DENSITY_HIP_ERR_ARGUMENT;
    const uint64_t first = offset / header->chunk_size, last = (offset + length - 1) / header->chunk_size;
    *first_chunk = (uint32_t)first;
    *chunk_count = (uint32_t)(last - first + 1);
    *skip = offset - first * header->chunk_size;
    return DENSITY_HIP_OK;
}

size_t density_hip_slice_bound(const density_hip_header_t* header, uint32_t first_chunk, uint32_t chunk_count) {
    return header ? slice_bound(*header, first_chunk, chunk_count) : 0;
}

int density_hip_slice_device(const void* d_container, size_t container_size, const density_hip_header_t* header, uint32_t first_chunk, uint32_t chunk_count, void* d_output,
                             size_t output_capacity, void* d_workspace, size_t workspace_size, void* stream, density_hip_header_t* header_out) {
    if (chunk_count == 0) { set_error("bad argument"); return DENSITY_HIP_ERR_ARGUMENT; }
    Repack r;
    if (const int rc = open_repack(d_container, container_size, header, d_output, stream, &r)) return rc;
    if (!header_is_containers(r.h)) { set_error("slice: not a container's header"); return DENSITY_HIP_ERR_ARGUMENT; }
    if ((uint64_t)first_chunk + chunk_count > r.h.n_chunks) { set_error("slice: the window is not inside the container's chunks"); return DENSITY_HIP_ERR_ARGUMENT; }
    if (output_capacity < slice_bound(r.h, first_chunk, chunk_count)) { set_error("output capacity below density_hip_slice_bound()"); return DENSITY_HIP_ERR_CAPACITY; }
    if (check_header(r.h, container_size) != DENSITY_HIP_OK) { set_error("bad container header (its length, or its trailer's, against container_size)"); return DENSITY_HIP_ERR_FORMAT; }
    if (const int rc = repack_workspace(&r, d_workspace, workspace_size)) return rc;
    return run_slice_container(r.c, (const uint8_t*)d_container, r.h, first_chunk, chunk_count, (uint8_t*)d_output, output_capacity, r.ws, r.s, header_out);
}

size_t density_hip_join_bound(const density_hip_join_part_t* parts, uint32_t n_parts) {
    JoinGeometry g;
    return join_geometry(parts, n_parts, &g) ? 0 : join_bound(g);
}

size_t density_hip_join_workspace_size(uint32_t n_parts, uint32_t n_chunks_out) {
    return (n_parts == 0 || n_parts > DENSITY_HIP_JOIN_MAX_PARTS || n_chunks_out == 0) ? 0 : plan_join(n_chunks_out).total;
}

int density_hip_join_device(const density_hip_join_part_t* parts, uint32_t n_parts, void* d_output, size_t output_capacity, void* d_workspace, size_t workspace_size,
                            void* stream, density_hip_header_t* header_out) {
    g_last_error.clear();
    JoinGeometry g;
    if (const char* why = join_geometry(parts, n_parts, &g)) { set_error(why); return DENSITY_HIP_ERR_ARGUMENT; }
    if (!d_output) { set_error("bad argument"); return DENSITY_HIP_ERR_ARGUMENT; }
    const uintptr_t o0 = (uintptr_t)d_output, o1 = o0 + output_capacity;
    for (uint32_t p = 0; p < n_parts; ++p) {
        const uintptr_t c0 = (uintptr_t)parts[p].container, c1 = c0 + parts[p].container_size;
        if (parts[p].chunk_count && c0 < o1 && o0 < c1) { set_error("join: the output overlaps a part"); return DENSITY_HIP_ERR_ARGUMENT; }
    }
    if (output_capacity < join_bound(g)) { set_error("output capacity below density_hip_join_bound()"); return DENSITY_HIP_ERR_CAPACITY; }
    if (const int rc = check_join_parts(parts, n_parts)) return rc;
    DeviceCtx* c = acquire_ctx();
    if (!c) return DENSITY_HIP_ERR_RUNTIME;
    std::lock_guard<std::mutex> lk(c->mu);
    hipStream_t s = stream ? (hipStream_t)stream : c->stream;
    const size_t need = plan_join(g.n_chunks).total;
    uint8_t* ws = nullptr;
    if (const int rc = resolve_workspace(c, d_workspace, workspace_size, need, need, &ws)) return rc;
    return run_join_container(c, parts, n_parts, g, (uint8_t*)d_output, output_capacity, ws, s, header_out);
}

int density_hip_decode_device(const void* d_container, size_t container_size, const density_hip_header_t* header, void* d_output,
                              size_t output_capacity, void* d_workspace, size_t workspace_size, void* stream, size_t* decoded_size_out) {
    g_last_error.clear();
    if (!d_container || container_size < sizeof(density_hip_header_t) || (!d_output && output_capacity)) { set_error("bad argument"); return DENSITY_HIP_ERR_ARGUMENT; }
    DeviceCtx* c = acquire_ctx();
    if (!c) return DENSITY_HIP_ERR_RUNTIME;
    std::lock_guard<std::mutex> lk(c->mu);
    density_hip_header_t h;
    hipStream_t s = stream ? (hipStream_t)stream : c->stream;
    if (const int rc = container_header(header, d_container, container_size, s, &h)) return rc;
    // a caller's workspace need only hold what the one-wave decoders want (the decode passes are then left out: DecodePlan::pass); the context's own
    // is sized for the passes, and what it holds is what the driver is told
    const DecodePlan dp = plan_decode(h.algo, h.n_chunks, h.chunk_size);
    uint8_t* ws = nullptr;
    if (const int rc = resolve_workspace(c, d_workspace, workspace_size, dp.total, dp.total_with_passes, &ws, &workspace_size)) return rc;
    return run_decode_container(c, (const uint8_t*)d_container, container_size, h, (uint8_t*)d_output, output_capacity, ws, s, decoded_size_out, workspace_size);
}

int density_hip_decode_device_verdicts(const void* d_container, size_t container_size, const density_hip_header_t* header, void* d_output, size_t output_capacity,
                                       void* d_workspace, size_t workspace_size, void* stream, uint32_t* d_verdicts, unsigned flags, uint32_t* damaged_out) {
    g_last_error.clear();
    if (!d_container || container_size < sizeof(density_hip_header_t) || (!d_output && output_capacity) || (flags & ~DENSITY_HIP_SALVAGE_BLANK) || (uintptr_t)d_verdicts % 4 != 0) {
        set_error("bad argument"); return DENSITY_HIP_ERR_ARGUMENT;
    }
    DeviceCtx* c = acquire_ctx();
    if (!c) return DENSITY_HIP_ERR_RUNTIME;
    std::lock_guard<std::mutex> lk(c->mu);
    density_hip_header_t h;
    hipStream_t s = stream ? (hipStream_t)stream : c->stream;
    if (const int rc = container_header(header, d_container, container_size, s, &h)) return rc;
    if (!(h.flags & DENSITY_HIP_FLAG_CHECKSUM)) { set_error("verdicts: the container is not sealed (no trailer to hold its chunks against)"); return DENSITY_HIP_ERR_ARGUMENT; }
    if (!d_verdicts && h.n_chunks) { set_error("bad argument"); return DENSITY_HIP_ERR_ARGUMENT; }
    const DecodePlan dp = plan_decode(h.algo, h.n_chunks, h.chunk_size);      // (the workspace rules of density_hip_decode_device)
    uint8_t* ws = nullptr;
    if (const int rc = resolve_workspace(c, d_workspace, workspace_size, dp.total, dp.total_with_passes, &ws, &workspace_size)) return rc;
    return run_decode_verdicts(c, (const uint8_t*)d_container, container_size, h, (uint8_t*)d_output, output_capacity, ws, s, workspace_size, d_verdicts, flags, damaged_out);
}

int density_hip_decode_device_recover(const void* d_container, size_t container_size, const density_hip_header_t* header, const void* d_parity, size_t parity_size,
                                      const density_hip_parity_header_t* parity_header, void* d_output, size_t output_capacity, void* d_workspace, size_t workspace_size,
                                      void* stream, uint32_t* d_verdicts, unsigned flags, uint32_t* damaged_out, uint32_t* recovered_out) {
    g_last_error.clear();
    if (!d_container || container_size < sizeof(density_hip_header_t) || (!d_output && output_capacity) || (flags & ~DENSITY_HIP_SALVAGE_BLANK) || (uintptr_t)d_verdicts % 4 != 0 || !d_parity) {
        set_error("bad argument"); return DENSITY_HIP_ERR_ARGUMENT;
    }
    DeviceCtx* c = acquire_ctx();
    if (!c) return DENSITY_HIP_ERR_RUNTIME;
    std::lock_guard<std::mutex> lk(c->mu);
    density_hip_header_t h;
    hipStream_t s = stream ? (hipStream_t)stream : c->stream;
    if (const int rc = container_header(header, d_container, container_size, s, &h)) return rc;
    if (!(h.flags & DENSITY_HIP_FLAG_CHECKSUM)) { set_error("recover: the container is not sealed (no trailer to hold its chunks against)"); return DENSITY_HIP_ERR_ARGUMENT; }
    if (!d_verdicts && h.n_chunks) { set_error("bad argument"); return DENSITY_HIP_ERR_ARGUMENT; }
    if (parity_size < sizeof(density_hip_parity_header_t)) { set_error("parity blob shorter than its header"); return DENSITY_HIP_ERR_FORMAT; }
    density_hip_parity_header_t ph;
    if (const int rc = api::parity_header(parity_header, d_parity, s, &ph)) return rc;
    if (const int rc = check_parity_header(ph, h, parity_size)) return rc;
    const DecodePlan dp = plan_decode(h.algo, h.n_chunks, h.chunk_size);      // (the workspace rules of density_hip_decode_device)
    uint8_t* ws = nullptr;
    if (const int rc = resolve_workspace(c, d_workspace, workspace_size, dp.total, dp.total_with_passes, &ws, &workspace_size)) return rc;
    const Recovery rec{(const uint8_t*)d_parity + sizeof(ph), ph.n_groups, ph.row_bytes, ph.version == 2, recovered_out};
    return run_decode_verdicts(c, (const uint8_t*)d_container, container_size, h, (uint8_t*)d_output, output_capacity, ws, s, workspace_size, d_verdicts, flags, damaged_out, &rec);
}

size_t density_hip_parity_size(size_t input_size, size_t chunk_size, uint32_t n_groups) { return parity_size_of(1, input_size, chunk_size, n_groups); }
size_t density_hip_parity2_size(size_t input_size, size_t chunk_size, uint32_t n_groups) { return parity_size_of(2, input_size, chunk_size, n_groups); }

int density_hip_parity_device(const void* d_input, size_t input_size, size_t chunk_size, uint32_t n_groups, void* d_parity, size_t parity_capacity, void* stream) {
    return parity_device(1, d_input, input_size, chunk_size, n_groups, d_parity, parity_capacity, stream);
}
int density_hip_parity2_device(const void* d_input, size_t input_size, size_t chunk_size, uint32_t n_groups, void* d_parity, size_t parity_capacity, void* stream) {
    return parity_device(2, d_input, input_size, chunk_size, n_groups, d_parity, parity_capacity, stream);
}

// the one place the geometry rules of a parity update live (include/density_hip.h): density_hip_parity_update_device and density_hip_parity_update go through it
int density_hip_parity_update_header(const density_hip_parity_header_t* header, uint64_t offset, size_t old_size, size_t new_size, density_hip_parity_header_t* header_out) {
    g_last_error.clear();
    if (!header || !parity_header_is_blobs(*header)) { set_error("parity update: not a parity blob's header"); return DENSITY_HIP_ERR_ARGUMENT; }
    const density_hip_parity_header_t& ph = *header;
    const bool same_size = old_size == new_size && offset <= ph.total_len && old_size <= ph.total_len - offset;
    const bool tail = offset <= ph.total_len && old_size == ph.total_len - offset;
    if (!same_size && !tail) { set_error("parity update: neither a same-size edit inside the input nor an edit of its tail"); return DENSITY_HIP_ERR_ARGUMENT; }
    const uint64_t total = same_size ? ph.total_len : offset + new_size;
    if (total < offset || chunk_count(total, ph.chunk_size) > 0xffffffffull) { set_error("parity update: the edited input is too long"); return DENSITY_HIP_ERR_ARGUMENT; }
    density_hip_parity_header_t after = make_parity_header(total, ph.chunk_size, ph.n_groups, ph.version);
    if (after.n_groups != ph.n_groups || (after.n_chunks && !after.n_groups) || after.row_bytes != ph.row_bytes) {
        set_error("parity update: the edited input's blob has other rows than this one (fewer chunks than groups, or a single short chunk changing length): make a new blob");
        return DENSITY_HIP_ERR_ARGUMENT;
    }
    if (after.version == 2 && parity_group_members(after) > kParityQMembers) { set_error("parity update: a group of more than 255 chunks (version 2): make a new blob"); return DENSITY_HIP_ERR_ARGUMENT; }
    if (header_out) *header_out = after;
    return DENSITY_HIP_OK;
}

int density_hip_parity_update_device(void* d_parity, size_t parity_size, const density_hip_parity_header_t* parity_header, uint64_t offset, const void* d_old, size_t old_size,
                                     const void* d_new, size_t new_size, void* stream, density_hip_parity_header_t* header_out) {
    g_last_error.clear();
    if (!d_parity || (!d_old && old_size) || (!d_new && new_size)) { set_error("bad argument"); return DENSITY_HIP_ERR_ARGUMENT; }
    if (parity_size < sizeof(density_hip_parity_header_t)) { set_error("parity blob shorter than its header"); return DENSITY_HIP_ERR_FORMAT; }
    density_hip_parity_header_t after;
    if (parity_header) {                                                      // (everything is decided before a device is acquired)
        if (const int rc = check_parity_update(*parity_header, parity_size, offset, old_size, new_size, &after)) return rc;
        if (header_out) *header_out = after;
        if (!old_size && !new_size) return DENSITY_HIP_OK;
    }
    DeviceCtx* c = acquire_ctx();
    if (!c) return DENSITY_HIP_ERR_RUNTIME;
    std::lock_guard<std::mutex> lk(c->mu);
    hipStream_t s = stream ? (hipStream_t)stream : c->stream;
    if (!parity_header) {
        density_hip_parity_header_t ph;
        if (const int rc = api::parity_header(nullptr, d_parity, s, &ph)) return rc;
        if (const int rc = check_parity_update(ph, parity_size, offset, old_size, new_size, &after)) return rc;
        if (header_out) *header_out = after;
        if (!old_size && !new_size) return DENSITY_HIP_OK;
    }
    Profiler prof(c, s);
    const hipError_t e = launch_parity_update((uint8_t*)d_parity, after, offset, (const uint8_t*)d_old, old_size, (const uint8_t*)d_new, new_size, s);
    prof.mark("parity_update");
    if (e != hipSuccess) { set_error("kernel launch (parity update)", e); return DENSITY_HIP_ERR_RUNTIME; }
    return DENSITY_HIP_OK;
}

int density_hip_checksum_device(const void* d_data, size_t size, size_t chunk_size, uint32_t* d_sums, void* stream) {
    g_last_error.clear();
    const size_t n_chunks = valid_chunk(chunk_size) ? chunk_count(size, chunk_size) : 0;
    if (!valid_chunk(chunk_size) || n_chunks > 0xffffffffull || (size && (!d_data || !d_sums)) || (uintptr_t)d_sums % 4 != 0) { set_error("bad argument"); return DENSITY_HIP_ERR_ARGUMENT; }
    DeviceCtx* c = acquire_ctx();
    if (!c) return DENSITY_HIP_ERR_RUNTIME;
    const hipError_t e = launch_checksum((const uint8_t*)d_data, size, (uint32_t)chunk_size, (uint32_t)n_chunks, d_sums, nullptr, nullptr, stream ? (hipStream_t)stream : c->stream);
    if (e != hipSuccess) { set_error("kernel launch (checksum)", e); return DENSITY_HIP_ERR_RUNTIME; }
    return DENSITY_HIP_OK;
}

int density_hip_seal_device(const void* d_input, size_t input_size, void* d_container, size_t container_capacity, const density_hip_header_t* header,
                            void* stream, density_hip_header_t* header_out) {
    g_last_error.clear();
    if (!d_container || container_capacity < sizeof(density_hip_header_t) || (!d_input && input_size)) { set_error("bad argument"); return DENSITY_HIP_ERR_ARGUMENT; }
    DeviceCtx* c = acquire_ctx();
    if (!c) return DENSITY_HIP_ERR_RUNTIME;
    std::lock_guard<std::mutex> lk(c->mu);
    const size_t need = plan_seal(input_size).total;
    uint8_t* ws = nullptr;
    if (const int rc = resolve_workspace(c, nullptr, 0, need, need, &ws)) return rc;
    return run_seal_container(c, (const uint8_t*)d_input, input_size, (uint8_t*)d_container, container_capacity, header, ws, stream ? (hipStream_t)stream : c->stream, header_out);
}

uint64_t density_hip_decode_pass_count(void) { return g_pass_decodes; }
void density_hip_stage_stats(uint64_t* out2) { if (out2) { out2[0] = density::g_stage_stats[0]; out2[1] = density::g_stage_stats[1]; } }
void density_hip_stream_stats(uint64_t* out4) { if (out4) for (int i = 0; i < 4; ++i) out4[i] = g_stream_stats[i]; }
size_t density_hip_auto_chunk(size_t input_size) { return auto_chunk(input_size); }
size_t density_hip_auto_chunk_for(int algo, size_t input_size) { return valid_algo(algo) ? auto_chunk(input_size, algo) : 0; }

void density_hip_set_profiling(int enabled) { g_profiling = enabled; }
void density_hip_set_kernel_variant(int variant) {
    g_variant = variant;                 // what this layer asks through variant(): kVarNoIndex, kVarBatchedStitch, kVarPipeAlways, kVarPipeNever, kVarNoRotor
    const auto on = [variant](int bits) { return (variant & bits) != 0; };
    density::g_force_simple = on(kVarSimple);
    density::g_force_pipeline = on(kVarRolePipeline);
    density::g_force_lane_codec = on(kVarLaneCodec);
    density::g_force_wave_codec = on(kVarWaveCodec);
    density::g_stage_audit = on(kVarStageAudit);
    density::g_force_serial_decode = on(kVarSerialDecode);
    density::g_serial_parse = on(kVarSerialParse);
    density::g_lion_one_wave = on(kVarLionOneWave);
    density::g_rotor_split = density::kRotorSplitDefault != on(kVarRotorOtherSplit);
}

int density_hip_last_timings(float* milliseconds, const char** names, int capacity) {
    int dev = -1;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= kMaxDevices) return 0;
    DeviceCtx* c = &g_ctx[dev];
    std::lock_guard<std::mutex> lk(c->mu);
    if (c->n_marks < 2) { c->n_marks = 0; return 0; }
    if (hipEventSynchronize(c->events[c->n_marks - 1]) != hipSuccess) { c->n_marks = 0; return 0; }
    int n = 0;
    for (size_t i = 1; i < c->n_marks && n < capacity; ++i) {
        if (!c->names[i]) continue;                       // start-of-call mark
        float ms = 0.f;
        (void)hipEventElapsedTime(&ms, c->events[i - 1], c->events[i]);
        if (milliseconds) milliseconds[n] = ms;
        if (names) names[n] = c->names[i];
        ++n;
    }
    c->n_marks = 0;
    return n;
}

int density_hip_selftest(void) {
    g_last_error.clear();
    return acquire_ctx() ? 0 : 1;
}

int density_hip_selftest_bits(void) {
    g_last_error.clear();
    int dev = -1;
    (void)acquire_ctx();
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= kMaxDevices || !g_ctx[dev].ready) return -1;
    return (int)g_ctx[dev].selftest_bits;
}

void density_hip_shutdown(void) {
    for (int d = 0; d < kMaxDevices; ++d) {
        DeviceCtx* c = &g_ctx[d];
        std::lock_guard<std::mutex> lk(c->mu);
        if (!c->ready) continue;
        int cur = -1;
        if (hipGetDevice(&cur) != hipSuccess || hipSetDevice(d) != hipSuccess) { (void)hipGetLastError(); continue; }
        (void)hipDeviceSynchronize();
        for (Buffer* b : {&c->work, &c->stage_in, &c->stage_out, &c->seg}) { if (b->p) (void)hipFree(b->p); b->p = nullptr; b->cap = 0; }
        c->pin_sizes.release();
        c->pin_meta.release();
        for (hipEvent_t ev : c->pipe_events) (void)hipEventDestroy(ev);
        c->pipe_events.clear();
        for (hipEvent_t ev : c->events) (void)hipEventDestroy(ev);
        c->events.clear(); c->names.clear(); c->n_marks = 0;
        for (hipStream_t* sp : {&c->up, &c->down, &c->kern[0], &c->kern[1], &c->kern[2], &c->kern[3], &c->stream, &c->stitch_stream}) { if (*sp) (void)hipStreamDestroy(*sp); *sp = nullptr; }
        for (auto& ev : c->batch_done) { if (ev) (void)hipEventDestroy(ev); ev = nullptr; }
        if (c->stitch_done) (void)hipEventDestroy(c->stitch_done);
        c->stitch_done = nullptr;
        c->ready = false;                                                           // the next call sets the context up again (self-test included)
        (void)hipSetDevice(cur);
    }
}
const char* density_hip_last_error(void) { return g_last_error.c_str(); }
#ifndef DENSITY_HIP_KERNELS_ID
#define DENSITY_HIP_KERNELS_ID "unversioned"
#endif
const char* density_hip_version(void) { return "density_hip 0.2 (gfx950; reference: density-rs 0.16.6; kernels " DENSITY_HIP_KERNELS_ID ")"; }

}  // extern "C"
