// api_host.hip — the host-pointer container calls (include/density_hip.h: density_hip_encode / density_hip_decode / density_hip_decoded_size):
// staged whole through device memory, or — Chameleon inputs worth three slices — pipelined in slices with the caller's buffers pinned in place.
#include "api_internal.hpp"

namespace density {
namespace api {

bool pipe_streams(DeviceCtx* c, uint32_t n_events) {
    hipError_t e = hipSuccess;
    if (!c->up) {
        e = hipStreamCreateWithFlags(&c->up, hipStreamNonBlocking);
        if (e == hipSuccess) e = hipStreamCreateWithFlags(&c->down, hipStreamNonBlocking);
        for (int i = 0; i < 4 && e == hipSuccess; ++i) e = hipStreamCreateWithFlags(&c->kern[i], hipStreamNonBlocking);
    }
    while (e == hipSuccess && c->pipe_events.size() < n_events) {
        hipEvent_t ev;
        e = hipEventCreateWithFlags(&ev, hipEventDisableTiming);
        if (e == hipSuccess) c->pipe_events.push_back(ev);
    }
    if (e != hipSuccess) { set_error("pipelined host path: streams / events", e); return false; }
    return true;
}

namespace {

// ---------------------------------------------------------------------------------------------------------------
// The host-pointer container calls, pipelined (Chameleon, inputs worth three slices and more: pipe_wanted).
// The caller's buffers are pinned in place for the duration of the call (hipHostRegister: microseconds on this platform,
// probes/host_register.hip), so that copies from and to them are asynchronous; the input goes up in slices of chunks on one stream,
// every slice is encoded / decoded on one of four kernel streams as soon as it has arrived — chunks are independent, the slices'
// kernels run side by side — and its result goes down on a third stream while later slices are still on their way up.  A PCIe link
// moves 56 GB/s one way and 46 each way at once (probes/pcie_duplex.hip): a call that moves N up and E down in sequence cannot do
// better than N / (N + E) x 56 = 35 GB/s; overlapped it is bound by the larger of the two.  Where pinning fails (memory that is
// already registered, read-only mappings) the plain staged path below is taken.
// ---------------------------------------------------------------------------------------------------------------
// Slices of whole chunks.  A slice's kernel takes as long as ONE chunk takes (0.11 ms per MiB of chunk: chunks run side by side, a chunk is a
// chain) and the kernels of different slices mostly queue up behind one another (the streams share a few hardware queues), so a slice
// must be worth ~10 chunk lengths of transfer or the kernels, not the link, set the pace: a twelfth of the input, ten chunks, 2 MiB at least —
// and the call is pipelined only where that makes three slices or more (measured, 4 MiB chunks: 64 MiB staged 28 / 29 GB/s, pipelined
// in slices of two chunks 31 / 21; 256 MiB 33 / 33 -> 46 / 45; 1 GiB 34 / 35 -> 50 / 48).
inline size_t pipe_slice_bytes(size_t total, size_t chunk) {
    size_t target = total / 12;
    if (target < 10 * chunk) target = 10 * chunk;
    if (target < (2u << 20)) target = 2u << 20;
    if (variant(kVarPipeAlways)) target = chunk;                                             // (tests: a slice per chunk, whatever the size)
    return target;
}
inline bool pipe_wanted(int algo, size_t n, size_t chunk, size_t n_chunks) {
    if (algo != DENSITY_HIP_CHAMELEON || n_chunks < 4 || variant(kVarPipeNever)) return false;
    return variant(kVarPipeAlways) || (n >= (32u << 20) && n >= 3 * pipe_slice_bytes(n, chunk));
}
inline uint32_t pipe_slice_chunks(size_t total, size_t chunk, size_t n_chunks) {
    const size_t target = pipe_slice_bytes(total, chunk);
    size_t per = (target + chunk - 1) / chunk;
    if (per < 1) per = 1;
    while ((n_chunks + per - 1) / per > kPipeMaxSlices) ++per;
    return (uint32_t)per;
}

// returns bytes decoded, 0 with the error set; *handled = false: not taken (the caller falls back to the staged path)
size_t decode_container_pipelined(DeviceCtx* c, const uint8_t* container, const density_hip_header_t& h, uint8_t* output, bool* handled) {
    *handled = false;
    const uint32_t nc = h.n_chunks;
    const size_t chunk = h.chunk_size, total = h.total_len;
    // (slices follow the PACKED layout: a paged blob's streams lie in pages — the staged call reads them in place; a sealed container is verified
    // against its trailer by the staged call, whole)
    if (!pipe_wanted(h.algo, total, chunk, nc) || (h.flags & (DENSITY_HIP_FLAG_SLOTTED | DENSITY_HIP_FLAG_PAGED | DENSITY_HIP_FLAG_CHECKSUM))) return 0;
    PinnedInPlace pin_in(container, h.container_len), pin_out(output, total);
    if (!pin_in || !pin_out) return 0;
    const bool with_index = h.flags & DENSITY_HIP_FLAG_BLOCK_INDEX;
    const size_t pbase = payload_base(nc, total, with_index);
    // where every chunk stream lies: the size table, read here on the host (the device's layout pass reads and checks it again)
    std::vector<uint64_t> offs(nc + 1);
    uint64_t off = pbase;
    for (uint32_t i = 0; i < nc; ++i) {
        uint32_t sz;
        std::memcpy(&sz, container + sizeof(density_hip_header_t) + 4 * (size_t)i, 4);
        offs[i] = off;
        if (sz > h.container_len || off > h.container_len - sz) { *handled = true; set_error("malformed or truncated container payload"); return 0; }
        off += sz;
        if (i + 1 < nc) off = align_up(off, 16);
    }
    offs[nc] = off;
    const uint32_t per = pipe_slice_chunks(total, chunk, nc), slices = (nc + per - 1) / per;
    if (!pipe_streams(c, 2 + 2 * slices)) return 0;
    const DecodePlan p = plan_decode(h.algo, nc, chunk);
    hipError_t e = ensure_staging(c, h.container_len, total, p.total);
    if (e != hipSuccess) { set_error("staging buffers", e); return 0; }
    *handled = true;
    uint8_t* d_in = (uint8_t*)c->stage_in.p;
    uint8_t* d_out = (uint8_t*)c->stage_out.p;
    uint8_t* ws = (uint8_t*)c->work.p;
    uint32_t* d_err = p.err(ws);
    uint64_t *d_sizes = p.sizes(ws), *d_offsets = p.offsets(ws), *d_produced = p.produced(ws);
    uint32_t* d_zmap = p.zmap(ws);
    const uint8_t* d_index = with_index ? d_in + index_base(nc) : nullptr;
    hipStream_t s = c->stream;
    hipEvent_t ev_head = c->pipe_events[0], ev_layout = c->pipe_events[1];
    e = hipMemsetAsync(d_err, 0, sizeof(uint32_t), s);
    if (e == hipSuccess) e = hipMemcpyAsync(d_in, container, pbase, hipMemcpyHostToDevice, c->up);          // header, size table, block index
    if (e == hipSuccess) e = hipEventRecord(ev_head, c->up);
    if (e == hipSuccess) e = hipStreamWaitEvent(s, ev_head, 0);
    if (e == hipSuccess) e = launch_layout_decode(d_in, h.container_len, nc, pbase, d_sizes, d_offsets, d_err, s, 0);
    if (e == hipSuccess) e = hipEventRecord(ev_layout, s);
    for (uint32_t k = 0; k < slices && e == hipSuccess; ++k) {
        const Slice sl = slice_of(k, per, nc, chunk, total);
        const uint32_t first = sl.first, count = sl.count;
        hipEvent_t ev_up = c->pipe_events[2 + 2 * k], ev_dec = c->pipe_events[3 + 2 * k];
        hipStream_t ks = c->kern[k & 3u];
        e = hipMemcpyAsync(d_in + offs[first], container + offs[first], offs[first + count] - offs[first], hipMemcpyHostToDevice, c->up);
        if (e == hipSuccess) e = hipEventRecord(ev_up, c->up);
        if (e == hipSuccess) e = hipStreamWaitEvent(ks, ev_layout, 0);
        if (e == hipSuccess) e = hipStreamWaitEvent(ks, ev_up, 0);
        if (e == hipSuccess) e = codec_decode(h.algo, d_in, d_offsets + first, d_sizes + first, count, d_out + sl.off, chunk, total - sl.off, true,
                                              d_index ? d_index + sl.off / 256 : nullptr, d_produced + first, d_err, nullptr,
                                              d_zmap ? d_zmap + (uint64_t)first * kZmapWordsPerChunk : nullptr, ks);
        if (e == hipSuccess) e = hipEventRecord(ev_dec, ks);
        if (e == hipSuccess) e = hipStreamWaitEvent(c->down, ev_dec, 0);
        if (e == hipSuccess) e = hipMemcpyAsync(output + sl.off, d_out + sl.off, sl.len, hipMemcpyDeviceToHost, c->down);
        if (e == hipSuccess) e = hipStreamWaitEvent(s, ev_dec, 0);
    }
    uint32_t h_err = 0;
    if (e == hipSuccess) e = read_back(s, d_err, &h_err);                                                     // (s waits for every slice's kernels)
    e = drain(e, {c->up, s, c->down, c->kern[0], c->kern[1], c->kern[2], c->kern[3]});
    if (e != hipSuccess) { set_error("decode (pipelined host path)", e); return 0; }
    if (h_err) { set_error("malformed or truncated container payload"); return 0; }
    return total;
}

size_t encode_container_pipelined(DeviceCtx* c, int algo, const uint8_t* input, size_t n, uint8_t* output, size_t cap, size_t chunk, bool* handled) {
    *handled = false;
    const EncodePlan p = plan_encode(algo, n, chunk);
    const size_t nc = p.n_chunks;
    if (!pipe_wanted(algo, n, chunk, nc) || nc > 0xffffffffull) return 0;
    const bool with_index = want_index(algo);
    const size_t pbase = payload_base(nc, n, with_index), bound = container_bound(algo, n, chunk);
    if (cap < pbase) return 0;                                                        // (the staged path reports it)
    PinnedInPlace pin_in(input, n), pin_out(output, std::min(cap, bound));            // (what the container can reach, not the caller's whole capacity)
    if (!pin_in || !pin_out) return 0;
    const uint32_t per = pipe_slice_chunks(n, chunk, nc), slices = (uint32_t)((nc + per - 1) / per);
    if (!pipe_streams(c, 3 * slices)) return 0;
    hipError_t e = ensure_staging(c, n, bound, p.total);
    if (e == hipSuccess) e = c->pin_sizes.ensure(8 * (size_t)slices);
    if (e != hipSuccess) { set_error("staging buffers", e); return 0; }
    *handled = true;
    uint8_t* d_in = (uint8_t*)c->stage_in.p;
    uint8_t* d_out = (uint8_t*)c->stage_out.p;                                       // the packed container, assembled on the device slice by slice
    uint8_t* ws = (uint8_t*)c->work.p;
    uint32_t* d_err = p.err(ws);
    uint64_t* h_ends = reinterpret_cast<uint64_t*>(c->pin_sizes.p);                  // the running end of the container behind every slice, as the device reports it
    const density_hip_header_t hdr = make_header(algo, chunk, nc, n, with_index ? DENSITY_HIP_FLAG_BLOCK_INDEX : 0);
    hipStream_t s = c->stream;
    e = hipMemsetAsync(d_err, 0, sizeof(uint32_t), s);
    if (e == hipSuccess) e = hipStreamSynchronize(s);                                 // (the kernel streams below do not wait for s)
    // Per slice: its input goes up, its chunks are encoded into their slots, the slice's place in the packed container follows from the running
    // end of its predecessor (write_buffer.rs:29-31's running total: the one sequential step, a scan over a few sizes), its streams are gathered
    // there, and the new running end comes back to the host, which then knows what to bring down.
    for (uint32_t k = 0; k < slices && e == hipSuccess; ++k) {
        const Slice sl = slice_of(k, per, nc, chunk, n);
        const bool is_last = k + 1 == slices;
        hipEvent_t ev_up = c->pipe_events[3 * k], ev_lay = c->pipe_events[3 * k + 1], ev_enc = c->pipe_events[3 * k + 2];
        hipStream_t ks = c->kern[k & 3u];
        e = hipMemcpyAsync(d_in + sl.off, input + sl.off, sl.len, hipMemcpyHostToDevice, c->up);
        if (e == hipSuccess) e = hipEventRecord(ev_up, c->up);
        if (e == hipSuccess) e = hipStreamWaitEvent(ks, ev_up, 0);
        hipEvent_t ev_pred = k ? c->pipe_events[3 * (k - 1) + 1] : nullptr;       // the predecessor's running end
        if (e == hipSuccess) e = encode_slice(p, ws, d_in, sl, k == 0, is_last, hdr, d_out, bound, ks, nullptr, ev_pred);
        if (e == hipSuccess) e = hipMemcpyAsync(h_ends + k, p.carry(ws), 8, hipMemcpyDeviceToHost, ks);
        if (e == hipSuccess) e = hipEventRecord(ev_lay, ks);
        if (e == hipSuccess) e = gather_slice(p, ws, sl, is_last, d_out, ks);
        if (e == hipSuccess) e = hipEventRecord(ev_enc, ks);
    }
    uint64_t begin = pbase, end = pbase;
    bool too_small = false;
    for (uint32_t k = 0; k < slices && e == hipSuccess && !too_small; ++k) {
        e = hipEventSynchronize(c->pipe_events[3 * k + 2]);
        if (e != hipSuccess) break;
        end = h_ends[k];
        if (end > cap || end > bound || end < begin) { too_small = true; break; }
        e = hipMemcpyAsync(output + begin, d_out + begin, end - begin, hipMemcpyDeviceToHost, c->down);
        begin = align_up(end, 16);
        if (k + 1 < slices) {
            if (begin > cap) { too_small = true; break; }
            std::memset(output + end, 0, begin - end);                                // the gap behind a slice's last stream (the gather zeroes those inside a slice)
        }
    }
    e = drain(e, {c->up, c->kern[0], c->kern[1], c->kern[2], c->kern[3]});
    if (e == hipSuccess && !too_small) e = hipMemcpyAsync(output, d_out, pbase, hipMemcpyDeviceToHost, c->down);   // header (written with the last slice), size table, block index
    e = drain(e, {c->down});
    uint32_t h_err = 0;
    if (e == hipSuccess) e = read_back(s, d_err, &h_err);
    if (e != hipSuccess) { set_error("encode (pipelined host path)", e); return 0; }
    if (h_err & 16u) { set_error("encode: device-side watchdog"); return 0; }
    if (h_err || too_small) { set_error("output buffer too small"); return 0; }
    return (size_t)end;
}

// the staged call: the input up whole, the packed container made on the device — and sealed there where asked — and down whole (ctx locked)
size_t encode_container_staged(DeviceCtx* c, int algo, const uint8_t* input, size_t input_size, uint8_t* output, size_t output_size, size_t chunk_size, bool seal) {
    const size_t packed = container_bound(algo, input_size, chunk_size), bound = packed + (seal ? seal_overhead(chunk_count(input_size, chunk_size)) : 0);
    const size_t ws_bytes = std::max(plan_encode(algo, input_size, chunk_size).total, seal ? plan_seal(input_size).total : 0);
    hipError_t e = ensure_staging(c, input_size ? input_size : 1, bound, ws_bytes);
    if (e == hipSuccess && input_size) e = copy_host_side_pinned(c->stage_in.p, input, input_size, hipMemcpyHostToDevice, c->stream);
    if (e != hipSuccess) { set_error("staging (H2D)", e); return 0; }
    density_hip_header_t h;
    if (run_encode_container(c, algo, (const uint8_t*)c->stage_in.p, input_size, (uint8_t*)c->stage_out.p, packed, chunk_size, (uint8_t*)c->work.p, c->stream, &h) != DENSITY_HIP_OK) return 0;
    if (seal && run_seal_container(c, (const uint8_t*)c->stage_in.p, input_size, (uint8_t*)c->stage_out.p, bound, &h, (uint8_t*)c->work.p, c->stream, &h) != DENSITY_HIP_OK) return 0;
    if (h.container_len > output_size) { set_error("output buffer too small"); return 0; }
    e = copy_host_side_pinned(output, c->stage_out.p, h.container_len, hipMemcpyDeviceToHost, c->stream);
    if (e != hipSuccess) { set_error("staging (D2H)", e); return 0; }
    return (size_t)h.container_len;
}

}  // namespace
}  // namespace api
}  // namespace density

using namespace density;
using namespace density::api;

namespace {
// The host-pointer verdict decode and, with `parity` (a blob of parity_size bytes), the recover decode: staged whole, like every sealed container.
size_t decode_verdicts_staged(const uint8_t* container, size_t container_size, const uint8_t* parity, size_t parity_size, uint8_t* output, size_t output_size,
                              uint32_t* verdicts, size_t verdict_capacity, unsigned flags, uint32_t* damaged_out, uint32_t* recovered_out) {
    g_last_error.clear();
    if (damaged_out) *damaged_out = 0;
    if (!container || container_size < sizeof(density_hip_header_t) || (!output && output_size) || (flags & ~DENSITY_HIP_SALVAGE_BLANK)) { set_error("bad argument"); return 0; }
    density_hip_header_t h;
    std::memcpy(&h, container, sizeof(h));
    if (check_header(h, container_size) != DENSITY_HIP_OK) { set_error("bad container header"); return 0; }
    if (!(h.flags & DENSITY_HIP_FLAG_CHECKSUM)) { set_error("verdicts: the container is not sealed (no trailer to hold its chunks against)"); return 0; }
    if (h.total_len > output_size) { set_error("output buffer too small"); return 0; }
    if (h.n_chunks > verdict_capacity || (!verdicts && h.n_chunks)) { set_error("verdict buffer too small"); return 0; }
    density_hip_parity_header_t ph{};
    if (parity) {
        if (parity_size < sizeof(ph)) { set_error("parity blob shorter than its header"); return 0; }
        std::memcpy(&ph, parity, sizeof(ph));
        if (check_parity_header(ph, h, parity_size) != DENSITY_HIP_OK) return 0;
    }
    if (h.total_len == 0) return 0;
    DeviceCtx* c = acquire_ctx();
    if (!c) return 0;
    std::lock_guard<std::mutex> lk(c->mu);
    // the verdict words lie behind the output in its staging buffer, the parity rows behind the container in its
    const size_t verdicts_at = align_up(h.total_len, kAlign), rows_at = align_up(h.container_len, kAlign), rows_bytes = parity ? parity_bytes(ph) - sizeof(ph) : 0;
    hipError_t e = ensure_staging(c, rows_at + rows_bytes, verdicts_at + 4 * (size_t)h.n_chunks, plan_decode(h.algo, h.n_chunks, h.chunk_size).total_with_passes);
    if (e == hipSuccess) e = copy_host_side_pinned(c->stage_in.p, container, h.container_len, hipMemcpyHostToDevice, c->stream);
    if (e == hipSuccess && parity) e = copy_host_side_pinned((uint8_t*)c->stage_in.p + rows_at, parity + sizeof(ph), rows_bytes, hipMemcpyHostToDevice, c->stream);
    if (e != hipSuccess) { set_error("staging (H2D)", e); return 0; }
    uint8_t* d_out = (uint8_t*)c->stage_out.p;
    uint32_t damaged = h.n_chunks;                                                                   // (written wherever the verdicts are valid)
    const Recovery rec{(const uint8_t*)c->stage_in.p + rows_at, ph.n_groups, ph.row_bytes, ph.version == 2, recovered_out};
    const int rc = run_decode_verdicts(c, (const uint8_t*)c->stage_in.p, h.container_len, h, d_out, h.total_len, (uint8_t*)c->work.p, c->stream, c->work.cap,
                                       reinterpret_cast<uint32_t*>(d_out + verdicts_at), flags, &damaged, parity ? &rec : nullptr);
    if (rc != DENSITY_HIP_OK && rc != DENSITY_HIP_ERR_CHECKSUM && rc != DENSITY_HIP_ERR_FORMAT) return 0;   // (those three come with verdicts: the driver reports no format error before it has them)
    const std::string said = g_last_error;
    e = copy_host_side_pinned(verdicts, d_out + verdicts_at, 4 * (size_t)h.n_chunks, hipMemcpyDeviceToHost, c->stream);
    if (e == hipSuccess && damaged < h.n_chunks) e = copy_host_side_pinned(output, d_out, h.total_len, hipMemcpyDeviceToHost, c->stream);
    if (e != hipSuccess) { set_error("staging (D2H)", e); return 0; }
    g_last_error = said;
    if (damaged_out) *damaged_out = damaged;
    return damaged < h.n_chunks ? (size_t)h.total_len : 0;
}

// density_hip_parity and density_hip_parity2: they differ in the blob's version
size_t parity_staged(uint8_t version, const uint8_t* input, size_t input_size, size_t chunk_size, uint32_t n_groups, uint8_t* parity, size_t parity_capacity) {
    g_last_error.clear();
    const size_t need = parity_size_of(version, input_size, chunk_size, n_groups);
    if (!need || (!input && input_size) || !parity) { set_error("bad argument"); return 0; }
    if (parity_capacity < need) { set_error("parity capacity below density_hip_parity_size() / density_hip_parity2_size()"); return 0; }
    DeviceCtx* c = acquire_ctx();
    if (!c) return 0;
    std::lock_guard<std::mutex> lk(c->mu);
    hipError_t e = ensure_staging(c, input_size, need, 0);
    if (e == hipSuccess) e = copy_host_side_pinned(c->stage_in.p, input, input_size, hipMemcpyHostToDevice, c->stream);
    if (e != hipSuccess) { set_error("staging (H2D)", e); return 0; }
    e = launch_parity_rows((const uint8_t*)c->stage_in.p, make_parity_header(input_size, chunk_size, n_groups, version), (uint8_t*)c->stage_out.p, c->stream);
    if (e != hipSuccess) { set_error("kernel launch (parity)", e); return 0; }
    e = copy_host_side_pinned(parity, c->stage_out.p, need, hipMemcpyDeviceToHost, c->stream);
    if (e != hipSuccess) { set_error("staging (D2H)", e); return 0; }
    return need;
}
}  // namespace

extern "C" {

size_t density_hip_encode(int algo, const uint8_t* input, size_t input_size, uint8_t* output, size_t output_size, size_t chunk_size) {
    g_last_error.clear();
    if (!take_geometry(algo, input_size, &chunk_size) || (!input && input_size) || !output) { set_error("bad argument"); return 0; }
    DeviceCtx* c = acquire_ctx();
    if (!c) return 0;
    std::lock_guard<std::mutex> lk(c->mu);
    {
        bool handled = false;
        const size_t r = encode_container_pipelined(c, algo, input, input_size, output, output_size, chunk_size, &handled);
        if (handled) return r;
    }
    return encode_container_staged(c, algo, input, input_size, output, output_size, chunk_size, false);
}

size_t density_hip_encode_sealed(int algo, const uint8_t* input, size_t input_size, uint8_t* output, size_t output_size, size_t chunk_size) {
    g_last_error.clear();
    if (!take_geometry(algo, input_size, &chunk_size) || (!input && input_size) || !output) { set_error("bad argument"); return 0; }
    DeviceCtx* c = acquire_ctx();
    if (!c) return 0;
    std::lock_guard<std::mutex> lk(c->mu);
    return encode_container_staged(c, algo, input, input_size, output, output_size, chunk_size, true);
}

size_t density_hip_decoded_size(const uint8_t* container, size_t container_size) {
    if (!container || container_size < sizeof(density_hip_header_t)) return 0;
    density_hip_header_t h;
    std::memcpy(&h, container, sizeof(h));
    return check_header(h, container_size) == DENSITY_HIP_OK ? (size_t)h.total_len : 0;
}

size_t density_hip_decode(const uint8_t* container, size_t container_size, uint8_t* output, size_t output_size) {
    g_last_error.clear();
    if (!container || container_size < sizeof(density_hip_header_t) || (!output && output_size)) { set_error("bad argument"); return 0; }
    density_hip_header_t h;
    std::memcpy(&h, container, sizeof(h));
    if (check_header(h, container_size) != DENSITY_HIP_OK) { set_error("bad container header"); return 0; }
    if (h.total_len > output_size) { set_error("output buffer too small"); return 0; }
    if (h.total_len == 0) return 0;
    DeviceCtx* c = acquire_ctx();
    if (!c) return 0;
    std::lock_guard<std::mutex> lk(c->mu);
    {
        bool handled = false;
        const size_t r = decode_container_pipelined(c, container, h, output, &handled);
        if (handled) return r;
    }
    hipError_t e = ensure_staging(c, h.container_len, h.total_len, plan_decode(h.algo, h.n_chunks, h.chunk_size).total_with_passes);
    if (e == hipSuccess) e = copy_host_side_pinned(c->stage_in.p, container, h.container_len, hipMemcpyHostToDevice, c->stream);
    if (e != hipSuccess) { set_error("staging (H2D)", e); return 0; }
    size_t produced = 0;
    if (run_decode_container(c, (const uint8_t*)c->stage_in.p, h.container_len, h, (uint8_t*)c->stage_out.p, h.total_len, (uint8_t*)c->work.p, c->stream, &produced, c->work.cap) != DENSITY_HIP_OK) return 0;
    e = copy_host_side_pinned(output, c->stage_out.p, produced, hipMemcpyDeviceToHost, c->stream);
    if (e != hipSuccess) { set_error("staging (D2H)", e); return 0; }
    return produced;
}

size_t density_hip_decode_verdicts(const uint8_t* container, size_t container_size, uint8_t* output, size_t output_size, uint32_t* verdicts, size_t verdict_capacity,
                                   unsigned flags, uint32_t* damaged_out) {
    return decode_verdicts_staged(container, container_size, nullptr, 0, output, output_size, verdicts, verdict_capacity, flags, damaged_out, nullptr);
}

size_t density_hip_decode_recover(const uint8_t* container, size_t container_size, const uint8_t* parity, size_t parity_size, uint8_t* output, size_t output_size,
                                  uint32_t* verdicts, size_t verdict_capacity, unsigned flags, uint32_t* damaged_out, uint32_t* recovered_out) {
    g_last_error.clear();
    if (recovered_out) *recovered_out = 0;
    if (!parity) { if (damaged_out) *damaged_out = 0; set_error("bad argument"); return 0; }
    return decode_verdicts_staged(container, container_size, parity, parity_size, output, output_size, verdicts, verdict_capacity, flags, damaged_out, recovered_out);
}

size_t density_hip_slice(const uint8_t* container, size_t container_size, uint32_t first_chunk, uint32_t chunk_count, uint8_t* output, size_t output_size) {
    g_last_error.clear();
    if (!container || container_size < sizeof(density_hip_header_t) || !output || chunk_count == 0) { set_error("bad argument"); return 0; }
    density_hip_header_t h;
    std::memcpy(&h, container, sizeof(h));
    if (!header_is_containers(h)) { set_error("slice: not a container's header"); return 0; }
    if ((uint64_t)first_chunk + chunk_count > h.n_chunks) { set_error("slice: the window is not inside the container's chunks"); return 0; }
    const size_t bound = slice_bound(h, first_chunk, chunk_count);
    if (output_size < bound) { set_error("output capacity below density_hip_slice_bound()"); return 0; }
    if (check_header(h, container_size) != DENSITY_HIP_OK) { set_error("bad container header (its length, or its trailer's, against container_size)"); return 0; }
    DeviceCtx* c = acquire_ctx();
    if (!c) return 0;
    std::lock_guard<std::mutex> lk(c->mu);
    // staged whole, like every sealed container: the container up, the window's packed container down
    hipError_t e = ensure_staging(c, h.container_len, bound, plan_decode(h.algo, h.n_chunks).total);
    if (e == hipSuccess) e = copy_host_side_pinned(c->stage_in.p, container, h.container_len, hipMemcpyHostToDevice, c->stream);
    if (e != hipSuccess) { set_error("staging (H2D)", e); return 0; }
    density_hip_header_t out_h;
    if (run_slice_container(c, (const uint8_t*)c->stage_in.p, h, first_chunk, chunk_count, (uint8_t*)c->stage_out.p, bound, (uint8_t*)c->work.p, c->stream, &out_h) != DENSITY_HIP_OK) return 0;
    e = copy_host_side_pinned(output, c->stage_out.p, out_h.container_len, hipMemcpyDeviceToHost, c->stream);
    if (e != hipSuccess) { set_error("staging (D2H)", e); return 0; }
    return (size_t)out_h.container_len;
}

size_t density_hip_join(const density_hip_join_part_t* parts, uint32_t n_parts, uint8_t* output, size_t output_size) {
    g_last_error.clear();
    JoinGeometry g;
    if (const char* why = join_geometry(parts, n_parts, &g)) { set_error(why); return 0; }
    if (!output) { set_error("bad argument"); return 0; }
    const size_t bound = join_bound(g);
    if (output_size < bound) { set_error("output capacity below density_hip_join_bound()"); return 0; }
    if (check_join_parts(parts, n_parts) != DENSITY_HIP_OK) return 0;
    DeviceCtx* c = acquire_ctx();
    if (!c) return 0;
    std::lock_guard<std::mutex> lk(c->mu);
    // staged whole, like every sealed container: the parts' containers up, one behind the other, the joined container down
    density_hip_join_part_t staged[DENSITY_HIP_JOIN_MAX_PARTS];
    size_t in_bytes = 0;
    for (uint32_t p = 0; p < n_parts; ++p) {
        staged[p] = parts[p];
        if (parts[p].chunk_count == 0) continue;
        staged[p].container = (const void*)in_bytes;                                     // (the offset for now: the buffer may still move)
        in_bytes += align_up(parts[p].header->container_len, kAlign);
    }
    hipError_t e = ensure_staging(c, in_bytes, bound, plan_join(g.n_chunks).total);
    for (uint32_t p = 0; p < n_parts && e == hipSuccess; ++p) {
        if (parts[p].chunk_count == 0) continue;
        staged[p].container = (const uint8_t*)c->stage_in.p + (size_t)staged[p].container;
        e = copy_host_side_pinned(const_cast<void*>(staged[p].container), parts[p].container, parts[p].header->container_len, hipMemcpyHostToDevice, c->stream);
    }
    if (e != hipSuccess) { set_error("staging (H2D)", e); return 0; }
    density_hip_header_t out_h;
    if (run_join_container(c, staged, n_parts, g, (uint8_t*)c->stage_out.p, bound, (uint8_t*)c->work.p, c->stream, &out_h) != DENSITY_HIP_OK) return 0;
    e = copy_host_side_pinned(output, c->stage_out.p, out_h.container_len, hipMemcpyDeviceToHost, c->stream);
    if (e != hipSuccess) { set_error("staging (D2H)", e); return 0; }
    return (size_t)out_h.container_len;
}

size_t density_hip_parity(const uint8_t* input, size_t input_size, size_t chunk_size, uint32_t n_groups, uint8_t* parity, size_t parity_capacity) {
    return parity_staged(1, input, input_size, chunk_size, n_groups, parity, parity_capacity);
}
size_t density_hip_parity2(const uint8_t* input, size_t input_size, size_t chunk_size, uint32_t n_groups, uint8_t* parity, size_t parity_capacity) {
    return parity_staged(2, input, input_size, chunk_size, n_groups, parity, parity_capacity);
}

// staged whole: the old bytes and the new ones side by side in the input's staging buffer, the blob in the output's, updated there and brought back
size_t density_hip_parity_update(uint8_t* parity, size_t parity_size, uint64_t offset, const uint8_t* old_data, size_t old_size, const uint8_t* new_data, size_t new_size) {
    g_last_error.clear();
    if (!parity || (!old_data && old_size) || (!new_data && new_size)) { set_error("bad argument"); return 0; }
    density_hip_parity_header_t ph, after;
    if (parity_size < sizeof(ph)) { set_error("parity blob shorter than its header"); return 0; }
    std::memcpy(&ph, parity, sizeof(ph));
    if (check_parity_update(ph, parity_size, offset, old_size, new_size, &after) != DENSITY_HIP_OK) return 0;
    const size_t bytes = parity_bytes(ph), new_at = align_up(old_size, kAlign);
    if (!old_size && !new_size) return bytes;
    DeviceCtx* c = acquire_ctx();
    if (!c) return 0;
    std::lock_guard<std::mutex> lk(c->mu);
    hipError_t e = ensure_staging(c, new_at + new_size, bytes, 0);
    if (e == hipSuccess) e = copy_host_side_pinned(c->stage_in.p, old_data, old_size, hipMemcpyHostToDevice, c->stream);
    if (e == hipSuccess) e = copy_host_side_pinned((uint8_t*)c->stage_in.p + new_at, new_data, new_size, hipMemcpyHostToDevice, c->stream);
    if (e == hipSuccess) e = copy_host_side_pinned(c->stage_out.p, parity, bytes, hipMemcpyHostToDevice, c->stream);
    if (e != hipSuccess) { set_error("staging (H2D)", e); return 0; }
    e = launch_parity_update((uint8_t*)c->stage_out.p, after, offset, (const uint8_t*)c->stage_in.p, old_size, (const uint8_t*)c->stage_in.p + new_at, new_size, c->stream);
    if (e != hipSuccess) { set_error("kernel launch (parity update)", e); return 0; }
    e = copy_host_side_pinned(parity, c->stage_out.p, bytes, hipMemcpyDeviceToHost, c->stream);
    if (e != hipSuccess) { set_error("staging (D2H)", e); return 0; }
    return bytes;
}

}  // extern "C"
