// kernels.hpp — host-side launchers of the gfx950 kernels (definitions in the .hip files of this directory).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdlib.h>

#include "../../include/density_hip.h"

namespace density {

// Tuning and diagnostic switches come from the environment only in a DENSITY_HIP_DEBUG build (python -m density_amd.build --debug ->
// libdensity_hip_debug.so; tools/build_variant.sh): the shipped library has no environment interface.
inline const char* debug_env(const char* name) {
#ifdef DENSITY_HIP_DEBUG
    return getenv(name);
#else
    (void)name;
    return nullptr;
#endif
}

// ---- chameleon.hip ----
extern bool g_force_simple;   // density_hip_set_kernel_variant(1)
// One wavefront per chunk.  Chunk c reads in[c*chunk_bytes ...) and writes its reference stream at
// out + c*out_stride; sizes[c] receives the stream length.
// d_index (nullable): one byte per 256-byte input block, numbered over the whole input (see include/density_hip.h).
hipError_t launch_chameleon_encode(const uint8_t* d_in, uint64_t total, uint64_t chunk_bytes, uint32_t n_chunks,
                                   uint8_t* d_out, uint64_t out_stride, uint64_t* d_sizes, uint8_t* d_index, uint32_t* d_zmap, uint32_t* d_err, hipStream_t stream);
// d_zmap (nullable -> one-wavefront kernels): kZmapWordsPerChunk words per chunk of scratch for the pipelined kernels' zero-entry maps.
// Chunk c reads the stream at in + offsets[c] (sizes[c] bytes) and writes out + c*out_stride.  With `exact`, a chunk
// that does not produce exactly min(out_stride, out_total - c*out_stride) bytes raises *d_err.
hipError_t launch_chameleon_decode(const uint8_t* d_in, const uint64_t* d_offsets, const uint64_t* d_sizes,
                                   uint32_t n_chunks, uint8_t* d_out, uint64_t out_stride, uint64_t out_total,
                                   bool exact, const uint8_t* d_index, uint32_t* d_zmap, uint64_t* d_produced, uint32_t* d_err, hipStream_t stream);
// the pipelined decoder keeps its zero-entry map in global memory: kZmapWordsPerChunk u32 per chunk, for at most
// kMaxPipelinedChunks chunks (more chunks than that, i.e. tiny chunks, run on the one-wavefront kernel)
constexpr uint32_t kZmapWordsPerChunk = 2048, kMaxPipelinedChunks = 16384;

// ---- rotor.hip, rotor_encode.hip, rotor_decode.hip (Chameleon wave-rotation kernels: the default encode / index-fed decode path) ----
// pages of a paged container: 64 KiB — a round of 16 blocks is at most 4224 bytes, so a page's unused tail is below 7 % and 2 % on average
constexpr uint32_t kPageShift = 16, kPageBytes = 1u << kPageShift;
// pages one chunk can need (a page is left when the next round's records do not fit: at most a round's worth unused per page), and the words of
// its directory
__host__ __device__ inline uint32_t pages_per_chunk(uint64_t worst_stream_bytes) { return (uint32_t)(worst_stream_bytes / (kPageBytes - 4352u)) + 2u; }
__host__ __device__ inline uint32_t page_dir_words(uint32_t pages) { return 4u * (pages + 1u); }
// what the paged DECODER takes (rotor_dev.hpp: kRotMaxBlocks blocks of index, kDecMaxPages directory entries in LDS): the encoder offers no more
constexpr uint64_t kPagedMaxChunk = 4ull << 20;
constexpr uint32_t kPagedMaxPages = 96;
bool rotor_encode_eligible(const uint8_t* d_in, uint64_t total, uint64_t chunk_bytes, uint32_t n_chunks);
// the rotation encoder writing a PAGED container's pages (d_pages: page 0) and directory; d_page_counter zeroed by the caller
hipError_t launch_rotor_encode_paged(const uint8_t* d_in, uint64_t total, uint64_t chunk_bytes, uint32_t n_chunks, uint8_t* d_pages, uint32_t page_limit,
                                     uint32_t* d_page_counter, uint32_t* d_dir, uint32_t dir_words, uint64_t* d_sizes, uint8_t* d_index, uint32_t* d_err, hipStream_t stream);
hipError_t launch_rotor_encode(const uint8_t* d_in, uint64_t total, uint64_t chunk_bytes, uint32_t n_chunks, uint8_t* d_out, uint64_t out_stride,
                               uint64_t* d_sizes, uint8_t* d_index, uint32_t* d_err, hipStream_t stream);
// Whole-stream-exact encoding in segments (api.hip::run_stream_encode_segmented): a chunk may start from a given dictionary image
// (table + zero-entry map, kSegImageBytes) and FSM state instead of a fresh one, and reports where it ended.
constexpr uint64_t kSegImageBytes = 128ull * 1024 + 8ull * 1024;
struct SegArgs {
    const uint8_t* init_images = nullptr;   // per chunk kSegImageBytes, or nullptr: fresh tables
    const uint32_t* init_guard = nullptr;   // per chunk: packed FSM state (rotor_dev.hpp::pack_guard); bit 31: start in speculation (fast) mode
    uint8_t* final_images = nullptr;        // per chunk: the dictionary image after the chunk
    uint32_t* final_guard = nullptr;        // per chunk: the FSM state after the chunk's last whole block
    uint32_t* raw_blocks = nullptr;         // per chunk: number of raw-copy blocks (pre-zeroed by the caller)
    // paged container (round 5, include/density_hip.h DENSITY_HIP_FLAG_PAGED): the streams live in pages of kPageBytes taken from one counter
    uint32_t* page_counter = nullptr;       // encoder: the next free page of the output
    uint32_t* page_dir = nullptr;           // per chunk page_dir_words words: {n_pages, 0, 0, 0}, then per page {page, first block, bytes used, 0}
    uint32_t page_dir_words = 0;
    uint32_t page_limit = 0;                // pages the output has room for (encoder) / the container holds (decoder)
    uint32_t lastwriters_only = 0;          // decoder: a pass that is run for its final dictionary alone — MAP quads are not looked up (their
                                            // slots are mostly empty in a dictionary that starts empty, and every empty read is a zero-entry question)
};
hipError_t launch_rotor_encode_seg(const uint8_t* d_in, uint64_t total, uint64_t chunk_bytes, uint32_t n_chunks, uint8_t* d_out, uint64_t out_stride,
                                   uint64_t* d_sizes, uint32_t* d_err, SegArgs seg, hipStream_t stream);
// per chunk (whole rounds only): the dictionary image a fresh table has after every block of the chunk was coded ("last writers")
hipError_t launch_rotor_lastwriters(const uint8_t* d_in, uint64_t chunk_bytes, uint32_t n_chunks, uint8_t* d_images, uint32_t* d_err, hipStream_t stream);
// start images of chunks first+1 .. first+count: base image, then the last-writer images of chunks first+1 .. laid over it one after the other
hipError_t launch_merge_images(const uint8_t* d_base, const uint8_t* d_lastwriters, uint8_t* d_start, uint32_t count, hipStream_t stream);
// offsets[first + i] = *d_carry + sizes[first] + .. + sizes[first + i - 1]; *d_carry moves to the end of the last one
hipError_t launch_scan_offsets(const uint64_t* d_sizes, uint32_t first, uint32_t count, uint64_t* d_carry, uint64_t* d_offsets, hipStream_t stream);
// byte-granular gather of chunk streams (d_src + i * src_stride, sizes[i]) to d_dst + offsets[i]
hipError_t launch_compact_bytes(const uint8_t* d_src, uint64_t src_stride, const uint64_t* d_sizes, const uint64_t* d_offsets, uint32_t n_chunks,
                                uint8_t* d_dst, hipStream_t stream);
// the index-fed decoder on segments of one stream: start dictionaries in, final dictionaries out (SegArgs: init_images / final_images)
hipError_t launch_rotor_decode_seg(const uint8_t* d_in, const uint64_t* d_offsets, const uint64_t* d_sizes, uint32_t n_chunks, uint8_t* d_out,
                                   uint64_t out_stride, uint64_t out_total, const uint8_t* d_index, uint32_t* d_zmap, uint64_t* d_produced, uint32_t* d_err,
                                   SegArgs seg, hipStream_t stream);
bool rotor_decode_eligible(const uint8_t* d_out, uint32_t n_chunks, uint64_t out_stride, uint64_t out_total, const uint8_t* d_index, const uint32_t* d_zmap);
hipError_t launch_rotor_decode(const uint8_t* d_in, const uint64_t* d_offsets, const uint64_t* d_sizes, uint32_t n_chunks, uint8_t* d_out,
                               uint64_t out_stride, uint64_t out_total, bool exact, const uint8_t* d_index, uint32_t* d_zmap,
                               uint64_t* d_produced, uint32_t* d_err, hipStream_t stream);
// LDS assumptions of the rotation kernels (ordered exchange lane order, token hand-off behind the exchanges, lane-reversed rollback)
hipError_t launch_rotor_selftest(uint32_t* d_fail, hipStream_t stream);
constexpr bool kRotorSplitDefault = false;   // which rotation encoder ships: the split one (8 chain + 8 emit waves, rotor_encode.hip) or the 8-wave one
extern bool g_rotor_split;     // density_hip_set_kernel_variant(2048): the OTHER rotation encoder than kRotorSplitDefault (A/B runs, cross-checks)
extern bool g_force_pipeline;  // density_hip_set_kernel_variant(4): the 16-wave role pipelines of chameleon.hip instead
extern bool g_exchange_unsafe, g_rotor_unsafe;   // start-up self-test verdicts (api.hip::acquire_ctx)

// ---- serial_codec.hip (Cheetah: one wave per chunk stream; Lion, and Cheetah as a cross-check: one lane per stream; tables in global memory) ----
extern bool g_force_lane_codec;   // density_hip_set_kernel_variant(16)
extern bool g_lion_one_wave;      // density_hip_set_kernel_variant(32768): Lion's decode on one wave per stream instead of two
uint64_t serial_table_bytes(int algo);
hipError_t launch_serial_encode(int algo, const uint8_t* d_in, uint64_t total, uint64_t chunk_bytes, uint32_t n_chunks, uint8_t* d_out,
                                uint64_t out_stride, uint64_t* d_sizes, uint8_t* d_tables, uint32_t n_slots, hipStream_t stream);
hipError_t launch_serial_decode(int algo, const uint8_t* d_in, const uint64_t* d_offsets, const uint64_t* d_sizes, uint32_t n_chunks,
                                uint8_t* d_out, uint64_t out_stride, uint64_t out_total, bool exact, uint64_t* d_produced, uint32_t* d_err,
                                uint8_t* d_tables, uint32_t n_slots, hipStream_t stream);

// The one-wave kernels (Cheetah, Lion) in the service of exchange_stages.hip: the chunks d_only marks, whole (the wave clears its tables itself);
// just the head of every chunk (head_bytes and more, until the blow-up protection is quiet; short or restless chunks are finished), tables (one slot per chunk: n_chunks x serial_table_bytes) and d_head_state (8 words per chunk) left
// behind; just the ragged end of the chunks d_tail_state marks (8 words per chunk), from the tables the passes wrote back
hipError_t launch_wave_encode_only(int algo, const uint8_t* d_in, uint64_t total, uint64_t chunk_bytes, uint32_t n_chunks, uint8_t* d_out, uint64_t out_stride,
                                   uint64_t* d_sizes, uint8_t* d_tables, uint32_t n_slots, const uint32_t* d_only, hipStream_t stream);
hipError_t launch_wave_encode_heads(int algo, const uint8_t* d_in, uint64_t total, uint64_t chunk_bytes, uint32_t n_chunks, uint8_t* d_out, uint64_t out_stride,
                                    uint64_t* d_sizes, uint8_t* d_tables, uint32_t* d_head_state, uint32_t head_bytes, uint32_t head_calm, hipStream_t stream);
hipError_t launch_wave_encode_tails(int algo, const uint8_t* d_in, uint64_t total, uint64_t chunk_bytes, uint32_t n_chunks, uint8_t* d_out, uint64_t out_stride,
                                    uint64_t* d_sizes, uint8_t* d_tables, const uint32_t* d_tail_state, hipStream_t stream);

// ---- exchange_stages.hip (Cheetah / Lion container encode, the default: three / seven passes of ordered LDS exchanges per chunk, then a size scan
// and the records) ----
extern bool g_force_wave_codec;   // density_hip_set_kernel_variant(32): the one-wave-per-stream encoders instead
extern bool g_stage_audit;        // density_hip_set_kernel_variant(64): count chunks kept / handed back (synchronises)
extern uint64_t g_stage_stats[2];
bool stage_encode_eligible(int algo, const uint8_t* d_in, uint64_t total, uint64_t chunk_bytes, uint32_t n_chunks);
uint64_t stage_scratch_bytes(int algo, uint64_t total, uint32_t n_chunks);
hipError_t launch_stage_encode(int algo, const uint8_t* d_in, uint64_t total, uint64_t chunk_bytes, uint32_t n_chunks, uint8_t* d_out, uint64_t out_stride,
                               uint64_t* d_sizes, uint8_t* d_tables, uint32_t n_slots, uint8_t* d_scratch, uint32_t* d_err, hipStream_t stream);

// ---- decode_passes.hip (Cheetah container decode, the default: records parsed per chunk, dictionary and prediction tables as ordered LDS
// exchange passes over the whole chunk, the chain of contexts alone on a team of four waves per chunk: decode_walk.hip) ----
extern bool g_force_serial_decode;   // density_hip_set_kernel_variant(128): the one-wave-per-stream decoder instead
extern bool g_serial_parse;          // density_hip_set_kernel_variant(1024): Cheetah's decode passes find the records by the one-wave walk alone
bool decode_pass_eligible(int algo, const uint8_t* d_in, const uint8_t* d_out, uint32_t n_chunks, uint64_t out_stride, uint64_t out_total);
uint64_t decode_pass_scratch_bytes(uint64_t out_stride, uint32_t n_chunks);
hipError_t launch_decode_passes(int algo, const uint8_t* d_in, const uint64_t* d_offsets, const uint64_t* d_sizes, uint32_t n_chunks, uint8_t* d_out,
                                uint64_t out_stride, uint64_t out_total, bool exact, uint64_t* d_produced, uint32_t* d_err, uint8_t* d_scratch,
                                hipStream_t stream);

// ---- stream_parse.hip: record boundaries of one calm Chameleon stream, in parallel ----
// d_info (16 words): 0 status (1 = a calm head was found), 1 first block behind the sequentially walked head, 2-3 its stream offset, 4 whole
// blocks of the stream, 5-6 stream offset where they end (the ragged end, if any, starts there), 7 first block of a pair of incompressible
// records behind the head (0xffffffff: none); in: 8 block / 9-10 stream offset the head walk starts at (0 / 0 for a whole stream; after a
// pair at block j: j / d_pos32[j], everything before being final).  d_index: one byte per whole block (MAP count; raw copies flagged),
// d_pos32[b]: stream offset of block b, d_chunk_offset[k]: stream offset of block k * chunk_blocks.
uint64_t stream_parse_workspace(uint64_t E);
hipError_t launch_stream_parse(const uint8_t* d_in, uint64_t E, uint64_t from_pos, uint8_t* d_ws, uint8_t* d_index, uint64_t index_cap, uint64_t* d_chunk_offset,
                               uint32_t chunk_blocks, uint32_t* d_pos32, uint32_t* d_info, hipStream_t stream);
// offsets / sizes of segments [first, first + count) of a parsed stream from the parse's d_chunk_offset (`end` != ~0: where the range's last segment ends)
hipError_t launch_seg_layout(const uint64_t* d_chunk_offset, uint32_t first, uint32_t count, uint64_t end, uint64_t* d_offsets, uint64_t* d_sizes, uint32_t* d_err, hipStream_t stream);

// ---- container.hip ----
// Exclusive scan of 16-byte-aligned chunk sizes -> payload offsets; writes the container header and the u32 size
// table (encode side).
// slot_stride != 0: a slotted container (DENSITY_HIP_FLAG_SLOTTED): payload i stays in its slot at payload_base + i * slot_stride
hipError_t launch_layout_encode(const uint64_t* d_sizes, uint32_t n_chunks, density_hip_header_t hdr, uint64_t payload_base, uint8_t* d_container,
                                uint64_t capacity, uint64_t* d_offsets, uint32_t* d_err, hipStream_t stream, uint64_t slot_stride = 0);
// the rotation decoder on a PAGED container: d_pages = page 0 (d_offsets: all zero), d_sizes the streams' lengths, the directory beside them
hipError_t launch_rotor_decode_paged(const uint8_t* d_pages, const uint64_t* d_offsets, const uint64_t* d_sizes, uint32_t n_chunks, uint8_t* d_out, uint64_t out_stride,
                                     uint64_t out_total, const uint8_t* d_index, const uint32_t* d_dir, uint32_t dir_words, uint32_t n_pages, uint32_t* d_zmap,
                                     uint64_t* d_produced, uint32_t* d_err, hipStream_t stream);
hipError_t launch_layout_encode_paged(const uint64_t* d_sizes, uint32_t n_chunks, density_hip_header_t hdr, uint64_t dir_base, uint64_t dir_end, uint64_t pages_base, uint8_t* d_container,
                                      uint64_t capacity, const uint32_t* d_page_counter, uint32_t* d_err, hipStream_t stream);
hipError_t launch_layout_decode_paged(const uint8_t* d_container, uint32_t n_chunks, uint64_t* d_sizes, uint64_t* d_offsets, hipStream_t stream);
// The same for a slice of the chunks (batched encode): offsets continue from *d_carry, which is left at the slice's end.
hipError_t launch_layout_encode_batch(const uint64_t* d_sizes, uint32_t first, uint32_t count, bool is_first, bool is_last, density_hip_header_t hdr,
                                      uint64_t payload_base, uint8_t* d_container, uint64_t capacity, uint64_t* d_offsets, uint64_t* d_carry, uint32_t* d_err,
                                      hipStream_t stream);
// Decode side: reads the u32 size table of a container, produces u64 sizes + offsets, validates against container_size.
hipError_t launch_layout_decode(const uint8_t* d_container, uint64_t container_size, uint32_t n_chunks, uint64_t payload_base,
                                uint64_t* d_sizes, uint64_t* d_offsets, uint32_t* d_err, hipStream_t stream, uint64_t slot_stride = 0);
// Gathers chunk streams from their worst-case slots into the packed container (the packed encode; density_hip_pack_device of a slotted container).
hipError_t launch_compact(const uint8_t* d_slots, uint64_t slot_stride, const uint64_t* d_sizes, const uint64_t* d_offsets,
                          uint32_t n_chunks, uint8_t* d_container, const uint32_t* d_err, hipStream_t stream, bool more_follow = false);
// (`more_follow`: the launch gathers one batch of a container and further streams follow its last one — the alignment gap behind that stream
// is then zero-filled like the gaps between the launch's own streams, so that a batched gather writes the same bytes as a single one)
// PAGED container -> packed container (density_hip_unpage_device; a paged part of a slice or join).  The check: a wave per chunk holds the chunk's directory against the size table and the
// container (n_pages: the pages it holds); d_sizes[c] = the stream's length, or 0 with bit 4 of *d_err where the gather may not follow the directory.
hipError_t launch_check_directory(const uint8_t* d_container, uint32_t n_chunks, uint64_t chunk_bytes, uint64_t total_len, uint64_t dir_base,
                                  uint32_t pages_per_chunk, uint32_t n_pages, uint64_t* d_sizes, uint32_t* d_err, hipStream_t stream);
// The gather: every page's used bytes to d_out + d_offsets[chunk] + the bytes of the chunk's pages in front of it (any alignment of either buffer), the zero
// gaps between the streams included; nothing where *d_err is set.
hipError_t launch_unpage(const uint8_t* d_container, uint32_t n_chunks, uint64_t dir_base, uint64_t pages_base, uint32_t pages_per_chunk,
                         const uint64_t* d_sizes, const uint64_t* d_offsets, uint8_t* d_out, const uint32_t* d_err, hipStream_t stream);
// Chunk windows [first, first + count) of one or several containers -> one packed container (density_hip_join_device; one part: density_hip_slice_device, and
// as the window [0, n_chunks) density_hip_pack_device and density_hip_unpage_device — api.hip has one driver for the four).
// The part table travels as a kernel argument (3 KiB of the 4 KiB there are: it is read when the launch is made, so the caller's table may go at once): per
// part where the container lies, where its streams end (`limit`), its total_len and payload base (paged: unused), how its streams lie (slot_stride: 0
// packed — the size table is scanned from chunk 0 for the window's place —, kJoinPaged paged, else slotted), the window.
constexpr uint32_t kJoinMaxParts = 64;                        // (DENSITY_HIP_JOIN_MAX_PARTS)
constexpr uint64_t kJoinPaged = ~0ull;
struct JoinSource { const uint8_t* in; uint64_t limit, total_len, src_base, slot_stride; uint32_t first, count; };
struct JoinSources { JoinSource p[kJoinMaxParts]; };
// The layout, one work-group, walks the parts in order (for a paged part d_lens[K_p + k] holds what launch_check_directory left for its window chunk k, K_p =
// the chunks of the parts in front) and carries the running output chunk number and destination offset across them.  Into d_out: `hdr` (n_chunks = the sum
// of the windows) with its container_len, every window's size-table entries, the zero gaps in front of the payloads and behind every stream but the output's
// last — the gaps between the parts too.  For the gather, one word per output chunk each: d_lens, d_src (the stream's ADDRESS: the parts lie in different
// allocations; 0 for a paged part's chunks, which launch_unpage moves) and d_dst_off (offset in d_out).  d_run (nullable): the bytes from the first stream's
// start to the last one's end where there is ONE part, else 0 — with one packed part, the window as the single run {d_src[0], *d_run, d_dst_off[0]}, gaps as they stand.
// Bit 4 of *d_err: a window entry above its chunk's worst case or slot, a window stream behind its part's `limit` (entries in front of a window are not
// judged); then no gap is written and *d_run = 0.
hipError_t launch_window_layout(const JoinSources& parts, uint32_t n_parts, uint32_t algo, uint64_t chunk_bytes, uint8_t* d_out, uint64_t capacity,
                                density_hip_header_t hdr, uint64_t out_base, uint64_t* d_lens, uint64_t* d_src, uint64_t* d_dst_off, uint64_t* d_run, uint32_t* d_err,
                                hipStream_t stream);
// `runs` byte runs, d_lens[r] bytes (at most longest_run) from address d_src[r] (0: not this kernel's run) to d_out + d_dst_off[r], any alignment of either;
// nothing where *d_err is set
hipError_t launch_run_gather(const uint64_t* d_src, const uint64_t* d_lens, const uint64_t* d_dst_off, uint32_t runs, uint64_t longest_run, uint8_t* d_out,
                             const uint32_t* d_err, hipStream_t stream);
// LDS same-address ordering self-test (ascending lane order within one ds instruction). *d_fail != 0 on violation.
hipError_t launch_selftest(uint32_t* d_fail, hipStream_t stream);

// ---- checksum.hip (sealed containers, DENSITY_HIP_FLAG_CHECKSUM: the content checksum C of checksum.hpp, one word per chunk) ----
constexpr uint32_t kErrChecksum = 0x100u;   // the bit of a decode's error word that says "decoded, but not what was sealed" (the codec kernels use bits 0..4)
// C of every `chunk` bytes of d_data (any alignment) into d_sums[n_chunks] (4-byte aligned; cleared here, not by the caller).  With d_expect
// (n_chunks words at any alignment: a trailer) d_sums is scratch and a difference raises kErrChecksum in *d_err instead.
hipError_t launch_checksum(const uint8_t* d_data, uint64_t size, uint32_t chunk, uint32_t n_chunks, uint32_t* d_sums, const uint8_t* d_expect, uint32_t* d_err,
                           hipStream_t stream);
// Verdicts: d_acc as launch_checksum with d_expect has just left it (the sums S, nothing else) against the trailer d_expect once more, one word per chunk:
// d_verdicts[c] = DENSITY_HIP_CHUNK_DAMAGED or 0 (4-byte aligned), *d_count (cleared here) the number of damaged chunks, kErrChecksum into *d_err.
hipError_t launch_chunk_verdicts(const uint32_t* d_acc, uint64_t size, uint32_t chunk, uint32_t n_chunks, const uint8_t* d_expect, uint32_t* d_verdicts,
                                 uint32_t* d_count, uint32_t* d_err, hipStream_t stream);
// zeros over chunk c's bytes of d_out (any alignment; the last chunk at its true length) for every c with d_verdicts[c] == DENSITY_HIP_CHUNK_DAMAGED
hipError_t launch_blank_chunks(uint8_t* d_out, uint64_t size, uint32_t chunk, uint32_t n_chunks, const uint32_t* d_verdicts, hipStream_t stream);
// Seals the container an encoder has just written for d_in, in place, from its header ON THE DEVICE: trailer, flag, new container_len.  d_geom: 4
// words, d_acc: a word per chunk (at most one per 256 bytes of input) of scratch.  *d_err bit 1: not this input's unsealed container; bit 2: the capacity
// does not hold the trailer — the container is then left as it was.
hipError_t launch_seal(const uint8_t* d_in, uint64_t input_size, uint8_t* d_container, uint64_t capacity, uint32_t* d_geom, uint32_t* d_acc, uint32_t* d_err,
                       hipStream_t stream);
// A trailer of n_chunks words to its place behind the packed container the layout and gather kernels have just written, gathered from n_parts runs: run p is
// `count` words at `src`, placed from entry `entry` on; the runs cover entries 0 .. n_chunks - 1 once (a join: a run per part; a slice, a pack, an unpage: one run)
struct TrailerRun { const uint8_t* src; uint32_t entry, count; };
struct TrailerRuns { TrailerRun p[kJoinMaxParts]; };
hipError_t launch_place_trailer(const TrailerRuns& runs, uint32_t n_parts, uint8_t* d_container, uint64_t capacity, uint32_t n_chunks, uint32_t* d_err,
                                hipStream_t stream);

// ---- parity.hip (recovery records: the parity blob "DHP1" of include/density_hip.h, and the rebuild behind a verdict decode) ----
// The blob of d_data (hdr.total_len bytes, any alignment) into d_blob (any alignment): hdr itself, then hdr.n_groups rows of hdr.row_bytes bytes — with
// hdr.version 2 as many Q rows (GF(2^8), from the same loads) behind them.
hipError_t launch_parity_rows(const uint8_t* d_data, const density_hip_parity_header_t& hdr, uint8_t* d_blob, hipStream_t stream);
// The blob at d_blob (any alignment) brought up to date after an edit of its input: input bytes [offset, offset + old_size) held d_old and hold d_new (new_size
// bytes; the shorter of the two counts as zero-padded; both at any alignment) now.  `after`: the blob's header after the edit (density_hip_parity_update_header) —
// version, chunk_size, n_groups and row_bytes are the blob's own, n_chunks and total_len are written into the blob.  Only the rows of the groups the edited chunks
// belong to are read and written, every 16-byte slot by one lane; an edit inside one chunk takes only the row tiles it covers.  A zero-length edit launches nothing.
hipError_t launch_parity_update(uint8_t* d_blob, const density_hip_parity_header_t& after, uint64_t offset, const uint8_t* d_old, uint64_t old_size, const uint8_t* d_new,
                                uint64_t new_size, hipStream_t stream);
// Behind launch_chunk_verdicts.  d_victim[g] (n_groups words of scratch) = the only chunk of group g with verdict DENSITY_HIP_CHUNK_DAMAGED, if there is exactly
// one: its bytes in d_out become row g of d_rows (n_groups rows of row_bytes bytes, any alignment) XOR the other members' bytes, and d_acc[victim] = 0.
// with_q (a version-2 blob: n_groups Q rows behind those; groups of at most 255): d_victim[g] names the group's only TWO damaged chunks as well, and both are
// rebuilt from the two rows and the other members' bytes.  The same with_q goes to launch_recover_verify: it says how d_victim is read.
hipError_t launch_recover_rebuild(uint8_t* d_out, uint64_t size, uint32_t chunk, uint32_t n_chunks, const uint8_t* d_rows, uint32_t n_groups, uint32_t row_bytes,
                                  bool with_q, const uint32_t* d_verdicts, uint32_t* d_victim, uint32_t* d_acc, hipStream_t stream);
// ... then the victims summed again into d_acc and held against the trailer d_expect: DENSITY_HIP_CHUNK_RECOVERED into d_verdicts where it matches now, one less in
// *d_damaged and one more in *d_recovered (cleared here) for each.
hipError_t launch_recover_verify(const uint8_t* d_out, uint64_t size, uint32_t chunk, uint32_t n_chunks, uint32_t n_groups, bool with_q, const uint32_t* d_victim,
                                 uint32_t* d_acc, const uint8_t* d_expect, uint32_t* d_verdicts, uint32_t* d_damaged, uint32_t* d_recovered, hipStream_t stream);

}  // namespace density
