/*
 * density_hip.h — C ABI of libdensity_hip.so, the MI355X (gfx950) implementation of density's
 * 4-byte-word dictionary-hash encode/decode hot path.
 *
 * Section 1 is the drop-in boundary: the nine `extern "C"` symbols the reference crate (density-rs 0.16.6)
 * itself exports, with identical names, signatures and return convention.  A reference-side FFI (Rust
 * `extern "C"` block, cgo, ctypes ...) binds exactly these; see INTEGRATION.md.
 *
 * Section 2 is additive: the chunked container that makes the path data-parallel (each chunk is an independent
 * reference stream), device-pointer + stream variants, and profiling hooks.  Nothing in section 2 changes the
 * meaning of section 1.
 *
 * All citations are file:line in the reference tree (src/...).
 */
#ifndef DENSITY_HIP_H
#define DENSITY_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ------------------------------------------------------------------------------------------------------------
 * 1. Reference-compatible symbols (host pointers, single reference-format stream, bit-exact with the crate).
 *    (One stream is one dependency chain; long Chameleon streams are still encoded and decoded in parallel segments on
 *    the device, with byte-identical results: DESIGN.md 4.7.)
 *
 *    Return value: bytes written; 0 on any failure (the reference maps Err to 0 via unwrap_or(0) and otherwise
 *    panics on a short buffer or truncated input; this library returns 0 instead and never writes past
 *    output_size).  An empty input also returns 0, as in the reference.
 *    `output_size` must be >= {algo}_safe_encode_buffer_size(input_size) for encode and >= the original length
 *    for decode (the stream does not carry its decoded length; codec/codec.rs:72-80).
 *
 *    These calls stage through device memory (H2D, kernels, D2H) on a per-device internal stream and are
 *    thread-safe.  How one stream is spread over the device: chameleon_encode / _decode of a few MiB
 *    and more in ~256 parallel segments; cheetah_encode / lion_encode of 64 / 192 KiB and more in passes of ordered LDS
 *    exchanges, cheetah_decode of 64 KiB and more in decode passes (everything but its chain of contexts in parallel);
 *    lion_decode and short streams on one wave or one work-group.  The data-parallel path proper is the container API
 *    of section 2.
 *    SLOWER THAN THE CRATE on one CPU core (10 MB of prose, buffers on the device, profiles/r06_benches_density.txt): cheetah_decode
 *    ~0.32 GB/s against 1.4 (its chain of contexts is one team of four waves on one CU), lion_decode ~0.09 GB/s against 0.84 (two waves,
 *    tables in memory); cheetah_encode 3.2 against 1.0 and lion_encode 1.0 against 0.65 only just win.  One stream is one dependency
 *    chain: a caller with more than one stream's worth of data wants the container calls, which are what this library is for.
 * ---------------------------------------------------------------------------------------------------------- */

/* algorithms/chameleon/chameleon.rs:70-73 */
size_t chameleon_encode(const uint8_t* input, size_t input_size, uint8_t* output, size_t output_size);
/* algorithms/chameleon/chameleon.rs:75-78 */
size_t chameleon_decode(const uint8_t* input, size_t input_size, uint8_t* output, size_t output_size);
/* algorithms/chameleon/chameleon.rs:80-83 -> codec/codec.rs:18-21 */
size_t chameleon_safe_encode_buffer_size(size_t size);

/* algorithms/cheetah/cheetah.rs:105-108 */
size_t cheetah_encode(const uint8_t* input, size_t input_size, uint8_t* output, size_t output_size);
/* algorithms/cheetah/cheetah.rs:110-113 */
size_t cheetah_decode(const uint8_t* input, size_t input_size, uint8_t* output, size_t output_size);
/* algorithms/cheetah/cheetah.rs:115-118 */
size_t cheetah_safe_encode_buffer_size(size_t size);

/* algorithms/lion/lion.rs:193-196 */
size_t lion_encode(const uint8_t* input, size_t input_size, uint8_t* output, size_t output_size);
/* algorithms/lion/lion.rs:198-201 */
size_t lion_decode(const uint8_t* input, size_t input_size, uint8_t* output, size_t output_size);
/* algorithms/lion/lion.rs:203-206 */
size_t lion_safe_encode_buffer_size(size_t size);

/* ------------------------------------------------------------------------------------------------------------
 * 2. Additive extensions (not in the reference).
 * ---------------------------------------------------------------------------------------------------------- */

enum { DENSITY_HIP_CHAMELEON = 0, DENSITY_HIP_CHEETAH = 1, DENSITY_HIP_LION = 2 };

enum {
    DENSITY_HIP_OK = 0,
    DENSITY_HIP_ERR_ARGUMENT = 1,     /* bad algo / chunk size / null pointer */
    DENSITY_HIP_ERR_CAPACITY = 2,     /* output or workspace too small */
    DENSITY_HIP_ERR_FORMAT = 3,       /* container header or payload malformed / truncated */
    DENSITY_HIP_ERR_RUNTIME = 4,      /* HIP runtime error, no gfx950 device, failed self-test */
    DENSITY_HIP_ERR_UNSUPPORTED = 5,  /* the device path does not take these buffers (a paged container or its output not 4-byte aligned) */
    DENSITY_HIP_ERR_CHECKSUM = 6      /* a sealed container decoded without a format error, but not to the bytes that were sealed */
};

/*
 * Chunked container ("DHC1").  The input is cut into chunks of `chunk_size` bytes (a multiple of 256, i.e. of
 * every algorithm's block size); chunk i is encoded as an independent reference stream — fresh zero tables and a
 * fresh ProtectionState, exactly what {Algo}::encode(&input[i*C..]) returns (chameleon.rs:45-48) — so chunks
 * encode and decode in parallel.  Layout (little-endian):
 *     [0,32)                 density_hip_header_t
 *     [32, 32+4*n_chunks)    u32 encoded size of each chunk payload
 *     (16-byte aligned)      optional block index, one byte per 256-byte input block (flags & DENSITY_HIP_FLAG_BLOCK_INDEX)
 *     payload i starts at the next 16-byte boundary after payload i-1 (payload 0 after the tables)
 * With one chunk (chunk_size >= total_len) the single payload IS the reference stream of the whole input.
 *
 * Block index (Chameleon): the reference stream marks neither record boundaries nor raw-copy blocks — both sides re-derive
 * them by walking the records and running the same ProtectionState FSM (codec/codec.rs:35-37 vs :89-91), a serial
 * pointer chase.  The index stores what that walk would find: byte b describes input block b (numbered over the whole
 * input): bit 7 = raw-copy block; bits 0..6 = number of MAP flags of the block's signature, 0..64 (record length
 * = 8 + 256 - 2*n), or 0x7f for the chunk's ragged last block (< 256 bytes).  It is redundant metadata —
 * payloads stay plain reference streams — and a container without it (flags == 0, e.g. one assembled by a CPU producer)
 * decodes through the record-walking path.
 */
#define DENSITY_HIP_FLAG_BLOCK_INDEX 1u
/* Slotted container (device-resident form): payload i is NOT packed behind payload i-1 but stays in the worst-case slot the encoder
 * wrote it to, at payload_base + i * slot_stride, slot_stride = round_up({algo}_safe_encode_buffer_size(chunk_size), 256); the size
 * table says how much of each slot is stream; container_len is the end of the last payload.  The chunk streams themselves are the
 * same bytes.  This is what density_hip_encode_device_slotted() produces and what density_hip_decode_device() also accepts: the
 * gather into the packed form (one more pass over every encoded byte: write_buffer.rs:29-31's running total has no parallel
 * equivalent until the sizes exist) is left to the moment the container leaves the device — density_hip_pack_device(), or the
 * host-pointer density_hip_encode(), which always returns the packed form. */
#define DENSITY_HIP_FLAG_SLOTTED 2u
/* Paged container (round 5; Chameleon, with the block index): the wire form WITHOUT a stitch pass.  The encoder places the streams itself, in
 * pages of DENSITY_HIP_PAGE_BYTES taken from one counter as the chunks ask for them: a chunk's stream leaves a page when the records of its next
 * round of 16 blocks (4 KiB of input, at most 4224 bytes) would not end inside it, so page changes fall on multiples of 16 blocks and a page's
 * unused tail is at most a round (2 % of a page on text).  Layout behind the block index:
 *     (16-byte aligned)   page directory, per chunk 16 * (1 + P) bytes, P = density_hip_paged_pages_per_chunk(chunk_size):
 *                             {u32 n_pages, 0, 0, 0}, then per page of the chunk, in stream order,
 *                             {u32 page, u32 first input block of the chunk coded there, u32 bytes of stream in the page, 0}
 *     (256-byte aligned)  page 0, page 1, ...   (container_len = this base + DENSITY_HIP_PAGE_BYTES * pages in use)
 * Chunk i's reference stream = the first `bytes` of each of its pages, concatenated; the u32 size table holds the sum.  A CPU reader does that and
 * calls the crate; density_hip_decode_device() reads the pages in place, and only from a container and into an output that are both
 * 4-byte aligned (anything else: DENSITY_HIP_ERR_UNSUPPORTED, nothing written; density_hip_decode() on host pointers stages it aligned). */
#define DENSITY_HIP_FLAG_PAGED 4u
/* Sealed container: any of the three forms above, for any algorithm, followed by a trailer of content checksums.  A flipped bit in a PLAIN quad, a
 * MAP hash or a raw-copy block is a valid stream: the reference decodes it, and so does this library, to total_len wrong bytes.  The trailer catches that.
 * With E the unsealed container_len: at T = round_up(E, 16) stand n_chunks little-endian u32, entry i = C(input chunk i) (the last chunk at its true
 * length), zero-padded to a multiple of 16 (the bytes [E, T) are zeros too); container_len becomes T + round_up(4 * n_chunks, 16) and this flag is
 * set.  A reader finds the trailer from the end: T = container_len - round_up(4 * n_chunks, 16).  Nothing in front of T moves: size table, block index,
 * directory, pages and payload offsets are those of the unsealed container.  A container of zero chunks seals to itself plus the flag.
 *     C(B), B of L bytes: m = ceil(L / 4) little-endian 32-bit words w_i, the last zero-padded; all arithmetic mod 2^32:
 *         S = sum over i of fmix32(w_i + 0x9E3779B1 * (i + 1));   C = fmix32(S + (uint32_t)L);
 *         fmix32(h): h ^= h >> 16; h *= 0x85ebca6b; h ^= h >> 13; h *= 0xc2b2ae35; h ^= h >> 16.
 * A sum, so that any split of a chunk over lanes, work-groups or host slices combines with one add; fmix32 is a bijection and the word's index goes
 * in, so one damaged word, or two different words exchanged, always change S; random damage passes with probability 2^-32.  It is an INTEGRITY CHECK,
 * NOT A MAC: anyone who can rewrite the payload can rewrite the trailer.  density_hip_checksum32() below computes C on the host.
 * density_hip_decode_device() / density_hip_decode() verify a sealed container: they decode as ever, sum their own output on the device and compare. */
#define DENSITY_HIP_FLAG_CHECKSUM 8u
#define DENSITY_HIP_PAGE_BYTES 65536u
#define DENSITY_HIP_MAGIC 0x31434844u /* "DHC1" */
#define DENSITY_HIP_DEFAULT_CHUNK (1u << 20)

typedef struct density_hip_header {
    uint32_t magic;          /* DENSITY_HIP_MAGIC */
    uint8_t  algo;           /* DENSITY_HIP_CHAMELEON ... */
    uint8_t  version;        /* 1 */
    uint16_t flags;          /* DENSITY_HIP_FLAG_* */
    uint32_t chunk_size;     /* bytes of input per chunk, multiple of 256 */
    uint32_t n_chunks;       /* ceil(total_len / chunk_size) */
    uint64_t total_len;      /* decoded length in bytes */
    uint64_t container_len;  /* total container length in bytes (header + table + padded payloads) */
} density_hip_header_t;

/* chunk_size 0 in the calls below means density_hip_auto_chunk_for(algo, input_size); for Chameleon (density_hip_auto_chunk): a chunk is one work-group
 * on one CU, small chunks restart the dictionary and cost ratio, every chunk start costs a table clear — so: 64 KiB up to 16 MiB of input, beyond
 * that the fewest whole waves of 256 chunks of at most 4 MiB with the input spread evenly over them in whole 4 KiB rounds (10 MB -> 64 KiB,
 * 100 MB -> 384 KiB = 255 chunks, 256 MiB -> 1 MiB, 1 GiB -> 4 MiB, 1.5 GiB -> 3 MiB = 512 chunks). */
size_t density_hip_auto_chunk(size_t input_size);
/* The same per algorithm, 64 KiB .. 1 MiB: Lion (one wave per chunk stream, memory-latency bound) takes the largest power of two that
 * still gives the device 700 streams, about three per CU (100 MB -> 128 KiB); Cheetah (decode passes: one chunk's chain of contexts per CU, in time proportional to the chunk)
 * one chunk per CU: the input over 256, rounded up to 4 KiB (100 MB -> 384 KiB). */
size_t density_hip_auto_chunk_for(int algo, size_t input_size);

/* Upper bound of the container size for `input_size` bytes (0 if the arguments are invalid). */
size_t density_hip_container_bound(int algo, size_t input_size, size_t chunk_size);

/* Host-pointer container codec (H2D, kernels, D2H). Return bytes written, 0 on failure.
 * Chameleon inputs worth three slices or more (32 MiB at least; a slice is a twelfth of the input, ten chunks at least) are pipelined: the
 * caller's buffers are pinned in place for the duration of the call (hipHostRegister), slices of chunks go up on one stream, through the
 * kernels on others, and down on a third: 46-52 GB/s at 256 MiB .. 1 GiB where the whole buffer staged in sequence gives 33-35.  The
 * container is byte for byte the same either way.  Where pinning fails the staged path is taken. */
size_t density_hip_encode(int algo, const uint8_t* input, size_t input_size, uint8_t* output, size_t output_size,
                          size_t chunk_size);
size_t density_hip_decode(const uint8_t* container, size_t container_size, uint8_t* output, size_t output_size);
/* density_hip_encode() followed by a seal on the device before the copy down (DENSITY_HIP_FLAG_CHECKSUM): the packed form with its trailer.
 * `output_size` must hold density_hip_container_bound() + density_hip_seal_overhead().  density_hip_decode() verifies a sealed container and returns
 * 0, with density_hip_last_error() naming the checksum, where the decoded bytes are not the sealed ones.  Sealed containers are staged whole: the
 * pipelined paths above take unsealed containers only, and the bytes do not depend on the path. */
size_t density_hip_encode_sealed(int algo, const uint8_t* input, size_t input_size, uint8_t* output, size_t output_size, size_t chunk_size);
/* Reads total_len from a host-resident container header (0 if malformed). */
size_t density_hip_decoded_size(const uint8_t* container, size_t container_size);

/* Device-resident container codec: pointers are device pointers on the current HIP device, `stream` is a
 * hipStream_t (NULL = the library's internal stream).  Work is enqueued on `stream`.
 *   - workspace: pass a device buffer of at least density_hip_{encode,decode}_workspace_size() bytes, or NULL to
 *     use the library's per-device cached workspace (then calls on different streams must not overlap).
 *     The encode workspace holds a worst-case slot per chunk (about 1.06 x the input) and, for Cheetah / Lion, a table slot per
 *     concurrent chunk stream (768 KiB / 1.75 MiB, at most 8 GiB) plus the scratch of the exchange passes (a dword per quad and
 *     the per-block masks: about 1.25 / 1.5 x the input).
 *   - header_out / decoded_size_out: optional HOST pointers; when non-NULL the call synchronises `stream` and
 *     fills them (and then also reports kernel-detected format errors).  When NULL the call is fully asynchronous.
 * Returns DENSITY_HIP_OK or an error code. */
size_t density_hip_encode_workspace_size(int algo, size_t input_size, size_t chunk_size);
size_t density_hip_decode_workspace_size(uint32_t n_chunks);
/* The same for a container of known shape: includes the scratch of Cheetah's decode passes (a dword and a half per quad: 1.5 x total_len
 * + 1/32; decode_passes.hip).  A workspace of only density_hip_decode_workspace_size() bytes still decodes — Cheetah on one wave per
 * chunk stream wherever it is smaller than density_hip_decode_workspace_size_for() (that size is set by Lion's tables, and for a few large
 * chunks it holds the passes' scratch too). */
size_t density_hip_decode_workspace_size_for(int algo, size_t total_len, size_t chunk_size);
int density_hip_encode_device(int algo, const void* d_input, size_t input_size, void* d_output, size_t output_capacity,
                              size_t chunk_size, void* d_workspace, size_t workspace_size, void* stream,
                              density_hip_header_t* header_out);
/* The same, leaving every chunk stream in its slot inside the output (DENSITY_HIP_FLAG_SLOTTED): no stitch pass.  `output_capacity` must be at
 * least density_hip_container_bound_slotted().  With one chunk the result is the ordinary (packed) container. */
size_t density_hip_container_bound_slotted(int algo, size_t input_size, size_t chunk_size);
int density_hip_encode_device_slotted(int algo, const void* d_input, size_t input_size, void* d_output, size_t output_capacity,
                                      size_t chunk_size, void* d_workspace, size_t workspace_size, void* stream,
                                      density_hip_header_t* header_out);
/* The same as a PAGED container (DENSITY_HIP_FLAG_PAGED above): wire-ready without a stitch pass.  Chameleon inputs of two and more chunks of 1 MiB and
 * more and less than about 3 GiB; anything else comes out slotted, as from density_hip_encode_device_slotted() — the header's flags say which.
 * `output_capacity` must be at least density_hip_container_bound_paged() (the pages every chunk could need; text ends far below it). */
size_t density_hip_container_bound_paged(int algo, size_t input_size, size_t chunk_size);
size_t density_hip_paged_pages_per_chunk(size_t chunk_size);
int density_hip_encode_device_paged(int algo, const void* d_input, size_t input_size, void* d_output, size_t output_capacity,
                                    size_t chunk_size, void* d_workspace, size_t workspace_size, void* stream,
                                    density_hip_header_t* header_out);
/* Slotted (or packed) container, sealed or not -> packed container: byte for byte what density_hip_encode_device() (+ density_hip_seal_device()) writes for
 * the same input.  The call is density_hip_slice_device() of the window [0, n_chunks) — one driver runs pack, unpage and slice —, so what that call says of
 * alignment, of the faults found on the device (a size-table entry above {algo}_safe_encode_buffer_size of its chunk's input or above its slot, streams that
 * run past the container: DENSITY_HIP_ERR_FORMAT, no payload byte written) and of the gaps (zeros, but a packed source moves as one run with the gaps between
 * its streams as they stand) holds here.  Its own: `output_capacity` at least density_hip_container_bound(), plus density_hip_seal_overhead() for a sealed
 * input (less: DENSITY_HIP_ERR_CAPACITY at once, nothing written); a PAGED container is DENSITY_HIP_ERR_UNSUPPORTED (density_hip_unpage_device is for those);
 * a container of no chunks is taken.  Workspace as for decode.  With header_out == NULL the call is asynchronous and reports nothing about the container it was
 * given (a refused size table leaves the payloads unwritten): pass header_out to have it validated.
 * Profiling marks: "layout_encode", "compact" and, for a sealed source, "move_trailer". */
int density_hip_pack_device(const void* d_container, size_t container_size, const density_hip_header_t* header, void* d_output,
                            size_t output_capacity, void* d_workspace, size_t workspace_size, void* stream, density_hip_header_t* header_out);
/* Paged container -> packed container: what density_hip_pack_device does for the slotted form, over the page directory — density_hip_slice_device() of the
 * window [0, n_chunks) of a paged source, through the same driver (profiling marks: "layout_encode", "unpage" and, sealed, "move_trailer").  The input is a PAGED
 * container, sealed or not; the output is the packed container of the same chunks with DENSITY_HIP_FLAG_BLOCK_INDEX (and DENSITY_HIP_FLAG_CHECKSUM if the
 * input was sealed): byte for byte what density_hip_encode_device() (+ density_hip_seal_device()) writes for the same input — header, size table, block
 * index, the 16-byte-aligned payloads with zero gaps, container_len, the trailer behind round_up(E, 16) — whatever order the pages were taken in.  The page
 * directory and the unused tails of the pages do not appear.  Both buffers at ANY byte alignment (the pages are not decoded, only moved).
 *   - `output_capacity`: at least density_hip_container_bound(), plus density_hip_seal_overhead() for a sealed input; less is DENSITY_HIP_ERR_CAPACITY at
 *     once, nothing written.  Workspace as for decode, or NULL.
 *   - a container that is not PAGED: DENSITY_HIP_ERR_ARGUMENT, nothing written (density_hip_pack_device is for those).
 *   - a directory the call cannot follow is DENSITY_HIP_ERR_FORMAT, found on the device by a check that runs in front of the gather, and then no payload
 *     byte of the output is written for any chunk: a chunk with 0 or more than density_hip_paged_pages_per_chunk() pages, a page number at or beyond the
 *     pages the container holds, a page's `bytes` above DENSITY_HIP_PAGE_BYTES, the `bytes` of a chunk's pages not adding up to its size-table entry, a
 *     size-table entry above {algo}_safe_encode_buffer_size of the chunk's input.  The "first input block" field is not interpreted: bytes are moved,
 *     streams are not parsed.
 *   - header_out == NULL: fully asynchronous, nothing is reported (a refused directory or a capacity the packed container outgrows leaves the payloads
 *     unwritten).  With header_out the call synchronises, returns the packed container's header and reports DENSITY_HIP_ERR_FORMAT / _CAPACITY. */
int density_hip_unpage_device(const void* d_container, size_t container_size, const density_hip_header_t* header, void* d_output,
                              size_t output_capacity, void* d_workspace, size_t workspace_size, void* stream, density_hip_header_t* header_out);
/* Slice: chunks [first_chunk, first_chunk + chunk_count) of a container as a container of their own — random access without touching a decoder.  The input is
 * a packed, slotted or PAGED container of any algorithm, sealed or not; the output is an ordinary PACKED container: magic, algo, version and chunk_size copied,
 * n_chunks = chunk_count, total_len = L = min(total_len, (first + count) * chunk_size) - first * chunk_size, flags = the source's DENSITY_HIP_FLAG_BLOCK_INDEX and
 * DENSITY_HIP_FLAG_CHECKSUM and nothing else; behind it size-table entries first .. first+count-1, the block-index bytes [first * chunk_size / 256, + ceil(L / 256)),
 * the payloads at 16-byte boundaries with zero gaps, container_len, and for a sealed source, behind round_up(E, 16), trailer entries first .. first+count-1,
 * zero-padded.  Every byte up to container_len is written: byte for byte the packed container the layout above describes for those chunk streams — for a container
 * this library made, what density_hip_encode_device() (+ density_hip_seal_device()) writes for input[first * chunk_size : + L] with the same chunk_size.  Every call
 * that takes a container takes the result: decode, verdicts, pack, the multi-rank wire form.  Both buffers at ANY byte alignment: streams are moved, not parsed.
 * A byte range is slice + decode + a pointer offset (density_amd.container.decode_range_device):
 *   density_hip_chunk_range: the chunks that cover input bytes [offset, offset + length), and *skip = offset - first_chunk * chunk_size, where the range starts in
 *     the slice's decoded bytes.  length == 0, offset + length > total_len or a header that is not a container's: DENSITY_HIP_ERR_ARGUMENT.  Pure host arithmetic.
 *   density_hip_slice_bound: the capacity the slice asks for: density_hip_container_bound(algo, L, chunk_size), plus density_hip_seal_overhead(L, chunk_size) for a
 *     sealed header; 0 for chunk_count == 0, first_chunk + chunk_count > n_chunks or a header that is not a container's.  Pure host arithmetic.
 *   density_hip_slice_device: workspace as for decode — density_hip_decode_workspace_size(n_chunks of the SOURCE) — or NULL.
 *   - chunk_count == 0, first_chunk + chunk_count > n_chunks, a header that is not a container's: DENSITY_HIP_ERR_ARGUMENT, nothing written.
 *   - output_capacity < density_hip_slice_bound(): DENSITY_HIP_ERR_CAPACITY at once, nothing written.
 *   - a header or trailer that does not fit container_size: DENSITY_HIP_ERR_FORMAT at once, nothing written.
 *   - DENSITY_HIP_ERR_FORMAT found on the device, by the layout kernel in front of the gather, and then no payload byte of the output is written: a size-table entry
 *     of the window above {algo}_safe_encode_buffer_size of its chunk's input; a window whose streams run past the container (packed) or past their slot (slotted);
 *     for a PAGED source every fault density_hip_unpage_device knows, in the directory entries of the window's chunks only.
 *   - DAMAGE OUTSIDE THE WINDOW IS NOT THIS CALL'S BUSINESS: a chunk in front of or behind the window may have a directory nobody can follow, a lying size, a flipped
 *     bit — the slice is made, and it is the slice of an intact container.  One exception cannot be seen without parsing streams: a lying size-table entry IN FRONT OF
 *     a packed window moves the window (a packed stream's place is the sum of the entries before it).  The slice then holds wrong bytes; a sealed slice says so when
 *     it is decoded.  (A packed source's window is moved in one run, with the gaps between its streams as they stand: zeros in every container of this format.)
 *   - header_out == NULL: fully asynchronous, no host round trip — the source offset of chunk first_chunk stays on the device — and nothing is reported (a refused
 *     window leaves the payloads unwritten).  With header_out the call synchronises, returns the slice's header and reports DENSITY_HIP_ERR_FORMAT / _CAPACITY.
 *     `header` may be NULL: it is then read back first, as in density_hip_decode_device.
 *   density_hip_slice: the host-pointer form, staged whole; returns the bytes written, 0 on failure with density_hip_last_error() set.
 * Profiling marks: "slice_layout", "slice_gather" and, for a sealed source, "move_trailer".
 * Out of scope: the parity blob "DHP1" cannot be sliced (its rows span the whole input: a slice wants a blob of its own, density_hip_parity_device of the decoded
 * window); chunk lists that are not a range; a range decode at this level (it is the three calls above). */
int density_hip_chunk_range(const density_hip_header_t* header, uint64_t offset, uint64_t length, uint32_t* first_chunk, uint32_t* chunk_count, uint64_t* skip);
size_t density_hip_slice_bound(const density_hip_header_t* header, uint32_t first_chunk, uint32_t chunk_count);
int density_hip_slice_device(const void* d_container, size_t container_size, const density_hip_header_t* header, uint32_t first_chunk, uint32_t chunk_count,
                             void* d_output, size_t output_capacity, void* d_workspace, size_t workspace_size, void* stream, density_hip_header_t* header_out);
size_t density_hip_slice(const uint8_t* container, size_t container_size, uint32_t first_chunk, uint32_t chunk_count, uint8_t* output, size_t output_size);
/* Join: chunk windows of several containers as ONE packed container — the slice's inverse.  Append is a join of two whole containers; replacing chunk k of A
 * by the one-chunk container B is join(A[0, k), B, A[k + 1, n)); a multi-rank container "DHCM" becomes a "DHC1" by joining its rows.  A part is
 * a window [first_chunk, first_chunk + chunk_count) of a packed, slotted or PAGED container, sealed or not; forms may differ from part to part.  No stream is
 * parsed or re-encoded: one pass over the encoded bytes.  The output is an ordinary PACKED container: magic, algo, version and chunk_size those of the parts,
 * n_chunks = N = the sum of the windows' counts, total_len = L = the sum of the windows' decoded lengths (a window's length as the slice defines it), flags = the
 * parts' common DENSITY_HIP_FLAG_BLOCK_INDEX and DENSITY_HIP_FLAG_CHECKSUM and nothing else; behind the header the windows' size-table entries in order, the
 * windows' block-index bytes concatenated, every stream at the next 16-byte boundary behind the one before with zeros in the gaps (the gap between the last
 * stream of one part and the first of the next too), container_len where the last stream ends, and for sealed parts, behind round_up(E, 16), the windows'
 * trailer entries concatenated and zero-padded.  Every byte up to container_len is written, none at or beyond it.  For containers this library made: byte for
 * byte what density_hip_encode_device() (+ density_hip_seal_device()) writes for the concatenation of the windows' inputs with the same chunk_size.  Every call
 * that takes a container takes the result.  All buffers at ANY byte alignment.
 *   A part: `container` a device pointer (density_hip_join_device) or a host pointer (density_hip_join); `header` a HOST copy of the part's first 32 bytes,
 *     REQUIRED — the output's geometry is host arithmetic; chunk_count == 0: the part is skipped and nothing of it is read, not even its pointers.
 *   - DENSITY_HIP_ERR_ARGUMENT on the host, nothing written, no device work: n_parts == 0 or above DENSITY_HIP_JOIN_MAX_PARTS, or N == 0; a part (not skipped) with
 *     a NULL pointer, a NULL header or a container_size below a header's 32 bytes; a header that is not a container's; a window outside its container's chunks; parts that differ in algo, chunk_size, the
 *     BLOCK_INDEX flag or the CHECKSUM flag; a part other than the last (of those not skipped) whose window's length is not chunk_count * chunk_size — a ragged
 *     chunk may only be the output's last, and block-index slices then concatenate without re-basing; N above 2^32 - 1; an output range that overlaps a part's
 *     range (the device call).
 *   - output_capacity < density_hip_join_bound(): DENSITY_HIP_ERR_CAPACITY at once, nothing written.
 *   - a part whose header or trailer does not fit its container_size: DENSITY_HIP_ERR_FORMAT at once, nothing written.
 *   - DENSITY_HIP_ERR_FORMAT found on the device, by the layout kernel in front of the gather, and then no payload byte is written for ANY part: the slice's faults,
 *     per part, judged in each part's window only — an entry above its chunk's worst case or its slot, a stream that runs past its container, for a PAGED part every
 *     fault density_hip_unpage_device knows.  Damage outside the windows is not this call's business; the slice's one exception holds per packed part: a lying
 *     entry in front of a packed window moves that window.
 *   density_hip_join_bound: density_hip_container_bound(algo, L, chunk_size), plus density_hip_seal_overhead(L, chunk_size) for sealed parts; 0 for anything the
 *     ARGUMENT list above refuses on the host.  Pure host arithmetic: no device, no HIP call.
 *   density_hip_join_workspace_size: what a caller's workspace must hold for n_parts parts (1 .. DENSITY_HIP_JOIN_MAX_PARTS, skipped ones need not count) and N
 *     output chunks; 0 outside that.  Pure host arithmetic.  d_workspace == NULL: the library's cached per-device workspace, which, like a caller's, must overlap
 *     neither the parts nor the output.
 *   - header_out == NULL: fully asynchronous — the part table and the headers it points to are read before the call returns, nothing is reported (refused windows
 *     leave the payloads unwritten), nothing about the sources crosses back to the host.  With header_out the call synchronises, returns the joined header and
 *     reports DENSITY_HIP_ERR_FORMAT / _CAPACITY.
 *   density_hip_join: the host-pointer form, staged whole; returns the bytes written, 0 on failure with density_hip_last_error() set.
 * Profiling marks: "join_layout", "join_gather" and, for sealed parts, "move_trailer".
 * A parity blob "DHP1" of A is kept current across an append or a replaced chunk by density_hip_parity_update_device (below), from the old and new bytes alone.
 * Out of scope: joining parity blobs (a blob's rows span its whole input); parts whose chunk
 * sizes differ, and re-chunking; a ragged chunk anywhere but at the end; in-place joins, where the output overlaps a part. */
#define DENSITY_HIP_JOIN_MAX_PARTS 64u
typedef struct density_hip_join_part {
    const void* container;
    size_t container_size;
    const density_hip_header_t* header;
    uint32_t first_chunk, chunk_count;
} density_hip_join_part_t;
size_t density_hip_join_bound(const density_hip_join_part_t* parts, uint32_t n_parts);
size_t density_hip_join_workspace_size(uint32_t n_parts, uint32_t n_chunks_out);
int density_hip_join_device(const density_hip_join_part_t* parts, uint32_t n_parts, void* d_output, size_t output_capacity, void* d_workspace, size_t workspace_size,
                            void* stream, density_hip_header_t* header_out);
size_t density_hip_join(const density_hip_join_part_t* parts, uint32_t n_parts, uint8_t* output, size_t output_size);
/* `header` may be NULL: it is then read back from the device (one small synchronous copy). */
int density_hip_decode_device(const void* d_container, size_t container_size, const density_hip_header_t* header,
                              void* d_output, size_t output_capacity, void* d_workspace, size_t workspace_size,
                              void* stream, size_t* decoded_size_out);

/* Sealed containers on the device (DENSITY_HIP_FLAG_CHECKSUM above).
 * density_hip_checksum_device: C of every `chunk_size` bytes (a multiple of 256) of a device buffer at any alignment into d_sums[ceil(size / chunk_size)]
 * (4-byte aligned; cleared by the call).  Asynchronous.
 * density_hip_seal_device: seals, in place, the container one of the three density_hip_encode_device* calls has just written for d_input; ordered on `stream`
 * behind that call.  What it needs — chunk size, chunk count, where the container ends — it reads from the header ON THE DEVICE; `header` (optional, HOST) only lets
 * it refuse at once what it would refuse anyway.  With header_out == NULL there is no host round trip: a one-work-group kernel in front of the sum kernel
 * checks the header and the capacity, one behind it writes the trailer, the flag and the new container_len, and a container_capacity too small for the
 * trailer leaves the container unsealed and is not reported (the same contract as the encode calls).  With header_out the call synchronises, returns the
 * sealed header and reports DENSITY_HIP_ERR_CAPACITY.  DENSITY_HIP_ERR_ARGUMENT: the container is sealed already, or input_size is not its total_len
 * (seen at once with `header`, on the device otherwise and then reported only with header_out).  Scratch (a word per chunk) comes from the library's
 * per-device workspace: calls on different streams must not overlap with other calls that use it.
 * density_hip_decode_device on a sealed container decodes as ever, sums its own output and compares it with the trailer on the device: with
 * decoded_size_out a mismatch is DENSITY_HIP_ERR_CHECKSUM and *decoded_size_out = 0 (format errors take precedence); without, nothing is reported, like
 * format errors.  density_hip_pack_device carries the trailer of a sealed slotted container along: byte for byte density_hip_encode_device + density_hip_seal_device
 * (`output_capacity`: density_hip_container_bound() + density_hip_seal_overhead()). */
int density_hip_checksum_device(const void* d_data, size_t size, size_t chunk_size, uint32_t* d_sums, void* stream);
int density_hip_seal_device(const void* d_input, size_t input_size, void* d_container, size_t container_capacity, const density_hip_header_t* header,
                            void* stream, density_hip_header_t* header_out);

/* Verdicts and salvage: which chunks of a sealed container are damaged, and the rest of it kept.
 * density_hip_decode_device_verdicts decodes exactly as density_hip_decode_device does (the same workspace rules, the same three forms, the same kernels) and
 * then answers per chunk: d_verdicts[i] (n_chunks words on the device, 4-byte aligned) is 0 if and only if the bytes now standing in chunk i's region of
 * d_output have the checksum the trailer holds for chunk i, DENSITY_HIP_CHUNK_DAMAGED otherwise.  The verdict is about the output's content, so it holds
 * whatever damaged the chunk: a flipped PLAIN quad that decodes silently, a signature the block index contradicts, a lying size table, a directory entry
 * the decoder refuses to read through — and a damaged trailer entry, which reports a chunk whose bytes are right.  No pass over the data is added: the sums
 * the verifying decode has just made are held against the trailer once more by a kernel of a thread per chunk.  With DENSITY_HIP_SALVAGE_BLANK in `flags` the
 * output region of every damaged chunk (the last chunk at its true length) is then overwritten with zeros: wrong bytes of the right length are what sealing
 * exists to prevent.  The output is kept in every case.
 *   - damaged_out == NULL: fully asynchronous, nothing is reported; the verdicts lie on the device for the caller's next kernel on `stream`, and the number
 *     of damaged chunks in the second 32-bit word of d_workspace where the caller passed one.
 *   - damaged_out (HOST): the call synchronises `stream`; DENSITY_HIP_OK with *damaged_out == 0 for an intact container, DENSITY_HIP_ERR_CHECKSUM with
 *     *damaged_out = the number of damaged chunks, DENSITY_HIP_ERR_FORMAT where a decoder raised a format error (it takes precedence, as in
 *     density_hip_decode_device; *damaged_out and the verdicts are valid then as well and say what survived).
 *   - an unsealed container has no trailer to hold the chunks against: DENSITY_HIP_ERR_ARGUMENT, nothing written.  So are unknown bits in `flags`.  A header or
 *     trailer that does not fit container_size is DENSITY_HIP_ERR_FORMAT at once; a container of zero chunks DENSITY_HIP_OK with a count of 0.
 * density_hip_decode_verdicts is the host-pointer form, staged whole like every sealed container: `verdicts` (HOST, verdict_capacity >= n_chunks words) and
 * *damaged_out (optional) are filled, and it returns total_len if at least one chunk is intact and no argument or capacity error occurred, else 0;
 * density_hip_last_error() says how many chunks were damaged ("" for an intact container).
 * Profiling marks: those of a sealed density_hip_decode_device, then "chunk_verdicts" and, when blanking runs, "blank_chunks". */
#define DENSITY_HIP_CHUNK_DAMAGED 1u
#define DENSITY_HIP_SALVAGE_BLANK 1u   /* flags: zero the output region of every damaged chunk */
int density_hip_decode_device_verdicts(const void* d_container, size_t container_size, const density_hip_header_t* header, void* d_output,
                                       size_t output_capacity, void* d_workspace, size_t workspace_size, void* stream, uint32_t* d_verdicts,
                                       unsigned flags, uint32_t* damaged_out);
size_t density_hip_decode_verdicts(const uint8_t* container, size_t container_size, uint8_t* output, size_t output_size, uint32_t* verdicts,
                                   size_t verdict_capacity, unsigned flags, uint32_t* damaged_out);

/* Recovery records: the parity blob "DHP1" and the decode that rebuilds damaged chunks from it.
 * The blob is a SIDECAR: it is not part of any container, no container flag announces it, and every call above behaves as it does without one.  It holds
 * n_groups XOR rows over the INPUT's chunks, interleaved so that adjacent chunks lie in different groups.  Layout (little-endian):
 *     [0,32)                          density_hip_parity_header_t
 *     [32, 32 + n_groups * row_bytes)  row 0, row 1, ...
 * row_bytes = round_up(min(chunk_size, total_len), 16); n_groups = min(requested, n_chunks); row g = XOR of the input chunks i with i % n_groups == g, each
 * zero-padded to row_bytes.  The blob depends on the input, chunk_size and n_groups alone — not on the algorithm, not on the container's form — so one blob
 * serves the packed, slotted and paged containers of all three algorithms made from that input with that chunk size.  An input of zero bytes gives a bare
 * header with n_groups 0.  The rows carry no checksum of their own: a rebuilt chunk is accepted only against the container's trailer, so a damaged row
 * cannot pass wrong bytes.  A chunk can be rebuilt as long as it is the only damaged chunk of its group: with G groups any burst of up to G neighbouring
 * chunks is recovered whole.  (A CPU reader rebuilds chunk k the same way: INTEGRATION.md.)
 *   density_hip_parity_size: the exact blob size; 0 for an invalid chunk_size — 0 included: pass the chunk size the container has, from its header or from
 *     density_hip_auto_chunk_for() — or for n_groups == 0 with a non-empty input.  Pure host arithmetic.
 *   density_hip_parity_device: the blob of a device buffer, asynchronous on `stream`; d_input and d_parity at any byte alignment.  A parity_capacity below
 *     density_hip_parity_size() is DENSITY_HIP_ERR_CAPACITY at once, nothing written.  Profiling mark: "parity_rows".
 *   density_hip_parity: the same on host pointers, staged whole; returns the bytes written, 0 on failure.
 *
 * Version 2 of the blob ("double parity") adds a second row per group over GF(2^8), as the Q of a P+Q RAID-6, so that any TWO damaged chunks of a group can be
 * rebuilt.  The header is the same 32 bytes with version 2 (reserved0 and reserved1 stay 0); with G = n_groups:
 *     [0,32)                                   density_hip_parity_header_t, version 2
 *     [32, 32 + G * row_bytes)                 P rows: byte for byte the rows of the version-1 blob of the same (input, chunk_size, n_groups)
 *     [32 + G * row_bytes, 32 + 2*G*row_bytes) Q rows
 * row_bytes, the clamp of n_groups and the zero padding are those of version 1.  Chunk i, a member of group g = i % G, has the place j = i / G in its group;
 * Q row g = XOR over the group's members of 2^j · D_i, where D_i is chunk i zero-padded to row_bytes and the product is taken bytewise in GF(2^8) with the
 * polynomial 0x11D and the generator 2.  Since 2^255 = 1 a group has at most 255 members: ceil(n_chunks / n_groups) > 255 is invalid geometry.  An input of
 * zero bytes gives a bare header with version 2 and n_groups 0.  (How a CPU reader rebuilds one chunk and two: INTEGRATION.md.)
 *   density_hip_parity2_size / density_hip_parity2_device / density_hip_parity2 mirror the three calls above — arguments, return convention, any alignment,
 *     asynchrony, refusals —; the size is also 0, and the device call DENSITY_HIP_ERR_ARGUMENT, for a group of more than 255 members.  Profiling mark: "parity2_rows".
 * Out of scope: a second attempt through Q for a single damaged chunk whose P row is itself damaged (one damaged chunk is rebuilt from P, Q is not read);
 * three or more damaged chunks in one group; any container flag announcing a blob of either version. */
#define DENSITY_HIP_PARITY_MAGIC 0x31504844u /* "DHP1" */
typedef struct density_hip_parity_header {
    uint32_t magic;          /* DENSITY_HIP_PARITY_MAGIC */
    uint8_t  version;        /* 1: P rows; 2: P rows, then Q rows */
    uint8_t  reserved0;      /* 0 */
    uint16_t reserved1;      /* 0 */
    uint32_t chunk_size;     /* of the input's cut, and of every container the blob serves */
    uint32_t n_chunks;       /* ceil(total_len / chunk_size) */
    uint64_t total_len;      /* bytes of input */
    uint32_t n_groups;       /* rows in the blob (version 2: of each kind): 1 .. n_chunks (0 for an empty input) */
    uint32_t row_bytes;      /* round_up(min(chunk_size, total_len), 16) */
} density_hip_parity_header_t;
size_t density_hip_parity_size(size_t input_size, size_t chunk_size, uint32_t n_groups);
int density_hip_parity_device(const void* d_input, size_t input_size, size_t chunk_size, uint32_t n_groups, void* d_parity, size_t parity_capacity, void* stream);
size_t density_hip_parity(const uint8_t* input, size_t input_size, size_t chunk_size, uint32_t n_groups, uint8_t* parity, size_t parity_capacity);
size_t density_hip_parity2_size(size_t input_size, size_t chunk_size, uint32_t n_groups);
int density_hip_parity2_device(const void* d_input, size_t input_size, size_t chunk_size, uint32_t n_groups, void* d_parity, size_t parity_capacity, void* stream);
size_t density_hip_parity2(const uint8_t* input, size_t input_size, size_t chunk_size, uint32_t n_groups, uint8_t* parity, size_t parity_capacity);
/* Parity update: a blob kept current after its input was edited or appended to (a join that replaces chunk k or appends: above), without reading the input again.
 * The blob is a linear code over the zero-padded input — P row g the XOR of its group's chunks, Q row g the XOR of 2^place · chunk — so an edit's effect on it is
 * the same code applied to old ^ new, and only the rows of the chunks the edit covers are touched.
 * The blob at d_parity (version 1 or 2, as its header says) is the blob of some input I; bytes [offset, offset + old_size) of I held `old`; they now hold `new`,
 * new_size bytes long; the blob is updated in place.  Two shapes of edit are valid, and both may hold at once:
 *   - same size: old_size == new_size and offset + old_size <= total_len — any byte offset and length, chunk-aligned or not;
 *   - tail: offset + old_size == total_len — the input's tail from `offset` on is replaced by `new`, total_len becomes offset + new_size: append (old_size == 0, also
 *     onto a ragged last chunk), truncation (new_size == 0), a tail of one length replaced by one of another.  The shorter of the two counts as zero-padded, which
 *     is exact: the blob pads with zeros.
 * The result is byte for byte what density_hip_parity_device / density_hip_parity2_device writes for the edited input with the blob's own chunk_size and n_groups;
 * n_chunks and total_len of the header are rewritten on the device.  Rows no touched chunk belongs to are not written; inside touched rows only positions the
 * edit covers can change.  Every 16-byte slot of a row is read, changed and written by one lane: no atomics, the same bytes every time.
 * The call CANNOT CHECK `old`: with a wrong `old` the blob becomes a wrong blob — which, as ever, cannot pass wrong bytes: every rebuild is held against the
 * container's trailer, and the chunk stays DENSITY_HIP_CHUNK_DAMAGED.
 *   density_hip_parity_update_header: host arithmetic only, the one place the geometry rules live: *header_out (optional) = the header the blob has after the
 *     edit.  DENSITY_HIP_OK, or DENSITY_HIP_ERR_ARGUMENT: a header that is not a blob's; an edit that is neither shape; offset + new_size overflowing or giving
 *     more than 2^32 - 1 chunks; an edited input whose blob would not have this blob's geometry — fewer chunks than n_groups (shrinking to empty; growing an
 *     empty blob, whose n_groups is 0) or round_up(min(chunk_size, new total_len), 16) != row_bytes (a one-chunk input shorter than chunk_size changing length
 *     beyond its row): make a new blob —; version 2: a group growing beyond 255 members.
 *   density_hip_parity_update_device: d_parity, d_old, d_new on the device at any byte alignment, none overlapping another; parity_header: optional HOST copy of the
 *     blob's first 32 bytes (NULL: read back, one small synchronous copy); header_out: optional HOST pointer, filled by host arithmetic — it never makes the call
 *     synchronise.  With parity_header the call is fully asynchronous on `stream`.
 *   - DENSITY_HIP_ERR_ARGUMENT, nothing written, no device work — with parity_header decided before any device is acquired: NULL d_parity, NULL d_old with
 *     old_size > 0, NULL d_new with new_size > 0, and whatever density_hip_parity_update_header refuses.
 *   - DENSITY_HIP_ERR_FORMAT, nothing written: the header checks of density_hip_decode_device_recover — magic, version, n_groups outside 1 .. n_chunks, a row_bytes
 *     that is not the formula's, a parity_size short of header plus rows (version 2: both kinds of rows), a version-2 header with groups of more than 255.
 *   - old_size == new_size == 0: DENSITY_HIP_OK, nothing launched.
 *   density_hip_parity_update: the host-pointer form, staged whole; returns the blob's size, 0 on failure with density_hip_last_error() set.
 * Profiling mark: "parity_update".
 * Out of scope: edits that insert or delete in the middle (every later chunk changes group and place); changing a blob's n_groups or chunk_size; slicing a blob. */
int density_hip_parity_update_header(const density_hip_parity_header_t* header, uint64_t offset, size_t old_size, size_t new_size,
                                     density_hip_parity_header_t* header_out);
int density_hip_parity_update_device(void* d_parity, size_t parity_size, const density_hip_parity_header_t* parity_header,
                                     uint64_t offset, const void* d_old, size_t old_size, const void* d_new, size_t new_size,
                                     void* stream, density_hip_parity_header_t* header_out);
size_t density_hip_parity_update(uint8_t* parity, size_t parity_size, uint64_t offset, const uint8_t* old_data, size_t old_size,
                                 const uint8_t* new_data, size_t new_size);
/* density_hip_decode_device_recover runs density_hip_decode_device_verdicts unchanged (the same kernels, the same workspace rules and sizes) and then, with the blob:
 *   - rebuild: for every group with exactly ONE damaged member k, chunk k's region of d_output is replaced by row g XOR the regions of the group's other
 *     members (the last chunk at its true length; no byte past total_len is written);
 *   - re-verify: chunk k is summed again and held against trailer entry k: a match makes its verdict DENSITY_HIP_CHUNK_RECOVERED, anything else (a damaged
 *     row, a damaged trailer entry) leaves it DENSITY_HIP_CHUNK_DAMAGED;
 *   - groups with two or more damaged members are left alone; DENSITY_HIP_SALVAGE_BLANK then zeroes whatever is STILL damaged.
 * With a version-2 blob a group with exactly TWO damaged members, at places a < b, is rebuilt as well: over the group's intact members (neither damaged region is
 * read) Pxy = P row ^ XOR D_j and Qxy = Q row ^ XOR 2^j · D_j, then with d = 2^(b-a) ^ 1:  D_a = (2^(b-a) / d) · Pxy ^ (2^(-a) / d) · Qxy,  D_b = Pxy ^ D_a, each
 * written at its true length.  Each of the two is summed and held against its OWN trailer entry, so one may become RECOVERED while the other stays DAMAGED.  A
 * group with one damaged member is rebuilt from its P row as with version 1 (Q is not read); groups with three or more are left alone.
 * So a verdict is not DENSITY_HIP_CHUNK_DAMAGED if and only if the region's bytes have the trailer's checksum.  *damaged_out = chunks still damaged,
 * *recovered_out = chunks rebuilt (both HOST, each optional; with either the call synchronises `stream`, with both NULL it is fully asynchronous and leaves the
 * two counts in the second and third 32-bit word of d_workspace where the caller passed one).  Returns DENSITY_HIP_OK when no chunk remains damaged — also where
 * a decoder raised a format error on the way: every chunk's content has been verified —, otherwise DENSITY_HIP_ERR_FORMAT if a decoder raised one, otherwise
 * DENSITY_HIP_ERR_CHECKSUM.
 *   - d_parity / parity_size: the blob on the device, at any byte alignment; parity_header: optional HOST copy of its first 32 bytes (NULL: read back, one
 *     small synchronous copy).
 *   - DENSITY_HIP_ERR_ARGUMENT, nothing written: an unsealed container, unknown bits in `flags`, a parity header whose chunk_size / n_chunks / total_len are not
 *     the container's.  DENSITY_HIP_ERR_FORMAT, nothing written: a wrong magic or version, n_groups outside 1 .. n_chunks, a row_bytes that is not the
 *     formula's, a parity_size short of header plus rows (version 2: plus both kinds of rows), a version-2 header with groups of more than 255 members.
 * density_hip_decode_recover is the host-pointer form, shaped like density_hip_decode_verdicts: it returns total_len if at least one chunk is not damaged and no
 * argument or capacity error occurred, else 0.
 * Profiling marks: those of density_hip_decode_device_verdicts up to "chunk_verdicts", then "recover_rebuild", "recover_verify" and, when blanking runs, "blank_chunks". */
#define DENSITY_HIP_CHUNK_RECOVERED 2u
int density_hip_decode_device_recover(const void* d_container, size_t container_size, const density_hip_header_t* header, const void* d_parity, size_t parity_size,
                                      const density_hip_parity_header_t* parity_header, void* d_output, size_t output_capacity, void* d_workspace,
                                      size_t workspace_size, void* stream, uint32_t* d_verdicts, unsigned flags, uint32_t* damaged_out, uint32_t* recovered_out);
size_t density_hip_decode_recover(const uint8_t* container, size_t container_size, const uint8_t* parity, size_t parity_size, uint8_t* output, size_t output_size,
                                  uint32_t* verdicts, size_t verdict_capacity, unsigned flags, uint32_t* damaged_out, uint32_t* recovered_out);

/* Device-resident single reference stream (the format of section 1, device pointers).  `size_out` is a HOST
 * pointer and must be non-NULL: the call synchronises `stream`. */
int density_hip_stream_encode_device(int algo, const void* d_input, size_t input_size, void* d_output,
                                     size_t output_capacity, void* stream, size_t* size_out);
int density_hip_stream_decode_device(int algo, const void* d_input, size_t input_size, void* d_output,
                                     size_t output_capacity, void* stream, size_t* size_out);

/* Profiling: when enabled, the device entry points bracket each kernel with HIP events on the launch stream.
 * density_hip_last_timings() synchronises the last event and returns the duration of every kernel launched on the
 * current device since the previous density_hip_last_timings() call (at most 8192 marks are kept), in launch order;
 * names[i] points to a static string.  Returns the number of entries written (<= capacity).  (The pipelined host-pointer container calls
 * run their slices on streams of their own and record no marks.) */
void density_hip_set_profiling(int enabled);
int density_hip_last_timings(float* milliseconds, const char** names, int capacity);

/* Test hook: how the reference-shaped Chameleon stream calls of a few MiB and more were served so far (process-wide counters):
 * out4[0] streams encoded in parallel segments, [1] passes those encodes took (1 per stream if every speculation held),
 * [2] streams decoded in parallel segments, [3] long streams decoded sequentially (mostly raw copies, or buffers the parallel path does not take). */
void density_hip_stream_stats(uint64_t* out4);
/* ... how many Cheetah decodes the decode passes (decode_passes.hip) have served so far (process-wide) ... */
uint64_t density_hip_decode_pass_count(void);
/* ... and of Cheetah container encodes under kernel variant bit 64: out2[0] chunks that went through the exchange passes, [1] how many
 * of them were handed back to the in-order kernel (raw-copy blocks, a ragged end). */
void density_hip_stage_stats(uint64_t* out2);

/* Test hook, bit mask: 1 = force the simple one-wavefront-per-chunk kernels, 2 = encode containers without the block index,
 * 4 = force the 16-wave role pipelines (chameleon.hip) instead of the default wave-rotation kernels (rotor.hip),
 * 8 = encode in batches with the stitch of one batch beside the encoding of the next, 16 = Cheetah / Lion on the
 * one-lane-per-stream kernels instead of the one-wave-per-stream kernels (serial_codec.hip), 32 = Cheetah containers on the
 * one-wave-per-stream encoder instead of the exchange passes (exchange_stages.hip), 64 = count the chunks the exchange passes
 * keep / hand back (density_hip_stage_stats; reads the verdicts back, so the encode call synchronises), 128 = Cheetah containers on the
 * one-wave-per-stream decoder instead of the decode passes (decode_passes.hip), 256 = the host-pointer container calls pipelined
 * whatever the size, a slice per chunk, 512 = never pipelined (below; the reference symbols on long streams too), 1024 = Cheetah's decode passes find
 * a chunk's records by the one-wave walk alone (no window kernels), 2048 = the other rotation encoder (8 chain + 8 emit waves),
 * 4096 / 8192 / 16384 = reserved (they selected one-wave forms of the walk over Cheetah's contexts, which are gone: accepted, and select nothing),
 * 32768 = Lion's container decode on one wave per stream (round 4's) instead of two.
 * Payload bytes are identical in every variant. */
void density_hip_set_kernel_variant(int variant);

/* Runs the LDS ordering self-tests the kernels rely on (also run lazily before first use). 0 = the library can run.
 * density_hip_selftest_bits() returns the raw failure mask (0 = everything passed, -1 = no usable device): bits 0..7 plain 16-bit
 * LDS write order (fatal), bits 8..11 lane order of the ordered exchange ds_mskor_rtn_b32 (only the one-wavefront kernels run),
 * bits 12..13 lane-reversed rollback / token hand-off behind the exchanges (the 16-wave role pipelines run instead of the
 * wave-rotation kernels). */
int density_hip_selftest(void);
int density_hip_selftest_bits(void);
/*
 * Multi-GPU placement (the arithmetic of density_amd/parallel.py for callers below Python).  The path shards by chunks with no
 * data-path collective: rank g of G encodes the chunk range density_hip_shard_range() gives it into a container of its own; ONE all-gather of
 * three u64 per rank — {chunks, payload bytes, input bytes} of the local container, the caller's collective (RCCL ncclAllGather over xGMI) —
 * then tells every rank, through density_hip_global_layout(), where its size-table entries, its block-index slice and its payload region sit in the
 * global container (every shard but the last covers whole chunks, so index slices concatenate; every payload region but the last non-empty one
 * is padded to 16 bytes).  Pure host arithmetic: no device, no HIP call.  Both return DENSITY_HIP_OK or DENSITY_HIP_ERR_ARGUMENT.
 */
typedef struct density_hip_shard {
    uint64_t chunk_first, chunk_end;   /* chunks [first, end) of the global input: contiguous, balanced to within one chunk */
    uint64_t byte_first, byte_end;     /* the same range in input bytes (chunk-aligned; the last shard ends at total_len) */
} density_hip_shard_t;
int density_hip_shard_range(size_t total_len, size_t chunk_size, uint32_t rank, uint32_t world, density_hip_shard_t* out);
typedef struct density_hip_global_layout {
    uint64_t n_chunks, total_len;                       /* of the global container */
    uint64_t index_at, index_bytes, payload_at;         /* its block index (index_bytes == 0 without DENSITY_HIP_FLAG_BLOCK_INDEX) and payload area */
    uint64_t container_len;
    uint64_t chunk_offset, payload_offset, input_offset; /* of `rank`: first size-table entry; bytes from payload_at; input bytes before it */
    uint64_t payload_bytes_padded;                      /* this rank's payload region as it sits in the global container */
} density_hip_global_layout_t;
int density_hip_global_layout(const uint64_t* chunks, const uint64_t* payload_bytes, const uint64_t* input_bytes, uint32_t world, uint32_t rank,
                              uint32_t flags, density_hip_global_layout_t* out);
/* (Sealed shards are not stitched: a flag word with DENSITY_HIP_FLAG_CHECKSUM, or any bit that is no container flag, is DENSITY_HIP_ERR_ARGUMENT.  Sealed
 * blobs travel whole in a DHCM super-container, below: a blob's length includes its trailer, and every blob is verified when it is decoded.) */

/* The content checksum C of a sealed container's chunk (DENSITY_HIP_FLAG_CHECKSUM above) on the HOST: pure arithmetic, no device, no HIP call.  What a CPU
 * reader links: decode chunk i with the crate, then compare density_hip_checksum32(chunk, len) with trailer entry i. */
uint32_t density_hip_checksum32(const uint8_t* data, size_t size);
/* Upper bound of what sealing adds to any density_hip_container_bound*(): 16 + round_up(4 * n_chunks, 16); 0 for invalid geometry.  chunk_size 0 = the
 * automatic chunk; that depends on the algorithm, which this call does not take, so it counts the chunks of the SMALLEST automatic chunk any algorithm
 * picks (64 KiB): an upper bound for all three. */
size_t density_hip_seal_overhead(size_t input_size, size_t chunk_size);

/*
 * Config 5's wire form: the MULTI-RANK container "DHCM" (round 6).  Every rank's own container — packed, slotted or PAGED, whatever the rank made: each is a
 * self-describing DHC1 blob of that rank's shard — travels as it stands; a 32-byte super-header and one 24-byte row per rank say where each blob lies:
 *
 *     [0,32)               density_hip_multi_header_t {magic "DHCM", version 1, algo, flags 0, n_ranks, chunk_size, total_len, container_len}
 *     [32, 32 + 24 R)      per rank {offset, length, input_bytes}: the blob's place from the start of the super-container (256-byte aligned), its length,
 *                          the input bytes it decodes to (rank r's output starts at the sum of the input_bytes before it)
 *     (256-byte aligned)   blob 0, blob 1, ...
 *
 * The only collective is still one all-gather of two u64 per rank {container length, input bytes} (ncclAllGather over xGMI); density_hip_multi_layout() then
 * gives every rank its row and the super-container's length — a rank can write its blob at its offset of a shared file, or send it there (parallel.py:
 * concat_multi_to_rank0).  A reader decodes blob by blob (density_hip_decode / _decode_device per row).  There is nothing in the reference to match (its
 * stream is one chain, codec/codec.rs:72-80).  Pure host arithmetic.
 */
#define DENSITY_HIP_MULTI_MAGIC 0x4D434844u /* "DHCM" little-endian */
typedef struct density_hip_multi_header {
    uint32_t magic;
    uint8_t version, algo;
    uint16_t flags;
    uint32_t n_ranks, chunk_size;
    uint64_t total_len, container_len;
} density_hip_multi_header_t;
typedef struct density_hip_multi_row { uint64_t offset, length, input_bytes; } density_hip_multi_row_t;
/* rows[r] for every rank and the header (algo / chunk_size as given) from the gathered {length, input_bytes}; returns DENSITY_HIP_OK or _ERR_ARGUMENT */
int density_hip_multi_layout(const uint64_t* lengths, const uint64_t* input_bytes, uint32_t n_ranks, int algo, size_t chunk_size,
                             density_hip_multi_header_t* header_out, density_hip_multi_row_t* rows_out);
/* Validates a super-container's front matter (magic, version, rows inside the container, in order, not overlapping, input bytes adding up) and copies
 * row `rank` out; container_size = bytes available.  DENSITY_HIP_OK / _ERR_FORMAT / _ERR_ARGUMENT. */
int density_hip_multi_row(const void* front, size_t front_size, size_t container_size, uint32_t rank, density_hip_multi_header_t* header_out, density_hip_multi_row_t* row_out);

/* Releases what the library holds on every device it has used (staging buffers, workspaces, streams, events); the next call sets them up
 * again.  Not needed for correctness — a process may simply exit — and must not run beside other calls into the library. */
void density_hip_shutdown(void);

/* Thread-local description of the last failure in this thread ("" if none). */
const char* density_hip_last_error(void);
/* "density_hip <version> (gfx950; reference: density-rs 0.16.6; kernels <id>)": <id> is a hash of the kernel sources the library was built from. */
const char* density_hip_version(void);

#ifdef __cplusplus
}
#endif
#endif /* DENSITY_HIP_H */
