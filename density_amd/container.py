"""Chunked container API (include/density_hip.h section 2): the data-parallel path.

Host-buffer calls stage through device memory; the *_device calls take device pointers (e.g. torch CUDA tensors'
data_ptr()) and a HIP stream handle and enqueue kernels only.
"""
import ctypes

from . import _lib
from .codec import ChecksumError, DecodeError, EncodeError, _ro, _rw


def container_bound(algo, input_size, chunk_size=0):
    return _lib.lib().density_hip_container_bound(_lib.ALGO_IDS[algo], input_size, chunk_size)


def encode(algo, input, output, chunk_size=0):
    ia, n, k1 = _ro(input)
    oa, cap, k2 = _rw(output)
    r = _lib.lib().density_hip_encode(_lib.ALGO_IDS[algo], ia, n, oa, cap, chunk_size)
    if r == 0:
        raise EncodeError(_lib.last_error())
    return r


def decoded_size(container):
    ia, n, k = _ro(container)
    return _lib.lib().density_hip_decoded_size(ia, n)


def decode(container, output):
    ia, n, k1 = _ro(container)
    oa, cap, k2 = _rw(output)
    r = _lib.lib().density_hip_decode(ia, n, oa, cap)
    if r == 0 and _lib.last_error():          # 0 with no error == a valid, empty container
        raise (ChecksumError if _lib.last_error().startswith("checksum") else DecodeError)(_lib.last_error())
    return r


def parse_header(raw32):
    h = _lib.Header.from_buffer_copy(bytes(raw32[:32]))
    return h


FLAG_BLOCK_INDEX = 1
FLAG_SLOTTED = 2
FLAG_PAGED = 4
FLAG_CHECKSUM = 8
PAGE_BYTES = 65536


def slot_stride(algo, chunk_size):
    """Distance between the payload slots of a slotted container (include/density_hip.h: DENSITY_HIP_FLAG_SLOTTED)."""
    safe = getattr(_lib.lib(), f"{algo}_safe_encode_buffer_size")(chunk_size)
    return (safe + 255) // 256 * 256


def block_index(container):
    """The container's block index (bytes, one per 256-byte input block) or None."""
    b = bytes(container)
    h = parse_header(b)
    if not (h.flags & FLAG_BLOCK_INDEX):
        return None
    base = (32 + 4 * h.n_chunks + 15) // 16 * 16
    return b[base:base + (h.total_len + 255) // 256]


def chunk_payloads(container):
    """Splits a host-resident container into its per-chunk reference streams (for parity checks)."""
    b = bytes(container)
    h = parse_header(b)
    sizes = [int.from_bytes(b[32 + 4 * i:36 + 4 * i], "little") for i in range(h.n_chunks)]
    off = (32 + 4 * h.n_chunks + 15) // 16 * 16
    if h.flags & FLAG_BLOCK_INDEX:
        off = (off + (h.total_len + 255) // 256 + 15) // 16 * 16
    if h.flags & FLAG_PAGED:
        # a chunk's stream = the used bytes of its pages, in directory order (include/density_hip.h): what a CPU reader does before it calls the crate
        ppc = int(_lib.lib().density_hip_paged_pages_per_chunk(h.chunk_size))
        pages_base = (off + 16 * (ppc + 1) * h.n_chunks + 255) // 256 * 256
        out = []
        for i, s in enumerate(sizes):
            d = off + 16 * (ppc + 1) * i
            n_pages = int.from_bytes(b[d:d + 4], "little")
            parts = []
            for k in range(n_pages):
                e = d + 16 * (k + 1)
                page, used = int.from_bytes(b[e:e + 4], "little"), int.from_bytes(b[e + 8:e + 12], "little")
                parts.append(b[pages_base + page * PAGE_BYTES:pages_base + page * PAGE_BYTES + used])
            stream = b"".join(parts)
            assert len(stream) == s, f"chunk {i}: the directory's bytes ({len(stream)}) are not the size table's ({s})"
            out.append(stream)
        return h, out
    out = []
    stride = slot_stride(_lib.ALGO_NAMES[h.algo], h.chunk_size) if h.flags & FLAG_SLOTTED else 0
    for i, s in enumerate(sizes):
        if stride:
            out.append(b[off + i * stride:off + i * stride + s])
        else:
            out.append(b[off:off + s])
            off = (off + s + 15) // 16 * 16
    return h, out


def _check(rc, exc):
    if rc == _lib.ERR_CHECKSUM:
        raise ChecksumError(f"density_hip error {rc}: {_lib.last_error()}")
    if rc != _lib.OK:
        raise exc(f"density_hip error {rc}: {_lib.last_error()}")


def checksum32(data):
    """The content checksum C of a sealed container's chunk (include/density_hip.h: DENSITY_HIP_FLAG_CHECKSUM), computed on the host."""
    ia, n, k = _ro(data)
    return int(_lib.lib().density_hip_checksum32(ia, n))


def seal_overhead(input_size, chunk_size=0):
    """Upper bound of what sealing adds to any container_bound*()."""
    return int(_lib.lib().density_hip_seal_overhead(input_size, chunk_size))


def chunk_checksums(container):
    """The trailer of a host-resident sealed container, one checksum per chunk, or None where the container is not sealed."""
    b = bytes(container)
    h = parse_header(b)
    if not (h.flags & FLAG_CHECKSUM):
        return None
    at = h.container_len - (4 * h.n_chunks + 15) // 16 * 16
    return [int.from_bytes(b[at + 4 * i:at + 4 * i + 4], "little") for i in range(h.n_chunks)]


def encode_sealed(algo, input, output, chunk_size=0):
    """As encode, sealed on the device before the copy down: the packed container with its trailer of content checksums."""
    ia, n, k1 = _ro(input)
    oa, cap, k2 = _rw(output)
    r = _lib.lib().density_hip_encode_sealed(_lib.ALGO_IDS[algo], ia, n, oa, cap, chunk_size)
    if r == 0:
        raise EncodeError(_lib.last_error())
    return r


def checksum_device(d_data, n, chunk_size, d_sums, stream=0):
    """Enqueue the checksums of every chunk_size bytes of device memory into d_sums (u32 per chunk, cleared by the call)."""
    _check(_lib.lib().density_hip_checksum_device(d_data, n, chunk_size, d_sums, stream), EncodeError)


def seal_device(d_in, n, d_container, cap, header=None, stream=0, want_header=True):
    """Seal, in place, the container an encode_device* call has just written for d_in.  Returns the sealed header (synchronises) or None."""
    hdr = _lib.Header() if want_header else None
    rc = _lib.lib().density_hip_seal_device(d_in, n, d_container, cap, ctypes.byref(header) if header is not None else None, stream,
                                            ctypes.byref(hdr) if want_header else None)
    _check(rc, EncodeError)
    return hdr


def encode_device(algo, d_in, n, d_out, cap, chunk_size=0, stream=0, workspace=(0, 0), want_header=True):
    """Enqueue a container encode of device memory.  Returns the header (synchronises) or None."""
    hdr = _lib.Header() if want_header else None
    rc = _lib.lib().density_hip_encode_device(_lib.ALGO_IDS[algo], d_in, n, d_out, cap, chunk_size, workspace[0], workspace[1], stream,
                                              ctypes.byref(hdr) if want_header else None)
    _check(rc, EncodeError)
    return hdr


def container_bound_slotted(algo, input_size, chunk_size=0):
    return _lib.lib().density_hip_container_bound_slotted(_lib.ALGO_IDS[algo], input_size, chunk_size)


def encode_device_slotted(algo, d_in, n, d_out, cap, chunk_size=0, stream=0, workspace=(0, 0), want_header=True):
    """As encode_device, but every chunk stream stays in its slot inside the container (no stitch pass): DENSITY_HIP_FLAG_SLOTTED."""
    hdr = _lib.Header() if want_header else None
    rc = _lib.lib().density_hip_encode_device_slotted(_lib.ALGO_IDS[algo], d_in, n, d_out, cap, chunk_size, workspace[0], workspace[1], stream,
                                                      ctypes.byref(hdr) if want_header else None)
    _check(rc, EncodeError)
    return hdr


def container_bound_paged(algo, n, chunk_size=0):
    return int(_lib.lib().density_hip_container_bound_paged(_lib.ALGO_IDS[algo], n, chunk_size))


def encode_device_paged(algo, d_in, n, d_out, cap, chunk_size=0, stream=0, workspace=(0, 0), want_header=True):
    """As encode_device, but wire-ready WITHOUT a stitch pass: the streams in pages taken from one counter (DENSITY_HIP_FLAG_PAGED; what the paged form
    is not for comes out slotted: see the header's flags)."""
    hdr = _lib.Header() if want_header else None
    rc = _lib.lib().density_hip_encode_device_paged(_lib.ALGO_IDS[algo], d_in, n, d_out, cap, chunk_size, workspace[0], workspace[1], stream,
                                                    ctypes.byref(hdr) if want_header else None)
    _check(rc, EncodeError)
    return hdr


def pack_device(d_container, container_size, d_out, cap, header=None, stream=0, workspace=(0, 0), want_header=True):
    """Slotted container -> packed container (the wire form).  Returns the packed container's header (synchronises) or None."""
    hdr = _lib.Header() if want_header else None
    rc = _lib.lib().density_hip_pack_device(d_container, container_size, ctypes.byref(header) if header is not None else None, d_out, cap,
                                            workspace[0], workspace[1], stream, ctypes.byref(hdr) if want_header else None)
    _check(rc, EncodeError)
    return hdr


def unpage_device(d_container, container_size, d_out, cap, header=None, stream=0, workspace=(0, 0), want_header=True):
    """Paged container (sealed or not) -> packed container, on the device: byte for byte what encode_device (+ seal_device) writes for the same input.
    Returns the packed container's header (synchronises) or None."""
    hdr = _lib.Header() if want_header else None
    rc = _lib.lib().density_hip_unpage_device(d_container, container_size, ctypes.byref(header) if header is not None else None, d_out, cap,
                                              workspace[0], workspace[1], stream, ctypes.byref(hdr) if want_header else None)
    _check(rc, EncodeError)
    return hdr


def unpage(blob):
    """Paged container (bytes or uint8 array, sealed or not) -> the packed container as a uint8 array, on the HOST: what unpage_device does, stated in
    numpy.  Header with the PAGED flag dropped, size table and block index as they stand, every chunk's stream — the used bytes of its pages in
    directory order — at the next 16-byte boundary behind the one before (zeros between), container_len where the last one ends; a sealed container's
    trailer follows at the next 16-byte boundary.  Raises ValueError for what is not a paged container and for a directory that cannot be followed."""
    import numpy as np
    src = np.frombuffer(bytes(blob), dtype=np.uint8) if isinstance(blob, (bytes, bytearray, memoryview)) else np.ascontiguousarray(blob, dtype=np.uint8).reshape(-1)
    if src.size < 32:
        raise ValueError("not a container")
    h = parse_header(src[:32].tobytes())
    nc = h.n_chunks
    sealed = bool(h.flags & FLAG_CHECKSUM)
    if h.magic != 0x31434844 or h.version != 1 or (h.flags & ~FLAG_CHECKSUM) != (FLAG_PAGED | FLAG_BLOCK_INDEX) or h.algo != _lib.ALGO_IDS["chameleon"]:
        raise ValueError("not a paged container")
    if h.chunk_size < 256 or h.chunk_size % 256 or nc != (h.total_len + h.chunk_size - 1) // h.chunk_size:
        raise ValueError("bad container header")
    ppc = int(_lib.lib().density_hip_paged_pages_per_chunk(h.chunk_size))
    dir_base = ((32 + 4 * nc + 15) // 16 * 16 + (h.total_len + 255) // 256 + 15) // 16 * 16
    pages_base = (dir_base + 16 * (ppc + 1) * nc + 255) // 256 * 256
    trailer = (4 * nc + 15) // 16 * 16 if sealed else 0
    body = h.container_len - trailer
    if h.container_len > src.size or body < pages_base or (body - pages_base) % PAGE_BYTES:
        raise ValueError("bad container header")
    n_pages = (body - pages_base) // PAGE_BYTES
    sizes = src[32:32 + 4 * nc].view("<u4").astype(np.int64)
    directory = src[dir_base:dir_base + 16 * (ppc + 1) * nc].view("<u4").astype(np.int64).reshape(nc, ppc + 1, 4)
    segments, at = [], dir_base                                  # (source offset, bytes, destination offset) of every page in use
    for i in range(nc):
        used = int(directory[i, 0, 0])
        if not 1 <= used <= ppc:
            raise ValueError(f"chunk {i}: {used} pages in the directory (1 .. {ppc})")
        pages, nbytes = directory[i, 1:used + 1, 0], directory[i, 1:used + 1, 2]
        if (pages >= n_pages).any():
            raise ValueError(f"chunk {i}: a page beyond the {n_pages} the container holds")
        if (nbytes > PAGE_BYTES).any():
            raise ValueError(f"chunk {i}: more than a page of bytes in a page")
        if int(nbytes.sum()) != int(sizes[i]):
            raise ValueError(f"chunk {i}: the directory's bytes ({int(nbytes.sum())}) are not the size table's ({int(sizes[i])})")
        length = min(h.chunk_size, h.total_len - i * h.chunk_size)
        if int(sizes[i]) > length + length // 256 * 8 + (8 if length % 256 else 0):
            raise ValueError(f"chunk {i}: a stream longer than the chunk's safe_encode_buffer_size")
        to = at
        for page, ln in zip(pages.tolist(), nbytes.tolist()):
            segments.append((pages_base + page * PAGE_BYTES, ln, to))
            to += ln
        end, at = to, (to + 15) // 16 * 16
    end = end if nc else dir_base
    total = ((end + 15) // 16 * 16 + trailer) if sealed else end
    out = np.zeros(total, dtype=np.uint8)
    out[32:dir_base] = src[32:dir_base]
    for frm, ln, to in segments:
        out[to:to + ln] = src[frm:frm + ln]
    if sealed:
        out[total - trailer:] = src[body:body + trailer]
    hdr = _lib.Header.from_buffer_copy(bytes(h))
    hdr.flags, hdr.container_len = h.flags & ~FLAG_PAGED, total
    out[:32] = np.frombuffer(bytes(hdr), dtype=np.uint8)
    return out


def chunk_range(header, offset, length):
    """(first chunk, chunk count, skip) of the chunks that cover input bytes [offset, offset + length) of the container `header` describes: the range starts
    `skip` bytes into what those chunks decode to.  Raises ValueError for length == 0, a range past total_len and a header that is not a container's."""
    first, count, skip = ctypes.c_uint32(0), ctypes.c_uint32(0), ctypes.c_uint64(0)
    if offset < 0 or length < 0 or offset >= 1 << 64 or length >= 1 << 64:
        raise ValueError(f"no chunk range for bytes [{offset}, {offset} + {length})")
    rc = _lib.lib().density_hip_chunk_range(ctypes.byref(header), offset, length, ctypes.byref(first), ctypes.byref(count), ctypes.byref(skip))
    if rc != _lib.OK:
        raise ValueError(f"no chunk range for bytes [{offset}, {offset} + {length}) of a container of {header.total_len} bytes")
    return first.value, count.value, skip.value


def slice_bound(header, first_chunk, chunk_count):
    """The capacity slice_device asks for; 0 for a window that is not inside the container's chunks."""
    if not (0 <= first_chunk < 1 << 32 and 0 <= chunk_count < 1 << 32):
        return 0
    return int(_lib.lib().density_hip_slice_bound(ctypes.byref(header), first_chunk, chunk_count))


def slice_device(d_container, container_size, first_chunk, chunk_count, d_out, cap, header=None, stream=0, workspace=(0, 0), want_header=True):
    """Chunks [first_chunk, first_chunk + chunk_count) of a container of any form (sealed or not) as a packed container of their own, on the device: for a
    container this library made, byte for byte what encode_device (+ seal_device) writes for that part of the input.  Returns the slice's header
    (synchronises, and a window the call cannot follow raises) or None."""
    if not (0 <= first_chunk < 1 << 32 and 0 <= chunk_count < 1 << 32):
        raise EncodeError(f"slice: no chunks [{first_chunk}, {first_chunk} + {chunk_count})")
    hdr = _lib.Header() if want_header else None
    rc = _lib.lib().density_hip_slice_device(d_container, container_size, ctypes.byref(header) if header is not None else None, first_chunk, chunk_count, d_out, cap,
                                             workspace[0], workspace[1], stream, ctypes.byref(hdr) if want_header else None)
    _check(rc, EncodeError)
    return hdr


def slice(container, first_chunk, chunk_count, output):
    """slice_device on host buffers, staged whole: returns the bytes written to `output` (at least slice_bound() bytes)."""
    ia, n, k1 = _ro(container)
    oa, cap, k2 = _rw(output)
    if not (0 <= first_chunk < 1 << 32 and 0 <= chunk_count < 1 << 32):
        raise EncodeError(f"slice: no chunks [{first_chunk}, {first_chunk} + {chunk_count})")
    r = _lib.lib().density_hip_slice(ia, n, first_chunk, chunk_count, oa, cap)
    if r == 0:
        raise EncodeError(_lib.last_error())
    return r


def _device_header(d_container):
    """The 32 bytes at a device address, read back through torch (on its current stream)."""
    import torch

    class _View:
        __cuda_array_interface__ = {"shape": (32,), "typestr": "|u1", "data": (int(d_container), False), "version": 2}
    return parse_header(bytes(torch.as_tensor(_View(), device="cuda").cpu().numpy()))


def decode_range_device(d_container, container_size, offset, length, header=None, stream=0, workspace=(0, 0)):
    """Input bytes [offset, offset + length) of a container on the device, from the chunks that cover them and no others: chunk_range, slice_device into a
    scratch tensor, decode_device of the slice into a tensor of the covering chunks' extent.  Returns the view [skip : skip + length] of that tensor (torch,
    uint8, on the current device).  Damage in chunks outside the range does not matter; a sealed container's chunks inside it are verified (ChecksumError).
    stream == 0 is the library's own stream, which is not ordered behind torch's: torch's current stream is synchronised first.  Raises ValueError for
    length == 0 and a range past the end, DecodeError for a container the calls refuse."""
    import torch
    if container_size < 32:
        raise DecodeError("not a container")
    if stream == 0:
        torch.cuda.current_stream().synchronize()
    h = header if header is not None else _device_header(d_container)
    first, count, skip = chunk_range(h, offset, length)
    cap = slice_bound(h, first, count)
    if cap == 0:
        raise DecodeError("bad container header")
    scratch = torch.empty(cap, dtype=torch.uint8, device="cuda")
    try:
        sh = slice_device(d_container, container_size, first, count, scratch.data_ptr(), cap, header=h, stream=stream, workspace=workspace)
    except EncodeError as e:
        raise DecodeError(str(e)) from None
    out = torch.empty(sh.total_len, dtype=torch.uint8, device="cuda")
    got = decode_device(scratch.data_ptr(), sh.container_len, out.data_ptr(), sh.total_len, header=sh, stream=stream, workspace=workspace)
    if got != sh.total_len:
        raise DecodeError(f"the slice decoded to {got} bytes, not {sh.total_len}")
    return out[skip:skip + length]


def decode_range(container, offset, length):
    """Input bytes [offset, offset + length) of a host-resident container, as a numpy uint8 array: chunk_range, slice, decode.  Raises as decode_range_device."""
    import numpy as np
    ia, n, k = _ro(container)
    if n < 32:
        raise DecodeError("not a container")
    h = parse_header(ctypes.string_at(ia, 32))
    first, count, skip = chunk_range(h, offset, length)
    cap = slice_bound(h, first, count)
    if cap == 0:
        raise DecodeError("bad container header")
    part = np.empty(cap, dtype=np.uint8)
    try:
        used = slice(container, first, count, part)
    except EncodeError as e:
        raise DecodeError(str(e)) from None
    sh = parse_header(part[:32].tobytes())
    out = np.empty(sh.total_len, dtype=np.uint8)
    if decode(part[:used], out) != sh.total_len:
        raise DecodeError(f"the slice did not decode to {sh.total_len} bytes")
    return out[skip:skip + length]


def _join_parts(parts, device):
    """The JoinPart array of [(container, container_size, header or None, first_chunk, chunk_count), ...] and what keeps its pointers alive.  A None header is read
    back from the device (device=True) or taken from the host array's first 32 bytes."""
    keep, arr = [], (_lib.JoinPart * max(len(parts), 1))()
    for i, (cont, size, header, first, count) in enumerate(parts):
        if not (0 <= first < 1 << 32 and 0 <= count < 1 << 32):
            raise EncodeError(f"join: no chunks [{first}, {first} + {count})")
        if device:
            addr = int(cont)
            if header is None and count and addr and size >= 32:
                header = _device_header(addr)
        else:
            addr, n, k = _ro(cont)
            keep.append(k)
            size = n if size is None else size
            if header is None and count and n >= 32:
                header = parse_header(ctypes.string_at(addr, 32))
        keep.append(header)
        arr[i] = _lib.JoinPart(addr, size, ctypes.pointer(header) if header is not None else None, first, count)
    return arr, keep


def join_bound(parts):
    """The capacity join_device asks for parts [(d_container, container_size, header, first_chunk, chunk_count), ...]; 0 for a list the call refuses on the host."""
    if not 0 < len(parts) <= _lib.JOIN_MAX_PARTS:
        return 0
    arr, keep = _join_parts(parts, True)
    return int(_lib.lib().density_hip_join_bound(arr, len(parts)))


def join_workspace_size(n_parts, n_chunks_out):
    return int(_lib.lib().density_hip_join_workspace_size(n_parts, n_chunks_out))


def join_device(parts, d_out, cap, stream=0, workspace=(0, 0), want_header=True):
    """Chunk windows of several containers as ONE packed container, on the device: parts = [(d_container, container_size, header or None, first_chunk,
    chunk_count), ...], each a window of a packed, slotted or paged container, sealed or not (all alike in algorithm, chunk size, block index and seal); a part
    with chunk_count == 0 is skipped.  For containers this library made, byte for byte what encode_device (+ seal_device) writes for the windows' inputs one
    behind the other.  A None header is read back first (on torch's current stream).  Returns the joined header (synchronises; a list the call refuses or
    cannot follow raises) or None."""
    if len(parts) > _lib.JOIN_MAX_PARTS:
        raise EncodeError(f"join: {len(parts)} parts, at most {_lib.JOIN_MAX_PARTS}")
    arr, keep = _join_parts(parts, True)
    hdr = _lib.Header() if want_header else None
    rc = _lib.lib().density_hip_join_device(arr, len(parts), d_out, cap, workspace[0], workspace[1], stream, ctypes.byref(hdr) if want_header else None)
    _check(rc, EncodeError)
    return hdr


def join(parts, output):
    """join_device on host arrays, staged whole: parts = [(container, first_chunk, chunk_count), ...]; returns the bytes written to `output`."""
    oa, cap, k2 = _rw(output)
    if len(parts) > _lib.JOIN_MAX_PARTS:
        raise EncodeError(f"join: {len(parts)} parts, at most {_lib.JOIN_MAX_PARTS}")
    arr, keep = _join_parts([(c, None, None, f, k) for c, f, k in parts], False)
    r = _lib.lib().density_hip_join(arr, len(parts), oa, cap)
    if r == 0:
        raise EncodeError(_lib.last_error())
    return r


def replace_chunks_device(d_container, container_size, first_chunk, d_new, new_size, d_out, cap, header=None, new_header=None, stream=0, workspace=(0, 0),
                          want_header=True):
    """Container A with its chunks from first_chunk on replaced by the chunks of container B (same algorithm, chunk size, block index and seal; B is typically
    the one-chunk container of a patched chunk): join(A[0, first), B, A[first + n_B, n_A)) into d_out.  B may reach or pass A's end — it is then the new end,
    and first_chunk == n_A appends — but a B that ends in a ragged chunk in front of chunks A keeps raises, as does a first_chunk behind A's end."""
    a = header if header is not None else _device_header(d_container)
    b = new_header if new_header is not None else _device_header(d_new)
    behind = first_chunk + b.n_chunks
    if not 0 <= first_chunk <= a.n_chunks:
        raise EncodeError(f"replace: no chunk {first_chunk} in a container of {a.n_chunks}")
    if behind < a.n_chunks and b.total_len != b.n_chunks * b.chunk_size:
        raise EncodeError("replace: the new chunks end in a ragged chunk, and chunks of the old container would follow it")
    parts = [(d_container, container_size, a, 0, first_chunk), (d_new, new_size, b, 0, b.n_chunks),
             (d_container, container_size, a, min(behind, a.n_chunks), max(a.n_chunks - behind, 0))]
    return join_device(parts, d_out, cap, stream=stream, workspace=workspace, want_header=want_header)


def decode_device(d_container, container_size, d_out, cap, header=None, stream=0, workspace=(0, 0), sync=True):
    size = ctypes.c_size_t(0)
    rc = _lib.lib().density_hip_decode_device(d_container, container_size, ctypes.byref(header) if header is not None else None, d_out, cap,
                                              workspace[0], workspace[1], stream, ctypes.byref(size) if sync else None)
    _check(rc, DecodeError)
    return size.value if sync else None


def decode_device_verdicts(d_container, container_size, d_out, cap, d_verdicts, header=None, stream=0, workspace=(0, 0), blank=True, sync=True):
    """decode_device of a SEALED container that keeps its output and says which chunks are damaged: d_verdicts (n_chunks u32 on the device) receives 0 for
    every chunk whose bytes in d_out have the trailer's checksum, _lib.CHUNK_DAMAGED for the others; with `blank` those chunks' bytes become zeros.
    Returns (return code, number of damaged chunks) — OK, ERR_CHECKSUM or ERR_FORMAT, each with valid verdicts — or None with sync=False (nothing is
    reported, the verdicts lie on the device).  Anything else (an unsealed container, a capacity) raises DecodeError."""
    damaged = ctypes.c_uint32(0)
    rc = _lib.lib().density_hip_decode_device_verdicts(d_container, container_size, ctypes.byref(header) if header is not None else None, d_out, cap,
                                                       workspace[0], workspace[1], stream, d_verdicts, _lib.SALVAGE_BLANK if blank else 0,
                                                       ctypes.byref(damaged) if sync else None)
    if rc not in (_lib.OK, _lib.ERR_CHECKSUM, _lib.ERR_FORMAT) or (rc == _lib.ERR_FORMAT and "chunks damaged" not in _lib.last_error()):
        _check(rc, DecodeError)
    return (rc, damaged.value) if sync else None


def decode_verdicts(container, output, blank=True):
    """decode of a SEALED host-resident container that keeps what survived: returns (bytes written, indices of the damaged chunks); with `blank` the bytes of
    those chunks are zeros.  Raises ChecksumError (damaged_chunks: all of them) where no chunk is intact, DecodeError for anything that is not damage."""
    ia, n, k1 = _ro(container)
    oa, cap, k2 = _rw(output)
    nc = parse_header(ctypes.string_at(ia, 32)).n_chunks if n >= 32 else 0
    verdicts = (ctypes.c_uint32 * max(nc, 1))()
    damaged = ctypes.c_uint32(0)
    r = _lib.lib().density_hip_decode_verdicts(ia, n, oa, cap, verdicts, nc, _lib.SALVAGE_BLANK if blank else 0, ctypes.byref(damaged))
    bad = [i for i in range(nc) if verdicts[i]] if damaged.value else []
    if r == 0 and _lib.last_error():          # 0 with no error == a valid, empty container
        if nc and damaged.value == nc:
            raise ChecksumError(_lib.last_error(), damaged_chunks=bad)
        raise DecodeError(_lib.last_error())
    return r, bad


def parity_size(input_size, chunk_size, n_groups):
    """The exact size of the parity blob "DHP1" (include/density_hip.h) of input_size bytes cut every chunk_size bytes — the chunk size the container has, not
    0 — with n_groups rows (at most one per chunk); 0 where the arguments are invalid."""
    return int(_lib.lib().density_hip_parity_size(input_size, chunk_size, n_groups))


def parse_parity_header(raw32):
    """The header of a host-resident parity blob of version 1 or 2; raises DecodeError where it is not one."""
    raw = bytes(raw32[:32])
    if len(raw) < 32:
        raise DecodeError("parity blob shorter than its header")
    h = _lib.ParityHeader.from_buffer_copy(raw)
    if h.magic != _lib.PARITY_MAGIC or h.version not in (1, 2):
        raise DecodeError("not a parity blob (magic, version)")
    return h


def parity_device(d_in, n, chunk_size, n_groups, d_parity, cap, stream=0):
    """Enqueue the parity blob of n bytes of device memory into d_parity (cap >= parity_size(); both at any alignment)."""
    _check(_lib.lib().density_hip_parity_device(d_in, n, chunk_size, n_groups, d_parity, cap, stream), EncodeError)


def parity(input, chunk_size, n_groups, output):
    """The parity blob of a host-resident input into `output`; returns the bytes written."""
    ia, n, k1 = _ro(input)
    oa, cap, k2 = _rw(output)
    r = _lib.lib().density_hip_parity(ia, n, chunk_size, n_groups, oa, cap)
    if r == 0:
        raise EncodeError(_lib.last_error())
    return r


def parity2_size(input_size, chunk_size, n_groups):
    """parity_size for version 2 of the blob (n_groups P rows, then as many Q rows over GF(2^8): any two chunks of a group can be rebuilt); 0 also where a
    group would have more than 255 chunks."""
    return int(_lib.lib().density_hip_parity2_size(input_size, chunk_size, n_groups))


def parity2_device(d_in, n, chunk_size, n_groups, d_parity, cap, stream=0):
    """parity_device for version 2 of the blob (cap >= parity2_size())."""
    _check(_lib.lib().density_hip_parity2_device(d_in, n, chunk_size, n_groups, d_parity, cap, stream), EncodeError)


def parity2(input, chunk_size, n_groups, output):
    """parity for version 2 of the blob; returns the bytes written."""
    ia, n, k1 = _ro(input)
    oa, cap, k2 = _rw(output)
    r = _lib.lib().density_hip_parity2(ia, n, chunk_size, n_groups, oa, cap)
    if r == 0:
        raise EncodeError(_lib.last_error())
    return r


def parity_update_header(header, offset, old_size, new_size):
    """The header a parity blob with `header` (a ParityHeader) has after an edit of its input — bytes [offset, offset + old_size) replaced by new_size bytes: a
    same-size edit anywhere, or an edit of the tail (append, truncation) — by host arithmetic alone; raises EncodeError for an edit parity_update_device refuses."""
    after = _lib.ParityHeader()
    _check(_lib.lib().density_hip_parity_update_header(ctypes.byref(header), offset, old_size, new_size, ctypes.byref(after)), EncodeError)
    return after


def parity_update_device(d_parity, parity_size, offset, d_old, old_size, d_new, new_size, parity_header=None, stream=0, want_header=True):
    """Enqueue the update of the parity blob (either version) at d_parity after an edit of its input: bytes [offset, offset + old_size) held the old_size bytes at
    d_old and hold the new_size bytes at d_new now (all three on the device, at any alignment) — a same-size edit anywhere, or one of the tail: append, truncation.
    The blob becomes what parity_device / parity2_device writes for the edited input; only the rows of the edited chunks are touched.  A wrong `old` cannot be
    seen: it gives a wrong blob, whose rebuilds fail the trailer check.  With parity_header (a ParityHeader) nothing synchronises; None: read back first.  Returns
    the blob's new header (host arithmetic) or None."""
    hdr = _lib.ParityHeader() if want_header else None
    rc = _lib.lib().density_hip_parity_update_device(d_parity, parity_size, ctypes.byref(parity_header) if parity_header is not None else None, offset, d_old, old_size,
                                                     d_new, new_size, stream, ctypes.byref(hdr) if want_header else None)
    _check(rc, EncodeError)
    return hdr


def parity_update(parity, offset, old, new):
    """parity_update_device on host arrays, staged whole: the writable blob `parity` is updated in place; returns the blob's size."""
    pa, pn, k1 = _rw(parity)
    oa, on, k2 = _ro(old)
    na, nn, k3 = _ro(new)
    r = _lib.lib().density_hip_parity_update(pa, pn, offset, oa, on, na, nn)
    if r == 0:
        raise EncodeError(_lib.last_error())
    return r


def decode_device_recover(d_container, container_size, d_parity, parity_size, d_out, cap, d_verdicts, header=None, parity_header=None, stream=0, workspace=(0, 0),
                          blank=True, sync=True):
    """decode_device_verdicts, then every chunk that is the only damaged one of its parity group — with a version-2 blob (parity2_device): one of the only two —
    rebuilt from the blob at d_parity and verified again: its verdict becomes _lib.CHUNK_RECOVERED.  Returns (return code, chunks still damaged, chunks recovered) — OK wherever nothing remains damaged, else
    ERR_FORMAT or ERR_CHECKSUM, each with valid verdicts — or None with sync=False.  Anything else (an unsealed container, a blob that is not this
    container's or is malformed, a capacity) raises DecodeError."""
    damaged, recovered = ctypes.c_uint32(0), ctypes.c_uint32(0)
    rc = _lib.lib().density_hip_decode_device_recover(d_container, container_size, ctypes.byref(header) if header is not None else None, d_parity, parity_size,
                                                      ctypes.byref(parity_header) if parity_header is not None else None, d_out, cap, workspace[0], workspace[1],
                                                      stream, d_verdicts, _lib.SALVAGE_BLANK if blank else 0, ctypes.byref(damaged) if sync else None,
                                                      ctypes.byref(recovered) if sync else None)
    if rc not in (_lib.OK, _lib.ERR_CHECKSUM, _lib.ERR_FORMAT) or (rc == _lib.ERR_FORMAT and "chunks damaged" not in _lib.last_error()):
        _check(rc, DecodeError)
    return (rc, damaged.value, recovered.value) if sync else None


def decode_recover(container, parity, output, blank=True):
    """decode_verdicts with a parity blob of either version (parity, parity2): returns (bytes written, indices of the chunks still damaged, indices of the chunks recovered).  Raises ChecksumError
    (damaged_chunks: all of them) where every chunk remains damaged, DecodeError for anything that is not damage."""
    ia, n, k1 = _ro(container)
    pa, pn, k3 = _ro(parity)
    oa, cap, k2 = _rw(output)
    nc = parse_header(ctypes.string_at(ia, 32)).n_chunks if n >= 32 else 0
    verdicts = (ctypes.c_uint32 * max(nc, 1))()
    damaged, recovered = ctypes.c_uint32(0), ctypes.c_uint32(0)
    r = _lib.lib().density_hip_decode_recover(ia, n, pa, pn, oa, cap, verdicts, nc, _lib.SALVAGE_BLANK if blank else 0, ctypes.byref(damaged), ctypes.byref(recovered))
    bad = [i for i in range(nc) if verdicts[i] == _lib.CHUNK_DAMAGED] if damaged.value else []
    if r == 0 and _lib.last_error():          # 0 with no error == a valid, empty container
        if nc and damaged.value == nc:
            raise ChecksumError(_lib.last_error(), damaged_chunks=bad)
        raise DecodeError(_lib.last_error())
    return r, bad, [i for i in range(nc) if verdicts[i] == _lib.CHUNK_RECOVERED] if recovered.value else []


def stream_encode_device(algo, d_in, n, d_out, cap, stream=0):
    size = ctypes.c_size_t(0)
    _check(_lib.lib().density_hip_stream_encode_device(_lib.ALGO_IDS[algo], d_in, n, d_out, cap, stream, ctypes.byref(size)), EncodeError)
    return size.value


def stream_decode_device(algo, d_in, n, d_out, cap, stream=0):
    size = ctypes.c_size_t(0)
    _check(_lib.lib().density_hip_stream_decode_device(_lib.ALGO_IDS[algo], d_in, n, d_out, cap, stream, ctypes.byref(size)), DecodeError)
    return size.value


def set_kernel_variant(variant):
    """Bit mask (test hook): 1 = simple one-wavefront kernels, 2 = containers without the block index."""
    _lib.lib().density_hip_set_kernel_variant(int(variant))


def set_profiling(on):
    _lib.lib().density_hip_set_profiling(1 if on else 0)


def last_timings(cap=8192):
    ms = (ctypes.c_float * cap)()
    names = (ctypes.c_char_p * cap)()
    n = _lib.lib().density_hip_last_timings(ms, names, cap)
    return [(names[i].decode(), float(ms[i])) for i in range(n)]
