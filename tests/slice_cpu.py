"""What a slice is, stated in numpy from the header's layout alone (include/density_hip.h): chunks [first, first + count) of a host-resident container of
any form, sealed or not, as the packed container of those chunk streams.  Test infrastructure — the expectation tests/test_gpu_slice.py holds
density_hip_slice_device to, itself held to the oracle in tests/test_slice_cpu.py — and never the code under test."""
import numpy as np

MAGIC, INDEX, SLOTTED, PAGED, CHECKSUM, PAGE = 0x31434844, 1, 2, 4, 8, 65536
BLOCK = {0: (256, 8), 1: (128, 8), 2: (64, 6)}                  # algo: (block bytes, signature bytes) of {algo}_safe_encode_buffer_size


def up(v, a):
    return (v + a - 1) // a * a


def safe_size(algo, n):
    b, s = BLOCK[algo]
    return n + n // b * s + (s if n % b else 0)


def header_of(blob):
    """(algo, flags, chunk_size, n_chunks, total_len, container_len)"""
    raw = bytes(blob[:32])
    assert int.from_bytes(raw[:4], "little") == MAGIC and raw[5] == 1
    return (raw[4], int.from_bytes(raw[6:8], "little"), int.from_bytes(raw[8:12], "little"), int.from_bytes(raw[12:16], "little"),
            int.from_bytes(raw[16:24], "little"), int.from_bytes(raw[24:32], "little"))


def windows(n):
    """the windows every container of n chunks is cut at: the first chunk, a pair, all but the first, the (ragged) last alone, everything"""
    out = []
    for first, count in [(0, 1), (1, 2), (1, n - 1), (n - 1, 1), (0, n)]:
        if count >= 1 and first + count <= n and (first, count) not in out:
            out.append((first, count))
    return out


def assemble(algo, chunk, total, streams, index=None, sums=None):
    """The packed container of `streams` (one reference stream per chunk of an input of `total` bytes cut every `chunk`): header, size table, the block
    index (`index`: its bytes, or None for a container without one), every stream at the next 16-byte boundary behind the one before with zeros between,
    container_len where the last one ends — and with `sums` (a checksum per chunk) the trailer at the next 16-byte boundary, zero-padded to 16."""
    n = len(streams)
    assert n == (total + chunk - 1) // chunk
    ix0 = up(32 + 4 * n, 16)
    at = up(ix0 + (total + 255) // 256, 16) if index is not None else ix0
    places, end = [], at
    for s in streams:
        places.append(at)
        end, at = at + len(s), up(at + len(s), 16)
    size = end if sums is None else up(end, 16) + up(4 * n, 16)
    out = np.zeros(size, dtype=np.uint8)
    flags = (INDEX if index is not None else 0) | (CHECKSUM if sums is not None else 0)
    out[:32] = np.frombuffer(MAGIC.to_bytes(4, "little") + bytes([algo, 1]) + flags.to_bytes(2, "little") + chunk.to_bytes(4, "little") + n.to_bytes(4, "little") +
                             total.to_bytes(8, "little") + size.to_bytes(8, "little"), dtype=np.uint8)
    out[32:32 + 4 * n] = np.array([len(s) for s in streams], dtype="<u4").view(np.uint8)
    if index is not None:
        assert len(index) == (total + 255) // 256
        out[ix0:ix0 + len(index)] = np.frombuffer(bytes(index), dtype=np.uint8)
    for p, s in zip(places, streams):
        out[p:p + len(s)] = np.frombuffer(bytes(s), dtype=np.uint8)
    if sums is not None:
        out[up(end, 16):up(end, 16) + 4 * n] = np.array(list(sums), dtype="<u4").view(np.uint8)
    return out


def chunk_streams(blob, wanted):
    """the reference streams of chunks `wanted` (a range) of a container of any form, read where the header's layout puts them"""
    src = np.ascontiguousarray(blob, dtype=np.uint8).reshape(-1)
    algo, flags, chunk, n, total, clen = header_of(src)
    sizes = src[32:32 + 4 * n].view("<u4").astype(np.int64)
    ix0 = up(32 + 4 * n, 16)
    base = up(ix0 + (total + 255) // 256, 16) if flags & INDEX else ix0
    out = []
    if flags & PAGED:
        ppc = safe_size(0, chunk) // (PAGE - 4352) + 2               # density_hip_paged_pages_per_chunk
        pages0 = up(base + 16 * (ppc + 1) * n, 256)
        for i in wanted:
            d = base + 16 * (ppc + 1) * i
            parts = []
            for k in range(int.from_bytes(bytes(src[d:d + 4]), "little")):
                e = d + 16 * (k + 1)
                page, used = int.from_bytes(bytes(src[e:e + 4]), "little"), int.from_bytes(bytes(src[e + 8:e + 12]), "little")
                parts.append(src[pages0 + page * PAGE:pages0 + page * PAGE + used].tobytes())
            out.append(b"".join(parts))
            assert len(out[-1]) == sizes[i], (i, len(out[-1]), int(sizes[i]))
        return out
    if flags & SLOTTED:
        stride = up(safe_size(algo, chunk), 256)
        return [src[base + i * stride:base + i * stride + sizes[i]].tobytes() for i in wanted]
    offsets = base + np.concatenate(([0], np.cumsum((sizes + 15) // 16 * 16)[:-1])) if n else []
    return [src[offsets[i]:offsets[i] + sizes[i]].tobytes() for i in wanted]


def slice_container(blob, first, count):
    """chunks [first, first + count) of `blob` as a packed container: uint8 array of container_len bytes"""
    src = np.ascontiguousarray(blob, dtype=np.uint8).reshape(-1)
    algo, flags, chunk, n, total, clen = header_of(src)
    assert count >= 1 and first + count <= n and clen <= src.size
    length = min(total, (first + count) * chunk) - first * chunk
    ix0 = up(32 + 4 * n, 16)
    index = src[ix0 + first * chunk // 256:][:(length + 255) // 256].tobytes() if flags & INDEX else None
    sums = None
    if flags & CHECKSUM:
        t = clen - up(4 * n, 16)
        sums = src[t + 4 * first:t + 4 * (first + count)].view("<u4").tolist()
    return assemble(algo, chunk, length, chunk_streams(src, range(first, first + count)), index, sums)
