"""The parity blob "DHP1" (include/density_hip.h: recovery records) and the rebuild of a chunk from it, in numpy: what a CPU producer or reader that follows the
header file would do.  Test infrastructure: it never calls the library."""
import struct

import numpy as np

MAGIC = 0x31504844          # "DHP1"
HEADER = struct.Struct("<IBBHIIQII")


def geometry(total, chunk, requested):
    """(n_chunks, n_groups, row_bytes) of the blob of `total` bytes cut every `chunk` bytes with `requested` groups asked for"""
    n_chunks = -(-total // chunk)
    return n_chunks, min(requested, n_chunks), (min(chunk, total) + 15) // 16 * 16


def size(total, chunk, requested):
    _, n_groups, row_bytes = geometry(total, chunk, requested)
    return HEADER.size + n_groups * row_bytes


def blob(data, chunk, requested):
    """the blob of `data` (uint8 array): the header, then row g = XOR of the chunks i with i % n_groups == g, each zero-padded to row_bytes"""
    data = np.asarray(data, dtype=np.uint8)
    n_chunks, n_groups, row_bytes = geometry(data.size, chunk, requested)
    rows = np.zeros((n_groups, row_bytes), dtype=np.uint8)
    for i in range(n_chunks):
        part = data[i * chunk:(i + 1) * chunk]
        rows[i % n_groups, :part.size] ^= part
    head = np.frombuffer(HEADER.pack(MAGIC, 1, 0, 0, chunk, n_chunks, data.size, n_groups, row_bytes), dtype=np.uint8)
    return np.concatenate([head, rows.reshape(-1)])


def parse(raw):
    """(chunk, n_chunks, total, n_groups, row_bytes, rows as a 2-d view) of a blob"""
    raw = np.asarray(raw, dtype=np.uint8)
    magic, version, r0, r1, chunk, n_chunks, total, n_groups, row_bytes = HEADER.unpack(raw[:HEADER.size].tobytes())
    assert (magic, version, r0, r1) == (MAGIC, 1, 0, 0)
    assert raw.size >= HEADER.size + n_groups * row_bytes
    return chunk, n_chunks, total, n_groups, row_bytes, raw[HEADER.size:HEADER.size + n_groups * row_bytes].reshape(n_groups, row_bytes)


def row_offset(raw, g, at=0):
    """where byte `at` of row g lies in the blob"""
    row_bytes = parse(raw)[4]
    return HEADER.size + g * row_bytes + at


def rebuild(raw, output, k):
    """chunk k as the blob and the OTHER chunks of its group in `output` (the decoded bytes, total long) give it: row XOR the other members, at k's true length"""
    chunk, n_chunks, total, n_groups, row_bytes, rows = parse(raw)
    output = np.asarray(output, dtype=np.uint8)
    assert output.size == total and k < n_chunks
    acc = rows[k % n_groups].copy()
    for i in range(k % n_groups, n_chunks, n_groups):
        if i != k:
            part = output[i * chunk:(i + 1) * chunk]
            acc[:part.size] ^= part
    return acc[:min(chunk, total - k * chunk)]
