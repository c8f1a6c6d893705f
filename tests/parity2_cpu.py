"""Version 2 of the parity blob "DHP1" (include/density_hip.h: double parity — P rows, then Q rows over GF(2^8)) and the rebuild of one and of two chunks of a
group from it, in numpy: what a CPU producer or reader that follows the header file would do.  Test infrastructure: it never calls the library.  The field's
multiplication goes through logarithm and exponential tables built from the polynomial 0x11D — deliberately not through the packed doubling the kernels use."""
import numpy as np

import parity_cpu
from parity_cpu import HEADER, MAGIC, geometry

MAX_MEMBERS = 255           # 2 has order 255: the places 0 .. 254 give 255 different powers

EXP = np.zeros(510, dtype=np.uint8)      # EXP[e] = 2^e, twice over so that the sum of two logarithms needs no modulo
LOG = np.zeros(256, dtype=np.int64)      # LOG[2^e] = e (LOG[0] is never read)
_x = 1
for _e in range(255):
    EXP[_e] = EXP[_e + 255] = _x
    LOG[_x] = _e
    _x <<= 1
    if _x & 0x100:
        _x ^= 0x11D
assert _x == 1, "2 does not generate the field"


def times(c, v):
    """the bytes of `v` times the constant c"""
    v = np.asarray(v, dtype=np.uint8)
    if c == 0:
        return np.zeros_like(v)
    return np.where(v == 0, 0, EXP[LOG[v] + LOG[c]]).astype(np.uint8)


def pow2(e):
    return int(EXP[e % 255])


def inverse(c):
    return int(EXP[(255 - LOG[c]) % 255])


def size(total, chunk, requested):
    """the blob's size; 0 where a group would have more than 255 members"""
    n_chunks, n_groups, row_bytes = geometry(total, chunk, requested)
    if n_groups and -(-n_chunks // n_groups) > MAX_MEMBERS:
        return 0
    return HEADER.size + 2 * n_groups * row_bytes


def blob(data, chunk, requested):
    """the blob of `data` (uint8 array): the header with version 2, P row g = XOR of the chunks i with i % n_groups == g, each zero-padded to row_bytes, then
    Q row g = XOR of 2^(i // n_groups) times those"""
    data = np.asarray(data, dtype=np.uint8)
    n_chunks, n_groups, row_bytes = geometry(data.size, chunk, requested)
    assert size(data.size, chunk, requested)
    p = np.zeros((n_groups, row_bytes), dtype=np.uint8)
    q = np.zeros((n_groups, row_bytes), dtype=np.uint8)
    for i in range(n_chunks):
        part = data[i * chunk:(i + 1) * chunk]
        p[i % n_groups, :part.size] ^= part
        q[i % n_groups, :part.size] ^= times(pow2(i // n_groups), part)
    head = np.frombuffer(HEADER.pack(MAGIC, 2, 0, 0, chunk, n_chunks, data.size, n_groups, row_bytes), dtype=np.uint8)
    return np.concatenate([head, p.reshape(-1), q.reshape(-1)])


def parse(raw):
    """(chunk, n_chunks, total, n_groups, row_bytes, P rows, Q rows as 2-d views) of a blob"""
    raw = np.asarray(raw, dtype=np.uint8)
    magic, version, r0, r1, chunk, n_chunks, total, n_groups, row_bytes = HEADER.unpack(raw[:HEADER.size].tobytes())
    assert (magic, version, r0, r1) == (MAGIC, 2, 0, 0)
    rows = n_groups * row_bytes
    assert raw.size >= HEADER.size + 2 * rows
    return (chunk, n_chunks, total, n_groups, row_bytes, raw[HEADER.size:HEADER.size + rows].reshape(n_groups, row_bytes),
            raw[HEADER.size + rows:HEADER.size + 2 * rows].reshape(n_groups, row_bytes))


def row_offset(raw, g, at=0, q=False):
    """where byte `at` of P row g (q: of Q row g) lies in the blob"""
    n_groups, row_bytes = parse(raw)[3:5]
    return HEADER.size + ((n_groups if q else 0) + g) * row_bytes + at


def as_version_1(raw):
    """the version-1 blob inside: the header with version 1 and the P rows"""
    n_groups, row_bytes = parse(raw)[3:5]
    v1 = np.array(raw[:HEADER.size + n_groups * row_bytes])
    v1[4] = 1
    return v1


def rebuild_one(raw, output, k):
    """chunk k from the P row and the other chunks of its group in `output`, as with version 1; Q is not read"""
    return parity_cpu.rebuild(as_version_1(raw), output, k)


def rebuild_two(raw, output, k1, k2):
    """chunks k1 < k2 of ONE group from both rows and the group's other chunks in `output` (neither k1's nor k2's region is read): each at its true length"""
    chunk, n_chunks, total, n_groups, row_bytes, p_rows, q_rows = parse(raw)
    output = np.asarray(output, dtype=np.uint8)
    g = k1 % n_groups
    assert output.size == total and k1 < k2 < n_chunks and k2 % n_groups == g
    pxy, qxy = p_rows[g].copy(), q_rows[g].copy()
    for i in range(g, n_chunks, n_groups):
        if i not in (k1, k2):
            part = output[i * chunk:(i + 1) * chunk]
            pxy[:part.size] ^= part
            qxy[:part.size] ^= times(pow2(i // n_groups), part)
    a, b = k1 // n_groups, k2 // n_groups
    over_d = inverse(pow2(b - a) ^ 1)
    c1 = int(times(over_d, [pow2(b - a)])[0])
    c2 = int(times(over_d, [pow2(255 - a)])[0])
    d_a = times(c1, pxy) ^ times(c2, qxy)
    d_b = pxy ^ d_a
    return d_a[:min(chunk, total - k1 * chunk)], d_b[:min(chunk, total - k2 * chunk)]
