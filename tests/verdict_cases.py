"""What the verdict tests (test_gpu_verdicts.py on the device, test_verdicts_cpu.py without one) share: the shapes, the inputs, where a chunk's stream lies in a
container of each form, and the positions at which one flipped bit is SILENT damage — a valid stream that the reference decodes to wrong bytes of the right
length.  Test infrastructure: it calls the oracle, never the library's decoders."""
import functools

import numpy as np

import datagen
import paged_cpu
from density_amd import _lib, container
from oracle import pyoracle

MIB = 1 << 20
# the smallest shapes at which each form exists, each with a ragged last chunk: (algo, form) -> (total bytes, chunk size)
SHAPES = {
    ("chameleon", "paged"): (3 * MIB + 12_345, MIB),               # (the paged form needs two chunks of 1 MiB: api_internal.hpp paged_eligible)
    ("chameleon", "packed"): (5 * 65536 + 12_345, 65536),
    ("chameleon", "slotted"): (5 * 65536 + 12_345, 65536),
    ("cheetah", "packed"): (5 * 65536 + 777, 65536),
    ("cheetah", "slotted"): (5 * 65536 + 777, 65536),
    ("lion", "packed"): (5 * 65536 + 777, 65536),
    ("lion", "slotted"): (5 * 65536 + 777, 65536),
}
KINDS = ["rep_text", "mixed"]
FLIP = 0x10
CANDIDATES = 64


@functools.lru_cache(maxsize=None)
def _input(kind, n):
    data = datagen.rep_text(n, period=100_003, seed=41) if kind == "rep_text" else datagen.by_kind("mixed", n, seed=43)
    data.setflags(write=False)
    return data


def input_of(algo, form, kind):
    n, chunk = SHAPES[(algo, form)]
    return _input(kind, n), chunk


def n_chunks(algo, form):
    n, chunk = SHAPES[(algo, form)]
    return -(-n // chunk)


def victims(algo, form):
    """first, middle and last chunk"""
    nc = n_chunks(algo, form)
    return [0, nc // 2, nc - 1]


def chameleon_plain_position(stream, n_bytes, from_block=1):
    """Stream offset of the first byte of a PLAIN quad (or of a raw-copy block's ninth byte) in the first record at or behind block `from_block` that has
    one: a flipped bit there leaves the signature, the record lengths and the block index as they were, so nothing but the content says it happened.
    Always in the item area, at least 8 bytes behind the record's start."""
    at = 0
    blocks = paged_cpu.walk_records(stream, n_bytes)
    for b, (index_byte, length) in enumerate(blocks):
        blen = min(256, n_bytes - 256 * b)
        if b >= min(from_block, len(blocks) - 1):
            if index_byte & 0x80:
                if length > 8:
                    return at + 8
            else:
                sig, item = int.from_bytes(stream[at:at + 8], "little"), at + 8
                for q in range(blen // 4):
                    if not (sig >> q) & 1:
                        return item
                    item += 2
        at += length
    raise AssertionError("no PLAIN quad in the chunk")


@functools.lru_cache(maxsize=None)
def silent_position(algo, kind, n, chunk, k):
    """(stream offset, silently decoding candidates among CANDIDATES) for chunk k of the input: Chameleon from the records, Cheetah and Lion the first of a
    seeded list of candidates at which the reference decodes the damaged stream to the full length, without error, and to different bytes."""
    part = _input(kind, n)[k * chunk:(k + 1) * chunk]
    stream = pyoracle.encode(algo, part)
    if algo == "chameleon":
        pos = chameleon_plain_position(stream, part.size, from_block=(part.size // 256) // 2)
        found = [pos]
    else:
        rng = np.random.default_rng(1000 * k + len(stream))
        found = []
        for pos in (int(v) for v in rng.integers(0, len(stream), size=CANDIDATES)):
            bad = bytearray(stream)
            bad[pos] ^= FLIP
            out = pyoracle.decode(algo, bytes(bad), part.size)
            if len(out) == part.size and out != part.tobytes():
                found.append(pos)
    bad = bytearray(stream)
    if found:
        bad[found[0]] ^= FLIP
        out = pyoracle.decode(algo, bytes(bad), part.size)
        assert len(out) == part.size and out != part.tobytes(), (algo, kind, k, found[0])
    return (found[0] if found else None), len(found)


def front_matter(h):
    """(offset of the block index, offset of what lies behind it: payload 0 / the page directory)"""
    ix = (32 + 4 * h.n_chunks + 15) // 16 * 16
    behind = (ix + (h.total_len + 255) // 256 + 15) // 16 * 16 if h.flags & container.FLAG_BLOCK_INDEX else ix
    return ix, behind


def stream_byte_at(blob, k, pos):
    """where byte `pos` of chunk k's stream lies in a host-resident container of any form"""
    h = container.parse_header(blob)
    _, base = front_matter(h)
    size = lambda i: int.from_bytes(bytes(blob[32 + 4 * i:36 + 4 * i]), "little")
    assert pos < size(k)
    if h.flags & container.FLAG_PAGED:
        ppc = int(_lib.lib().density_hip_paged_pages_per_chunk(h.chunk_size))
        pages_base = (base + 16 * (ppc + 1) * h.n_chunks + 255) // 256 * 256
        d = base + 16 * (ppc + 1) * k
        for j in range(int.from_bytes(bytes(blob[d:d + 4]), "little")):
            e = d + 16 * (j + 1)
            page, used = int.from_bytes(bytes(blob[e:e + 4]), "little"), int.from_bytes(bytes(blob[e + 8:e + 12]), "little")
            if pos < used:
                return pages_base + page * container.PAGE_BYTES + pos
            pos -= used
        raise AssertionError("the directory does not reach the position")
    if h.flags & container.FLAG_SLOTTED:
        return base + k * container.slot_stride(_lib.ALGO_NAMES[h.algo], h.chunk_size) + pos
    for i in range(k):
        base = (base + size(i) + 15) // 16 * 16
    return base + pos


def trailer_at(blob):
    h = container.parse_header(blob)
    return h.container_len - (4 * h.n_chunks + 15) // 16 * 16
