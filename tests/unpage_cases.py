"""Inputs and CPU-made expectations shared by tests/test_unpage_cpu.py and tests/test_gpu_unpage.py (test infrastructure: it calls the oracle).  Paged
containers come from tests/paged_cpu.py, the packed container they must turn into is assembled HERE from the oracle's chunk streams by the header's layout
(include/density_hip.h), never by the code under test.  Everything is built once per session and handed out read-only."""
import functools

import numpy as np

import datagen
import paged_cpu
from density_amd import _lib, container
from oracle import pyoracle

KiB = 1 << 10
# name: (kind, n, chunk, pages per chunk) — the smallest inputs at which every seam case occurs: `bytes % 16` of the pages taking (almost) every residue (a),
# raw-copy streams longer than their input and a last stream shorter than one store (b), compressible text (c), every seam 16-aligned (d), many seams in
# one chunk (e), a single chunk (f), a single chunk of one short page (g)
CASES = {
    "a": ("mixed", 6 * 192 * KiB + 4321, 192 * KiB, [3, 3, 3, 3, 3, 3, 1]),
    "b": ("random", 3 * 128 * KiB + 5, 128 * KiB, [3, 3, 3, 1]),
    "c": ("rep-text", 4 * 256 * KiB, 256 * KiB, [3, 3, 3, 3]),
    "d": ("zeros", 2 * 256 * KiB + 1, 256 * KiB, [3, 3, 1]),
    "e": ("prose", (1 << 20) + 17, 1 << 20, [11, 1]),
    "f": ("random", 128 * KiB, 128 * KiB, [3]),
    "g": ("mixed", 40, 256, [1]),
}
SHUFFLED = ("a", "c", "e")
ORDERS = [(name, False) for name in CASES] + [(name, True) for name in SHUFFLED]


def _frozen(a):
    a.setflags(write=False)
    return a


@functools.lru_cache(maxsize=None)
def data(name):
    kind, n, chunk, _ = CASES[name]
    return _frozen(datagen.rep_text(n) if kind == "rep-text" else datagen.by_kind(kind, n, seed=7))


@functools.lru_cache(maxsize=None)
def streams(name):
    _, n, chunk, _ = CASES[name]
    return tuple(pyoracle.encode(paged_cpu.ALGO, data(name)[i:i + chunk]) for i in range(0, n, chunk))


def geometry(n, chunk):
    """(chunks, pages per chunk the directory has room for, offset of the block index, of the directory, of page 0)"""
    nc = (n + chunk - 1) // chunk
    ppc = int(_lib.lib().density_hip_paged_pages_per_chunk(chunk))
    ix0 = (32 + 4 * nc + 15) // 16 * 16
    dir0 = (ix0 + (n + 255) // 256 + 15) // 16 * 16
    return nc, ppc, ix0, dir0, (dir0 + 16 * (ppc + 1) * nc + 255) // 256 * 256


def page_counts(blob, name):
    _, n, chunk, _ = CASES[name]
    nc, ppc, _, dir0, _ = geometry(n, chunk)
    return [int.from_bytes(bytes(blob[dir0 + 16 * (ppc + 1) * i:][:4]), "little") for i in range(nc)]


@functools.lru_cache(maxsize=None)
def paged(name, shuffled=False):
    """The paged container of case `name`, its pages in chunk order or shuffled by np.random.default_rng(3)."""
    _, n, chunk, want = CASES[name]
    blob = paged_cpu.build(data(name), chunk)
    assert page_counts(blob, name) == want, (name, page_counts(blob, name))
    if shuffled:
        blob = paged_cpu.build(data(name), chunk, page_order=list(np.random.default_rng(3).permutation(sum(want))))
    return _frozen(blob)


@functools.lru_cache(maxsize=None)
def packed(name):
    """The packed container of case `name` from the oracle's streams: header with flags = BLOCK_INDEX, size table, the index bytes of the paged blob,
    payloads at 16-byte boundaries with zeros between, container_len = the end of the last payload."""
    _, n, chunk, _ = CASES[name]
    nc, _, ix0, dir0, _ = geometry(n, chunk)
    ss = streams(name)
    at, places = dir0, []
    for s in ss:
        places.append(at)
        end, at = at + len(s), (at + len(s) + 15) // 16 * 16
    out = np.zeros(end, dtype=np.uint8)
    hdr = _lib.Header()
    hdr.magic, hdr.algo, hdr.version, hdr.flags = 0x31434844, 0, 1, 1
    hdr.chunk_size, hdr.n_chunks, hdr.total_len, hdr.container_len = chunk, nc, n, end
    out[:32] = np.frombuffer(bytes(hdr), dtype=np.uint8)
    out[32:32 + 4 * nc] = np.array([len(s) for s in ss], dtype="<u4").view(np.uint8)
    out[ix0:ix0 + (n + 255) // 256] = paged(name)[ix0:ix0 + (n + 255) // 256]
    for p, s in zip(places, ss):
        out[p:p + len(s)] = np.frombuffer(s, dtype=np.uint8)
    return _frozen(out)


def sealed(blob, name):
    """`blob` (either form) of case `name` with the trailer the header describes: at T = round_up(E, 16) a checksum per chunk of the INPUT
    (density_hip_checksum32), zero-padded to 16; the flag, the new container_len."""
    _, n, chunk, _ = CASES[name]
    nc = (n + chunk - 1) // chunk
    E = blob.size
    T = (E + 15) // 16 * 16
    out = np.zeros(T + (4 * nc + 15) // 16 * 16, dtype=np.uint8)
    out[:E] = blob
    sums = [container.checksum32(np.ascontiguousarray(data(name)[i:i + chunk])) for i in range(0, n, chunk)]
    out[T:T + 4 * nc] = np.array(sums, dtype="<u4").view(np.uint8)
    hdr = container.parse_header(out[:32].tobytes())
    hdr.flags |= container.FLAG_CHECKSUM
    hdr.container_len = out.size
    out[:32] = np.frombuffer(bytes(hdr), dtype=np.uint8)
    return out


def put32(blob, at, value):
    blob[at:at + 4] = np.frombuffer(int(value).to_bytes(4, "little"), dtype=np.uint8)


def get32(blob, at):
    return int.from_bytes(bytes(blob[at:at + 4]), "little")


def format_mutations(name="a"):
    """{what: a copy of the paged container of case `name` with one directory the call cannot follow}"""
    _, n, chunk, _ = CASES[name]
    nc, ppc, _, dir0, _ = geometry(n, chunk)
    blob = paged(name)

    def head(c): return dir0 + 16 * (ppc + 1) * c
    def entry(c, k): return head(c) + 16 * (k + 1)
    out = {}
    bad = blob.copy(); put32(bad, entry(1, 1), 0x7fff); out["page number 0x7fff"] = bad
    bad = blob.copy(); put32(bad, entry(3, 0) + 8, 65538); out["bytes = 65538"] = bad
    bad = blob.copy(); put32(bad, entry(0, 0) + 8, get32(blob, entry(0, 0) + 8) - 2); out["bytes minus 2 in one entry"] = bad
    bad = blob.copy(); put32(bad, head(4), 0); out["a chunk with 0 pages"] = bad
    bad = blob.copy(); put32(bad, head(5), 200); out["a chunk with 200 pages"] = bad
    # a size-table entry above the chunk's safe_encode_buffer_size, the directory in step with it (the last chunk: 4321 bytes of input, one page)
    safe = 4321 + 4321 // 256 * 8 + 8
    bad = blob.copy(); put32(bad, 32 + 4 * (nc - 1), safe + 1); put32(bad, entry(nc - 1, 0) + 8, safe + 1); out["size above safe_encode_buffer_size"] = bad
    return out
