"""Sealed containers without a GPU (include/density_hip.h: DENSITY_HIP_FLAG_CHECKSUM): the host checksum density_hip_checksum32 against known answers and a
numpy model, the arithmetic of density_hip_seal_overhead, and what the header check and the Python readers make of a sealed container assembled here from the
oracle's streams (packed, and paged from tests/paged_cpu.py) with the trailer appended as the header file specifies it."""
import ctypes

import numpy as np
import pytest

import datagen
import paged_cpu
from density_amd import _lib, container
from oracle import pyoracle

M32 = 0xFFFFFFFF


def model(data):
    """C(B) of include/density_hip.h in numpy: little-endian words, the last zero-padded; S = sum fmix32(w_i + 0x9E3779B1 (i + 1)); C = fmix32(S + L)."""
    def fmix(h):
        h = h ^ (h >> np.uint64(16)); h = (h * np.uint64(0x85EBCA6B)) & np.uint64(M32)
        h = h ^ (h >> np.uint64(13)); h = (h * np.uint64(0xC2B2AE35)) & np.uint64(M32)
        return h ^ (h >> np.uint64(16))
    b = bytes(data)
    w = np.frombuffer(b + bytes(-len(b) % 4), dtype="<u4").astype(np.uint64)
    i = np.arange(1, w.size + 1, dtype=np.uint64)
    s = int(fmix((w + np.uint64(0x9E3779B1) * i) & np.uint64(M32)).sum()) & M32
    return int(fmix(np.uint64((s + len(b)) & M32)))


def c32(b):
    b = bytes(b)
    return int(_lib.lib().density_hip_checksum32(ctypes.c_char_p(b), len(b)))


KNOWN = [(b"", 0x00000000), (b"a", 0x1D4879CC), (b"abc", 0x6AEC4E25), (b"abcd", 0x63363931), (bytes(256), 0xE019641A), (bytes(range(256)), 0xD30E59AC),
         (bytes(257), 0x94E90AEB), ((bytes(range(256)) * 4096)[:1048323], 0x65F03662),
         (np.random.default_rng(1).integers(0, 256, 65536, dtype=np.uint8).tobytes(), 0x11069B39)]


@pytest.mark.parametrize("k", range(len(KNOWN)))
def test_known_answers(k):
    data, want = KNOWN[k]
    assert c32(data) == want
    assert model(data) == want
    if data:
        assert container.checksum32(np.frombuffer(data, dtype=np.uint8)) == want


def test_checksum32_matches_the_model_on_random_strings():
    rng = np.random.default_rng(7)
    lengths = list(range(71)) + [4096 + d for d in range(-3, 4)]
    lengths += [int(rng.choice(lengths)) for _ in range(200 - len(lengths))]
    assert len(lengths) == 200
    for n in lengths:
        b = rng.integers(0, 256, n, dtype=np.uint8).tobytes()
        assert c32(b) == model(b), n
    # the word's index goes in: two different words exchanged change the sum, and so does a trailing zero byte
    assert c32(b"abcdefgh") != c32(b"efghabcd")
    assert c32(bytes(7)) != c32(bytes(8))


def test_seal_overhead_arithmetic():
    so = _lib.lib().density_hip_seal_overhead
    for n, c in [(0, 256), (1, 256), (1000, 256), (4 * 65536, 65536), (4 * 65536 + 1, 65536), ((1 << 30) + 5, 4 << 20), (900_001, 65536)]:
        nc = -(-n // c)
        assert so(n, c) == 16 + (4 * nc + 15) // 16 * 16, (n, c)
    assert so(10, 100) == 0 and so(10, 255) == 0 and so(10, (1 << 30) + 256) == 0
    # chunk_size 0: the chunks of the smallest automatic chunk of any algorithm, an upper bound for all three
    for n in (0, 1, 10_000_000, 100_000_000, 1 << 30):
        for a in range(3):
            auto = _lib.lib().density_hip_auto_chunk_for(a, n)
            assert so(n, 0) >= so(n, auto) > 0, (n, a)
    assert container.seal_overhead(1000, 256) == 32


def packed_container(algo, data, chunk):
    """The packed layout of include/density_hip.h without a block index, from the oracle's streams."""
    streams = [pyoracle.encode(algo, data[i:i + chunk]) for i in range(0, data.size, chunk)]
    nc = len(streams)
    out = bytearray((32 + 4 * nc + 15) // 16 * 16)
    for i, s in enumerate(streams):
        out[32 + 4 * i:36 + 4 * i] = len(s).to_bytes(4, "little")
        out += bytes(-len(out) % 16) + s
    h = _lib.Header(0x31434844, _lib.ALGO_IDS[algo], 1, 0, chunk, nc, data.size, len(out))
    out[:32] = bytes(h)
    return bytes(out), streams


def seal(blob, data):
    """The trailer of include/density_hip.h appended on the CPU: T = round_up(E, 16), a word per chunk, zero-padded to 16; flag 8, the new container_len."""
    h = container.parse_header(blob)
    sums = [model(data[i:i + h.chunk_size]) for i in range(0, data.size, h.chunk_size)]
    trailer = b"".join(s.to_bytes(4, "little") for s in sums)
    out = bytearray(blob) + bytes(-len(blob) % 16) + trailer + bytes(-len(trailer) % 16)
    h.flags |= container.FLAG_CHECKSUM
    h.container_len = len(out)
    out[:32] = bytes(h)
    return np.frombuffer(bytes(out), dtype=np.uint8), sums


def _decoded_size(blob, size=None):
    b = bytes(blob)
    return int(_lib.lib().density_hip_decoded_size(ctypes.c_char_p(b), len(b) if size is None else size))


@pytest.mark.parametrize("form", ["packed", "paged"])
def test_sealed_container_assembled_on_the_cpu(form):
    if form == "packed":
        data = datagen.mixed(5 * 4096 + 77, seed=9)
        blob, streams = packed_container("cheetah", data, 4096)
    else:
        data = datagen.rep_text(2 * (1 << 20) + 4321, period=100_003, seed=9)
        blob = paged_cpu.build(data, 1 << 20).tobytes()
        streams = container.chunk_payloads(blob)[1]
        assert streams == [pyoracle.encode("chameleon", data[i:i + (1 << 20)]) for i in range(0, data.size, 1 << 20)]
    h0 = container.parse_header(blob)
    assert _decoded_size(blob) == data.size and container.chunk_checksums(blob) is None
    sealed, sums = seal(blob, data)
    h = container.parse_header(sealed)
    tb = (4 * h.n_chunks + 15) // 16 * 16
    assert h.flags == h0.flags | 8 and h.container_len == (h0.container_len + 15) // 16 * 16 + tb == sealed.size
    assert _decoded_size(sealed) == data.size
    assert container.decoded_size(sealed) == data.size
    # a container_size that cuts into the trailer
    for cut in (1, 4, tb):
        assert _decoded_size(sealed, sealed.size - cut) == 0, cut
    # a container_len too short to hold a trailer behind the front matter
    short = bytearray(sealed.tobytes())
    hs = container.parse_header(short)
    front = _pages_base(h0) if form == "paged" else (32 + 4 * h.n_chunks + 15) // 16 * 16      # (the pages' base | the payload base without a block index)
    hs.container_len = front + tb - 16
    short[:32] = bytes(hs)
    assert _decoded_size(short) == 0
    hs.container_len = front + tb
    short[:32] = bytes(hs)
    assert _decoded_size(short) == data.size                                    # (the header check alone: all streams empty would be the decoder's finding)
    if form == "paged":                                                        # the whole-pages rule holds for what lies in front of the trailer
        hs.container_len = h.container_len + 16
        short[:32] = bytes(hs)
        assert _decoded_size(bytes(short) + bytes(16)) == 0
    # unknown flag bits are still refused
    hs = container.parse_header(sealed)
    hs.flags |= 16
    assert _decoded_size(bytes(hs) + sealed.tobytes()[32:]) == 0
    # the readers
    assert container.chunk_checksums(sealed) == sums == [container.checksum32(data[i:i + h.chunk_size]) for i in range(0, data.size, h.chunk_size)]
    assert container.chunk_payloads(sealed)[1] == streams
    assert container.block_index(sealed) == container.block_index(blob)


def _pages_base(h):
    off = ((32 + 4 * h.n_chunks + 15) // 16 * 16 + (h.total_len + 255) // 256 + 15) // 16 * 16
    ppc = int(_lib.lib().density_hip_paged_pages_per_chunk(h.chunk_size))
    return (off + 16 * (ppc + 1) * h.n_chunks + 255) // 256 * 256


def test_zero_chunks_seal_to_themselves_plus_the_flag():
    h = _lib.Header(0x31434844, 0, 1, 8, 65536, 0, 0, 32)
    assert _decoded_size(bytes(h)) == 0                                         # total_len 0 (and a valid header: see below)
    assert container.chunk_checksums(bytes(h)) == []
    h.n_chunks = 1                                                              # ... while one that claims a chunk is malformed either way
    assert _decoded_size(bytes(h) + bytes(32)) == 0


def test_global_layout_refuses_sealed_shards():
    """density_hip_global_layout stitches unsealed shards only: flag 8, like any bit that is no container flag, is an argument error."""
    A = ctypes.c_uint64 * 2
    out = _lib.GlobalLayout()
    call = lambda flags: _lib.lib().density_hip_global_layout(A(3, 2), A(1000, 500), A(3 * 4096, 2 * 4096), 2, 0, flags, ctypes.byref(out))
    assert call(0) == _lib.OK and call(1) == _lib.OK
    assert call(8) == _lib.ERR_ARGUMENT and call(9) == _lib.ERR_ARGUMENT and call(16) == _lib.ERR_ARGUMENT


def test_error_code_and_exception():
    from density_amd import ChecksumError, DecodeError
    assert _lib.ERR_CHECKSUM == 6 and issubclass(ChecksumError, DecodeError)
