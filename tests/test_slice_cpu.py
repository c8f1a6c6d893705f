"""Slices without a device.  (1) tests/slice_cpu.py — the numpy statement of what density_hip_slice_device writes — against the oracle: the slice of a
CPU-built container, in every form, is the packed container assembled from the oracle's streams of that part of the input.  (2) The two pure-arithmetic
entry points, density_hip_chunk_range and density_hip_slice_bound, through the library against the formulas of include/density_hip.h."""
import ctypes

import numpy as np
import pytest

import slice_cpu
import unpage_cases as uc
from density_amd import _lib, container
from oracle import pyoracle


def _forms(name):
    yield "paged", uc.paged(name)
    if name in uc.SHUFFLED:
        yield "shuffled", uc.paged(name, True)
    yield "packed", uc.packed(name)
    yield "sealed paged", uc.sealed(uc.paged(name), name)
    yield "sealed packed", uc.sealed(uc.packed(name), name)


def _slotted(name):
    """case `name` as a slotted container: every oracle stream in its worst-case slot, by the header's layout"""
    _, n, chunk, _ = uc.CASES[name]
    nc, _, ix0, base, _ = uc.geometry(n, chunk)
    ss = uc.streams(name)
    stride = container.slot_stride("chameleon", chunk)
    end = base + (nc - 1) * stride + len(ss[-1])
    out = np.zeros(end, dtype=np.uint8)
    out[:base] = uc.packed(name)[:base]
    hdr = container.parse_header(out[:32].tobytes())
    hdr.flags, hdr.container_len = container.FLAG_BLOCK_INDEX | container.FLAG_SLOTTED, end
    out[:32] = np.frombuffer(bytes(hdr), dtype=np.uint8)
    for i, s in enumerate(ss):
        out[base + i * stride:base + i * stride + len(s)] = np.frombuffer(s, dtype=np.uint8)
    return out


def _expected(name, first, count, sealed):
    """the packed container of the oracle's streams of data[first * chunk : ...], with the trailer of container.checksum32 where sealed"""
    _, n, chunk, _ = uc.CASES[name]
    part = uc.data(name)[first * chunk:(first + count) * chunk]
    streams = [pyoracle.encode("chameleon", part[i:i + chunk]) for i in range(0, part.size, chunk)]
    assert tuple(streams) == uc.streams(name)[first:first + count]                  # (chunks are independent streams: the part's are the whole's)
    ix0 = uc.geometry(n, chunk)[2]
    index = uc.paged(name)[ix0 + first * chunk // 256:][:(part.size + 255) // 256].tobytes()
    sums = [container.checksum32(np.ascontiguousarray(part[i:i + chunk])) for i in range(0, part.size, chunk)] if sealed else None
    return slice_cpu.assemble(0, chunk, part.size, streams, index, sums)


@pytest.mark.parametrize("name", list(uc.CASES))
def test_the_model_against_the_oracle(name):
    _, n, chunk, _ = uc.CASES[name]
    nc = (n + chunk - 1) // chunk
    for first, count in slice_cpu.windows(nc):
        want = {False: _expected(name, first, count, False), True: _expected(name, first, count, True)}
        for form, blob in _forms(name):
            got = slice_cpu.slice_container(blob, first, count)
            w = want[form.startswith("sealed")]
            assert got.size == w.size and np.array_equal(got, w), (form, first, count)
            h = container.parse_header(got[:32].tobytes())
            assert (h.n_chunks, h.chunk_size, h.container_len) == (count, chunk, got.size)
            assert h.total_len == min(n, (first + count) * chunk) - first * chunk
            assert h.flags == container.FLAG_BLOCK_INDEX | (container.FLAG_CHECKSUM if form.startswith("sealed") else 0)
    # the whole window of a packed container is that container
    assert np.array_equal(slice_cpu.slice_container(uc.packed(name), 0, nc), uc.packed(name))
    assert np.array_equal(slice_cpu.slice_container(uc.sealed(uc.paged(name), name), 0, nc), uc.sealed(uc.packed(name), name))


@pytest.mark.parametrize("name", ["a", "b"])
def test_the_model_reads_slots(name):
    _, n, chunk, _ = uc.CASES[name]
    nc = (n + chunk - 1) // chunk
    blob = _slotted(name)
    assert tuple(container.chunk_payloads(blob)[1]) == uc.streams(name)
    for sealed in (False, True):
        src = uc.sealed(blob, name) if sealed else blob
        for first, count in slice_cpu.windows(nc):
            assert np.array_equal(slice_cpu.slice_container(src, first, count), _expected(name, first, count, sealed)), (sealed, first, count)


def _header(algo, total, chunk, flags=0):
    h = _lib.Header()
    h.magic, h.algo, h.version, h.flags = 0x31434844, algo, 1, flags
    h.chunk_size, h.n_chunks, h.total_len, h.container_len = chunk, (total + chunk - 1) // chunk, total, 0
    return h


def _range(h, offset, length):
    first, count, skip = ctypes.c_uint32(77), ctypes.c_uint32(77), ctypes.c_uint64(77)
    rc = _lib.lib().density_hip_chunk_range(ctypes.byref(h), offset, length, ctypes.byref(first), ctypes.byref(count), ctypes.byref(skip))
    return rc, first.value, count.value, skip.value


def test_chunk_range_against_the_formula():
    chunk, total = 65536, 5 * 65536 + 777
    h = _header(1, total, chunk)
    cases = [(0, 1), (chunk - 1, 2), (chunk + 5, 2 * chunk), (total - 1, 1), (0, total),
             (3 * chunk + 9, total - 3 * chunk - 9),                                # offset + length == total_len
             (2 * chunk + 100, 50),                                                  # inside one chunk
             (4 * chunk + 1, chunk + 700),                                           # ends in the ragged chunk
             (chunk, chunk), (chunk, chunk + 1)]
    for offset, length in cases:
        first, last = offset // chunk, (offset + length - 1) // chunk
        assert _range(h, offset, length) == (_lib.OK, first, last - first + 1, offset - first * chunk), (offset, length)
        assert container.chunk_range(h, offset, length) == (first, last - first + 1, offset - first * chunk)
    for offset, length in [(0, 0), (5, 0), (total, 0), (total, 1), (0, total + 1), (total - 1, 2), (1 << 63, 1 << 63), ((1 << 64) - 1, 2)]:
        assert _range(h, offset, length)[0] == _lib.ERR_ARGUMENT, (offset, length)
        with pytest.raises(ValueError):
            container.chunk_range(h, offset, length)
    bad = _header(1, total, chunk)
    bad.magic = 0
    assert _range(bad, 0, 1)[0] == _lib.ERR_ARGUMENT
    assert _lib.lib().density_hip_chunk_range(None, 0, 1, None, None, None) == _lib.ERR_ARGUMENT


def test_slice_bound_against_the_formula():
    L = _lib.lib()
    for algo, name in _lib.ALGO_NAMES.items():
        for total, chunk in [(5 * 65536 + 777, 65536), (3 * (1 << 20) + 12_345, 1 << 20), (1100 * 256 + 100, 256), (65536, 65536), (40, 256)]:
            nc = (total + chunk - 1) // chunk
            for flags in (0, container.FLAG_BLOCK_INDEX, container.FLAG_CHECKSUM, container.FLAG_SLOTTED | container.FLAG_CHECKSUM):
                h = _header(algo, total, chunk, flags)
                for first, count in slice_cpu.windows(nc):
                    length = min(total, (first + count) * chunk) - first * chunk
                    want = container.container_bound(name, length, chunk) + (container.seal_overhead(length, chunk) if flags & container.FLAG_CHECKSUM else 0)
                    assert want > 0 and L.density_hip_slice_bound(ctypes.byref(h), first, count) == want == container.slice_bound(h, first, count)
                    # what the model writes for worst-case streams fits: every stream as long as {algo}_safe_encode_buffer_size lets it be
                    worst = [bytes(slice_cpu.safe_size(algo, min(chunk, length - i))) for i in range(0, length, chunk)]
                    if len(worst) <= 8:
                        made = slice_cpu.assemble(algo, chunk, length, worst, bytes((length + 255) // 256) if flags & 1 else None, [0] * len(worst) if flags & 8 else None)
                        assert made.size <= want
                for first, count in [(0, 0), (1, 0), (nc, 1), (0, nc + 1), (nc - 1, 2), (0xffffffff, 1), (1, 0xffffffff)]:
                    assert L.density_hip_slice_bound(ctypes.byref(h), first, count) == 0, (first, count)
    paged = _header(0, 3 * (1 << 20) + 5, 1 << 20, container.FLAG_PAGED | container.FLAG_BLOCK_INDEX | container.FLAG_CHECKSUM)
    assert L.density_hip_slice_bound(ctypes.byref(paged), 1, 2) == container.container_bound("chameleon", 2 << 20, 1 << 20) + container.seal_overhead(2 << 20, 1 << 20)
    bad = _header(0, 1000, 256)
    bad.n_chunks = 3
    assert L.density_hip_slice_bound(ctypes.byref(bad), 0, 1) == 0 and L.density_hip_slice_bound(None, 0, 1) == 0
