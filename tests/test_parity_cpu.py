"""Recovery records, what can be checked without a device: density_hip_parity_size against the header file's formula, the parity header's layout, the calls
and constants as the header, the Python binding and the Rust shim declare them, and the numpy model of the blob (parity_cpu.py, which the device tests hold
the kernels against) rebuilding every chunk it promises to."""
import ctypes
import os
import re

import numpy as np
import pytest

import datagen
import parity_cpu
from density_amd import DecodeError, _lib, container

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CALLS = ["density_hip_parity_size", "density_hip_parity_device", "density_hip_parity", "density_hip_decode_device_recover", "density_hip_decode_recover"]
CONSTANTS = {"DENSITY_HIP_CHUNK_RECOVERED": "2", "DENSITY_HIP_PARITY_MAGIC": "0x31504844"}

# (input bytes, chunk size, groups asked for)
SHAPES = [
    (1000, 65536, 1),                       # one chunk, shorter than the chunk size: the row is the input rounded up to 16
    (1000, 65536, 5),                       # ... and more groups than chunks
    (65536, 65536, 1),                      # one chunk exactly
    (5 * 65536 + 777, 65536, 2),            # a ragged last chunk
    (5 * 65536 + 777, 65536, 6),            # a group per chunk
    (5 * 65536 + 777, 65536, 7),            # clamps to 6
    (3 * 256 + 1, 256, 3),                  # the smallest chunk
    ((1 << 30) + 5, 4 << 20, 16),
    (0, 65536, 4),                          # zero bytes: a bare header
    (0, 65536, 0),
]
INVALID = [(1000, 0, 2), (1000, 100, 2), (1000, 65536 + 1, 2), (1000, (1 << 30) + 256, 2), (1000, 65536, 0), (1 << 42, 256, 2)]


def test_parity_size_is_the_formula():
    size = _lib.lib().density_hip_parity_size
    for n, chunk, groups in SHAPES:
        n_chunks = -(-n // chunk)
        want = 32 + min(groups, n_chunks) * ((min(chunk, n) + 15) // 16 * 16)
        assert size(n, chunk, groups) == want == parity_cpu.size(n, chunk, groups) == container.parity_size(n, chunk, groups), (n, chunk, groups)
    assert size(0, 65536, 4) == 32
    for n, chunk, groups in INVALID:
        assert size(n, chunk, groups) == 0, (n, chunk, groups)


def test_parity_header_is_32_bytes():
    assert ctypes.sizeof(_lib.ParityHeader) == 32 == parity_cpu.HEADER.size
    offsets = {name: getattr(_lib.ParityHeader, name).offset for name, _ in _lib.ParityHeader._fields_}
    assert offsets == {"magic": 0, "version": 4, "reserved0": 5, "reserved1": 6, "chunk_size": 8, "n_chunks": 12, "total_len": 16, "n_groups": 24, "row_bytes": 28}
    data = datagen.by_kind("mixed", 3 * 256 + 1, seed=5)
    h = container.parse_parity_header(parity_cpu.blob(data, 256, 3))
    assert (h.magic, h.version, h.chunk_size, h.n_chunks, h.total_len, h.n_groups, h.row_bytes) == (_lib.PARITY_MAGIC, 1, 256, 4, 769, 3, 256)
    with pytest.raises(DecodeError):
        container.parse_parity_header(b"DHC1" + bytes(28))
    with pytest.raises(DecodeError):
        container.parse_parity_header(b"DHP1")


def test_header_binding_and_rust_shim_declare_the_same():
    header = open(os.path.join(ROOT, "include", "density_hip.h")).read()
    rust = open(os.path.join(ROOT, "bindings", "rust", "src", "lib.rs")).read()
    for name, value in CONSTANTS.items():
        assert re.search(r"^#define %s %su\b" % (name, value), header, flags=re.M), name
        assert re.search(r"pub const %s: u32 = %s;" % (name, value), rust), name
    assert (_lib.CHUNK_RECOVERED, _lib.PARITY_MAGIC) == (2, 0x31504844)
    bare = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    for name in CALLS:
        assert re.search(r"^(int|size_t) %s\(" % name, header, flags=re.M), name
        assert name in _lib.SYMBOLS and hasattr(_lib.lib(), name)
        c_args = re.search(r"%s\(([^;]*)\);" % name, bare).group(1).split(",")
        rust_args = re.search(r"pub fn %s\(([^;]*)\) ->" % name, rust, flags=re.S).group(1).split(",")
        assert [a.split()[-1].lstrip("*") for a in c_args] == [a.split(":")[0].strip() for a in rust_args], name
        assert len(c_args) == len(_lib.SYMBOLS[name][1]), name
    # the struct, field for field
    c_fields = re.findall(r"(\w+);", re.search(r"typedef struct density_hip_parity_header \{(.*?)\}", bare, flags=re.S).group(1))
    rust_fields = re.findall(r"pub (\w+):", re.search(r"pub struct DensityHipParityHeader \{(.*?)\}", rust, flags=re.S).group(1))
    assert c_fields == rust_fields == [name for name, _ in _lib.ParityHeader._fields_]


@pytest.mark.parametrize("n,chunk,groups", [(5 * 4096 + 777, 4096, 1), (5 * 4096 + 777, 4096, 2), (5 * 4096 + 777, 4096, 4), (5 * 4096 + 777, 4096, 6), (5 * 4096 + 777, 4096, 7),
                                            (1000, 4096, 3), (4 * 256, 256, 3)])
def test_model_rebuilds_any_single_chunk_of_every_group(n, chunk, groups):
    data = datagen.by_kind("mixed", n, seed=17)
    blob = parity_cpu.blob(data, chunk, groups)
    c, n_chunks, total, n_groups, row_bytes, rows = parity_cpu.parse(blob)
    assert (c, n_chunks, total, n_groups) == (chunk, -(-n // chunk), n, min(groups, n_chunks)) and blob.size == parity_cpu.size(n, chunk, groups)
    assert row_bytes % 16 == 0 and row_bytes - 16 < min(chunk, n) <= row_bytes
    for k in range(n_chunks):
        wrecked = data.copy()
        wrecked[k * chunk:(k + 1) * chunk] = 0xEE
        assert np.array_equal(parity_cpu.rebuild(blob, wrecked, k), data[k * chunk:(k + 1) * chunk]), k
    # a burst of n_groups neighbours: one chunk per group, each rebuilt from the members that are left
    for first in range(n_chunks - n_groups + 1):
        wrecked = data.copy()
        wrecked[first * chunk:(first + n_groups) * chunk] = 0xEE
        for k in range(first, first + n_groups):
            assert np.array_equal(parity_cpu.rebuild(blob, wrecked, k), data[k * chunk:(k + 1) * chunk]), (first, k)
    # two chunks of one group: the row cannot tell them apart
    if n_chunks > n_groups:
        wrecked = data.copy()
        wrecked[0:chunk] = 0xEE
        wrecked[n_groups * chunk:(n_groups + 1) * chunk] = 0xEE
        assert not np.array_equal(parity_cpu.rebuild(blob, wrecked, 0), data[:chunk])


def test_a_rebuilt_chunk_has_the_sealed_checksum():
    """what a CPU reader does: XOR, then density_hip_checksum32 against the trailer's entry"""
    n, chunk = 5 * 4096 + 777, 4096
    data = datagen.by_kind("prose", n, seed=3)
    sums = [container.checksum32(data[i:i + chunk]) for i in range(0, n, chunk)]
    blob = parity_cpu.blob(data, chunk, 2)
    for k in (0, 3, 5):
        wrecked = data.copy()
        wrecked[k * chunk + 9] ^= 0x10
        assert container.checksum32(wrecked[k * chunk:(k + 1) * chunk]) != sums[k]
        assert container.checksum32(parity_cpu.rebuild(blob, wrecked, k)) == sums[k]
        bad_row = blob.copy()
        bad_row[parity_cpu.row_offset(blob, k % 2, 100)] ^= 0x01
        assert container.checksum32(parity_cpu.rebuild(bad_row, wrecked, k)) != sums[k]
