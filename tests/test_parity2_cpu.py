"""Double parity (version 2 of the parity blob: include/density_hip.h), what can be checked without a device: density_hip_parity2_size against the header
file's formula and its limit of 255 chunks a group, the three calls as the header, the Python binding and the Rust shim declare them, and the numpy model of the
blob (parity2_cpu.py, which the device tests hold the kernels against) rebuilding every pair of chunks it promises to."""
import itertools
import os
import re

import numpy as np
import pytest

import datagen
import parity2_cpu
import parity_cpu
from density_amd import DecodeError, _lib, container
from test_parity_cpu import INVALID, SHAPES

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CALLS = ["density_hip_parity2_size", "density_hip_parity2_device", "density_hip_parity2"]


def test_parity2_size_is_the_formula():
    size = _lib.lib().density_hip_parity2_size
    for n, chunk, groups in SHAPES:
        n_chunks = -(-n // chunk)
        want = 32 + 2 * min(groups, n_chunks) * ((min(chunk, n) + 15) // 16 * 16)
        assert size(n, chunk, groups) == want == parity2_cpu.size(n, chunk, groups) == container.parity2_size(n, chunk, groups), (n, chunk, groups)
        assert want - 32 == 2 * (container.parity_size(n, chunk, groups) - 32)
    assert size(0, 65536, 4) == 32
    for n, chunk, groups in INVALID:
        assert size(n, chunk, groups) == 0, (n, chunk, groups)


def test_a_group_has_at_most_255_members():
    size = _lib.lib().density_hip_parity2_size
    n = 255 * 256 + 100                                    # 256 chunks of 256 bytes
    assert size(n, 256, 2) == 32 + 2 * 2 * 256 == parity2_cpu.size(n, 256, 2)            # 128 members a group
    assert size(n, 256, 1) == 0 == parity2_cpu.size(n, 256, 1)                           # 256 members
    assert container.parity_size(n, 256, 1) == 32 + 256                                  # (version 1 has no such limit)
    assert size(255 * 256, 256, 1) == 32 + 2 * 256 == parity2_cpu.size(255 * 256, 256, 1)   # 255 members: the longest group


def test_header_is_version_2():
    data = datagen.by_kind("mixed", 3 * 256 + 1, seed=5)
    blob = parity2_cpu.blob(data, 256, 3)
    h = container.parse_parity_header(blob)
    assert (h.magic, h.version, h.reserved0, h.reserved1, h.chunk_size, h.n_chunks, h.total_len, h.n_groups, h.row_bytes) == (_lib.PARITY_MAGIC, 2, 0, 0, 256, 4, 769, 3, 256)
    assert blob.size == 32 + 2 * 3 * 256
    three = blob.copy()
    three[4] = 3
    with pytest.raises(DecodeError):
        container.parse_parity_header(three)
    empty = parity2_cpu.blob(np.zeros(0, dtype=np.uint8), 65536, 4)
    h = container.parse_parity_header(empty)
    assert empty.size == 32 and (h.version, h.n_groups, h.n_chunks, h.total_len) == (2, 0, 0, 0)


def test_header_binding_and_rust_shim_declare_the_same():
    header = open(os.path.join(ROOT, "include", "density_hip.h")).read()
    rust = open(os.path.join(ROOT, "bindings", "rust", "src", "lib.rs")).read()
    bare = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    for name in CALLS:
        assert re.search(r"^(int|size_t) %s\(" % name, header, flags=re.M), name
        assert name in _lib.SYMBOLS and hasattr(_lib.lib(), name)
        c_args = re.search(r"%s\(([^;]*)\);" % name, bare).group(1).split(",")
        rust_args = re.search(r"pub fn %s\(([^;]*)\) ->" % name, rust, flags=re.S).group(1).split(",")
        assert [a.split()[-1].lstrip("*") for a in c_args] == [a.split(":")[0].strip() for a in rust_args], name
        assert len(c_args) == len(_lib.SYMBOLS[name][1]), name
        # ... and the same arguments as the version-1 call it mirrors
        v1 = re.search(r"%s\(([^;]*)\);" % name.replace("parity2", "parity"), bare).group(1)
        assert [a.strip() for a in v1.split(",")] == [a.strip() for a in c_args], name
        assert _lib.SYMBOLS[name] == _lib.SYMBOLS[name.replace("parity2", "parity")], name


@pytest.mark.parametrize("n,chunk,groups", [(n, chunk, groups) for n, chunk, groups in SHAPES if 0 < n <= 1 << 20] + [(5 * 4096 + 777, 4096, 2)])
def test_p_rows_are_the_version_1_rows(n, chunk, groups):
    data = datagen.by_kind("mixed", n, seed=17)
    v1, v2 = parity_cpu.blob(data, chunk, groups), parity2_cpu.blob(data, chunk, groups)
    assert v2.size == parity2_cpu.size(n, chunk, groups) == 2 * v1.size - 32
    assert np.array_equal(parity2_cpu.as_version_1(v2), v1)
    assert np.array_equal(v2[:4], v1[:4]) and v2[4] == 2 and np.array_equal(v2[5:v1.size], v1[5:])


@pytest.mark.parametrize("groups", [1, 2, 3])
def test_model_rebuilds_any_pair_of_every_group(groups):
    n, chunk = 5 * 65536 + 777, 65536
    data = datagen.by_kind("mixed", n, seed=17)
    blob = parity2_cpu.blob(data, chunk, groups)
    n_chunks = 6
    pairs = [(k1, k2) for k1, k2 in itertools.combinations(range(n_chunks), 2) if k1 % groups == k2 % groups]
    assert len(pairs) == {1: 15, 2: 6, 3: 3}[groups] and any(k2 == n_chunks - 1 for _, k2 in pairs)        # (pairs with the ragged last chunk among them)
    for k1, k2 in pairs:
        wrecked = data.copy()
        wrecked[k1 * chunk:(k1 + 1) * chunk] = 0xEE
        wrecked[k2 * chunk:(k2 + 1) * chunk] = 0x77
        d1, d2 = parity2_cpu.rebuild_two(blob, wrecked, k1, k2)
        assert np.array_equal(d1, data[k1 * chunk:(k1 + 1) * chunk]) and np.array_equal(d2, data[k2 * chunk:(k2 + 1) * chunk]), (k1, k2)
    # one lost chunk: from P, as with version 1
    for k in range(n_chunks):
        wrecked = data.copy()
        wrecked[k * chunk:(k + 1) * chunk] = 0xEE
        assert np.array_equal(parity2_cpu.rebuild_one(blob, wrecked, k), data[k * chunk:(k + 1) * chunk]), k


def test_model_rebuilds_pairs_of_the_longest_group():
    n, chunk = 255 * 256 - 100, 256                      # 255 members, the last one ragged
    data = datagen.by_kind("mixed", n, seed=23)
    blob = parity2_cpu.blob(data, chunk, 1)
    for k1, k2 in ((0, 254), (0, 1), (253, 254), (7, 200)):
        wrecked = data.copy()
        wrecked[k1 * chunk:(k1 + 1) * chunk] = 0xEE
        wrecked[k2 * chunk:(k2 + 1) * chunk] = 0x77
        d1, d2 = parity2_cpu.rebuild_two(blob, wrecked, k1, k2)
        assert np.array_equal(d1, data[k1 * chunk:(k1 + 1) * chunk]) and np.array_equal(d2, data[k2 * chunk:(k2 + 1) * chunk]), (k1, k2)


def test_a_damaged_q_row_fails_the_sealed_checksum():
    """what a CPU reader does: the solve, then density_hip_checksum32 of each chunk against its trailer entry"""
    n, chunk = 5 * 4096 + 777, 4096
    data = datagen.by_kind("prose", n, seed=3)
    sums = [container.checksum32(data[i:i + chunk]) for i in range(0, n, chunk)]
    blob = parity2_cpu.blob(data, chunk, 2)
    for k1, k2 in ((0, 2), (1, 5), (3, 5)):
        wrecked = data.copy()
        wrecked[k1 * chunk + 9] ^= 0x10
        wrecked[k2 * chunk + 9] ^= 0x10
        d1, d2 = parity2_cpu.rebuild_two(blob, wrecked, k1, k2)
        assert (container.checksum32(d1), container.checksum32(d2)) == (sums[k1], sums[k2])
        bad_row = blob.copy()
        bad_row[parity2_cpu.row_offset(blob, k1 % 2, 100, q=True)] ^= 0x01
        d1, d2 = parity2_cpu.rebuild_two(bad_row, wrecked, k1, k2)
        assert container.checksum32(d1) != sums[k1] and container.checksum32(d2) != sums[k2]
        # Q is not read for one lost chunk
        wrecked[k2 * chunk + 9] ^= 0x10
        assert container.checksum32(parity2_cpu.rebuild_one(bad_row, wrecked, k1)) == sums[k1]
