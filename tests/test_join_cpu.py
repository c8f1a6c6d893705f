"""Joins without a device.  (1) tests/join_cpu.py — the numpy statement of what density_hip_join_device writes — against the oracle: the join of CPU-built
containers, in every form, is the packed container assembled from the oracle's streams of the inputs one behind the other, and its streams decode to them;
a container cut in two slices joins back to itself.  (2) The two pure-arithmetic entry points, density_hip_join_bound and density_hip_join_workspace_size,
through the library against the formulas of include/density_hip.h."""
import ctypes

import numpy as np
import pytest

import join_cpu
import paged_cpu
import slice_cpu
import unpage_cases as uc
from density_amd import _lib, container
from oracle import pyoracle

FORMS = ["packed", "paged", "shuffled"]


def _blob(name, form, seal):
    blob = uc.packed(name) if form == "packed" else uc.paged(name, form == "shuffled" and name in uc.SHUFFLED)
    return uc.sealed(blob, name) if seal else blob


def _expected(data, chunk, seal):
    """the packed container of the oracle's streams of `data` cut every `chunk`, with its block index and, sealed, the trailer of container.checksum32"""
    pieces = [np.ascontiguousarray(data[i:i + chunk]) for i in range(0, data.size, chunk)]
    streams = [pyoracle.encode("chameleon", p) for p in pieces]
    index = b"".join(bytes(b for b, _ in paged_cpu.walk_records(s, p.size)) for s, p in zip(streams, pieces))
    return slice_cpu.assemble(0, chunk, data.size, streams, index, [container.checksum32(p) for p in pieces] if seal else None), streams, pieces


@pytest.mark.parametrize("seal", [False, True])
def test_the_model_against_the_oracle(seal):
    chunk = uc.CASES["c"][2]
    assert uc.CASES["d"][2] == chunk and uc.CASES["c"][1] % chunk == 0 and uc.CASES["d"][1] % chunk != 0
    data = np.concatenate([uc.data("c"), uc.data("d")])
    want, streams, pieces = _expected(data, chunk, seal)
    nc, nd = 4, 3
    for fc in FORMS:
        for fd in FORMS:
            got = join_cpu.join_containers([(_blob("c", fc, seal), 0, nc), (_blob("d", fd, seal), 0, nd)])
            assert got.size == want.size and np.array_equal(got, want), (fc, fd)
    h = container.parse_header(want[:32].tobytes())
    assert (h.n_chunks, h.total_len, h.chunk_size, h.container_len) == (nc + nd, data.size, chunk, want.size)
    assert h.flags == container.FLAG_BLOCK_INDEX | (container.FLAG_CHECKSUM if seal else 0)
    for s, p in zip(slice_cpu.chunk_streams(want, range(nc + nd)), pieces):      # the joined container's streams decode, through the reference, to the input
        assert pyoracle.decode("chameleon", s, p.size) == p.tobytes()
    # skipped parts are not there, and windows are taken where they are asked for
    got = join_cpu.join_containers([(_blob("d", "paged", seal), 1, 0), (_blob("c", "paged", seal), 1, 2), (_blob("c", "packed", seal), 0, 0), (_blob("d", "packed", seal), 1, 2)])
    part = np.concatenate([uc.data("c")[chunk:3 * chunk], uc.data("d")[chunk:]])
    assert np.array_equal(got, _expected(part, chunk, seal)[0])


@pytest.mark.parametrize("form,seal", [("packed", False), ("paged", True), ("shuffled", False), ("packed", True)])
def test_two_slices_join_back_to_the_container(form, seal):
    blob = _blob("a", form, seal)
    n = container.parse_header(blob[:32].tobytes()).n_chunks
    whole = slice_cpu.slice_container(blob, 0, n)
    for k in range(1, n):
        halves = [slice_cpu.slice_container(blob, 0, k), slice_cpu.slice_container(blob, k, n - k)]
        assert np.array_equal(join_cpu.join_containers([(halves[0], 0, k), (halves[1], 0, n - k)]), whole), k
        assert np.array_equal(join_cpu.join_containers([(blob, 0, k), (halves[1], 0, n - k)]), whole), k


def test_the_model_refuses_what_the_call_refuses():
    with pytest.raises(AssertionError):
        join_cpu.join_containers([(uc.packed("d"), 0, 3), (uc.packed("c"), 0, 4)])        # a ragged chunk in front of others
    with pytest.raises(AssertionError):
        join_cpu.join_containers([(uc.packed("c"), 0, 4), (uc.sealed(uc.packed("d"), "d"), 0, 3)])
    with pytest.raises(AssertionError):
        join_cpu.join_containers([(uc.packed("c"), 0, 4), (uc.packed("a"), 0, 1)])        # another chunk size


# ---- host arithmetic through the library ----

def _header(algo, total, chunk, flags=0):
    h = _lib.Header()
    h.magic, h.algo, h.version, h.flags = 0x31434844, algo, 1, flags
    h.chunk_size, h.n_chunks, h.total_len, h.container_len = chunk, (total + chunk - 1) // chunk, total, 0
    return h


SOMEWHERE = 0x1000          # a pointer that is not NULL: the bound reads no container


def _parts(rows):
    """(JoinPart array, its length) of [(header or None, first, count), ...] or of rows that name pointer and size too"""
    arr = (_lib.JoinPart * max(len(rows), 1))()
    for i, row in enumerate(rows):
        ptr, size, h, first, count = row if len(row) == 5 else (SOMEWHERE, 1 << 40) + tuple(row)
        arr[i] = _lib.JoinPart(ptr, size, ctypes.pointer(h) if h is not None else None, first, count)
    return arr, len(rows)


def _bound(rows):
    return int(_lib.lib().density_hip_join_bound(*_parts(rows)))


def test_join_bound_against_the_formula():
    for algo, name in _lib.ALGO_NAMES.items():
        for chunk, totals in [(65536, [4 * 65536, 2 * 65536, 3 * 65536 + 777]), (1 << 20, [2 << 20, (2 << 20) + 12_345]), (256, [1100 * 256, 256 * 7 + 100])]:
            for flags in (0, container.FLAG_BLOCK_INDEX, container.FLAG_CHECKSUM, container.FLAG_BLOCK_INDEX | container.FLAG_CHECKSUM):
                forms = [0, container.FLAG_SLOTTED, 0]
                rows = [(_header(algo, t, chunk, flags | f), 0, (t + chunk - 1) // chunk) for t, f in zip(totals, forms)]
                L = sum(totals)
                want = container.container_bound(name, L, chunk) + (container.seal_overhead(L, chunk) if flags & container.FLAG_CHECKSUM else 0)
                assert want > 0 and _bound(rows) == want, (name, chunk, flags)
                assert container.join_bound([(SOMEWHERE, 1 << 40) + r for r in rows]) == want
                # windows, and skipped parts anywhere — one with nothing behind its pointers too
                rows2 = [(None, 5, 0), (rows[0][0], 1, 1), (0, 0, None, 0, 0), (rows[-1][0], 0, rows[-1][2])]
                L2 = chunk + totals[-1]
                want2 = container.container_bound(name, L2, chunk) + (container.seal_overhead(L2, chunk) if flags & container.FLAG_CHECKSUM else 0)
                assert _bound(rows2) == want2
    # the cases of the model's test: c then d, and a paged part beside a packed one
    for seal in (False, True):
        rows = [(container.parse_header(b[:32].tobytes()), 0, n) for b, n in ((uc.sealed(uc.paged("c"), "c") if seal else uc.paged("c"), 4),
                                                                              (uc.sealed(uc.packed("d"), "d") if seal else uc.packed("d"), 3))]
        L = uc.CASES["c"][1] + uc.CASES["d"][1]
        assert _bound(rows) == container.container_bound("chameleon", L, 256 << 10) + (container.seal_overhead(L, 256 << 10) if seal else 0)


def test_join_bound_is_zero_for_what_the_host_refuses():
    chunk = 65536
    a, b = _header(1, 4 * chunk, chunk), _header(1, 2 * chunk + 5, chunk)
    assert _bound([(a, 0, 4), (b, 0, 3)]) > 0
    refused = {
        "no parts": [],
        "65 parts": [(a, 0, 1)] * 65,
        "all parts skipped": [(a, 0, 0), (b, 2, 0)],
        "a NULL header": [(a, 0, 4), (None, 0, 3)],
        "a NULL pointer": [(a, 0, 4), (0, 1 << 40, b, 0, 3)],
        "a container shorter than a header": [(a, 0, 4), (SOMEWHERE, 31, b, 0, 3)],
        "another algorithm": [(a, 0, 4), (_header(2, 2 * chunk + 5, chunk), 0, 3)],
        "another chunk size": [(a, 0, 4), (_header(1, 2 * chunk + 5, 2 * chunk), 0, 2)],
        "another index flag": [(a, 0, 4), (_header(1, 2 * chunk + 5, chunk, container.FLAG_BLOCK_INDEX), 0, 3)],
        "another seal flag": [(a, 0, 4), (_header(1, 2 * chunk + 5, chunk, container.FLAG_CHECKSUM), 0, 3)],
        "a ragged window that is not last": [(b, 0, 3), (a, 0, 4)],
        "a ragged window in front of a skipped part and a live one": [(b, 2, 1), (a, 0, 0), (a, 0, 1)],
        "a window outside the chunks": [(a, 0, 4), (b, 1, 3)],
        "a window that starts behind the chunks": [(a, 4, 1)],
        "a window whose end wraps": [(a, 0xffffffff, 2)],
        "not a container's header": [(a, 0, 4), (_header(1, 2 * chunk + 5, chunk + 1), 0, 3)],
    }
    bad_magic = _header(1, 4 * chunk, chunk)
    bad_magic.magic ^= 1
    refused["a wrong magic"] = [(bad_magic, 0, 4)]
    for what, rows in refused.items():
        assert _bound(rows) == 0, what
    assert int(_lib.lib().density_hip_join_bound(None, 1)) == 0
    # 64 parts are taken; a ragged LAST window is; a ragged window in front of skipped parts only is
    assert _bound([(a, 0, 1)] * 64) == container.container_bound("cheetah", 64 * chunk, chunk)
    assert _bound([(a, 1, 2), (b, 2, 1), (a, 0, 0)]) == container.container_bound("cheetah", 2 * chunk + 5, chunk)
    # more chunks than a header counts: 64 windows of 2^26 chunks of 256 bytes
    big = _header(0, 256 << 26, 256)
    assert _bound([(big, 0, 1 << 26)] * 63) > 0 and _bound([(big, 0, 1 << 26)] * 64) == 0


def test_join_workspace_size_is_monotone():
    size = _lib.lib().density_hip_join_workspace_size
    ns, ps = (1, 2, 31, 32, 33, 1100, 2273, 1 << 20, 0xffffffff), (1, 2, 17, 64)
    table = [[int(size(p, n)) for p in ps] for n in ns]
    for n, row in zip(ns, table):
        assert all(v > 0 for v in row) and row == sorted(row), (n, row)
        assert row[0] >= 3 * 8 * n, "three words per output chunk"
    for column in zip(*table):
        assert list(column) == sorted(column), column
    assert container.join_workspace_size(3, 7) == int(size(3, 7))
    for p, n in [(0, 5), (65, 5), (3, 0)]:
        assert int(size(p, n)) == 0
