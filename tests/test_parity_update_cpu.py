"""Parity update (include/density_hip.h: density_hip_parity_update_header / _device and the host-pointer form), what can be checked without a device: the three
calls as the header, the Python binding and the Rust shim declare them; density_hip_parity_update_header against the numpy models' headers of the edited input
for every edit the device tests run, and its refusals; the device call refusing an invalid edit from a host header without a device; and the claim the kernel
rests on — the blob is linear over the zero-padded input — in numpy, for both versions."""
import ctypes
import os
import re

import numpy as np
import pytest

import parity2_cpu
import parity_cpu
import parity_update_cases as pc
from density_amd import EncodeError, _lib, container

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CALLS = ["density_hip_parity_update_header", "density_hip_parity_update_device", "density_hip_parity_update"]
SHAPES = [(pc.TOTAL, pc.CHUNK, g) for g in pc.GROUPS] + pc.TILE_SHAPES + [pc.LONG]


def header_of(version, total, chunk, groups):
    """the header the model's blob of `total` bytes has, without making the rows"""
    n_chunks, n_groups, row_bytes = parity_cpu.geometry(total, chunk, groups)
    return _lib.ParityHeader(_lib.PARITY_MAGIC, version, 0, 0, chunk, n_chunks, total, n_groups, row_bytes)


def fields(h):
    return tuple(getattr(h, name) for name, _ in _lib.ParityHeader._fields_)


def update_header(h, edit):
    """(return code, the header written) of density_hip_parity_update_header"""
    after = _lib.ParityHeader()
    rc = _lib.lib().density_hip_parity_update_header(ctypes.byref(h), edit[0], edit[1], edit[2], ctypes.byref(after))
    return rc, after


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
    for wrapper in ("parity_update_header", "parity_update_device", "parity_update"):
        assert getattr(container, wrapper).__doc__


@pytest.mark.parametrize("version", [1, 2])
def test_update_header_is_the_models_header_of_the_edited_input(version):
    m, seen = pc.model(version), 0
    for total, chunk, groups in SHAPES:
        edits = [(total, e) for e in pc.same_size_edits(total, chunk)] + pc.tail_edits(total, chunk, min(groups, -(-total // chunk)))
        if (total, chunk, groups) == pc.LONG:
            edits.append((total, (100 * chunk, 101 * chunk, 101 * chunk)))
        for base, edit in edits:
            h = header_of(version, base, chunk, groups)
            rc, after = update_header(h, edit)
            if not pc.valid(base, chunk, groups, version, edit):
                assert rc == _lib.ERR_ARGUMENT, (base, chunk, groups, edit)
                continue
            seen += 1
            assert rc == _lib.OK, (base, chunk, groups, edit, _lib.last_error())
            new_total = base - edit[1] + edit[2]
            want = m.blob(np.zeros(new_total, dtype=np.uint8), chunk, h.n_groups)[:32]
            assert fields(after) == fields(container.parse_parity_header(want)), (base, chunk, groups, edit)
            assert fields(container.parity_update_header(h, *edit)) == fields(after)
            assert (after.n_groups, after.row_bytes, after.version, after.chunk_size) == (h.n_groups, h.row_bytes, version, chunk)
    assert seen > 80


def test_update_header_takes_a_one_chunk_input_that_stays_in_its_row():
    h = header_of(1, 1000, 65536, 3)
    assert (h.n_groups, h.row_bytes) == (1, 1008)
    rc, after = update_header(h, (1000, 0, 8))                      # 1008 bytes: the row still holds them
    assert rc == _lib.OK and (after.total_len, after.n_chunks, after.row_bytes) == (1008, 1, 1008)
    assert update_header(h, (1000, 0, 9))[0] == _lib.ERR_ARGUMENT   # 1009: the blob would have rows of 1024
    assert update_header(h, (990, 10, 0))[0] == _lib.ERR_ARGUMENT   # 990: rows of 992
    assert update_header(h, (993, 7, 0))[0] == _lib.OK              # 993: still 1008


REFUSALS = [
    # (version, total, chunk, groups, edit)
    (1, pc.TOTAL, pc.CHUNK, 2, (100, 10, 11)),                              # neither shape: sizes differ, not at the tail
    (1, pc.TOTAL, pc.CHUNK, 2, (pc.TOTAL - 5, 10, 10)),                     # ... a same-size edit that reaches past the end
    (1, pc.TOTAL, pc.CHUNK, 2, (pc.TOTAL + 1, 0, 0)),                       # ... an offset behind the end
    (1, pc.TOTAL, pc.CHUNK, 2, (pc.TOTAL - 5, 6, 0)),                       # ... old bytes the input does not have
    (1, pc.TOTAL, pc.CHUNK, 2, (pc.TOTAL, 0, (1 << 64) - pc.TOTAL)),        # offset + new_size overflows
    (1, 256 * 4, 256, 2, (256 * 4, 0, 256 * ((1 << 32) - 4))),              # 2^32 chunks
    (1, pc.TOTAL, pc.CHUNK, 3, (2 * pc.CHUNK, pc.TOTAL - 2 * pc.CHUNK, 0)),  # fewer chunks than groups
    (1, pc.TOTAL, pc.CHUNK, 3, (0, pc.TOTAL, 0)),                           # shrinking to empty
    (1, 0, pc.CHUNK, 4, (0, 0, 100)),                                       # an empty blob (no groups) growing
    (2, 0, pc.CHUNK, 4, (0, 0, 100)),
    (1, 1000, pc.CHUNK, 1, (1000, 0, 1000)),                                # a one-chunk input shorter than its chunk size growing: other rows
    (2, 1000, pc.CHUNK, 1, (500, 500, 0)),                                  # ... and shrinking
    (2, 255 * 256, 256, 1, (255 * 256, 0, 1)),                              # version 2: the 256th member of a group
]


def test_update_header_refusals():
    for version, total, chunk, groups, edit in REFUSALS:
        assert not pc.valid(total, chunk, groups, version, edit)
        h = header_of(version, total, chunk, groups)
        before = fields(h)
        after = _lib.ParityHeader()
        marker = fields(after)
        assert _lib.lib().density_hip_parity_update_header(ctypes.byref(h), *edit, ctypes.byref(after)) == _lib.ERR_ARGUMENT, (version, total, chunk, groups, edit)
        assert fields(after) == marker and fields(h) == before and _lib.last_error()
        with pytest.raises(EncodeError):
            container.parity_update_header(h, *edit)
    assert "new blob" in _lib.last_error()
    # what version 2 refuses, version 1 takes
    h = header_of(1, 255 * 256, 256, 1)
    rc, after = update_header(h, (255 * 256, 0, 1))
    assert rc == _lib.OK and (after.n_chunks, after.total_len) == (256, 255 * 256 + 1)
    # a header that is no blob's, a NULL header; header_out is optional
    for field, value in (("magic", 0x31434844), ("version", 3), ("n_groups", 0), ("n_groups", 7), ("row_bytes", 65520), ("n_chunks", 5), ("chunk_size", 100)):
        h = header_of(1, pc.TOTAL, pc.CHUNK, 2)
        setattr(h, field, value)
        assert update_header(h, (0, 16, 16))[0] == _lib.ERR_ARGUMENT, field
    assert _lib.lib().density_hip_parity_update_header(None, 0, 16, 16, None) == _lib.ERR_ARGUMENT
    assert _lib.lib().density_hip_parity_update_header(ctypes.byref(header_of(1, pc.TOTAL, pc.CHUNK, 2)), 0, 16, 16, None) == _lib.OK


def test_device_call_refuses_from_a_host_header_without_a_device():
    """decided on the host: the pointers are never followed (they point nowhere), and no device is asked for"""
    call = _lib.lib().density_hip_parity_update_device
    nowhere = 0x1000
    for version, total, chunk, groups, edit in REFUSALS:
        h = header_of(version, total, chunk, groups)
        size = 32 + version * h.n_groups * h.row_bytes
        out = _lib.ParityHeader()
        rc = call(nowhere, size, ctypes.byref(h), edit[0], nowhere, edit[1], nowhere, edit[2], None, ctypes.byref(out))
        assert rc == _lib.ERR_ARGUMENT and fields(out) == fields(_lib.ParityHeader()), (version, total, chunk, groups, edit)
    h = header_of(2, pc.TOTAL, pc.CHUNK, 2)
    size = 32 + 2 * 2 * pc.CHUNK
    assert call(0, size, ctypes.byref(h), 0, nowhere, 16, nowhere, 16, None, None) == _lib.ERR_ARGUMENT            # NULL blob
    assert call(nowhere, size, ctypes.byref(h), 0, 0, 16, nowhere, 16, None, None) == _lib.ERR_ARGUMENT            # NULL old with old bytes
    assert call(nowhere, size, ctypes.byref(h), 0, nowhere, 16, 0, 16, None, None) == _lib.ERR_ARGUMENT            # NULL new with new bytes
    assert call(nowhere, size - 1, ctypes.byref(h), 0, nowhere, 16, nowhere, 16, None, None) == _lib.ERR_FORMAT    # a blob shorter than its rows
    assert call(nowhere, 31, ctypes.byref(h), 0, nowhere, 16, nowhere, 16, None, None) == _lib.ERR_FORMAT
    for field, value in (("magic", 0x31434844), ("version", 3), ("n_groups", 0), ("n_groups", 7), ("row_bytes", 65520)):
        bad = header_of(2, pc.TOTAL, pc.CHUNK, 2)
        setattr(bad, field, value)
        assert call(nowhere, size, ctypes.byref(bad), 0, nowhere, 16, nowhere, 16, None, None) == _lib.ERR_FORMAT, field
    # a zero-length edit: OK, nothing to do, the header as it was — NULL old and new are fine with no bytes
    out = _lib.ParityHeader()
    assert call(nowhere, size, ctypes.byref(h), 100, 0, 0, 0, 0, None, ctypes.byref(out)) == _lib.OK and fields(out) == fields(h)
    # the host-pointer form: 0 and a message
    blob = parity2_cpu.blob(pc.input_of(3 * 256 + 1), 256, 2)
    with pytest.raises(EncodeError):
        container.parity_update(blob.copy(), 10, np.zeros(5, dtype=np.uint8), np.zeros(6, dtype=np.uint8))
    assert _lib.last_error()


def rows_of(version, blob):
    return np.asarray(blob[32:])


@pytest.mark.parametrize("version", [1, 2])
@pytest.mark.parametrize("total,chunk,groups,edit", [
    (5 * 4096 + 777, 4096, 2, (4096 - 5, 11, 11)),                        # across a chunk boundary
    (5 * 4096 + 777, 4096, 2, (4096 + 100, 2 * 4096, 2 * 4096)),          # over chunks 1..3: two members of group 1
    (5 * 4096 + 777, 4096, 3, (2 * 4096 + 9, 2 * 4096 + 1000, 2 * 4096 + 1000)),
    (5 * 4096 + 777, 4096, 2, (5 * 4096 + 777, 0, 1000)),                 # append onto the ragged chunk
    (5 * 4096 + 777, 4096, 2, (5 * 4096 + 777, 0, 5 * 4096 + 100)),       # ... and across it, round the groups more than once
    (5 * 4096 + 777, 4096, 2, (4 * 4096 - 3, 4096 + 780, 0)),             # truncation
    (5 * 4096 + 777, 4096, 1, (5 * 4096, 777, 9000)),                     # a tail of another length
    (255 * 256, 256, 1, (100 * 256, 101 * 256, 101 * 256)),               # places 100 .. 200 of the longest group
])
def test_the_blob_is_linear_over_the_zero_padded_input(version, total, chunk, groups, edit):
    """model(I) ^ model(I zero-padded ^ I' zero-padded) == model(I'), rows only: what lets the kernel work from old ^ new alone — and an input's zero padding to
    the longer of the two lengths changes no row"""
    m = pc.model(version)
    data, new = pc.input_of(total), pc.new_bytes(edit[2])
    after = pc.edited(data, edit, new)
    longest = max(data.size, after.size)
    delta = np.zeros(longest, dtype=np.uint8)
    delta[:data.size] ^= data
    delta[:after.size] ^= after
    assert not delta[:edit[0]].any() and (edit[1] != edit[2] or not delta[edit[0] + edit[1]:].any())
    a, b, d = m.blob(data, chunk, groups), m.blob(after, chunk, groups), m.blob(delta, chunk, groups)
    assert a.size == b.size == d.size
    assert np.array_equal(rows_of(version, a) ^ rows_of(version, d), rows_of(version, b))
    # ... and the rows of groups no edited chunk belongs to are the same before and after
    n_groups, row_bytes = container.parse_parity_header(a).n_groups, container.parse_parity_header(a).row_bytes
    touched = {i % n_groups for i in range(edit[0] // chunk, -(-(edit[0] + max(edit[1], edit[2])) // chunk))}
    for kind in range(version):
        for g in set(range(n_groups)) - touched:
            at = 32 + (kind * n_groups + g) * row_bytes
            assert np.array_equal(a[at:at + row_bytes], b[at:at + row_bytes]), (kind, g)
