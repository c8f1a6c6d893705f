"""Parity update (include/density_hip.h: density_hip_parity_update_device and its host-pointer form): a parity blob of either version kept current after its
input was edited, appended to or truncated, from the old and the new bytes alone.

The expected blob is always the numpy model (parity_cpu.py / parity2_cpu.py) run on the EDITED input with the blob's own n_groups, and the blob the device
updates is the MODEL's blob of the old input — so no two kernels are checked against each other.  The blob, the old bytes and the new bytes each lie in 0xA5
guards, which are checked; old and new must come back unchanged.  The shapes and edits are those of parity_update_cases.py.

A library call with a NULL stream runs on the library's own stream, not torch's: buffers filled with torch are synchronised first."""
import ctypes

import numpy as np
import pytest

import parity2_cpu
import parity_cpu
import parity_update_cases as pc
import verdict_cases as vc
from density_amd import EncodeError, _lib, container
from test_gpu_parity import DAMAGED, OK, POISON, RECOVERED, check_contract, recover_decode
from test_gpu_verdicts import flipped, sealed

pytestmark = pytest.mark.gpu

GUARD = 64


def guarded(arr, offset=0):
    """(tensor, device address): `arr` at GUARD + offset bytes into a buffer of 0xA5 with GUARD bytes and more behind it"""
    import torch
    buf = torch.full((GUARD + offset + arr.size + GUARD,), POISON, dtype=torch.uint8, device="cuda")
    if arr.size:
        buf[GUARD + offset:GUARD + offset + arr.size] = torch.from_numpy(np.ascontiguousarray(arr))
    return buf, buf.data_ptr() + GUARD + offset


def content(buf, size, offset=0):
    """the `size` bytes guarded() placed, the guards around them checked"""
    got = buf.cpu().numpy()
    at = GUARD + offset
    assert (got[:at] == POISON).all() and (got[at + size:] == POISON).all(), "bytes around the buffer written"
    return got[at:at + size]


def update(blob, offset, old, new, offsets=(0, 0, 0), with_header=True, stream=0):
    """One density_hip_parity_update_device on the host blob `blob`: (the blob afterwards, the header returned).  Guards checked, old and new unchanged."""
    import torch
    d_blob, bptr = guarded(blob, offsets[0])
    d_old, optr = guarded(old, offsets[1])
    d_new, nptr = guarded(new, offsets[2])
    torch.cuda.synchronize()
    hdr = container.parity_update_device(bptr, blob.size, offset, optr if old.size else 0, old.size, nptr if new.size else 0, new.size,
                                         parity_header=container.parse_parity_header(blob) if with_header else None, stream=stream)
    torch.cuda.synchronize()
    assert np.array_equal(content(d_old, old.size, offsets[1]), old) and np.array_equal(content(d_new, new.size, offsets[2]), new), "old or new bytes written"
    return content(d_blob, blob.size, offsets[0]), hdr


def fields(h):
    return tuple(getattr(h, name) for name, _ in _lib.ParityHeader._fields_)


def check_edit(version, total, chunk, groups, edit, offsets=(0, 0, 0), with_header=True):
    data, new = pc.input_of(total), pc.new_bytes(edit[2])
    before, want, after = pc.blobs(version, data, chunk, groups, edit, new)
    assert before.size == want.size
    got, hdr = update(before, edit[0], np.array(data[edit[0]:edit[0] + edit[1]]), new, offsets, with_header)
    assert np.array_equal(got, want), (version, total, chunk, groups, edit, offsets, np.flatnonzero(got != want)[:8])
    assert fields(hdr) == fields(container.parse_parity_header(want))


# ------------------------------------------------------------------------------------------------------------------------------------------
# same-size edits

@pytest.mark.parametrize("version", [1, 2])
@pytest.mark.parametrize("groups", pc.GROUPS)
def test_same_size_edits(version, groups):
    """every whole chunk, ranges inside a slot, across a slot, a tile and a chunk boundary, ranges over three chunks (with two groups: two members of one group,
    from place 0 and from place 1)"""
    edits = pc.same_size_edits(pc.TOTAL, pc.CHUNK)
    assert len(edits) == 6 + 6 and all(pc.valid(pc.TOTAL, pc.CHUNK, groups, version, e) for e in edits)
    for edit in edits:
        check_edit(version, pc.TOTAL, pc.CHUNK, groups, edit)


@pytest.mark.parametrize("version", [1, 2])
@pytest.mark.parametrize("total,chunk,groups", pc.TILE_SHAPES)
def test_chunk_sizes_around_the_row_tile(version, total, chunk, groups):
    for edit in pc.same_size_edits(total, chunk):
        check_edit(version, total, chunk, groups, edit)


@pytest.mark.parametrize("version", [1, 2])
def test_longest_group(version):
    """255 members in one group: chunks 100 .. 200 — Horner over 101 members, then the product with 2^100 —, the whole input, the last member alone"""
    total, chunk, groups = pc.LONG
    for edit in ((100 * chunk, 101 * chunk, 101 * chunk), (0, total, total), (254 * chunk, chunk, chunk), (17 * chunk + 3, 40, 40)):
        check_edit(version, total, chunk, groups, edit)


@pytest.mark.parametrize("version", [1, 2])
def test_any_alignment(version):
    """the blob, the old bytes and the new bytes at byte offsets 0, 1 and 3 of their buffers; the header read back from the device as well"""
    edits = [(pc.CHUNK - 5, 11, 11), (3 * pc.CHUNK, pc.CHUNK, pc.CHUNK), (5 * pc.CHUNK, 777, 777), (pc.TOTAL, 0, 1000)]
    for offsets in ((1, 0, 0), (0, 1, 0), (0, 0, 1), (3, 1, 0), (0, 3, 1), (1, 0, 3), (3, 3, 3)):
        for edit in edits:
            check_edit(version, pc.TOTAL, pc.CHUNK, 2, edit, offsets, with_header=offsets[0] != 3)


# ------------------------------------------------------------------------------------------------------------------------------------------
# edits of the tail

@pytest.mark.parametrize("version", [1, 2])
@pytest.mark.parametrize("groups", [1, 2, 3])
def test_tail_edits(version, groups):
    """append at a chunk boundary, onto the ragged chunk, over five chunks and more; truncation by part of the ragged chunk, by more than a chunk, down to
    n_groups chunks; a tail of 1000 replaced by 70 000"""
    edits = pc.tail_edits(pc.TOTAL, pc.CHUNK, groups)
    assert len(edits) == 7
    for base, edit in edits:
        assert pc.valid(base, pc.CHUNK, groups, version, edit), edit
        check_edit(version, base, pc.CHUNK, groups, edit)


@pytest.mark.parametrize("version", [1, 2])
def test_one_chunk_shorter_than_its_size(version):
    """a row of 1008 bytes: edits inside it, and a tail that stays inside the row's length"""
    for edit in ((3, 990, 990), (1000, 0, 8), (993, 7, 0), (990, 10, 15)):
        assert pc.valid(1000, 65536, 3, version, edit)
        check_edit(version, 1000, 65536, 3, edit)


@pytest.mark.parametrize("version", [1, 2])
def test_a_chain_of_edits(version):
    """a same-size edit, an append, a same-size edit in the appended part, a truncation — one after the other on one blob"""
    chunk, groups = pc.CHUNK, 2
    data = np.array(pc.input_of(pc.TOTAL))
    blob = pc.model(version).blob(data, chunk, groups)
    chain = [(chunk + 77, 3000, 3000), (pc.TOTAL, 0, 2 * chunk + 55), (6 * chunk + 10, chunk, chunk), (4 * chunk + 5, None, 0)]
    for i, (offset, old_size, new_size) in enumerate(chain):
        old_size = data.size - offset if old_size is None else old_size
        new = pc.new_bytes(new_size, seed=100 + i)
        blob, hdr = update(blob, offset, data[offset:offset + old_size].copy(), new)
        data = pc.edited(data, (offset, old_size, new_size), new)
        assert hdr.total_len == data.size
    assert data.size == 4 * chunk + 5
    assert np.array_equal(blob, pc.model(version).blob(data, chunk, groups)), np.flatnonzero(blob != pc.model(version).blob(data, chunk, groups))[:8]


# ------------------------------------------------------------------------------------------------------------------------------------------
# refusals, the asynchronous form, host pointers

def test_refusals_write_nothing():
    import torch
    call = _lib.lib().density_hip_parity_update_device
    data = pc.input_of(pc.TOTAL)
    some, sptr = guarded(np.array(data[:70_000]))

    def refused(blob, edit, want_rc, size=None, with_header=True):
        d_blob, bptr = guarded(blob)
        before = d_blob.cpu().numpy()
        torch.cuda.synchronize()
        h = _lib.ParityHeader.from_buffer_copy(bytes(blob[:32])) if with_header else None
        out = _lib.ParityHeader()
        rc = call(bptr, blob.size if size is None else size, ctypes.byref(h) if h is not None else None, edit[0], sptr, edit[1], sptr, edit[2], None, ctypes.byref(out))
        torch.cuda.synchronize()
        assert rc == want_rc, (edit, rc, _lib.last_error())
        assert np.array_equal(d_blob.cpu().numpy(), before), "a refused update wrote to the blob"
        assert fields(out) == fields(_lib.ParityHeader()) and _lib.last_error()

    for version in (1, 2):
        m = pc.model(version)
        blob = m.blob(data, pc.CHUNK, 3)
        for with_header in (True, False):
            refused(blob, (2 * pc.CHUNK, pc.TOTAL - 2 * pc.CHUNK, 0), _lib.ERR_ARGUMENT, with_header=with_header)      # fewer chunks than groups
            refused(blob, (100, 10, 11), _lib.ERR_ARGUMENT, with_header=with_header)                                 # neither shape
            refused(blob, (pc.TOTAL - 5, 10, 10), _lib.ERR_ARGUMENT, with_header=with_header)
            refused(blob, (0, 16, 16), _lib.ERR_FORMAT, size=blob.size - 1, with_header=with_header)                 # a blob short of its rows
        refused(blob, (2 * pc.CHUNK, pc.TOTAL - 2 * pc.CHUNK, 0), _lib.ERR_ARGUMENT)
        assert "new blob" in _lib.last_error()
        refused(m.blob(data[:1000], pc.CHUNK, 1), (1000, 0, 1000), _lib.ERR_ARGUMENT)                                # a one-chunk blob with a short row growing
        refused(m.blob(data[:1000], pc.CHUNK, 1), (1000, 0, 1000), _lib.ERR_ARGUMENT, with_header=False)
        refused(m.blob(data[:0], pc.CHUNK, 4), (0, 0, 100), _lib.ERR_ARGUMENT)                                       # an empty blob growing
        for at, value in ((0, 0x43), (4, 3), (4, 0)):                                                                # magic, version
            bad = blob.copy()
            bad[at] = value
            refused(bad, (0, 16, 16), _lib.ERR_FORMAT)
            refused(bad, (0, 16, 16), _lib.ERR_FORMAT, with_header=False)
    # the 256th member of a group: version 2 refuses, version 1 takes it
    total, chunk, groups = pc.LONG
    refused(parity2_cpu.blob(pc.input_of(total), chunk, groups), (total, 0, 1), _lib.ERR_ARGUMENT)
    check_edit(1, total, chunk, groups, (total, 0, 1))
    # NULL pointers
    blob = parity_cpu.blob(data, pc.CHUNK, 3)
    h = container.parse_parity_header(blob)
    d_blob, bptr = guarded(blob)
    torch.cuda.synchronize()
    assert call(0, blob.size, ctypes.byref(h), 0, sptr, 16, sptr, 16, None, None) == _lib.ERR_ARGUMENT
    assert call(bptr, blob.size, ctypes.byref(h), 0, 0, 16, sptr, 16, None, None) == _lib.ERR_ARGUMENT
    assert call(bptr, blob.size, ctypes.byref(h), 0, sptr, 16, 0, 16, None, None) == _lib.ERR_ARGUMENT
    torch.cuda.synchronize()
    assert np.array_equal(content(d_blob, blob.size), blob)
    with pytest.raises(EncodeError) as e:
        container.parity_update_device(bptr, blob.size, 100, sptr, 10, sptr, 11, parity_header=h)
    assert f"error {_lib.ERR_ARGUMENT}" in str(e.value)


@pytest.mark.parametrize("version", [1, 2])
def test_asynchronous_form_and_marks(version):
    """With a host header nothing is read back: the device's copy of the header is 0xA5 but for what the kernel writes — n_chunks and total_len —, the header
    returned is host arithmetic, and the call runs on the caller's stream.  One mark.  A zero-length edit does nothing."""
    import torch
    total, chunk, groups = pc.TOTAL, pc.CHUNK, 2
    edit = (total - 1000, 1000, 70_000)
    data, new = pc.input_of(total), pc.new_bytes(edit[2])
    before, want, after = pc.blobs(version, data, chunk, groups, edit, new)
    h = container.parse_parity_header(before)
    masked = before.copy()
    masked[:32] = POISON
    stream = torch.cuda.Stream()
    container.last_timings()
    container.set_profiling(True)
    try:
        with torch.cuda.stream(stream):
            d_blob, bptr = guarded(masked)
            d_old, optr = guarded(np.array(data[edit[0]:]))
            d_new, nptr = guarded(new)
            hdr = container.parity_update_device(bptr, before.size, edit[0], optr, edit[1], nptr, edit[2], parity_header=h, stream=stream.cuda_stream)
        assert fields(hdr) == fields(container.parse_parity_header(want))                  # (before anything is synchronised)
        torch.cuda.synchronize()
        names = [name for name, _ in container.last_timings()]
    finally:
        container.set_profiling(False)
    assert names == ["parity_update"], names
    got = content(d_blob, before.size)
    expect = want.copy()
    expect[:12], expect[24:32] = POISON, POISON
    assert np.array_equal(got, expect), np.flatnonzero(got != expect)[:8]
    assert np.array_equal(content(d_old, edit[1]), data[edit[0]:]) and np.array_equal(content(d_new, edit[2]), new)
    # a zero-length edit: OK, nothing launched (no mark), the blob untouched, the header as it was — with the header given and with it read back
    container.set_profiling(True)
    try:
        for with_header in (True, False):
            got, hdr = update(before, 12345, np.zeros(0, dtype=np.uint8), np.zeros(0, dtype=np.uint8), with_header=with_header)
            assert np.array_equal(got, before) and fields(hdr) == fields(h)
        names = [name for name, _ in container.last_timings()]
    finally:
        container.set_profiling(False)
    assert names == [], names


@pytest.mark.parametrize("version", [1, 2])
def test_host_pointers(version):
    total, chunk, groups = pc.TOTAL, pc.CHUNK, 2
    data = pc.input_of(total)
    for edit in ((chunk - 5, chunk + 11, chunk + 11), (total, 0, 2 * chunk + 9)):
        new = pc.new_bytes(edit[2])
        before, want, after = pc.blobs(version, data, chunk, groups, edit, new)
        room = np.full(before.size + 100, POISON, dtype=np.uint8)
        room[:before.size] = before
        old = np.array(data[edit[0]:edit[0] + edit[1]])
        keep_old, keep_new = old.copy(), new.copy()
        assert container.parity_update(room[:before.size], edit[0], old, new) == before.size
        assert np.array_equal(room[:before.size], want) and (room[before.size:] == POISON).all()
        assert np.array_equal(old, keep_old) and np.array_equal(new, keep_new)
    with pytest.raises(EncodeError):
        container.parity_update(room[:before.size], 100, old[:10], new[:11])
    assert "neither" in _lib.last_error()


# ------------------------------------------------------------------------------------------------------------------------------------------
# end to end: a chunk replaced by a join, the records kept by the update

def test_replaced_chunk_is_recovered_with_the_updated_blob_only():
    """Cheetah, packed, sealed, a version-2 blob with two groups.  Chunk 2 is replaced through join(A[0, 2), B, A[3, n)), B the one-chunk sealed container of the
    new bytes (those of chunk 4, so that a silent flip in them is known); the blob is updated from the old and new chunk bytes.  One silent flip each in chunks
    0 and 2 of the joined container — members of one group: the recover decode with the UPDATED blob returns the new input, both RECOVERED.  The STALE blob is
    the blob of the input with the OLD chunk 2: its solve for the pair gives chunk 0 as it is and chunk 2 as it WAS, which the trailer refuses — the replaced
    chunk stays DAMAGED although the caller paid for recovery records, and no wrong byte passes."""
    algo, form, kind, k, donor = "cheetah", "packed", "mixed", 2, 4
    data, chunk, cont, h1, _, _ = sealed(algo, form, kind)
    n = h1.n_chunks
    new = np.array(data[donor * chunk:(donor + 1) * chunk])
    old = np.array(data[k * chunk:(k + 1) * chunk])
    assert new.size == old.size == chunk and not np.array_equal(new, old)
    room = np.zeros(container.container_bound(algo, chunk, chunk) + container.seal_overhead(chunk, chunk), dtype=np.uint8)
    patch = room[:container.encode_sealed(algo, new, room, chunk)].copy()
    whole = np.array(cont)
    joined = np.zeros(container.container_bound(algo, data.size, chunk) + container.seal_overhead(data.size, chunk), dtype=np.uint8)
    joined = joined[:container.join([(whole, 0, k), (patch, 0, 1), (whole, k + 1, n - k - 1)], joined)].copy()
    hj = container.parse_header(joined)
    after = pc.edited(data, (k * chunk, chunk, chunk), new)
    assert (hj.n_chunks, hj.total_len) == (n, data.size) and hj.flags & container.FLAG_CHECKSUM

    stale = parity2_cpu.blob(data, chunk, 2)
    updated, hdr = update(stale, k * chunk, old, new)
    assert np.array_equal(updated, parity2_cpu.blob(after, chunk, 2))

    flips = []
    for i, source in ((0, 0), (k, donor)):                  # (chunk i's stream is the stream of input chunk `source`: chunks are encoded on their own)
        pos, found = vc.silent_position(algo, kind, data.size, chunk, source)
        assert found >= 1
        flips.append(vc.stream_byte_at(joined, i, pos))
    bad = flipped(joined, *flips)
    for blank in (False, True):
        rc, damaged, recovered, got, verdicts = recover_decode(bad, updated, after.size, blank, header=hj)
        assert (rc, damaged, recovered) == (_lib.OK, 0, 2), (rc, damaged, recovered)
        assert np.array_equal(got, after) and [int(v) for v in verdicts] == [RECOVERED if i in (0, k) else OK for i in range(n)]
        assert check_contract(after, chunk, got, verdicts, blank) == (set(), {0, k})
        rc, damaged, recovered, got, verdicts = recover_decode(bad, stale, after.size, blank, header=hj)
        assert (rc, damaged, recovered) == (_lib.ERR_CHECKSUM, 1, 1), (rc, damaged, recovered)
        assert check_contract(after, chunk, got, verdicts, blank) == ({k}, {0})
        assert [int(v) for v in verdicts] == [RECOVERED if i == 0 else DAMAGED if i == k else OK for i in range(n)]
        if not blank:
            assert np.array_equal(got[k * chunk:(k + 1) * chunk], old), "the stale blob's chunk 2 is the old chunk 2"
