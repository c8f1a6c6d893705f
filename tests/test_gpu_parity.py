"""Recovery records (include/density_hip.h: the parity blob "DHP1", density_hip_parity_device / density_hip_decode_device_recover and their host-pointer forms).

The blob is held byte for byte against the numpy model (parity_cpu.py).  The recover decode is held against ground truth — the input the container was made
from — and against the contract

    after a recover decode, chunk i's verdict is not DAMAGED  iff  the bytes now standing in chunk i's region of the output are input chunk i

with RECOVERED exactly at the chunks that were damaged and are the only damaged ones of their parity groups.  The containers, and every kind of damage, are those
of test_gpu_verdicts.py: a silent PLAIN flip, a lying size table, a trailer entry.  The blobs handed to the decoder are the MODEL's unless a test says otherwise,
so the two kernels are not checked against each other.  Outputs are pre-filled with 0xA5 and verdicts with a pattern so that stale values cannot pass.

A library call with a NULL stream runs on the library's own stream, not torch's: buffers filled with torch are synchronised first."""
import ctypes
import functools

import numpy as np
import pytest

import parity_cpu
import verdict_cases as vc
from density_amd import ChecksumError, DecodeError, _lib, container
from test_gpu_checksum import to_device
from test_gpu_verdicts import flipped, sealed, silent_damage_at, verdict_decode

pytestmark = pytest.mark.gpu

CASES = [(algo, form, kind) for (algo, form) in vc.SHAPES for kind in vc.KINDS]
ALGOS = ["chameleon", "cheetah", "lion"]
POISON, VERDICT_POISON = 0xA5, 0x5A5A5A5A
GROUPS = 2
ROW_TILE = 16384      # parity.hip: kParTile, what a work-group takes of a row per trip
OK, DAMAGED, RECOVERED = 0, _lib.CHUNK_DAMAGED, _lib.CHUNK_RECOVERED


@functools.lru_cache(maxsize=None)
def model_blob(algo, form, kind, groups=GROUPS):
    data, chunk = vc.input_of(algo, form, kind)
    blob = parity_cpu.blob(data, chunk, groups)
    blob.setflags(write=False)
    return blob


def device_blob(data, chunk, groups, in_offset=0, out_offset=0):
    """density_hip_parity_device of `data` at in_offset of its buffer into 0xA5 at out_offset of another: the blob, with the bytes around it checked"""
    import torch
    size = container.parity_size(data.size, chunk, groups)
    assert size == parity_cpu.size(data.size, chunk, groups)
    src, sptr = to_device(np.array(data), offset=in_offset, tail=32)
    out = torch.full((out_offset + size + 64,), POISON, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    container.parity_device(sptr, data.size, chunk, groups, out.data_ptr() + out_offset, size)
    torch.cuda.synchronize()
    got = out.cpu().numpy()
    assert (got[:out_offset] == POISON).all() and (got[out_offset + size:] == POISON).all(), "bytes around the blob written"
    return got[out_offset:out_offset + size]


def recover_decode(blob, parity, n, blank, header=None, parity_header=None, offset=0, parity_offset=0, workspace=None, sync=True, parity_size=None):
    """One recover decode of `blob` with `parity` into 0xA5 at `offset` of its buffer: (return code, still damaged, recovered, the n output bytes, the verdict
    words) — with sync=False the first three are None and everything is read after a device synchronise.  The bytes around the output and the words around
    the verdicts must stay as they were."""
    import torch
    nc = container.parse_header(blob).n_chunks
    dev = torch.from_numpy(np.array(blob)).cuda()
    par, pptr = to_device(np.array(parity), offset=parity_offset)
    out = torch.full((offset + n + 64,), POISON, dtype=torch.uint8, device="cuda")
    verdicts = torch.full((nc + 2,), VERDICT_POISON, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    res = container.decode_device_recover(dev.data_ptr(), blob.size, pptr, parity.size if parity_size is None else parity_size, out.data_ptr() + offset, n,
                                          verdicts.data_ptr() + 4, header=header, parity_header=parity_header, workspace=workspace or (0, 0), blank=blank, sync=sync)
    torch.cuda.synchronize()
    got, v = out.cpu().numpy(), verdicts.cpu().numpy()
    assert (got[:offset] == POISON).all() and (got[offset + n:] == POISON).all(), "bytes around the output written"
    assert v[0] == VERDICT_POISON and v[-1] == VERDICT_POISON, "words around the verdicts written"
    rc, damaged, recovered = res if sync else (None, None, None)
    return rc, damaged, recovered, got[offset:offset + n], v[1:-1]


def check_contract(data, chunk, got, verdicts, blank):
    """verdict != DAMAGED iff the region is the input chunk; blanked, a damaged region is all zeros.  Returns (still damaged, recovered) as sets."""
    damaged, recovered = set(), set()
    for i in range(-(-data.size // chunk)):
        region, want = got[i * chunk:(i + 1) * chunk], data[i * chunk:(i + 1) * chunk]
        same = np.array_equal(region, want)
        assert verdicts[i] in (OK, DAMAGED, RECOVERED), (i, int(verdicts[i]))
        if verdicts[i] != DAMAGED:
            assert same, f"chunk {i}: verdict {int(verdicts[i])}, bytes wrong"
        elif blank:
            assert not region.any(), f"chunk {i}: damaged and not blanked"
        else:
            assert not same, f"chunk {i}: verdict DAMAGED, bytes right"
        if verdicts[i] == DAMAGED:
            damaged.add(i)
        if verdicts[i] == RECOVERED:
            recovered.add(i)
    return damaged, recovered


# ------------------------------------------------------------------------------------------------------------------------------------------
# the blob

@pytest.mark.parametrize("groups", [1, 2, 4, 6, 7])
def test_blob_is_the_model(groups):
    data, chunk = vc.input_of("cheetah", "packed", "mixed")
    assert (data.size, chunk) == (5 * 65536 + 777, 65536)
    want = parity_cpu.blob(data, chunk, groups)
    h = container.parse_parity_header(want)
    assert h.n_groups == min(groups, 6) and h.row_bytes == 65536
    for in_offset in (0, 1, 3):
        for out_offset in (0, 5):
            got = device_blob(data, chunk, groups, in_offset, out_offset)
            assert np.array_equal(got, want), (groups, in_offset, out_offset, np.flatnonzero(got != want)[:8])


@pytest.mark.parametrize("total,chunk,groups", [
    (1000, 65536, 3),                                   # one chunk, shorter than its size: a row of 1008 bytes
    (0, 65536, 4),                                      # zero bytes: a bare header
    (3 * (ROW_TILE - 256) + 1001, ROW_TILE - 256, 2),   # chunk sizes at the row tile and 256 either side of it, the last chunk ending inside a 16-byte slot
    (3 * ROW_TILE + 1001, ROW_TILE, 2),
    (3 * (ROW_TILE + 256) + 1001, ROW_TILE + 256, 2),
    (2 * (ROW_TILE + 256) + 16, ROW_TILE + 256, 3),
])
def test_blob_edge_shapes(total, chunk, groups):
    data = vc._input("mixed", 5 * 65536 + 777)[:total]
    want = parity_cpu.blob(data, chunk, groups)
    assert want.size == 32 + min(groups, -(-total // chunk)) * ((min(total, chunk) + 15) // 16 * 16)
    for in_offset, out_offset in ((0, 0), (7, 9)):
        got = device_blob(data, chunk, groups, in_offset, out_offset)
        assert np.array_equal(got, want), (np.flatnonzero(got != want)[:8])


def test_blob_refusals():
    import torch
    data, chunk = vc.input_of("cheetah", "packed", "mixed")
    src, sptr = to_device(np.array(data))
    size = container.parity_size(data.size, chunk, GROUPS)
    out = torch.full((size,), POISON, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    call = _lib.lib().density_hip_parity_device
    assert call(sptr, data.size, chunk, GROUPS, out.data_ptr(), size - 1, 0) == _lib.ERR_CAPACITY
    assert call(sptr, data.size, 0, GROUPS, out.data_ptr(), size, 0) == _lib.ERR_ARGUMENT
    assert call(sptr, data.size, chunk, 0, out.data_ptr(), size, 0) == _lib.ERR_ARGUMENT
    assert call(sptr, data.size, chunk, GROUPS, 0, size, 0) == _lib.ERR_ARGUMENT
    torch.cuda.synchronize()
    assert (out.cpu().numpy() == POISON).all()
    with pytest.raises(Exception) as e:
        container.parity_device(sptr, data.size, chunk, GROUPS, out.data_ptr(), size - 1)
    assert f"error {_lib.ERR_CAPACITY}" in str(e.value)


# ------------------------------------------------------------------------------------------------------------------------------------------
# recovery

@pytest.mark.parametrize("algo,form,kind", CASES)
def test_one_silent_flip_is_recovered(algo, form, kind):
    data, chunk, blob, h1, _, _ = sealed(algo, form, kind)
    parity = model_blob(algo, form, kind)
    assert data.size % chunk != 0
    for k in vc.victims(algo, form):
        bad = flipped(blob, silent_damage_at(algo, form, kind, k))
        rc, damaged, recovered, got, verdicts = recover_decode(bad, parity, data.size, True, header=h1)
        assert np.array_equal(got, data), (k, np.flatnonzero(got != data)[:8])
        assert [int(v) for v in verdicts] == [RECOVERED if i == k else OK for i in range(h1.n_chunks)], (k, verdicts)
        assert (rc, damaged, recovered) == (_lib.OK, 0, 1), (k, rc, damaged, recovered)
        assert _lib.last_error() == ""


@pytest.mark.parametrize("algo,form", list(vc.SHAPES))
def test_intact_container_and_marks(algo, form):
    kind = "rep_text"
    data, chunk, blob, h1, _, _ = sealed(algo, form, kind)
    for blank in (False, True):
        container.last_timings()
        container.set_profiling(True)
        try:
            rc, damaged, recovered, got, verdicts = recover_decode(blob, model_blob(algo, form, kind), data.size, blank, header=h1)
            names = [name for name, _ in container.last_timings()]
        finally:
            container.set_profiling(False)
        assert (rc, damaged, recovered) == (_lib.OK, 0, 0) and not verdicts.any() and np.array_equal(got, data)
        assert names == ["layout_decode", f"{algo}_decode_chunks", "checksum_verify", "chunk_verdicts", "recover_rebuild", "recover_verify"] + (["blank_chunks"] if blank else []), names


@pytest.mark.parametrize("algo", ALGOS)
def test_more_than_one_damaged_chunk(algo):
    form, kind = "packed", "mixed"
    data, chunk, blob, h1, _, _ = sealed(algo, form, kind)
    parity = model_blob(algo, form, kind)
    k = 2
    assert h1.n_chunks == 6 and container.parse_parity_header(parity).n_groups == 2
    # neighbours lie in different groups: both come back
    bad = flipped(blob, silent_damage_at(algo, form, kind, k), silent_damage_at(algo, form, kind, k + 1))
    for blank in (False, True):
        rc, damaged, recovered, got, verdicts = recover_decode(bad, parity, data.size, blank)                    # (both headers read from the device)
        assert (rc, damaged, recovered) == (_lib.OK, 0, 2) and np.array_equal(got, data)
        assert check_contract(data, chunk, got, verdicts, blank) == (set(), {k, k + 1})
    # k and k + 2 share a group: the row cannot give either back, and neither is touched
    bad = flipped(blob, silent_damage_at(algo, form, kind, k), silent_damage_at(algo, form, kind, k + 2))
    plain = verdict_decode(bad, data.size, False)[2]
    for blank in (False, True):
        rc, damaged, recovered, got, verdicts = recover_decode(bad, parity, data.size, blank)
        assert (rc, damaged, recovered) == (_lib.ERR_CHECKSUM, 2, 0), (rc, damaged, recovered)
        assert check_contract(data, chunk, got, verdicts, blank) == ({k, k + 2}, set())
        assert "2 of 6 chunks damaged, 0 recovered" in _lib.last_error(), _lib.last_error()
        if not blank:
            assert np.array_equal(got, plain), "an unrecoverable group's chunks are left as the decoder made them"
    # one group lost, the other recovered: k, k + 2 and k + 1
    bad = flipped(bad, silent_damage_at(algo, form, kind, k + 1))
    rc, damaged, recovered, got, verdicts = recover_decode(bad, parity, data.size, True)
    assert (rc, damaged, recovered) == (_lib.ERR_CHECKSUM, 2, 1)
    assert check_contract(data, chunk, got, verdicts, True) == ({k, k + 2}, {k + 1})
    # a group per chunk: every chunk may go at once
    every = flipped(blob, *[silent_damage_at(algo, form, kind, i) for i in vc.victims(algo, form)])
    rc, damaged, recovered, got, verdicts = recover_decode(every, model_blob(algo, form, kind, 6), data.size, True)
    assert (rc, damaged, recovered) == (_lib.OK, 0, 3) and np.array_equal(got, data)


@pytest.mark.parametrize("algo,form", list(vc.SHAPES))
def test_a_lying_size_table_is_recovered(algo, form):
    """chunk k's size-table entry lowered by 2 (test_gpu_verdicts.py: test_loud_damage_keeps_the_other_chunks): whatever the decoder makes of it — a format
    error, wrong bytes, or the right ones — every chunk's content is verified in the end, and that is what the return code says."""
    kind = "rep_text"
    data, chunk, blob, h1, _, _ = sealed(algo, form, kind)
    for k in vc.victims(algo, form):
        table = blob.copy()
        size = int.from_bytes(bytes(blob[32 + 4 * k:36 + 4 * k]), "little")
        table[32 + 4 * k:36 + 4 * k] = np.frombuffer((size - 2).to_bytes(4, "little"), dtype=np.uint8)
        rc0, count0, _, verdicts0 = verdict_decode(table, data.size, False, header=h1)
        hit = {i for i, v in enumerate(verdicts0) if v}
        assert rc0 != _lib.OK and hit <= {k}
        rc, damaged, recovered, got, verdicts = recover_decode(table, model_blob(algo, form, kind), data.size, True, header=h1)
        assert (rc, damaged, recovered) == (_lib.OK, 0, len(hit)), (k, rc0, rc, damaged, recovered)
        assert np.array_equal(got, data) and check_contract(data, chunk, got, verdicts, True) == (set(), hit)


@pytest.mark.parametrize("algo,form", [("chameleon", "paged"), ("chameleon", "packed"), ("cheetah", "slotted"), ("lion", "packed")])
def test_damaged_parity_never_passes_wrong_bytes(algo, form):
    kind = "mixed"
    data, chunk, blob, h1, _, _ = sealed(algo, form, kind)
    parity = model_blob(algo, form, kind)
    for k in vc.victims(algo, form):
        length = min(chunk, data.size - k * chunk)
        bad_parity = flipped(parity, parity_cpu.row_offset(parity, k % GROUPS, length // 2), bit=0x01)
        bad = flipped(blob, silent_damage_at(algo, form, kind, k))
        for blank in (False, True):
            rc, damaged, recovered, got, verdicts = recover_decode(bad, bad_parity, data.size, blank, header=h1)
            assert (rc, damaged, recovered) == (_lib.ERR_CHECKSUM, 1, 0), (k, rc, damaged, recovered)
            assert check_contract(data, chunk, got, verdicts, blank) == ({k}, set())
        # the same row under an intact container: nobody reads it
        rc, damaged, recovered, got, verdicts = recover_decode(blob, bad_parity, data.size, True, header=h1)
        assert (rc, damaged, recovered) == (_lib.OK, 0, 0) and not verdicts.any() and np.array_equal(got, data)


@pytest.mark.parametrize("algo,form", list(vc.SHAPES))
def test_damaged_trailer_entry_stays_damaged(algo, form):
    """Entry k no longer holds chunk k's checksum: the chunk is rebuilt — to the bytes it had — and still does not match, so it stays DAMAGED; without
    blanking its bytes are the input's."""
    kind = "rep_text"
    data, chunk, blob, h1, _, _ = sealed(algo, form, kind)
    parity = model_blob(algo, form, kind)
    for k in vc.victims(algo, form):
        bad = flipped(blob, vc.trailer_at(blob) + 4 * k + 1, bit=0x04)
        rc, damaged, recovered, got, verdicts = recover_decode(bad, parity, data.size, False, header=h1)
        assert (rc, damaged, recovered) == (_lib.ERR_CHECKSUM, 1, 0) and [int(v) for v in verdicts] == [DAMAGED if i == k else OK for i in range(h1.n_chunks)]
        assert np.array_equal(got, data)
        rc, damaged, recovered, got, verdicts = recover_decode(bad, parity, data.size, True, header=h1)
        assert (rc, damaged, recovered) == (_lib.ERR_CHECKSUM, 1, 0) and [int(v) for v in verdicts] == [DAMAGED if i == k else OK for i in range(h1.n_chunks)]
        want = data.copy()
        want[k * chunk:(k + 1) * chunk] = 0
        assert np.array_equal(got, want)


# ------------------------------------------------------------------------------------------------------------------------------------------
# refusals

def test_refusals_write_nothing():
    import torch
    algo, form, kind = "cheetah", "packed", "mixed"
    data, chunk, blob, h1, plain, h0 = sealed(algo, form, kind)
    parity = np.array(model_blob(algo, form, kind))
    ph = container.parse_parity_header(parity)
    k = 3
    bad = flipped(blob, silent_damage_at(algo, form, kind, k))
    sdev, pdev, udev = torch.from_numpy(bad).cuda(), torch.from_numpy(parity).cuda(), torch.from_numpy(plain).cuda()
    out = torch.full((data.size,), POISON, dtype=torch.uint8, device="cuda")
    verdicts = torch.full((h1.n_chunks,), VERDICT_POISON, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    call = _lib.lib().density_hip_decode_device_recover

    def refused(container_dev, container_size, parity_size, parity_header, flags=1, verdict_shift=0):
        damaged, recovered = ctypes.c_uint32(77), ctypes.c_uint32(78)
        rc = call(container_dev.data_ptr(), container_size, None, pdev.data_ptr(), parity_size, ctypes.byref(parity_header) if parity_header is not None else None,
                  out.data_ptr(), data.size, 0, 0, 0, verdicts.data_ptr() + verdict_shift, flags, ctypes.byref(damaged), ctypes.byref(recovered))
        torch.cuda.synchronize()
        assert (damaged.value, recovered.value) == (77, 78)
        assert (out.cpu().numpy() == POISON).all() and (verdicts.cpu().numpy() == VERDICT_POISON).all(), "a refused call wrote"
        return rc

    def header_with(**fields):
        h = _lib.ParityHeader.from_buffer_copy(bytes(ph))
        for name, value in fields.items():
            setattr(h, name, value)
        return h

    # argument errors: an unsealed container, unknown flag bits, a verdict buffer that is not word-aligned, a blob that is another container's
    assert refused(udev, plain.size, parity.size, None) == _lib.ERR_ARGUMENT
    assert refused(sdev, bad.size, parity.size, None, flags=2) == _lib.ERR_ARGUMENT
    assert refused(sdev, bad.size, parity.size, None, flags=3) == _lib.ERR_ARGUMENT
    assert refused(sdev, bad.size, parity.size, None, verdict_shift=2) == _lib.ERR_ARGUMENT
    assert refused(sdev, bad.size, parity.size, header_with(chunk_size=2 * chunk)) == _lib.ERR_ARGUMENT
    assert refused(sdev, bad.size, parity.size, header_with(n_chunks=h1.n_chunks - 1)) == _lib.ERR_ARGUMENT
    assert refused(sdev, bad.size, parity.size, header_with(total_len=data.size - 1)) == _lib.ERR_ARGUMENT
    # format errors: magic, version, n_groups outside 1 .. n_chunks, a row length that is not the formula's, a blob cut short
    assert refused(sdev, bad.size, parity.size, header_with(magic=container.parse_header(blob).magic)) == _lib.ERR_FORMAT
    assert refused(sdev, bad.size, parity.size, header_with(version=2)) == _lib.ERR_FORMAT
    assert refused(sdev, bad.size, parity.size, header_with(n_groups=0)) == _lib.ERR_FORMAT
    assert refused(sdev, bad.size, parity.size, header_with(n_groups=h1.n_chunks + 1)) == _lib.ERR_FORMAT
    assert refused(sdev, bad.size, parity.size, header_with(row_bytes=ph.row_bytes - 16)) == _lib.ERR_FORMAT
    assert refused(sdev, bad.size, parity.size, header_with(row_bytes=ph.row_bytes + 16)) == _lib.ERR_FORMAT
    assert refused(sdev, bad.size, parity.size - 1, None) == _lib.ERR_FORMAT
    assert refused(sdev, bad.size, 31, None) == _lib.ERR_FORMAT
    assert refused(sdev, bad.size, parity.size, header_with(n_groups=3)) == _lib.ERR_FORMAT          # (three rows of this length do not fit the two there are)
    assert refused(sdev, bad.size - 16, parity.size, None) == _lib.ERR_FORMAT                       # (the container cut short, as for the verdict call)
    # ... and the same headers where the call finds them itself, on the device
    for fields, want in ((dict(total_len=data.size - 1), _lib.ERR_ARGUMENT), (dict(version=2), _lib.ERR_FORMAT)):
        pdev[:32] = torch.from_numpy(np.frombuffer(bytes(header_with(**fields)), dtype=np.uint8).copy()).cuda()
        torch.cuda.synchronize()
        assert refused(sdev, bad.size, parity.size, None) == want
    # the Python layer raises, as for the verdict call
    with pytest.raises(DecodeError) as e:
        recover_decode(plain, parity, data.size, True, header=h0)
    assert e.type is DecodeError and f"error {_lib.ERR_ARGUMENT}" in str(e.value), str(e.value)
    with pytest.raises(DecodeError) as e:
        recover_decode(bad, parity, data.size, True, parity_header=header_with(version=2))
    assert f"error {_lib.ERR_FORMAT}" in str(e.value), str(e.value)


def test_zero_chunks():
    import torch
    h = _lib.Header(0x31434844, 0, 1, container.FLAG_CHECKSUM, 65536, 0, 0, 32)
    dev = torch.from_numpy(np.frombuffer(bytes(h), dtype=np.uint8).copy()).cuda()
    par = torch.from_numpy(device_blob(np.zeros(0, dtype=np.uint8), 65536, 4).copy()).cuda()
    torch.cuda.synchronize()
    damaged, recovered = ctypes.c_uint32(77), ctypes.c_uint32(78)
    rc = _lib.lib().density_hip_decode_device_recover(dev.data_ptr(), 32, None, par.data_ptr(), 32, None, 0, 0, 0, 0, 0, 0, 1, ctypes.byref(damaged), ctypes.byref(recovered))
    assert (rc, damaged.value, recovered.value) == (_lib.OK, 0, 0)


# ------------------------------------------------------------------------------------------------------------------------------------------
# other paths

@pytest.mark.parametrize("algo,form", [("chameleon", "paged"), ("cheetah", "packed"), ("lion", "slotted")])
def test_asynchronous_form(algo, form):
    """Both out pointers NULL: nothing is reported; verdicts, the rebuilt output and — in the caller's workspace of exactly density_hip_decode_workspace_size_for()
    bytes, second and third word — the counts lie on the device.  The blob is the device's own, made on the same stream in front of the decode."""
    import torch
    kind = "mixed"
    data, chunk, blob, h1, _, _ = sealed(algo, form, kind)
    k = vc.victims(algo, form)[1]
    bad = flipped(blob, silent_damage_at(algo, form, kind, k))
    need = int(_lib.lib().density_hip_decode_workspace_size_for(_lib.ALGO_IDS[algo], data.size, chunk))
    ws = torch.zeros(need + 64, dtype=torch.uint8, device="cuda")
    ws[need:] = POISON
    parity = device_blob(data, chunk, GROUPS)
    assert np.array_equal(parity, model_blob(algo, form, kind))
    rc, damaged, recovered, got, verdicts = recover_decode(bad, parity, data.size, True, header=h1, parity_header=container.parse_parity_header(parity),
                                                           workspace=(ws.data_ptr(), need), sync=False, parity_offset=3)
    assert np.array_equal(got, data) and check_contract(data, chunk, got, verdicts, True) == (set(), {k})
    words = ws[:12].cpu().numpy().view(np.uint32)
    assert words[1] == 0 and words[2] == 1, words
    assert (ws[need:].cpu().numpy() == POISON).all(), "bytes behind the workspace written"


@pytest.mark.parametrize("algo,form", [("chameleon", "packed"), ("chameleon", "slotted"), ("cheetah", "slotted"), ("lion", "packed")])
def test_placement(algo, form):
    """the output and the blob at odd offsets (the rebuild kernel's ragged heads and tails), the caller's workspace at its smallest size; the first and the last
    chunk damaged — groups 0 and 1"""
    import torch
    kind = "rep_text"
    data, chunk, blob, h1, _, _ = sealed(algo, form, kind)
    nc = h1.n_chunks
    for need in (int(_lib.lib().density_hip_decode_workspace_size(nc)), int(_lib.lib().density_hip_decode_workspace_size_for(_lib.ALGO_IDS[algo], data.size, chunk))):
        ws = torch.zeros(need, dtype=torch.uint8, device="cuda")
        bad = flipped(blob, silent_damage_at(algo, form, kind, 0), silent_damage_at(algo, form, kind, nc - 1))
        for offset, parity_offset in ((1, 0), (7, 5), (13, 16), (16, 1)):
            rc, damaged, recovered, got, verdicts = recover_decode(bad, model_blob(algo, form, kind), data.size, False, header=h1, offset=offset,
                                                                   parity_offset=parity_offset, workspace=(ws.data_ptr(), need))
            assert (rc, damaged, recovered) == (_lib.OK, 0, 2) and np.array_equal(got, data), (offset, parity_offset, np.flatnonzero(got != data)[:8])
            assert check_contract(data, chunk, got, verdicts, False) == (set(), {0, nc - 1})


@pytest.mark.parametrize("algo", ALGOS)
def test_host_pointers(algo):
    kind = "mixed"
    data, chunk, blob, h1, plain, _ = sealed(algo, "packed", kind)
    want = model_blob(algo, "packed", kind)
    # the blob
    room = np.full(want.size + 100, POISON, dtype=np.uint8)
    assert container.parity(np.array(data), chunk, GROUPS, room) == want.size
    assert np.array_equal(room[:want.size], want) and (room[want.size:] == POISON).all()
    from density_amd import EncodeError
    with pytest.raises(EncodeError):
        container.parity(np.array(data), chunk, GROUPS, room[:want.size - 1])
    with pytest.raises(EncodeError):
        container.parity(np.array(data), 0, GROUPS, room)
    # the decode
    k = vc.victims(algo, "packed")[1]
    bad = flipped(blob, silent_damage_at(algo, "packed", kind, k))
    for blank in (False, True):
        back = np.full(data.size + 100, POISON, dtype=np.uint8)
        n, damaged, recovered = container.decode_recover(bad, want, back, blank=blank)
        assert (n, damaged, recovered) == (data.size, [], [k]) and np.array_equal(back[:data.size], data) and (back[data.size:] == POISON).all()
        assert _lib.last_error() == ""
    back = np.full(data.size, POISON, dtype=np.uint8)
    assert container.decode_recover(blob, want, back) == (data.size, [], []) and np.array_equal(back, data)
    # two of one group: reported, blanked, the rest kept
    two = flipped(bad, silent_damage_at(algo, "packed", kind, k + 2))
    n, damaged, recovered = container.decode_recover(two, want, back)
    assert (n, damaged, recovered) == (data.size, [k, k + 2], []) and "2 of 6 chunks damaged" in _lib.last_error()
    expect = data.copy()
    expect[k * chunk:(k + 1) * chunk] = 0
    expect[(k + 2) * chunk:(k + 3) * chunk] = 0
    assert np.array_equal(back, expect)
    # every trailer entry damaged: nothing can be vouched for
    t = vc.trailer_at(blob)
    with pytest.raises(ChecksumError) as e:
        container.decode_recover(flipped(blob, *[t + 4 * i for i in range(h1.n_chunks)]), want, back)
    assert e.value.damaged_chunks == tuple(range(h1.n_chunks))
    # unsealed, a blob of another shape, an output too small: 0, nothing written
    back[:] = POISON
    with pytest.raises(DecodeError):
        container.decode_recover(plain, want, back)
    with pytest.raises(DecodeError):
        container.decode_recover(bad, parity_cpu.blob(data[:-1], chunk, GROUPS), back)
    with pytest.raises(DecodeError):
        container.decode_recover(bad, want[:-1], back)
    with pytest.raises(DecodeError):
        container.decode_recover(bad, want, back[:-1])
    assert (back == POISON).all()
