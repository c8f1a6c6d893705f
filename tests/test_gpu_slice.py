"""density_hip_slice_device / density_hip_slice: chunks [first, first + count) of a container of any form as a packed container of their own, and the
range decode made of it (container.decode_range_device / decode_range).  The expectation is always the bytes of tests/slice_cpu.py (held to the oracle in
tests/test_slice_cpu.py), compared whole: container_len and every byte below it; for containers the library made, density_hip_encode_device
(+ density_hip_seal_device) of the part of the input besides.  Outputs are pre-filled so that stale bytes cannot pass.

A library call with a NULL stream runs on the library's own stream, not torch's: buffers filled with torch are synchronised first."""
import ctypes
import functools

import numpy as np
import pytest

import datagen
import paged_cpu
import slice_cpu
import unpage_cases as uc
import verdict_cases as vc
from density_amd import ChecksumError, DecodeError, EncodeError, _lib, container
from oracle import pyoracle

pytestmark = pytest.mark.gpu

FILL, GUARD = 0xA5, 256
KIND = "mixed"


def _stream():
    import torch
    torch.cuda.synchronize()
    return 0


def _buffers(blob, in_off=0, out_off=0, cap=0):
    """The blob on the device at byte offset in_off of its allocation; an output of `cap` bytes at byte offset out_off, pre-filled, GUARD bytes behind it."""
    import torch
    d = torch.zeros(in_off + blob.size, dtype=torch.uint8, device="cuda")
    d[in_off:] = torch.from_numpy(np.array(blob)).cuda()
    out = torch.full((out_off + cap + GUARD,), FILL, dtype=torch.uint8, device="cuda")
    return d, out


def _slice(blob, first, count, in_off=0, out_off=0, header=True):
    """(header, the output allocation from out_off on as numpy, capacity) of one synchronous call"""
    h = container.parse_header(bytes(blob[:32]))
    cap = container.slice_bound(h, first, count)
    assert cap > 0
    d, out = _buffers(blob, in_off, out_off, cap)
    hdr = container.slice_device(d.data_ptr() + in_off, blob.size, first, count, out.data_ptr() + out_off, cap, header=h if header else None, stream=_stream())
    return hdr, out.cpu().numpy()[out_off:], cap


def _rc(blob, first, count, cap=None, want_header=True, header=True):
    """(return code, output allocation as numpy) of the raw call"""
    import torch
    h = container.parse_header(bytes(blob[:32]))
    cap = container.slice_bound(h, first, count) if cap is None else cap
    d, out = _buffers(blob, cap=cap)
    hdr = _lib.Header()
    rc = _lib.lib().density_hip_slice_device(d.data_ptr(), blob.size, ctypes.byref(h) if header else None, first, count, out.data_ptr(), cap, 0, 0, _stream(),
                                             ctypes.byref(hdr) if want_header else None)
    torch.cuda.synchronize()
    return rc, out.cpu().numpy()


def _check_output(got, hdr, want, cap):
    assert hdr.container_len == want.size
    assert bytes(hdr) == want[:32].tobytes()
    assert np.array_equal(got[:want.size], want), int(np.flatnonzero(got[:want.size] != want)[0])
    assert (got[want.size:] == FILL).all(), "bytes at and beyond container_len keep the fill, the guards behind the capacity too"
    assert got.size == cap + GUARD and want.size <= cap


def _decodes_to(blob, want):
    """decode_device of a host-resident container returns `want`"""
    import torch
    d = torch.from_numpy(np.array(blob)).cuda()
    back = torch.full((want.size + 64,), FILL, dtype=torch.uint8, device="cuda")
    assert container.decode_device(d.data_ptr(), blob.size, back.data_ptr(), want.size, stream=_stream()) == want.size
    got = back.cpu().numpy()
    assert np.array_equal(got[:want.size], want) and (got[want.size:] == FILL).all()


# ---- CPU-built Chameleon containers ----

CPU_SOURCES = [(name, form, seal) for name in "abdeg" for form in ["paged", "packed"] + (["shuffled"] if name in "ae" else []) for seal in (False, True)]


def _cpu_blob(name, form, seal):
    blob = uc.packed(name) if form == "packed" else uc.paged(name, form == "shuffled")
    return uc.sealed(blob, name) if seal else blob


@pytest.mark.parametrize("name,form,seal", CPU_SOURCES)
def test_cpu_built_containers_slice_to_the_models_bytes(name, form, seal):
    blob = _cpu_blob(name, form, seal)
    _, n, chunk, _ = uc.CASES[name]
    for first, count in slice_cpu.windows(-(-n // chunk)):
        want = slice_cpu.slice_container(blob, first, count)
        hdr, got, cap = _slice(blob, first, count)
        _check_output(got, hdr, want, cap)
        assert hdr.flags == container.FLAG_BLOCK_INDEX | (container.FLAG_CHECKSUM if seal else 0)
        if seal:                                                                    # a container like any other: it decodes, and verifies, to the input's window
            _decodes_to(got[:want.size], uc.data(name)[first * chunk:(first + count) * chunk])


# ---- the library's own containers ----

@functools.lru_cache(maxsize=None)
def _own(algo, form):
    """(input, chunk size, sealed container on the host, unsealed container on the host), made once on the device"""
    from test_gpu_verdicts import sealed
    data, chunk, blob, h1, plain, h0 = sealed(algo, form, KIND)
    plain.setflags(write=False)
    return data, chunk, blob, plain


def _encoded(algo, part, chunk, seal):
    """density_hip_encode_device (+ density_hip_seal_device) of `part`: the container as numpy"""
    import torch
    x = torch.from_numpy(np.array(part)).cuda()
    cap = container.container_bound(algo, part.size, chunk) + container.seal_overhead(part.size, chunk)
    cont = torch.zeros(cap, dtype=torch.uint8, device="cuda")
    hdr = container.encode_device(algo, x.data_ptr(), part.size, cont.data_ptr(), cap, chunk, stream=_stream())
    if seal:
        hdr = container.seal_device(x.data_ptr(), part.size, cont.data_ptr(), cap, header=hdr, stream=_stream())
    return cont[:hdr.container_len].cpu().numpy()


@pytest.mark.parametrize("seal", [False, True])
@pytest.mark.parametrize("algo,form", list(vc.SHAPES))
def test_the_librarys_own_containers_slice_to_what_encode_device_writes(algo, form, seal):
    data, chunk, sealed_blob, plain = _own(algo, form)
    blob = sealed_blob if seal else plain
    for first, count in slice_cpu.windows(vc.n_chunks(algo, form)):
        want = slice_cpu.slice_container(blob, first, count)
        hdr, got, cap = _slice(blob, first, count)
        _check_output(got, hdr, want, cap)
        part = data[first * chunk:(first + count) * chunk]
        if count >= 2:
            made = _encoded(algo, part, chunk, seal)
            assert made.size == want.size and np.array_equal(made, want), (first, count)
        if seal:
            _decodes_to(got[:want.size], part)


@pytest.mark.parametrize("algo,form", [("chameleon", "packed"), ("cheetah", "slotted"), ("chameleon", "paged")])
def test_both_buffers_at_any_byte_alignment(algo, form):
    data, chunk, blob, _ = _own(algo, form)
    for first, count in [(1, 2), (0, vc.n_chunks(algo, form))]:
        hdr, got, cap = _slice(blob, first, count, in_off=1, out_off=3)
        _check_output(got, hdr, slice_cpu.slice_container(blob, first, count), cap)


def test_the_header_may_be_read_back_from_the_device():
    _, _, blob, _ = _own("lion", "slotted")
    hdr, got, cap = _slice(blob, 1, 3, header=False)
    _check_output(got, hdr, slice_cpu.slice_container(blob, 1, 3), cap)


def test_the_host_pointer_form():
    for algo, form in [("chameleon", "paged"), ("lion", "packed")]:
        _, _, blob, _ = _own(algo, form)
        h = container.parse_header(blob)
        want = slice_cpu.slice_container(blob, 1, 2)
        out = np.full(container.slice_bound(h, 1, 2) + 16, FILL, dtype=np.uint8)
        assert container.slice(blob, 1, 2, out[:-16]) == want.size
        assert np.array_equal(out[:want.size], want) and (out[-16:] == FILL).all()
        for first, count in [(0, 0), (h.n_chunks, 1), (1, h.n_chunks)]:
            with pytest.raises(EncodeError):
                container.slice(blob, first, count, out)
        with pytest.raises(EncodeError):
            container.slice(blob, 1, 2, out[:want.size - 1])


# ---- the one place where a slice is not a one-part join: a packed window moves as ONE run, the gaps between its streams as they stand ----

def gap_plants(blob, first, count):
    """[(the blob with one byte of the gap behind chunk k's stream changed to `value`, offset of that byte from chunk `first`'s stream, k is the window's
    last chunk, value)] for the last two chunks of window [first, first + count) of a packed container (tests/test_gpu_join.py plants the same)"""
    n = container.parse_header(bytes(blob[:32])).n_chunks
    sizes = [uc.get32(blob, 32 + 4 * i) for i in range(n)]
    starts = [_payload_at(blob, 0, n) + sum(slice_cpu.up(v, 16) for v in sizes[:i]) for i in range(n)]
    out = []
    for k in (first + count - 2, first + count - 1):
        assert sizes[k] % 16 != 0, "a gap stands behind the stream"
        at = starts[k] + sizes[k] + (16 - sizes[k] % 16) // 2
        assert at < starts[k + 1] and not blob[at]
        for value in (FILL, FILL ^ 0xFF):
            bad = blob.copy()
            bad[at] = value
            out.append((bad, at - starts[first], k == first + count - 1, value))
    return out


def test_a_packed_window_takes_the_gaps_between_its_streams_as_they_stand():
    blob = uc.packed("a")
    intact = slice_cpu.slice_container(blob, 1, 2)
    for bad, rel, behind_the_last, value in gap_plants(blob, 1, 2):
        want = intact.copy()
        if not behind_the_last:
            want[_payload_at(blob, 1, 2) + rel] = value                             # ... and nowhere else
        hdr, got, cap = _slice(bad, 1, 2)
        _check_output(got, hdr, want, cap)                                          # (behind the window's last stream: not the slice's byte, the fill stays)


# ---- the scan's carry: more chunks in front of the window than one tile of the scan holds ----

@functools.lru_cache(maxsize=None)
def _many_chunks():
    """a CPU-built packed Chameleon container of 1100 chunks of 256 bytes and a ragged one of 100"""
    chunk, n = 256, 1100 * 256 + 100
    data = datagen.by_kind("mixed", n, seed=7)
    streams = [pyoracle.encode("chameleon", data[i:i + chunk]) for i in range(0, n, chunk)]
    index = b"".join(bytes(b for b, _ in paged_cpu.walk_records(s, min(chunk, n - i * chunk))) for i, s in enumerate(streams))
    blob = slice_cpu.assemble(0, chunk, n, streams, index)
    blob.setflags(write=False)
    return blob


@pytest.mark.parametrize("first,count", [(1023, 3), (1024, 76), (0, 1100)])
def test_windows_behind_the_scans_first_tile(first, count):
    blob = _many_chunks()
    hdr, got, cap = _slice(blob, first, count)
    _check_output(got, hdr, slice_cpu.slice_container(blob, first, count), cap)


# ---- use: damage outside the window does not matter, damage inside is found when the sealed slice is decoded ----

@pytest.mark.parametrize("algo,form", [("chameleon", "packed"), ("chameleon", "paged"), ("cheetah", "slotted"), ("lion", "packed")])
def test_a_flip_outside_the_window_is_not_in_the_slice_and_one_inside_fails_its_decode(algo, form):
    import torch
    from test_gpu_verdicts import silent_damage_at
    data, chunk, blob, _ = _own(algo, form)
    nc = vc.n_chunks(algo, form)
    k = nc // 2
    bad = blob.copy()
    bad[silent_damage_at(algo, form, KIND, k)] ^= vc.FLIP
    for first, count in [(0, k), (k + 1, nc - k - 1)]:                              # the chunks in front of the damaged one, and those behind it
        hdr, got, cap = _slice(bad, first, count)
        want = slice_cpu.slice_container(blob, first, count)
        _check_output(got, hdr, want, cap)
        _decodes_to(got[:want.size], data[first * chunk:(first + count) * chunk])
    hdr, got, cap = _slice(bad, 1, nc - 1)                                          # the damaged chunk inside: the slice is made ...
    _check_output(got, hdr, slice_cpu.slice_container(bad, 1, nc - 1), cap)
    d = torch.from_numpy(got[:hdr.container_len].copy()).cuda()
    back = torch.zeros(hdr.total_len, dtype=torch.uint8, device="cuda")
    size = ctypes.c_size_t(7)
    rc = _lib.lib().density_hip_decode_device(d.data_ptr(), hdr.container_len, None, back.data_ptr(), hdr.total_len, 0, 0, _stream(), ctypes.byref(size))
    assert rc == _lib.ERR_CHECKSUM and size.value == 0                              # ... and says so when it is decoded


# ---- decode_range_device / decode_range ----

def _ranges(total, chunk):
    return [(0, 1), (chunk - 1, 2), (chunk + 5, 2 * chunk), (total - 1, 1), (0, total)]


@pytest.mark.parametrize("algo,form", [("chameleon", "paged"), ("chameleon", "slotted"), ("cheetah", "packed"), ("lion", "slotted")])
def test_decode_range_device_returns_the_inputs_bytes(algo, form):
    import torch
    data, chunk, blob, plain = _own(algo, form)
    for src in (blob, plain):
        d = torch.from_numpy(np.array(src)).cuda()
        h = container.parse_header(src)
        for offset, length in _ranges(data.size, chunk):
            got = container.decode_range_device(d.data_ptr(), src.size, offset, length, header=h if offset else None)
            assert got.dtype == torch.uint8 and got.numel() == length
            assert np.array_equal(got.cpu().numpy(), data[offset:offset + length]), (offset, length)
        for offset, length in [(0, 0), (5, 0), (data.size, 1), (data.size - 1, 2), (0, data.size + 1)]:
            with pytest.raises(ValueError):
                container.decode_range_device(d.data_ptr(), src.size, offset, length, header=h)


def test_decode_range_on_host_arrays():
    data, chunk, blob, _ = _own("chameleon", "packed")
    for offset, length in _ranges(data.size, chunk):
        got = container.decode_range(blob, offset, length)
        assert np.array_equal(got, data[offset:offset + length]), (offset, length)
    for offset, length in [(0, 0), (data.size, 1), (0, data.size + 1)]:
        with pytest.raises(ValueError):
            container.decode_range(blob, offset, length)


def test_a_range_beside_a_damaged_chunk_decodes_and_one_over_it_raises():
    import torch
    from test_gpu_verdicts import silent_damage_at
    data, chunk, blob, _ = _own("chameleon", "paged")
    bad = blob.copy()
    bad[silent_damage_at("chameleon", "paged", KIND, 1)] ^= vc.FLIP
    d = torch.from_numpy(bad).cuda()
    got = container.decode_range_device(d.data_ptr(), bad.size, 2 * chunk + 17, chunk)
    assert np.array_equal(got.cpu().numpy(), data[2 * chunk + 17:3 * chunk + 17])
    with pytest.raises(ChecksumError):
        container.decode_range_device(d.data_ptr(), bad.size, chunk - 1, 2)
    with pytest.raises(DecodeError):
        container.decode_range(bad, chunk + 9, 100)


# ---- refusals ----

def test_argument_and_capacity_refusals_leave_the_output_untouched():
    for blob in (uc.paged("a"), uc.sealed(uc.packed("a"), "a"), _own("cheetah", "slotted")[2]):
        h = container.parse_header(bytes(blob[:32]))
        nc = h.n_chunks
        for first, count in [(0, 0), (3, 0), (nc, 1), (0, nc + 1), (nc - 1, 2), (0xffffffff, 1), (1, 0xffffffff)]:
            rc, got = _rc(blob, first, count, cap=1 << 16)
            assert rc == _lib.ERR_ARGUMENT and (got == FILL).all(), (first, count)
        rc, got = _rc(blob, 1, 2, cap=container.slice_bound(h, 1, 2) - 1)
        assert rc == _lib.ERR_CAPACITY and (got == FILL).all()
        rc, got = _rc(blob, 1, 2, cap=container.slice_bound(h, 1, 2) - 1, want_header=False)
        assert rc == _lib.ERR_CAPACITY and (got == FILL).all()
        not_a_header = np.array(blob)
        not_a_header[0] ^= 1                                                        # the magic
        rc, got = _rc(not_a_header, 1, 2, cap=1 << 20)
        assert rc == _lib.ERR_ARGUMENT and (got == FILL).all()
        rc, got = _rc(not_a_header, 1, 2, cap=1 << 20, header=False)
        assert rc == _lib.ERR_ARGUMENT and (got == FILL).all()
        cut = np.array(blob)[:-1]                                                   # shorter than its container_len says
        rc, got = _rc(cut, 1, 2)
        assert rc == _lib.ERR_FORMAT and (got == FILL).all()
        rc, got = _rc(blob, 1, 2)
        assert rc == _lib.OK


# the chunk each mutation of unpage_cases.format_mutations damages
MUTATED_CHUNK = {"page number 0x7fff": 1, "bytes = 65538": 3, "bytes minus 2 in one entry": 0, "a chunk with 0 pages": 4, "a chunk with 200 pages": 5,
                 "size above safe_encode_buffer_size": 6}


def _payload_at(blob, first, count):
    h = container.parse_header(bytes(blob[:32]))
    length = min(h.total_len, (first + count) * h.chunk_size) - first * h.chunk_size
    ix0 = slice_cpu.up(32 + 4 * count, 16)
    return slice_cpu.up(ix0 + (length + 255) // 256, 16) if h.flags & container.FLAG_BLOCK_INDEX else ix0


@pytest.mark.parametrize("what", list(MUTATED_CHUNK))
def test_a_directory_fault_inside_the_window_is_a_format_error_and_one_outside_is_not_seen(what):
    assert set(MUTATED_CHUNK) == set(uc.format_mutations())
    blob, good, k = uc.format_mutations()[what], uc.paged("a"), MUTATED_CHUNK[what]
    inside = [(k, 1), (max(k - 1, 0), 2), (0, 7)]
    for first, count in inside:
        rc, got = _rc(blob, first, count)
        assert rc == _lib.ERR_FORMAT, (first, count, rc, _lib.last_error())
        assert (got[_payload_at(blob, first, count):] == FILL).all(), "no payload byte is written"
        rc, got = _rc(blob, first, count, want_header=False)
        assert rc == _lib.OK and (got[_payload_at(blob, first, count):] == FILL).all()
    outside = [w for w in [(0, k), (k + 1, 6 - k)] if w[1] > 0]
    for first, count in outside:
        hdr, got, cap = _slice(blob, first, count)
        _check_output(got, hdr, slice_cpu.slice_container(good, first, count), cap)


def test_size_table_faults_of_packed_and_slotted_windows():
    """an entry above its chunk's worst case, a window that runs past the container, an entry above its slot: refused inside the window, not seen behind it"""
    _, _, _, packed = _own("chameleon", "packed")
    _, _, _, slotted = _own("lion", "slotted")
    for blob, algo in ((packed, 0), (slotted, 2)):
        h = container.parse_header(blob)
        for value in (slice_cpu.safe_size(algo, h.chunk_size) + 1, 0x7fffffff):
            bad = blob.copy()
            uc.put32(bad, 32 + 4 * 3, value)
            for first, count in [(3, 1), (2, 3), (0, h.n_chunks)]:
                rc, got = _rc(bad, first, count)
                assert rc == _lib.ERR_FORMAT, (first, count, rc)
                assert (got[_payload_at(bad, first, count):] == FILL).all()
                rc, got = _rc(bad, first, count, want_header=False)
                assert rc == _lib.OK and (got[_payload_at(bad, first, count):] == FILL).all()
            hdr, got, cap = _slice(bad, 0, 3)                                       # the fault behind the window
            _check_output(got, hdr, slice_cpu.slice_container(blob, 0, 3), cap)
    # a packed window that would run past the container: the last entry says more than is there
    bad = packed.copy()
    last = container.parse_header(packed).n_chunks - 1
    uc.put32(bad, 32 + 4 * last, uc.get32(packed, 32 + 4 * last) + 64)
    rc, got = _rc(bad, last, 1)
    assert rc == _lib.ERR_FORMAT and (got[_payload_at(bad, last, 1):] == FILL).all()


# ---- profiling marks ----

def test_profiling_marks_and_the_asynchronous_form_on_a_callers_stream_and_workspace():
    import torch
    for algo, form in [("chameleon", "paged"), ("chameleon", "packed"), ("cheetah", "slotted")]:
        _, _, sealed_blob, plain = _own(algo, form)
        for blob, marks in ((plain, ["slice_layout", "slice_gather"]), (sealed_blob, ["slice_layout", "slice_gather", "move_trailer"])):
            h = container.parse_header(blob)
            cap = container.slice_bound(h, 1, 3)
            d, out = _buffers(blob, cap=cap)
            ws_size = int(_lib.lib().density_hip_decode_workspace_size(h.n_chunks))
            ws = torch.empty(ws_size, dtype=torch.uint8, device="cuda")
            s = torch.cuda.Stream()
            torch.cuda.synchronize()
            container.set_profiling(True)
            try:
                container.last_timings()
                assert container.slice_device(d.data_ptr(), blob.size, 1, 3, out.data_ptr(), cap, header=h, stream=s.cuda_stream, workspace=(ws.data_ptr(), ws_size),
                                              want_header=False) is None
                s.synchronize()
                names = [name for name, _ in container.last_timings()]
            finally:
                container.set_profiling(False)
            assert names == marks
            got = out.cpu().numpy()
            _check_output(got, container.parse_header(got[:32].tobytes()), slice_cpu.slice_container(blob, 1, 3), cap)
