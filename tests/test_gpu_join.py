"""density_hip_join_device / density_hip_join: the chunk windows of several containers, of any form, as ONE packed container — and what is made of it:
container.replace_chunks_device and parallel.multi_to_container_device.  The expectation is always the bytes of tests/join_cpu.py (held to the oracle in
tests/test_join_cpu.py), compared whole: the header, every byte below container_len and the fill beyond; for containers the library made,
density_hip_encode_device (+ density_hip_seal_device) of the windows' inputs one behind the other besides.  Outputs are pre-filled so that stale bytes
cannot pass.

A library call with a NULL stream runs on the library's own stream, not torch's: buffers filled with torch are synchronised first."""
import ctypes
import functools

import numpy as np
import pytest

import datagen
import join_cpu
import paged_cpu
import slice_cpu
import unpage_cases as uc
import verdict_cases as vc
from density_amd import EncodeError, _lib, container, parallel
from oracle import pyoracle

pytestmark = pytest.mark.gpu

FILL, GUARD = 0xA5, 256
KIND = "mixed"


def _stream():
    import torch
    torch.cuda.synchronize()
    return 0


def _upload(blob, off=0, tail=0):
    """the blob on the device at byte offset `off` of its allocation"""
    import torch
    d = torch.zeros(off + blob.size + tail, dtype=torch.uint8, device="cuda")
    d[off:off + blob.size] = torch.from_numpy(np.array(blob)).cuda()
    return d


def _rows(parts, in_offs=None):
    """[(blob, first, count), ...] on the device: (the tensors that own the memory, rows as container.join_device takes them)"""
    keep, rows = [], []
    for i, (blob, first, count) in enumerate(parts):
        off = in_offs[i] if in_offs else 0
        keep.append(_upload(blob, off))
        rows.append((keep[-1].data_ptr() + off, blob.size, container.parse_header(bytes(blob[:32])), first, count))
    return keep, rows


def _output(cap, out_off=0):
    import torch
    return torch.full((out_off + cap + GUARD,), FILL, dtype=torch.uint8, device="cuda")


def _join(parts, in_offs=None, out_off=0):
    """(header, the output allocation from out_off on as numpy, capacity) of one synchronous call at the capacity density_hip_join_bound() names"""
    keep, rows = _rows(parts, in_offs)
    cap = container.join_bound(rows)
    assert cap > 0
    out = _output(cap, out_off)
    hdr = container.join_device(rows, out.data_ptr() + out_off, cap, stream=_stream())
    return hdr, out.cpu().numpy()[out_off:], cap


def _raw(rows, n_parts, d_out, cap, want_header=True):
    """the return code of the raw call on rows (pointer, size, header or None, first, count)"""
    import torch
    arr = (_lib.JoinPart * max(len(rows), 1))()
    for i, (ptr, size, h, first, count) in enumerate(rows):
        arr[i] = _lib.JoinPart(ptr, size, ctypes.pointer(h) if h is not None else None, first, count)
    hdr = _lib.Header()
    rc = _lib.lib().density_hip_join_device(arr, n_parts, d_out, cap, 0, 0, _stream(), ctypes.byref(hdr) if want_header else None)
    torch.cuda.synchronize()
    return rc


def _rc(parts, cap=None, want_header=True):
    """(return code, output allocation as numpy) of the raw call on host blobs"""
    keep, rows = _rows(parts)
    cap = container.join_bound(rows) if cap is None else cap
    out = _output(cap)
    rc = _raw(rows, len(rows), out.data_ptr(), cap, want_header)
    return rc, out.cpu().numpy()


def _check_output(got, hdr, want, cap):
    assert hdr.container_len == want.size
    assert bytes(hdr) == want[:32].tobytes()
    assert np.array_equal(got[:want.size], want), int(np.flatnonzero(got[:want.size] != want)[0])
    assert (got[want.size:] == FILL).all(), "bytes at and beyond container_len keep the fill, the guards behind the capacity too"
    assert got.size == cap + GUARD and want.size <= cap


def _joins_to_the_model(parts, **kw):
    hdr, got, cap = _join(parts, **kw)
    want = join_cpu.join_containers(parts)
    _check_output(got, hdr, want, cap)
    return want


def _decodes_to(blob, want):
    """decode_device of a host-resident container returns `want` (a sealed one is verified on the way)"""
    import torch
    d = torch.from_numpy(np.array(blob)).cuda()
    back = torch.full((want.size + 64,), FILL, dtype=torch.uint8, device="cuda")
    assert container.decode_device(d.data_ptr(), blob.size, back.data_ptr(), want.size, stream=_stream()) == want.size
    got = back.cpu().numpy()
    assert np.array_equal(got[:want.size], want) and (got[want.size:] == FILL).all()


def _payload_at(parts):
    """where the joined container's first stream stands"""
    n = sum(c for _, _, c in parts)
    length = sum(join_cpu.window_len(b, f, c) for b, f, c in parts if c)
    ix0 = slice_cpu.up(32 + 4 * n, 16)
    flags = container.parse_header(bytes(parts[0][0][:32])).flags
    return slice_cpu.up(ix0 + (length + 255) // 256, 16) if flags & container.FLAG_BLOCK_INDEX else ix0


# ---- 1. CPU-built Chameleon containers, forms mixed in one call ----

def _cpu_blob(name, form, seal):
    blob = uc.packed(name) if form == "packed" else uc.paged(name, form == "shuffled")
    return uc.sealed(blob, name) if seal else blob


@pytest.mark.parametrize("seal", [False, True])
@pytest.mark.parametrize("forms", [("shuffled", "packed"), ("packed", "paged"), ("paged", "paged"), ("packed", "packed")])
def test_cpu_built_containers_c_then_d(forms, seal):
    parts = [(_cpu_blob("c", forms[0], seal), 0, 4), (_cpu_blob("d", forms[1], seal), 0, 3)]
    want = _joins_to_the_model(parts)
    assert container.parse_header(want[:32].tobytes()).flags == container.FLAG_BLOCK_INDEX | (container.FLAG_CHECKSUM if seal else 0)
    if seal:                                                                        # a container like any other: it decodes, and verifies, to the inputs
        _decodes_to(want, np.concatenate([uc.data("c"), uc.data("d")]))


@pytest.mark.parametrize("seal", [False, True])
def test_cpu_built_windows_of_one_container_in_three_forms(seal):
    chunk = uc.CASES["a"][2]
    parts = [(_cpu_blob("a", "packed", seal), 3, 3), (_cpu_blob("a", "shuffled", seal), 1, 2), (_cpu_blob("a", "paged", seal), 0, 0),
             (_cpu_blob("a", "packed", seal), 0, 1), (_cpu_blob("a", "paged", seal), 6, 1)]
    want = _joins_to_the_model(parts)
    if seal:
        a = uc.data("a")
        _decodes_to(want, np.concatenate([a[3 * chunk:6 * chunk], a[chunk:3 * chunk], a[:chunk], a[6 * chunk:]]))


def test_a_packed_window_as_the_only_part_has_zeros_in_its_gaps_whatever_the_source_holds_there():
    """where a one-part join is not a slice (tests/test_gpu_slice.py: the slice takes the gap's byte along)"""
    from test_gpu_slice import gap_plants
    blob = uc.packed("a")
    want = join_cpu.join_containers([(blob, 1, 2)])
    assert np.array_equal(want, slice_cpu.slice_container(blob, 1, 2))
    for bad, _, _, _ in gap_plants(blob, 1, 2):
        hdr, got, cap = _join([(bad, 1, 2)])
        _check_output(got, hdr, want, cap)


# ---- 2. the library's own containers ----

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


@functools.lru_cache(maxsize=None)
def _whole(algo, form, seal):
    """what encode_device (+ seal_device) writes for the whole input of shape (algo, form)"""
    data, chunk, _, _ = _own(algo, form)
    made = _encoded(algo, data, chunk, seal)
    made.setflags(write=False)
    return made


@pytest.mark.parametrize("seal", [False, True])
@pytest.mark.parametrize("algo,form", list(vc.SHAPES))
def test_a_container_split_in_two_joins_back_to_what_encode_device_writes(algo, form, seal):
    data, chunk, sealed_blob, plain = _own(algo, form)
    blob, n = sealed_blob if seal else plain, vc.n_chunks(algo, form)
    whole = _whole(algo, form, seal)
    for k in (1, n - 1):
        parts = [(blob, 0, k), (blob, k, n - k)]
        hdr, got, cap = _join(parts)
        _check_output(got, hdr, join_cpu.join_containers(parts), cap)
        _check_output(got, hdr, whole, cap)
    if seal:
        _decodes_to(got[:whole.size], data)


@pytest.mark.parametrize("seal", [False, True])
@pytest.mark.parametrize("algo,form", list(vc.SHAPES))
def test_a_slice_is_a_join_of_one_part(algo, form, seal):
    import torch
    _, _, sealed_blob, plain = _own(algo, form)
    blob = sealed_blob if seal else plain
    h = container.parse_header(bytes(blob[:32]))
    d = _upload(blob)
    for first, count in slice_cpu.windows(vc.n_chunks(algo, form)):
        row = (d.data_ptr(), blob.size, h, first, count)
        cap = container.join_bound([row])
        assert cap == container.slice_bound(h, first, count)
        joined, sliced = _output(cap), _output(cap)
        hj = container.join_device([row], joined.data_ptr(), cap, stream=_stream())
        hs = container.slice_device(d.data_ptr(), blob.size, first, count, sliced.data_ptr(), cap, header=h, stream=_stream())
        assert bytes(hj) == bytes(hs) and 32 < hj.container_len <= cap
        joined, sliced = joined.cpu().numpy(), sliced.cpu().numpy()
        assert np.array_equal(joined[:hj.container_len], sliced[:hj.container_len]), (first, count)
        assert (joined[hj.container_len:] == FILL).all() and (sliced[hj.container_len:] == FILL).all()


@pytest.mark.parametrize("seal", [False, True])
@pytest.mark.parametrize("algo,form,order", [("chameleon", "paged", [(2, 1), (0, 2), (3, 1)]), ("cheetah", "packed", [(3, 2), (0, 1), (1, 2), (5, 1)]),
                                             ("lion", "slotted", [(4, 1), (2, 2), (0, 2), (5, 1)])])
def test_a_permutation_of_whole_chunk_windows_is_the_encode_of_the_permuted_input(algo, form, order, seal):
    data, chunk, sealed_blob, plain = _own(algo, form)
    blob = sealed_blob if seal else plain
    parts = [(blob, first, count) for first, count in order]
    permuted = np.concatenate([data[first * chunk:(first + count) * chunk] for first, count in order])
    assert permuted.size == data.size
    hdr, got, cap = _join(parts)
    _check_output(got, hdr, join_cpu.join_containers(parts), cap)
    _check_output(got, hdr, _encoded(algo, permuted, chunk, seal), cap)


@pytest.mark.parametrize("seal", [False, True])
def test_mixed_forms_in_one_call(seal):
    pick = lambda algo, form: _own(algo, form)[2 if seal else 3]
    # packed with slotted: the two shapes share their input
    parts = [(pick("chameleon", "packed"), 0, 2), (pick("chameleon", "slotted"), 2, 3), (pick("chameleon", "packed"), 5, 1)]
    hdr, got, cap = _join(parts)
    _check_output(got, hdr, join_cpu.join_containers(parts), cap)
    _check_output(got, hdr, _whole("chameleon", "packed", seal), cap)
    # the paged shape's first chunk, the rest from a packed container of the same input
    packed = _whole("chameleon", "paged", seal)
    assert not container.parse_header(packed[:32].tobytes()).flags & (container.FLAG_PAGED | container.FLAG_SLOTTED)
    parts = [(pick("chameleon", "paged"), 0, 1), (packed, 1, 3)]
    hdr, got, cap = _join(parts)
    _check_output(got, hdr, join_cpu.join_containers(parts), cap)
    _check_output(got, hdr, packed, cap)
    parts = [(packed, 0, 2), (pick("chameleon", "paged"), 2, 2)]
    hdr, got, cap = _join(parts)
    _check_output(got, hdr, packed, cap)


# ---- 3. replace ----

@pytest.mark.parametrize("seal", [False, True])
@pytest.mark.parametrize("algo,form", [("chameleon", "paged"), ("cheetah", "slotted"), ("lion", "packed")])
def test_replacing_a_chunk_is_the_encode_of_the_patched_input(algo, form, seal):
    data, chunk, sealed_blob, plain = _own(algo, form)
    blob, n = sealed_blob if seal else plain, vc.n_chunks(algo, form)
    for k in (n // 2, n - 1):                                                       # a whole chunk in the middle, the ragged last one
        patched = data.copy()
        piece = patched[k * chunk:(k + 1) * chunk]
        piece[:] = datagen.by_kind("prose", piece.size, seed=11 + k)
        new = _encoded(algo, piece, chunk, seal)
        hb = container.parse_header(new[:32].tobytes())
        assert (hb.n_chunks, hb.chunk_size, hb.total_len) == (1, chunk, piece.size)
        a, b = _upload(blob), _upload(new)
        cap = container.container_bound(algo, data.size, chunk) + container.seal_overhead(data.size, chunk)
        out = _output(cap)
        _stream()
        hdr = container.replace_chunks_device(a.data_ptr(), blob.size, k, b.data_ptr(), new.size, out.data_ptr(), cap, header=None if k == n - 1 else container.parse_header(blob),
                                              new_header=None if k == n - 1 else hb)
        _check_output(out.cpu().numpy(), hdr, _encoded(algo, patched, chunk, seal), cap)


def test_replace_refuses_a_ragged_chunk_in_front_of_kept_ones_and_appends_behind_whole_chunks():
    data, chunk, _, plain = _own("cheetah", "packed")
    n = vc.n_chunks("cheetah", "packed")
    ragged = _encoded("cheetah", data[(n - 1) * chunk:], chunk, False)
    a, b = _upload(plain), _upload(ragged)
    cap = 2 * container.container_bound("cheetah", data.size, chunk)
    out = _output(cap)
    _stream()
    for first in (1, n + 1):
        with pytest.raises(EncodeError):
            container.replace_chunks_device(a.data_ptr(), plain.size, first, b.data_ptr(), ragged.size, out.data_ptr(), cap)
    with pytest.raises(EncodeError):                                                # an append behind a ragged end: the join itself refuses
        container.replace_chunks_device(a.data_ptr(), plain.size, n, b.data_ptr(), ragged.size, out.data_ptr(), cap)
    assert (out.cpu().numpy() == FILL).all()
    # behind whole chunks it appends: A's first two chunks as a container of their own, then the ragged one
    front = _encoded("cheetah", data[:2 * chunk], chunk, False)
    a = _upload(front)
    _stream()
    hdr = container.replace_chunks_device(a.data_ptr(), front.size, 2, b.data_ptr(), ragged.size, out.data_ptr(), cap)
    _check_output(out.cpu().numpy(), hdr, _encoded("cheetah", np.concatenate([data[:2 * chunk], data[(n - 1) * chunk:]]), chunk, False), cap)


# ---- 4. any byte alignment ----

@pytest.mark.parametrize("seal", [False, True])
def test_every_buffer_at_any_byte_alignment(seal):
    pick = lambda algo, form: _own(algo, form)[2 if seal else 3]
    packed = _whole("chameleon", "paged", seal)
    _joins_to_the_model([(pick("chameleon", "paged"), 0, 1), (packed, 1, 1), (pick("chameleon", "paged"), 2, 2)], in_offs=[1, 2, 3], out_off=3)
    _joins_to_the_model([(pick("lion", "slotted"), 0, 2), (pick("lion", "packed"), 2, 3), (pick("lion", "slotted"), 5, 1)], in_offs=[3, 1, 2], out_off=3)
    _joins_to_the_model([(_cpu_blob("a", "shuffled", seal), 0, 3), (_cpu_blob("a", "packed", seal), 3, 4)], in_offs=[1, 2], out_off=3)


# ---- 5. the scans' carries: windows behind the first tile of a source's scan, part seams inside the output's tiles ----

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


def test_more_chunks_than_the_scans_tiles_hold():
    blob = _many_chunks()
    parts = [(blob, 0, 1100), (blob, 1023, 77), (blob, 5, 1096)]
    want = _joins_to_the_model(parts)
    h = container.parse_header(want[:32].tobytes())
    assert h.n_chunks == 2273 and h.total_len == 2272 * 256 + 100


# ---- 6. what the host refuses ----

def test_host_refusals_leave_the_output_untouched():
    _, _, sealed_blob, plain = _own("cheetah", "packed")
    other_algo = _own("lion", "packed")[3]
    other_chunk = _whole("chameleon", "paged", False)
    n = vc.n_chunks("cheetah", "packed")
    keep, rows = _rows([(plain, 0, n - 1), (plain, 1, n - 1), (sealed_blob, 0, 2), (other_algo, 0, 2), (other_chunk, 0, 2), (_own("chameleon", "packed")[3], 0, 2)])
    whole, tail, sealed_row, lion_row, mib_row, cham_row = rows
    h = whole[2]

    def with_header(row, **changes):
        g = _lib.Header.from_buffer_copy(bytes(row[2]))
        for k, v in changes.items():
            setattr(g, k, v)
        return row[:2] + (g,) + row[3:]

    refused = {
        "no parts": ([whole], 0),
        "65 parts": ([(whole[0], whole[1], h, 0, 1)] * 65, 65),
        "all parts skipped": ([whole[:3] + (0, 0), tail[:3] + (2, 0)], 2),
        "a NULL pointer": ([whole, (0,) + tail[1:]], 2),
        "a NULL header": ([whole, tail[:2] + (None,) + tail[3:]], 2),
        "not a container's header": ([whole, with_header(tail, magic=h.magic ^ 1)], 2),
        "a window outside its chunks": ([whole, tail[:3] + (2, n - 1)], 2),
        "another algorithm": ([whole, lion_row], 2),
        "another chunk size": ([cham_row, mib_row], 2),
        "another index flag": ([cham_row, with_header(cham_row, flags=0)], 2),
        "another seal flag": ([whole, sealed_row], 2),
        "a ragged window that is not last": ([tail, whole], 2),
    }
    cap = 1 << 22
    out = _output(cap)
    for what, (part_rows, n_parts) in refused.items():
        for want_header in (True, False):
            assert _raw(part_rows, n_parts, out.data_ptr(), cap, want_header) == _lib.ERR_ARGUMENT, what
    assert (out.cpu().numpy() == FILL).all()
    # the capacity, a byte short; a container a byte short of what its header says
    good = [whole[:3] + (0, 2), tail]
    bound = container.join_bound(good)
    for want_header in (True, False):
        assert _raw(good, 2, out.data_ptr(), bound - 1, want_header) == _lib.ERR_CAPACITY
        assert _raw([good[0], (tail[0], tail[1] - 1) + tail[2:]], 2, out.data_ptr(), cap, want_header) == _lib.ERR_FORMAT
    assert _raw([sealed_row, (sealed_row[0], sealed_row[1] - 1) + sealed_row[2:]], 2, out.data_ptr(), cap) == _lib.ERR_FORMAT
    assert (out.cpu().numpy() == FILL).all()
    assert _raw(good, 2, out.data_ptr(), bound) == _lib.OK


def test_an_output_that_overlaps_a_part_is_refused():
    import torch
    _, _, _, plain = _own("cheetah", "packed")
    h = container.parse_header(plain)
    cap = container.join_bound([(1, plain.size, h, 0, 2)])
    room = torch.full((plain.size + cap + GUARD,), FILL, dtype=torch.uint8, device="cuda")      # the part, and room for an output behind it
    room[:plain.size] = torch.from_numpy(np.array(plain)).cuda()
    other = _upload(plain)
    base = room.data_ptr()
    for d_out, size in [(base + plain.size - 1, cap), (base, cap), (base + 32, cap)]:             # the last byte, the whole part, inside it
        assert _raw([(other.data_ptr(), plain.size, h, 0, 1), (base, plain.size, h, 1, 1)], 2, d_out, size) == _lib.ERR_ARGUMENT
    got = room.cpu().numpy()
    assert np.array_equal(got[:plain.size], plain) and (got[plain.size:] == FILL).all()
    assert _raw([(other.data_ptr(), plain.size, h, 0, 1), (base, plain.size, h, 1, 1)], 2, base + plain.size, cap) == _lib.OK      # side by side is no overlap
    assert _raw([(base, 0, None, 0, 0), (other.data_ptr(), plain.size, h, 0, 2)], 2, base, cap) == _lib.OK                          # a skipped part's range is nobody's


# ---- 7. what the device finds ----

def _refused_on_the_device(parts):
    at = _payload_at(parts)
    rc, got = _rc(parts)
    assert rc == _lib.ERR_FORMAT, (rc, _lib.last_error())
    assert (got[at:] == FILL).all(), "no payload byte of any part is written"
    rc, got = _rc(parts, want_header=False)
    assert rc == _lib.OK and (got[at:] == FILL).all()


def test_a_size_table_fault_in_the_second_parts_window_stops_every_part():
    for first_part in ((uc.paged("c"), 0, 4), (uc.packed("c"), 1, 2)):
        good = uc.packed("d")
        for value in (slice_cpu.safe_size(0, 256 << 10) + 1, 0x7fffffff):
            bad = good.copy()
            uc.put32(bad, 32 + 4 * 1, value)
            for window in [(1, 1), (0, 3), (1, 2)]:
                _refused_on_the_device([first_part, (bad,) + window])
            _joins_to_the_model([first_part, (bad, 0, 1)])                          # the fault behind the window is not seen
            assert np.array_equal(join_cpu.join_containers([first_part, (bad, 0, 1)]), join_cpu.join_containers([first_part, (good, 0, 1)]))
    # a packed window whose last stream runs past its container (one that ends 8 bytes early, and says so), and an entry above its slot
    bad = uc.packed("d")[:-8].copy()
    bad[24:32] = np.frombuffer(int(bad.size).to_bytes(8, "little"), dtype=np.uint8)
    _refused_on_the_device([(uc.paged("c"), 0, 4), (bad, 2, 1)])
    _joins_to_the_model([(uc.paged("c"), 0, 4), (bad, 0, 2)])
    _, _, _, slotted = _own("lion", "slotted")
    _, _, _, packed = _own("lion", "packed")
    bad = slotted.copy()
    uc.put32(bad, 32 + 4 * 3, slice_cpu.safe_size(2, 65536) + 1)
    _refused_on_the_device([(packed, 0, 2), (bad, 2, 4)])
    want = _joins_to_the_model([(packed, 0, 2), (bad, 4, 2)])
    assert np.array_equal(want, join_cpu.join_containers([(packed, 0, 2), (slotted, 4, 2)]))


# the chunk each mutation of unpage_cases.format_mutations damages
MUTATED_CHUNK = {"page number 0x7fff": 1, "bytes = 65538": 3, "bytes minus 2 in one entry": 0, "a chunk with 0 pages": 4, "a chunk with 200 pages": 5,
                 "size above safe_encode_buffer_size": 6}


@pytest.mark.parametrize("what", list(MUTATED_CHUNK))
def test_a_directory_fault_inside_a_window_is_a_format_error_and_one_outside_is_not_seen(what):
    assert set(MUTATED_CHUNK) == set(uc.format_mutations())
    blob, good, k = uc.format_mutations()[what], uc.paged("a"), MUTATED_CHUNK[what]
    front = (uc.packed("a"), 0, 2)
    inside = [(k, 1), (0, 7)] + ([(k - 1, 2)] if k else [(0, 2)])
    for window in inside:
        _refused_on_the_device([front, (blob,) + window])
    outside = [w for w in [(0, k), (k + 1, 6 - k)] if w[1] > 0]
    for window in outside:
        parts = [front, (blob,) + window]
        hdr, got, cap = _join(parts)
        _check_output(got, hdr, join_cpu.join_containers([front, (good,) + window]), cap)


# ---- 8. damage travels to the right place ----

@pytest.mark.parametrize("algo,forms,windows,j", [("cheetah", ("packed", "slotted"), [(1, 3), (2, 4)], 3), ("chameleon", (None, "paged"), [(0, 1), (1, 3)], 2),
                                                  ("lion", ("slotted", "packed"), [(0, 2), (0, 6)], 3)])
def test_a_silent_flip_in_a_part_is_named_at_its_output_chunk(algo, forms, windows, j):
    from test_gpu_verdicts import silent_damage_at, verdict_decode
    data, chunk, second, _ = _own(algo, forms[1])
    first = _own(algo, forms[0])[2] if forms[0] else _whole(algo, forms[1], True)
    bad = second.copy()
    bad[silent_damage_at(algo, forms[1], KIND, j)] ^= vc.FLIP
    parts = [(first,) + windows[0], (bad,) + windows[1]]
    want = _joins_to_the_model(parts)
    where = windows[0][1] + (j - windows[1][0])                                     # K_2 + j
    total = container.parse_header(want[:32].tobytes()).total_len
    rc, damaged, got, verdicts = verdict_decode(want, total, blank=False)
    assert damaged == 1 and np.flatnonzero(verdicts).tolist() == [where]
    expect = np.concatenate([data[f * chunk:(f + c) * chunk] for f, c in windows])
    for i in range(len(verdicts)):
        assert np.array_equal(got[i * chunk:(i + 1) * chunk], expect[i * chunk:(i + 1) * chunk]) == (i != where), i


# ---- 9. the asynchronous form ----

def test_the_asynchronous_form_on_a_callers_stream_and_workspace_and_the_profiling_marks():
    import torch
    for seal, marks in ((False, ["join_layout", "join_gather"]), (True, ["join_layout", "join_gather", "move_trailer"])):
        pick = lambda algo, form: _own(algo, form)[2 if seal else 3]
        for parts in ([(pick("chameleon", "paged"), 0, 2), (_whole("chameleon", "paged", seal), 2, 2)],
                      [(pick("cheetah", "slotted"), 0, 0), (pick("cheetah", "packed"), 1, 2), (pick("cheetah", "slotted"), 3, 3)]):
            keep, rows = _rows(parts)
            cap = container.join_bound(rows)
            out = _output(cap)
            ws_size = container.join_workspace_size(sum(1 for p in parts if p[2]), sum(p[2] for p in parts))
            ws = torch.empty(ws_size + GUARD, dtype=torch.uint8, device="cuda")
            ws[ws_size:] = FILL
            s = torch.cuda.Stream()
            torch.cuda.synchronize()
            container.set_profiling(True)
            try:
                container.last_timings()
                assert container.join_device(rows, out.data_ptr(), cap, stream=s.cuda_stream, workspace=(ws.data_ptr(), ws_size), want_header=False) is None
                s.synchronize()
                names = [name for name, _ in container.last_timings()]
            finally:
                container.set_profiling(False)
            assert names == marks
            got = out.cpu().numpy()
            _check_output(got, container.parse_header(got[:32].tobytes()), join_cpu.join_containers(parts), cap)
            assert (ws[ws_size:].cpu().numpy() == FILL).all(), "the workspace of density_hip_join_workspace_size() is all the call uses"
            with pytest.raises(EncodeError):                                        # a workspace a byte short is refused, not overrun
                container.join_device(rows, out.data_ptr(), cap, stream=s.cuda_stream, workspace=(ws.data_ptr(), ws_size - 1))


# ---- 10. host pointers ----

def test_the_host_pointer_form():
    for seal in (False, True):
        pick = lambda algo, form: _own(algo, form)[2 if seal else 3]
        for parts in ([(pick("chameleon", "paged"), 0, 1), (_whole("chameleon", "paged", seal), 1, 3)],
                      [(pick("lion", "packed"), 4, 1), (pick("lion", "slotted"), 0, 0), (pick("lion", "slotted"), 0, 4), (pick("lion", "packed"), 5, 1)]):
            want = join_cpu.join_containers(parts)
            cap = container.join_bound([(1, b.size, container.parse_header(b), f, c) for b, f, c in parts])
            out = np.full(cap + 16, FILL, dtype=np.uint8)
            assert container.join(parts, out[:-16]) == want.size
            assert np.array_equal(out[:want.size], want) and (out[want.size:] == FILL).all()
            with pytest.raises(EncodeError):
                container.join(parts, out[:cap - 1])
    a, b = _own("lion", "packed")[3], _own("cheetah", "packed")[3]
    out = np.full(1 << 22, FILL, dtype=np.uint8)
    for parts in ([], [(a, 0, 0)], [(a, 0, 2), (b, 2, 2)], [(a, 5, 1), (a, 0, 1)], [(a, 0, 7)], [(a, 0, 1)] * 65, [(a, 0, 2), (a[:-1], 2, 4)]):
        with pytest.raises(EncodeError):
            container.join(parts, out)
    assert (out == FILL).all()


# ---- 11. a multi-rank container "DHCM" becomes one DHC1, without a process group ----

def _shard(algo, form, data, chunk, seal=True):
    """a shard's sealed container as its rank would make it: (device tensor, length)"""
    import torch
    encoders = {"paged": (container.encode_device_paged, container.container_bound_paged), "slotted": (container.encode_device_slotted, container.container_bound_slotted),
                "packed": (container.encode_device, container.container_bound)}
    fn, bound = encoders[form]
    x = torch.from_numpy(np.array(data)).cuda()
    cap = bound(algo, data.size, chunk) + container.seal_overhead(data.size, chunk)
    cont = torch.zeros(cap, dtype=torch.uint8, device="cuda")
    hdr = fn(algo, x.data_ptr(), data.size, cont.data_ptr(), cap, chunk, stream=_stream())
    flag = {"paged": container.FLAG_PAGED, "slotted": container.FLAG_SLOTTED, "packed": 0}[form]
    assert hdr.n_chunks == 1 or hdr.flags & (container.FLAG_PAGED | container.FLAG_SLOTTED) == flag      # (one chunk: the forms are one, and the header says packed)
    if seal:
        hdr = container.seal_device(x.data_ptr(), data.size, cont.data_ptr(), cap, header=hdr, stream=_stream())
    return cont, hdr.container_len


def _super_container(blobs, input_bytes, algo, chunk):
    import torch
    front, rows, total = parallel.multi_layout([ln for _, ln in blobs], input_bytes, algo, chunk)
    out = torch.zeros(total, dtype=torch.uint8, device="cuda")
    out[:len(front)] = torch.frombuffer(bytearray(front), dtype=torch.uint8).cuda()
    for (t, ln), (off, _, _) in zip(blobs, rows):
        if ln:
            out[off:off + ln] = t[:ln]
    return out


def test_a_multi_rank_container_becomes_one_container():
    """Two cuts.  Four ranks' worth of a 1 MiB-chunk input cut by shard_chunks for two ranks — a paged shard of two whole chunks, a slotted one with the ragged
    end — with an empty rank's row between them; and an input of two chunks cut for three ranks, which leaves rank 0 empty (a paged shard needs two chunks,
    so this cut has none: its shards have one chunk each, where every form is the packed one)."""
    import torch
    data, chunk = vc.input_of("chameleon", "paged", KIND)
    (_, _, a0, a1), (_, _, b0, b1) = (parallel.shard_chunks(data.size, chunk, r, 2) for r in range(2))
    assert (a0, a1) == (0, 2 * chunk) and (b0, b1) == (2 * chunk, data.size)
    empty = (torch.zeros(0, dtype=torch.uint8, device="cuda"), 0)
    blobs = [_shard("chameleon", "paged", data[a0:a1], chunk), empty, _shard("chameleon", "slotted", data[b0:b1], chunk)]
    multi = _super_container(blobs, [a1 - a0, 0, b1 - b0], 0, chunk)
    torch.cuda.synchronize()
    got = parallel.multi_to_container_device(multi)
    torch.cuda.synchronize()
    want = _whole("chameleon", "paged", True)
    assert got.device == multi.device and got.numel() == want.size and np.array_equal(got.cpu().numpy(), want)
    out = torch.full((container.container_bound("chameleon", data.size, chunk) + container.seal_overhead(data.size, chunk) + GUARD,), FILL, dtype=torch.uint8, device="cuda")
    got = parallel.multi_to_container_device(multi, out=out)
    torch.cuda.synchronize()
    assert got.data_ptr() == out.data_ptr() and np.array_equal(got.cpu().numpy(), want) and (out[want.size:].cpu().numpy() == FILL).all()
    with pytest.raises(ValueError):
        parallel.multi_to_container_device(multi, out=out[:want.size - 1])

    data, chunk = vc.input_of("cheetah", "packed", KIND)
    data = data[:chunk + 777]
    cuts = [parallel.shard_chunks(data.size, chunk, r, 3) for r in range(3)]
    assert [c[1] - c[0] for c in cuts] == [0, 1, 1]
    blobs = [empty, _shard("cheetah", "slotted", data[cuts[1][2]:cuts[1][3]], chunk), _shard("cheetah", "packed", data[cuts[2][2]:cuts[2][3]], chunk)]
    multi = _super_container(blobs, [c[3] - c[2] for c in cuts], 1, chunk)
    torch.cuda.synchronize()
    got = parallel.multi_to_container_device(multi)
    torch.cuda.synchronize()
    assert np.array_equal(got.cpu().numpy(), _encoded("cheetah", data, chunk, True))
