"""Double parity (include/density_hip.h: version 2 of the parity blob "DHP1", density_hip_parity2_device and its host-pointer form, and the recover decode
with such a blob: any TWO damaged chunks of a parity group are rebuilt).

The blob is held byte for byte against the numpy model (parity2_cpu.py, whose field arithmetic goes through tables, not the kernels' packed doubling).  The
recover decode is held against ground truth — the input the container was made from — and against the contract of test_gpu_parity.py

    after a recover decode, chunk i's verdict is not DAMAGED  iff  the bytes now standing in chunk i's region of the output are input chunk i

The containers, the kinds of damage, the poisoned outputs and the guards around them are those of test_gpu_parity.py.  The blobs handed to the decoder are the
MODEL's unless a test says otherwise, so the two kernels are not checked against each other."""
import functools

import numpy as np
import pytest

import datagen
import parity2_cpu
import parity_cpu
import verdict_cases as vc
from density_amd import _lib, container
from oracle import pyoracle
from test_gpu_checksum import to_device
from test_gpu_parity import DAMAGED, OK, POISON, RECOVERED, ROW_TILE, check_contract, recover_decode
from test_gpu_verdicts import flipped, sealed, silent_damage_at, verdict_decode

pytestmark = pytest.mark.gpu

ALGOS = ["chameleon", "cheetah", "lion"]
GROUPS = 2
PAIRS = [(0, 2), (1, 3), (3, 5), (2, 4)]      # of one group with two groups; (3, 5) holds the ragged last chunk of the six-chunk shapes


@functools.lru_cache(maxsize=None)
def model_blob(algo, form, kind, groups=GROUPS):
    data, chunk = vc.input_of(algo, form, kind)
    blob = parity2_cpu.blob(data, chunk, groups)
    blob.setflags(write=False)
    return blob


def pairs_of(algo, form):
    """PAIRS as far as the shape has the chunks (the paged shape has four: its (1, 3) holds the ragged one)"""
    found = [p for p in PAIRS if p[1] < vc.n_chunks(algo, form)]
    assert len(found) >= 2
    return found


def device_blob(data, chunk, groups, in_offset=0, out_offset=0):
    """density_hip_parity2_device of `data` at in_offset of its buffer into 0xA5 at out_offset of another: the blob, with the bytes around it checked"""
    import torch
    size = container.parity2_size(data.size, chunk, groups)
    assert size == parity2_cpu.size(data.size, chunk, groups) and size > 0
    src, sptr = to_device(np.array(data), offset=in_offset, tail=32)
    out = torch.full((out_offset + size + 64,), POISON, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    container.parity2_device(sptr, data.size, chunk, groups, out.data_ptr() + out_offset, size)
    torch.cuda.synchronize()
    got = out.cpu().numpy()
    assert (got[:out_offset] == POISON).all() and (got[out_offset + size:] == POISON).all(), "bytes around the blob written"
    return got[out_offset:out_offset + size]


def two_flips(algo, form, kind, k1, k2):
    return flipped(sealed(algo, form, kind)[2], silent_damage_at(algo, form, kind, k1), silent_damage_at(algo, form, kind, k2))


# ------------------------------------------------------------------------------------------------------------------------------------------
# the blob

@pytest.mark.parametrize("groups", [1, 2, 3, 6, 7])
def test_blob_is_the_model(groups):
    data, chunk = vc.input_of("cheetah", "packed", "mixed")
    assert (data.size, chunk) == (5 * 65536 + 777, 65536)
    want = parity2_cpu.blob(data, chunk, groups)
    h = container.parse_parity_header(want)
    assert (h.version, h.n_groups, h.row_bytes) == (2, min(groups, 6), 65536) and want.size == 32 + 2 * h.n_groups * 65536
    for in_offset in (0, 1, 3):
        for out_offset in (0, 5):
            got = device_blob(data, chunk, groups, in_offset, out_offset)
            assert np.array_equal(got, want), (groups, in_offset, out_offset, np.flatnonzero(got != want)[:8])


@pytest.mark.parametrize("total,chunk,groups", [
    (1000, 65536, 3),                                   # one chunk, shorter than its size: two rows of 1008 bytes
    (0, 65536, 4),                                      # zero bytes: a bare header
    (3 * (ROW_TILE - 256) + 1001, ROW_TILE - 256, 2),   # chunk sizes at the row tile and 256 either side of it, the last chunk ending inside a 16-byte slot
    (3 * ROW_TILE + 1001, ROW_TILE, 2),
    (3 * (ROW_TILE + 256) + 1001, ROW_TILE + 256, 2),
    (2 * (ROW_TILE + 256) + 16, ROW_TILE + 256, 3),
    (255 * 256, 256, 1),                                # the longest group, 255 members: the longest chain of doublings, an odd trip count of the loop unrolled twice
    (255 * 256 + 100, 256, 2),                          # 128 members a group: an even one, the last chunk ragged
])
def test_blob_edge_shapes(total, chunk, groups):
    data = vc._input("mixed", 5 * 65536 + 777)[:total]
    want = parity2_cpu.blob(data, chunk, groups)
    assert want.size == 32 + 2 * min(groups, -(-total // chunk)) * ((min(total, chunk) + 15) // 16 * 16) and want[4] == 2
    for in_offset, out_offset in ((0, 0), (7, 9)):
        got = device_blob(data, chunk, groups, in_offset, out_offset)
        assert np.array_equal(got, want), (np.flatnonzero(got != want)[:8])


def test_blob_refusals():
    import torch
    data, chunk = vc.input_of("cheetah", "packed", "mixed")
    src, sptr = to_device(np.array(data))
    size = container.parity2_size(data.size, chunk, GROUPS)
    out = torch.full((size,), POISON, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    call = _lib.lib().density_hip_parity2_device
    assert call(sptr, data.size, chunk, GROUPS, out.data_ptr(), size - 1, 0) == _lib.ERR_CAPACITY
    assert call(sptr, data.size, 0, GROUPS, out.data_ptr(), size, 0) == _lib.ERR_ARGUMENT
    assert call(sptr, data.size, chunk, 0, out.data_ptr(), size, 0) == _lib.ERR_ARGUMENT
    assert call(sptr, data.size, chunk, GROUPS, 0, size, 0) == _lib.ERR_ARGUMENT
    # 256 chunks in one group: one more than the field has powers of 2 (version 1 takes the geometry)
    n = 255 * 256 + 100
    assert n <= data.size and container.parity2_size(n, 256, 1) == 0 and container.parity_size(n, 256, 1) == 32 + 256 <= size
    assert call(sptr, n, 256, 1, out.data_ptr(), size, 0) == _lib.ERR_ARGUMENT
    torch.cuda.synchronize()
    assert (out.cpu().numpy() == POISON).all()
    with pytest.raises(Exception) as e:
        container.parity2_device(sptr, data.size, chunk, GROUPS, out.data_ptr(), size - 1)
    assert f"error {_lib.ERR_CAPACITY}" in str(e.value)


def test_profiling_mark():
    data = vc._input("mixed", 5 * 65536 + 777)[:3 * 4096 + 5]
    container.last_timings()
    container.set_profiling(True)
    try:
        device_blob(data, 4096, 2)
        names = [name for name, _ in container.last_timings()]
    finally:
        container.set_profiling(False)
    assert names == ["parity2_rows"], names


# ------------------------------------------------------------------------------------------------------------------------------------------
# recovery

@pytest.mark.parametrize("algo,form", list(vc.SHAPES))
def test_two_silent_flips_in_one_group_are_recovered(algo, form):
    kind = "mixed"
    data, chunk, blob, h1, _, _ = sealed(algo, form, kind)
    parity = model_blob(algo, form, kind)
    assert data.size % chunk != 0 and container.parse_parity_header(parity).n_groups == GROUPS
    for k1, k2 in pairs_of(algo, form):
        bad = two_flips(algo, form, kind, k1, k2)
        for blank in (False, True):
            rc, damaged, recovered, got, verdicts = recover_decode(bad, parity, data.size, blank, header=h1)
            assert np.array_equal(got, data), (k1, k2, blank, np.flatnonzero(got != data)[:8])
            assert [int(v) for v in verdicts] == [RECOVERED if i in (k1, k2) else OK for i in range(h1.n_chunks)], (k1, k2, verdicts)
            assert (rc, damaged, recovered) == (_lib.OK, 0, 2), (k1, k2, rc, damaged, recovered)
            assert _lib.last_error() == ""


@pytest.mark.parametrize("algo", ALGOS)
def test_three_of_one_group_are_left_alone(algo):
    form, kind = "packed", "mixed"
    data, chunk, blob, h1, _, _ = sealed(algo, form, kind)
    parity = model_blob(algo, form, kind, 1)
    lost = (0, 2, 5)
    bad = flipped(blob, *[silent_damage_at(algo, form, kind, k) for k in lost])
    plain = verdict_decode(bad, data.size, False)[2]
    for blank in (False, True):
        rc, damaged, recovered, got, verdicts = recover_decode(bad, parity, data.size, blank)
        assert (rc, damaged, recovered) == (_lib.ERR_CHECKSUM, 3, 0), (rc, damaged, recovered)
        assert check_contract(data, chunk, got, verdicts, blank) == (set(lost), set())
        assert "3 of 6 chunks damaged, 0 recovered" in _lib.last_error(), _lib.last_error()
        if not blank:
            assert np.array_equal(got, plain), "an unrecoverable group's chunks are left as the decoder made them"


@pytest.mark.parametrize("algo", ALGOS)
def test_a_pair_in_one_group_and_a_single_in_the_other(algo):
    form, kind = "packed", "mixed"
    data, chunk, blob, h1, _, _ = sealed(algo, form, kind)
    parity = model_blob(algo, form, kind)
    bad = flipped(two_flips(algo, form, kind, 0, 2), silent_damage_at(algo, form, kind, 3))
    # ... and group 1's Q row damaged: its single chunk comes back through P, Q unread
    q_damaged = flipped(parity, parity2_cpu.row_offset(parity, 1, chunk // 2, q=True), bit=0x01)
    for blob2 in (parity, q_damaged):
        for blank in (False, True):
            rc, damaged, recovered, got, verdicts = recover_decode(bad, blob2, data.size, blank, header=h1)
            assert (rc, damaged, recovered) == (_lib.OK, 0, 3) and np.array_equal(got, data)
            assert check_contract(data, chunk, got, verdicts, blank) == (set(), {0, 2, 3})


@pytest.mark.parametrize("q_row", [True, False])
@pytest.mark.parametrize("algo,form", [("chameleon", "paged"), ("cheetah", "slotted"), ("lion", "packed")])
def test_a_damaged_row_never_passes_wrong_bytes(algo, form, q_row):
    """one bit of the group's Q row (of its P row) flipped, in the middle of the row — of as much of the row as both chunks of the pair cover"""
    kind = "mixed"
    data, chunk, blob, h1, _, _ = sealed(algo, form, kind)
    parity = model_blob(algo, form, kind)
    for k1, k2 in pairs_of(algo, form)[:2]:
        bad_parity = flipped(parity, parity2_cpu.row_offset(parity, k1 % GROUPS, min(chunk, data.size - k2 * chunk) // 2, q=q_row), bit=0x01)
        for blank in (False, True):
            rc, damaged, recovered, got, verdicts = recover_decode(two_flips(algo, form, kind, k1, k2), bad_parity, data.size, blank, header=h1)
            assert (rc, damaged, recovered) == (_lib.ERR_CHECKSUM, 2, 0), (k1, k2, rc, damaged, recovered)
            assert check_contract(data, chunk, got, verdicts, blank) == ({k1, k2}, set())
        # the same blob with one loss: the Q row is not read, the damaged P row cannot pass
        rc, damaged, recovered, got, verdicts = recover_decode(flipped(blob, silent_damage_at(algo, form, kind, k1)), bad_parity, data.size, True, header=h1)
        assert (rc, damaged, recovered) == ((_lib.OK, 0, 1) if q_row else (_lib.ERR_CHECKSUM, 1, 0)), (k1, rc, damaged, recovered)
        assert check_contract(data, chunk, got, verdicts, True) == ((set(), {k1}) if q_row else ({k1}, set()))
        # ... and under an intact container: nobody reads either row
        rc, damaged, recovered, got, verdicts = recover_decode(blob, bad_parity, data.size, True, header=h1)
        assert (rc, damaged, recovered) == (_lib.OK, 0, 0) and not verdicts.any() and np.array_equal(got, data)


@pytest.mark.parametrize("algo,form", list(vc.SHAPES))
def test_one_of_a_pair_has_a_damaged_trailer_entry(algo, form):
    """k1's bytes are damaged, k2's trailer entry is: both are rebuilt — k2 to the bytes it had — and each is held against its own entry"""
    kind = "mixed"
    data, chunk, blob, h1, _, _ = sealed(algo, form, kind)
    parity = model_blob(algo, form, kind)
    for k1, k2 in pairs_of(algo, form)[:2]:
        for flesh, entry in ((k1, k2), (k2, k1)):
            bad = flipped(flipped(blob, silent_damage_at(algo, form, kind, flesh)), vc.trailer_at(blob) + 4 * entry + 1, bit=0x04)
            rc, damaged, recovered, got, verdicts = recover_decode(bad, parity, data.size, False, header=h1)
            assert (rc, damaged, recovered) == (_lib.ERR_CHECKSUM, 1, 1), (flesh, entry, rc, damaged, recovered)
            assert [int(v) for v in verdicts] == [RECOVERED if i == flesh else DAMAGED if i == entry else OK for i in range(h1.n_chunks)]
            assert np.array_equal(got, data)
            rc, damaged, recovered, got, verdicts = recover_decode(bad, parity, data.size, True, header=h1)
            assert (rc, damaged, recovered) == (_lib.ERR_CHECKSUM, 1, 1)
            want = data.copy()
            want[entry * chunk:(entry + 1) * chunk] = 0
            assert np.array_equal(got, want)


def test_long_group():
    """forty members in one group: constants at places of 8 and more, the largest distance between the two, neighbours at the group's end"""
    chunk, n = 4096, 39 * 4096 + 1234
    data = datagen.rep_text(n, period=100_003, seed=41)
    room = np.zeros(container.container_bound("chameleon", n, chunk) + container.seal_overhead(n, chunk), dtype=np.uint8)
    blob = room[:container.encode_sealed("chameleon", data, room, chunk)]
    h1 = container.parse_header(blob)
    assert h1.n_chunks == 40 and h1.flags & container.FLAG_CHECKSUM and not h1.flags & (container.FLAG_PAGED | container.FLAG_SLOTTED)
    parity = parity2_cpu.blob(data, chunk, 1)

    def silent(k):
        part = data[k * chunk:(k + 1) * chunk]
        stream = pyoracle.encode("chameleon", part)
        pos = vc.chameleon_plain_position(stream, part.size)
        at = vc.stream_byte_at(blob, k, pos)
        assert blob[at] == stream[pos]
        return at

    for k1, k2 in ((0, 39), (7, 8), (38, 39)):
        bad = flipped(blob, silent(k1), silent(k2))
        assert sorted(np.flatnonzero(verdict_decode(bad, n, False)[3])) == [k1, k2]
        for blank in (False, True):
            rc, damaged, recovered, got, verdicts = recover_decode(bad, parity, n, blank, header=h1)
            assert (rc, damaged, recovered) == (_lib.OK, 0, 2), (k1, k2, rc, damaged, recovered)
            assert np.array_equal(got, data), (k1, k2, np.flatnonzero(got != data)[:8])
            assert check_contract(data, chunk, got, verdicts, blank) == (set(), {k1, k2})


# ------------------------------------------------------------------------------------------------------------------------------------------
# other paths

@pytest.mark.parametrize("algo,form", [("chameleon", "packed"), ("chameleon", "slotted"), ("cheetah", "slotted"), ("lion", "packed")])
def test_placement(algo, form):
    """the output and the blob at odd offsets (the pair's ragged heads and tails), the caller's workspace at both its sizes and 0xA5 behind it; two pairs, one with
    the ragged last chunk"""
    import torch
    kind = "mixed"
    data, chunk, blob, h1, _, _ = sealed(algo, form, kind)
    nc = h1.n_chunks
    for need in (int(_lib.lib().density_hip_decode_workspace_size(nc)), int(_lib.lib().density_hip_decode_workspace_size_for(_lib.ALGO_IDS[algo], data.size, chunk))):
        ws = torch.zeros(need + 64, dtype=torch.uint8, device="cuda")
        ws[need:] = POISON
        for (k1, k2), (offset, parity_offset) in zip(((3, 5), (0, 2), (1, 5), (3, 5)), ((1, 0), (7, 5), (13, 16), (16, 1))):
            rc, damaged, recovered, got, verdicts = recover_decode(two_flips(algo, form, kind, k1, k2), model_blob(algo, form, kind), data.size, False, header=h1,
                                                                   offset=offset, parity_offset=parity_offset, workspace=(ws.data_ptr(), need))
            assert (rc, damaged, recovered) == (_lib.OK, 0, 2) and np.array_equal(got, data), (offset, parity_offset, np.flatnonzero(got != data)[:8])
            assert check_contract(data, chunk, got, verdicts, False) == (set(), {k1, k2})
        assert (ws[need:].cpu().numpy() == POISON).all(), "bytes behind the workspace written"


@pytest.mark.parametrize("algo,form", [("chameleon", "paged"), ("cheetah", "packed"), ("lion", "slotted")])
def test_asynchronous_form(algo, form):
    """Both out pointers NULL: verdicts, the rebuilt output and — in the caller's workspace, second and third word — the counts lie on the device.  The blob is
    the device's own."""
    import torch
    kind = "mixed"
    data, chunk, blob, h1, _, _ = sealed(algo, form, kind)
    k1, k2 = pairs_of(algo, form)[1]
    need = int(_lib.lib().density_hip_decode_workspace_size_for(_lib.ALGO_IDS[algo], data.size, chunk))
    ws = torch.zeros(need + 64, dtype=torch.uint8, device="cuda")
    ws[need:] = POISON
    parity = device_blob(data, chunk, GROUPS)
    assert np.array_equal(parity, model_blob(algo, form, kind))
    rc, damaged, recovered, got, verdicts = recover_decode(two_flips(algo, form, kind, k1, k2), parity, data.size, True, header=h1,
                                                           parity_header=container.parse_parity_header(parity), workspace=(ws.data_ptr(), need), sync=False, parity_offset=3)
    assert np.array_equal(got, data) and check_contract(data, chunk, got, verdicts, True) == (set(), {k1, k2})
    words = ws[:12].cpu().numpy().view(np.uint32)
    assert words[1] == 0 and words[2] == 2, words
    assert (ws[need:].cpu().numpy() == POISON).all(), "bytes behind the workspace written"


@pytest.mark.parametrize("algo", ALGOS)
def test_host_pointers(algo):
    kind = "mixed"
    data, chunk, blob, h1, _, _ = sealed(algo, "packed", kind)
    want = model_blob(algo, "packed", kind)
    room = np.full(want.size + 100, POISON, dtype=np.uint8)
    assert container.parity2(np.array(data), chunk, GROUPS, room) == want.size
    assert np.array_equal(room[:want.size], want) and (room[want.size:] == POISON).all()
    from density_amd import EncodeError
    with pytest.raises(EncodeError):
        container.parity2(np.array(data), chunk, GROUPS, room[:want.size - 1])
    with pytest.raises(EncodeError):
        container.parity2(np.array(data[:255 * 256 + 100]), 256, 1, room)
    k = vc.victims(algo, "packed")[1]
    bad = two_flips(algo, "packed", kind, k, k + 2)
    for blank in (False, True):
        back = np.full(data.size + 100, POISON, dtype=np.uint8)
        n, damaged, recovered = container.decode_recover(bad, want, back, blank=blank)
        assert (n, damaged, recovered) == (data.size, [], [k, k + 2]) and np.array_equal(back[:data.size], data) and (back[data.size:] == POISON).all()
        assert _lib.last_error() == ""


@pytest.mark.parametrize("algo", ALGOS)
def test_version_1_is_unchanged(algo):
    form, kind = "packed", "mixed"
    data, chunk, blob, h1, _, _ = sealed(algo, form, kind)
    v2 = model_blob(algo, form, kind)
    v1 = parity_cpu.blob(data, chunk, GROUPS)
    assert np.array_equal(parity2_cpu.as_version_1(v2), v1)
    bad = two_flips(algo, form, kind, 2, 4)
    for blank in (False, True):
        rc, damaged, recovered, got, verdicts = recover_decode(bad, v1, data.size, blank, header=h1)
        assert (rc, damaged, recovered) == (_lib.ERR_CHECKSUM, 2, 0), (rc, damaged, recovered)
        assert check_contract(data, chunk, got, verdicts, blank) == ({2, 4}, set())
    # ... and a version-2 header in front of a blob of version-1 length is no blob
    short = v1.copy()
    short[4] = 2
    with pytest.raises(Exception) as e:
        recover_decode(bad, short, data.size, True, header=h1)
    assert f"error {_lib.ERR_FORMAT}" in str(e.value), str(e.value)
