"""Verdicts and salvage (include/density_hip.h: density_hip_decode_device_verdicts / density_hip_decode_verdicts): a sealed container says WHICH chunks are
damaged, and the rest of it is kept.

The contract, checked against ground truth (the input the container was made from), not against the library:

    after a verdict decode, chunk i's verdict word is 0  iff  the bytes now standing in chunk i's region of the output are input chunk i

for every form, every algorithm, and whatever damaged the chunk — a flipped PLAIN quad that decodes silently, a signature bit, a lying size table.  (One case
is about the trailer instead: see test_trailer_damage_reports_a_chunk_whose_bytes_are_right.)  Outputs are pre-filled with 0xA5 so that stale bytes cannot pass.

A library call with a NULL stream runs on the library's own stream, not torch's: buffers filled with torch are synchronised first."""
import ctypes
import functools

import numpy as np
import pytest

import verdict_cases as vc
from density_amd import ChecksumError, DecodeError, _lib, container, parallel
from oracle import pyoracle
from test_gpu_checksum import sealed_on_device, to_device

pytestmark = pytest.mark.gpu

CASES = [(algo, form, kind) for (algo, form) in vc.SHAPES for kind in vc.KINDS]
ALGOS = ["chameleon", "cheetah", "lion"]
POISON, VERDICT_POISON = 0xA5, 0x5A5A5A5A


@functools.lru_cache(maxsize=None)
def sealed(algo, form, kind):
    """(input, chunk size, sealed container on the host, its header, the unsealed container, its header): made once on the device, never written again"""
    data, chunk = vc.input_of(algo, form, kind)
    src, sptr = to_device(np.array(data))
    out, optr, cap, h0, before, h1 = sealed_on_device(algo, form, sptr, data.size, chunk)
    blob = out.cpu().numpy()[:h1.container_len].copy()
    want = {"paged": container.FLAG_PAGED, "slotted": container.FLAG_SLOTTED, "packed": 0}[form]
    assert h1.flags & (container.FLAG_PAGED | container.FLAG_SLOTTED) == want and h1.flags & container.FLAG_CHECKSUM
    assert h1.n_chunks == vc.n_chunks(algo, form) and data.size % chunk != 0
    blob.setflags(write=False)
    plain = before[:h0.container_len].copy()
    return data, chunk, blob, h1, plain, h0


def flipped(blob, *positions, bit=vc.FLIP):
    bad = blob.copy()
    for at in positions:
        bad[at] ^= bit
    return bad


def silent_damage_at(algo, form, kind, k):
    """the container offset of one SILENT flip in chunk k's stream (verdict_cases.silent_position, mapped through the form's layout)"""
    data, chunk, blob, h1, _, _ = sealed(algo, form, kind)
    pos, found = vc.silent_position(algo, kind, data.size, chunk, k)
    assert found >= 1, f"none of {vc.CANDIDATES} candidates decodes silently in the reference"
    stream = container.chunk_payloads(blob)[1][k]
    assert stream == pyoracle.encode(algo, data[k * chunk:(k + 1) * chunk])
    at = vc.stream_byte_at(blob, k, pos)
    assert blob[at] == stream[pos]
    return at


def verdict_decode(blob, n, blank, header=None, offset=0, workspace=None, sync=True):
    """One verdict decode of `blob` into 0xA5 at `offset` of its buffer: (return code, count, the n output bytes, the verdict words) — with sync=False code and
    count are None and everything is read after a device synchronise.  The bytes around the output and the words around the verdicts must stay as they were."""
    import torch
    nc = container.parse_header(blob).n_chunks
    dev = torch.from_numpy(np.array(blob)).cuda()
    out = torch.full((offset + n + 64,), POISON, dtype=torch.uint8, device="cuda")
    verdicts = torch.full((nc + 2,), VERDICT_POISON, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    res = container.decode_device_verdicts(dev.data_ptr(), blob.size, out.data_ptr() + offset, n, verdicts.data_ptr() + 4, header=header, blank=blank,
                                           workspace=workspace or (0, 0), sync=sync)
    torch.cuda.synchronize()
    got, v = out.cpu().numpy(), verdicts.cpu().numpy()
    assert (got[:offset] == POISON).all() and (got[offset + n:] == POISON).all(), "bytes around the output written"
    assert v[0] == VERDICT_POISON and v[-1] == VERDICT_POISON, "words around the verdicts written"
    rc, damaged = res if sync else (None, None)
    return rc, damaged, got[offset:offset + n], v[1:-1]


def check_contract(data, chunk, got, verdicts, blank):
    """verdict == 0 iff the region is the input chunk; blanked, a damaged region is all zeros.  Returns the damaged set."""
    damaged = set()
    for i in range(-(-data.size // chunk)):
        region, want = got[i * chunk:(i + 1) * chunk], data[i * chunk:(i + 1) * chunk]
        same = np.array_equal(region, want)
        assert verdicts[i] in (0, _lib.CHUNK_DAMAGED), (i, int(verdicts[i]))
        if not blank:
            assert (verdicts[i] == 0) == same, f"chunk {i}: verdict {int(verdicts[i])}, bytes {'right' if same else 'wrong'}"
        elif verdicts[i] == 0:
            assert same, f"chunk {i}: verdict 0, bytes wrong"
        else:
            assert not region.any(), f"chunk {i}: damaged and not blanked"
        if verdicts[i]:
            damaged.add(i)
    return damaged


def both_ways(data, chunk, bad, header=None, **kw):
    """the contract without and with blanking: (return code, count, damaged set), the same both times"""
    seen = []
    for blank in (False, True):
        rc, count, got, verdicts = verdict_decode(bad, data.size, blank, header=header, **kw)
        damaged = check_contract(data, chunk, got, verdicts, blank)
        assert count == len(damaged)
        seen.append((rc, count, damaged))
    assert seen[0] == seen[1], seen
    return seen[0]


@pytest.mark.parametrize("algo,form,kind", CASES)
def test_silent_damage_costs_one_chunk(algo, form, kind):
    data, chunk, blob, h1, _, _ = sealed(algo, form, kind)
    for k in vc.victims(algo, form):
        bad = flipped(blob, silent_damage_at(algo, form, kind, k))
        rc, count, damaged = both_ways(data, chunk, bad, header=h1)      # (the contract says the other chunks' bytes are the input's)
        assert damaged == {k} and count == 1 and rc == _lib.ERR_CHECKSUM, (k, rc, count, damaged)


@pytest.mark.parametrize("algo,form,kind", CASES)
def test_loud_damage_keeps_the_other_chunks(algo, form, kind):
    """A signature bit of chunk k's first record; chunk k's size-table entry lowered by 2.  What the decoder makes of either is its own business: the
    contract holds for every chunk, and no chunk but k is touched by it."""
    data, chunk, blob, h1, _, _ = sealed(algo, form, kind)
    for k in vc.victims(algo, form):
        signature = flipped(blob, vc.stream_byte_at(blob, k, 0), bit=0x01)
        table = blob.copy()
        size = int.from_bytes(bytes(blob[32 + 4 * k:36 + 4 * k]), "little")
        table[32 + 4 * k:36 + 4 * k] = np.frombuffer((size - 2).to_bytes(4, "little"), dtype=np.uint8)
        for what, bad in (("signature", signature), ("size table", table)):
            rc, count, damaged = both_ways(data, chunk, bad, header=h1)
            assert damaged <= {k}, (what, k, damaged)
            assert rc != _lib.OK, (what, k)


@pytest.mark.parametrize("algo,form", list(vc.SHAPES))
def test_two_damaged_chunks(algo, form):
    kind = "mixed"
    data, chunk, blob, h1, _, _ = sealed(algo, form, kind)
    first, _, last = vc.victims(algo, form)
    bad = flipped(blob, silent_damage_at(algo, form, kind, first), silent_damage_at(algo, form, kind, last))
    rc, count, damaged = both_ways(data, chunk, bad)                   # (header read from the device)
    assert (rc, count, damaged) == (_lib.ERR_CHECKSUM, 2, {first, last})


@pytest.mark.parametrize("algo,form", list(vc.SHAPES))
def test_trailer_damage_reports_a_chunk_whose_bytes_are_right(algo, form):
    """The one case where the contract's right-hand side is about the TRAILER: entry k no longer holds chunk k's checksum, so chunk k is reported although
    every byte of it decoded right — and with blanking its right bytes go, because nothing vouches for them."""
    data, chunk, blob, h1, _, _ = sealed(algo, form, "rep_text")
    for k in vc.victims(algo, form):
        bad = flipped(blob, vc.trailer_at(blob) + 4 * k + 1, bit=0x04)
        rc, count, got, verdicts = verdict_decode(bad, data.size, False, header=h1)
        assert (rc, count) == (_lib.ERR_CHECKSUM, 1) and [i for i, v in enumerate(verdicts) if v] == [k]
        assert np.array_equal(got, data)
        rc, count, got, verdicts = verdict_decode(bad, data.size, True, header=h1)
        assert (rc, count) == (_lib.ERR_CHECKSUM, 1) and [i for i, v in enumerate(verdicts) if v] == [k]
        want = data.copy()
        want[k * chunk:(k + 1) * chunk] = 0
        assert np.array_equal(got, want)


@pytest.mark.parametrize("algo,form,kind", CASES)
def test_intact_container(algo, form, kind):
    data, chunk, blob, h1, _, _ = sealed(algo, form, kind)
    for blank in (False, True):
        container.last_timings()
        container.set_profiling(True)
        try:
            rc, count, got, verdicts = verdict_decode(blob, data.size, blank, header=h1)
            names = [name for name, _ in container.last_timings()]
        finally:
            container.set_profiling(False)
        assert (rc, count) == (_lib.OK, 0) and not verdicts.any() and np.array_equal(got, data)
        assert _lib.last_error() == ""
        assert names == ["layout_decode", f"{algo}_decode_chunks", "checksum_verify", "chunk_verdicts"] + (["blank_chunks"] if blank else []), names


@pytest.mark.parametrize("algo", ALGOS)
def test_unsealed_container_is_an_argument_error(algo):
    data, chunk, blob, h1, plain, h0 = sealed(algo, "packed", "rep_text")
    for header in (h0, None):
        with pytest.raises(DecodeError) as e:
            verdict_decode(plain, data.size, True, header=header)
        assert e.type is DecodeError and f"error {_lib.ERR_ARGUMENT}" in str(e.value), str(e.value)
    # nothing written: the same call again, looked at from outside
    import torch
    dev = torch.from_numpy(plain).cuda()
    out = torch.full((data.size,), POISON, dtype=torch.uint8, device="cuda")
    verdicts = torch.full((h0.n_chunks,), VERDICT_POISON, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    damaged = ctypes.c_uint32(77)
    rc = _lib.lib().density_hip_decode_device_verdicts(dev.data_ptr(), plain.size, None, out.data_ptr(), data.size, 0, 0, 0, verdicts.data_ptr(), 1, ctypes.byref(damaged))
    torch.cuda.synchronize()
    assert rc == _lib.ERR_ARGUMENT and damaged.value == 77
    assert (out.cpu().numpy() == POISON).all() and (verdicts.cpu().numpy() == VERDICT_POISON).all()
    # unknown flag bits, a verdict buffer that is not word-aligned; a sealed container cut short is a format error at once
    sdev = torch.from_numpy(np.array(blob)).cuda()
    torch.cuda.synchronize()
    call = _lib.lib().density_hip_decode_device_verdicts
    assert call(sdev.data_ptr(), blob.size, None, out.data_ptr(), data.size, 0, 0, 0, verdicts.data_ptr(), 2, None) == _lib.ERR_ARGUMENT
    assert call(sdev.data_ptr(), blob.size, None, out.data_ptr(), data.size, 0, 0, 0, verdicts.data_ptr() + 2, 1, None) == _lib.ERR_ARGUMENT
    assert call(sdev.data_ptr(), blob.size - 16, None, out.data_ptr(), data.size, 0, 0, 0, verdicts.data_ptr(), 1, None) == _lib.ERR_FORMAT
    torch.cuda.synchronize()
    assert (out.cpu().numpy() == POISON).all() and (verdicts.cpu().numpy() == VERDICT_POISON).all()


def test_zero_chunks():
    import torch
    h = _lib.Header(0x31434844, 0, 1, container.FLAG_CHECKSUM, 65536, 0, 0, 32)
    dev = torch.from_numpy(np.frombuffer(bytes(h), dtype=np.uint8).copy()).cuda()
    torch.cuda.synchronize()
    damaged = ctypes.c_uint32(77)
    assert _lib.lib().density_hip_decode_device_verdicts(dev.data_ptr(), 32, None, 0, 0, 0, 0, 0, 0, 1, ctypes.byref(damaged)) == _lib.OK
    assert damaged.value == 0


@pytest.mark.parametrize("algo,form", [("chameleon", "paged"), ("cheetah", "packed"), ("lion", "slotted")])
def test_asynchronous_form(algo, form):
    """damaged_out = NULL: nothing is reported; verdicts, blanked output and — in the caller's workspace, second word — the count lie on the device."""
    import torch
    kind = "mixed"
    data, chunk, blob, h1, _, _ = sealed(algo, form, kind)
    k = vc.victims(algo, form)[1]
    bad = flipped(blob, silent_damage_at(algo, form, kind, k))
    need = int(_lib.lib().density_hip_decode_workspace_size_for(_lib.ALGO_IDS[algo], data.size, chunk))
    ws = torch.zeros(need, dtype=torch.uint8, device="cuda")
    rc, count, got, verdicts = verdict_decode(bad, data.size, True, header=h1, workspace=(ws.data_ptr(), need), sync=False)
    assert check_contract(data, chunk, got, verdicts, True) == {k}
    words = ws[:8].cpu().numpy().view(np.uint32)
    assert words[1] == 1 and words[0] == 0x100, words


@pytest.mark.parametrize("algo,form", [("chameleon", "packed"), ("chameleon", "slotted"), ("cheetah", "slotted"), ("lion", "packed")])
def test_placement(algo, form):
    """the output at odd offsets (the blanking kernel's ragged heads and tails), the caller's workspace at its smallest size"""
    import torch
    kind = "rep_text"
    data, chunk, blob, h1, _, _ = sealed(algo, form, kind)
    nc = h1.n_chunks
    need = int(_lib.lib().density_hip_decode_workspace_size(nc))
    ws = torch.zeros(need, dtype=torch.uint8, device="cuda")
    bad = flipped(blob, silent_damage_at(algo, form, kind, 0), silent_damage_at(algo, form, kind, nc - 1))
    for offset in (1, 7, 13):
        rc, count, damaged = both_ways(data, chunk, bad, header=h1, offset=offset, workspace=(ws.data_ptr(), need))
        assert (rc, count, damaged) == (_lib.ERR_CHECKSUM, 2, {0, nc - 1})


@pytest.mark.parametrize("algo", ALGOS)
def test_host_pointers(algo):
    kind = "mixed"
    data, chunk, blob, h1, plain, _ = sealed(algo, "packed", kind)
    k = vc.victims(algo, "packed")[1]
    bad = flipped(blob, silent_damage_at(algo, "packed", kind, k))
    for blank in (False, True):
        back = np.full(data.size + 100, POISON, dtype=np.uint8)
        n, damaged = container.decode_verdicts(bad, back, blank=blank)
        assert n == data.size and damaged == [k] and (back[data.size:] == POISON).all()
        assert "1 of 6 chunks damaged" in _lib.last_error(), _lib.last_error()
        verdicts = np.zeros(h1.n_chunks, dtype=np.uint32)
        verdicts[damaged] = 1
        assert check_contract(data, chunk, back[:data.size], verdicts, blank) == {k}
    back = np.full(data.size, POISON, dtype=np.uint8)
    assert container.decode_verdicts(blob, back) == (data.size, []) and np.array_equal(back, data) and _lib.last_error() == ""
    # every chunk damaged: nothing survives, 0 and a ChecksumError that names them all
    t = vc.trailer_at(blob)
    with pytest.raises(ChecksumError) as e:
        container.decode_verdicts(flipped(blob, *[t + 4 * i for i in range(h1.n_chunks)]), back)
    assert e.value.damaged_chunks == tuple(range(h1.n_chunks))
    # unsealed, a verdict buffer too small, an output too small: 0, nothing written
    back[:] = POISON
    with pytest.raises(DecodeError):
        container.decode_verdicts(plain, back)
    with pytest.raises(DecodeError):
        container.decode_verdicts(blob, back[:-1])
    v = (ctypes.c_uint32 * h1.n_chunks)()
    assert _lib.lib().density_hip_decode_verdicts(blob.ctypes.data, blob.size, back.ctypes.data, back.size, v, h1.n_chunks - 1, 1, None) == 0
    assert (back == POISON).all()
    # the existing calls raise as before, and do not know the chunks
    with pytest.raises(ChecksumError) as e:
        container.decode(bad, back) if algo != "chameleon" else container.decode(flipped(blob, t), back)
    assert e.value.damaged_chunks == ()


def test_multi_rank_salvage():
    import torch
    algo, form = "chameleon", "packed"
    parts, blobs = [], []
    for kind in vc.KINDS:
        data, chunk, blob, h1, _, _ = sealed(algo, form, kind)
        parts.append(data)
        blobs.append(blob)
    k = 3
    blobs[1] = flipped(blobs[1], silent_damage_at(algo, form, vc.KINDS[1], k))
    front, rows, total = parallel.multi_layout([b.size for b in blobs], [d.size for d in parts], 0, chunk)
    whole = np.zeros(total, dtype=np.uint8)
    whole[:len(front)] = np.frombuffer(front, dtype=np.uint8)
    for b, (off, ln, _) in zip(blobs, rows):
        whole[off:off + ln] = b
    dev = torch.from_numpy(whole).cuda()
    n = sum(d.size for d in parts)
    out = torch.full((n,), POISON, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    assert parallel.decode_multi_device(dev, out, salvage=True) == [(1, [k])]
    torch.cuda.synchronize()
    got = out.cpu().numpy()
    assert np.array_equal(got[:parts[0].size], parts[0])
    second = np.zeros(parts[1].size, dtype=np.uint32)
    second[k] = 1
    assert check_contract(parts[1], chunk, got[parts[0].size:], second, True) == {k}
    # without salvage the damaged blob ends the walk, as before
    with pytest.raises(ChecksumError):
        parallel.decode_multi_device(dev, out)
    # `out`: too short, not bytes, not contiguous — refused before anything is decoded
    out[:] = POISON
    torch.cuda.synchronize()
    for wrong in (out[:n - 1], torch.zeros(n, dtype=torch.int32, device="cuda"), torch.zeros(2 * n, dtype=torch.uint8, device="cuda")[::2], torch.zeros(n, dtype=torch.uint8)):
        for salvage in (False, True):
            with pytest.raises(ValueError):
                parallel.decode_multi_device(dev, wrong, salvage=salvage)
    assert (out.cpu().numpy() == POISON).all()
