"""Sealed containers on the device (include/density_hip.h: DENSITY_HIP_FLAG_CHECKSUM): the sum kernel against the numpy model at every shape and alignment
at which it takes another path, the seal of all three container forms, unsealed containers left exactly as they were, and the reason for the feature —
a flipped payload bit that the reference decodes to wrong bytes of the right length is a ChecksumError.

A library call with a NULL stream runs on the library's own stream, not torch's: buffers filled with torch are synchronised first."""
import os

import numpy as np
import pytest

import datagen
from density_amd import ChecksumError, DecodeError, EncodeError, _lib, container, parallel
from oracle import pyoracle
from test_checksum_cpu import model
from test_gpu_buffer_contracts import Region

pytestmark = pytest.mark.gpu

ALGOS = ["chameleon", "cheetah", "lion"]
SESSION_VARIANT = int(os.environ.get("DENSITY_TEST_VARIANT", "0") or 0)      # (conftest.py: the whole session on another kernel family)
BOUNDS = {"packed": container.container_bound, "slotted": container.container_bound_slotted, "paged": container.container_bound_paged}
ENCODERS = {"packed": container.encode_device, "slotted": container.encode_device_slotted, "paged": container.encode_device_paged}


def to_device(arr, offset=0, tail=0):
    """(tensor that owns the memory, device address of arr's copy at `offset` bytes into it)"""
    import torch
    buf = torch.zeros(offset + arr.size + tail, dtype=torch.uint8, device="cuda")
    buf[offset:offset + arr.size] = torch.from_numpy(np.ascontiguousarray(arr))
    torch.cuda.synchronize()
    return buf, buf.data_ptr() + offset


def zeros(n, offset=0):
    import torch
    buf = torch.zeros(offset + n, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    return buf, buf.data_ptr() + offset


def host(buf, offset=0, n=None):
    import torch
    torch.cuda.synchronize()
    return buf[offset:None if n is None else offset + n].cpu().numpy()


def chunk_sums(data, chunk):
    return [model(data[i:i + chunk]) for i in range(0, data.size, chunk)]


def trailer_bytes(n_chunks):
    return (4 * n_chunks + 15) // 16 * 16


# ------------------------------------------------------------------------------------------------------------------------------------------
# 1. the sum kernel
# ------------------------------------------------------------------------------------------------------------------------------------------
# one byte; a chunk's last word padded; many one-tile chunks and a ragged one; exactly two 32 KiB tiles; a ragged last chunk that is no multiple of 4;
# chunks of several tiles; chunks of 128 tiles each (the atomics of many work-groups meet in one accumulator)
SUM_SHAPES = [(1, 256, "random"), (255, 256, "prose"), (4099, 256, "random"), (65536, 65536, "prose"), (900_001, 65536, "random"),
              (3 * (1 << 20) + 12345, 1 << 18, "prose"), (9 * (1 << 20) + 3, 4 << 20, "zeros")]


@pytest.mark.parametrize("n,chunk,kind", SUM_SHAPES)
def test_checksum_device_matches_the_model(n, chunk, kind):
    import torch
    data = datagen.by_kind(kind, n, seed=17)
    want = chunk_sums(data, chunk)
    assert len(want) == -(-n // chunk)
    for off in (0, 1, 2, 3):
        buf, ptr = to_device(data, off, tail=64)
        sums = torch.full((len(want),), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        for again in (0, 1):                                           # the accumulators are cleared by the call, not by the caller
            container.checksum_device(ptr, n, chunk, sums.data_ptr())
            got = [int(v) & 0xFFFFFFFF for v in host(sums)]
            assert got == want, (off, again, [hex(g) for g in got[:4]], [hex(w) for w in want[:4]])


def test_checksum_device_arguments():
    buf, ptr = zeros(1024)
    sums, sp = zeros(64)
    for bad_chunk in (0, 100, 255, (1 << 30) + 256):
        with pytest.raises(EncodeError):
            container.checksum_device(ptr, 1024, bad_chunk, sp)
    with pytest.raises(EncodeError):
        container.checksum_device(ptr, 1024, 256, sp + 2)               # d_sums: words
    container.checksum_device(ptr, 0, 256, sp)                          # nothing to sum


# ------------------------------------------------------------------------------------------------------------------------------------------
# 2. seal and round trip, all forms
# ------------------------------------------------------------------------------------------------------------------------------------------
SEAL_SHAPES = [("prose", 3 * (1 << 20) + 12345, 1 << 18), ("mixed", 40 * 4096 + 77, 4096), ("random", 900_001, 65536), ("prose", 70_000, 1 << 20)]


def sealed_on_device(algo, form, d_src, n, chunk, header=True, offset=0, slack=0):
    """encode_device* + seal_device into a zeroed buffer: (buffer, address, capacity, unsealed header or None, clone before the seal or None, sealed header or None)"""
    cap = BOUNDS[form](algo, n, chunk) + container.seal_overhead(n, chunk) + slack
    out, optr = zeros(cap, offset)
    if header:
        h0 = ENCODERS[form](algo, d_src, n, optr, cap, chunk)
        before = host(out, offset).copy()
        h1 = container.seal_device(d_src, n, optr, cap, header=h0)
        return out, optr, cap, h0, before, h1
    ENCODERS[form](algo, d_src, n, optr, cap, chunk, want_header=False)
    container.seal_device(d_src, n, optr, cap, header=None, want_header=False)
    return out, optr, cap, None, None, None


def check_sealed(algo, data, chunk, h0, before, h1, blob):
    """what the header file says of a sealed container, against the unsealed one it was made from"""
    n = data.size
    nc = -(-n // chunk)
    t = (h0.container_len + 15) // 16 * 16
    assert h1.flags == h0.flags | container.FLAG_CHECKSUM and (h1.n_chunks, h1.total_len, h1.chunk_size) == (nc, n, chunk)
    assert h1.container_len == t + trailer_bytes(nc)
    got_h = container.parse_header(blob)
    assert (got_h.flags, got_h.container_len) == (h1.flags, h1.container_len)
    # nothing in front of the trailer moves: the flags and container_len fields are the only bytes that differ (the buffer was zeroed: so are [E, T))
    same = blob[:t] == before[:t]
    same[6:8] = True
    same[24:32] = True
    assert same.all(), np.flatnonzero(~same)[:8]
    assert not before[h0.container_len:t].any()
    want = chunk_sums(data, chunk)
    assert container.chunk_checksums(blob[:h1.container_len]) == want
    assert not blob[t + 4 * nc:h1.container_len].any()
    _, payloads = container.chunk_payloads(blob[:h1.container_len])
    assert len(payloads) == nc
    for i in sorted({0, nc // 2, nc - 1}):
        assert payloads[i] == pyoracle.encode(algo, data[i * chunk:(i + 1) * chunk]), i


def decode_back(ptr, size, data, header=None, offset=0):
    back, bptr = zeros(data.size + 100, offset)
    got = container.decode_device(ptr, size, bptr, data.size + 100, header=header)
    res = host(back, offset)
    assert got == data.size and np.array_equal(res[:data.size], data) and not res[data.size:].any()


@pytest.mark.parametrize("kind,n,chunk", SEAL_SHAPES)
@pytest.mark.parametrize("algo", ALGOS)
def test_seal_and_round_trip(algo, kind, n, chunk):
    data = datagen.by_kind(kind, n, seed=23)
    src, sptr = to_device(data)
    blobs = {}
    for form in ("packed", "slotted"):
        out, optr, cap, h0, before, h1 = sealed_on_device(algo, form, sptr, n, chunk)
        blob = host(out)
        check_sealed(algo, data, chunk, h0, before, h1, blob)
        assert bool(h1.flags & container.FLAG_SLOTTED) == (form == "slotted" and n > chunk)
        decode_back(optr, h1.container_len, data, header=h1)
        blobs[form] = blob[:h1.container_len].copy()
        # the same with nothing on the host: no header in, none out, the input at +3 and the container at +5
        src3, sptr3 = to_device(data, 3)
        out2, optr2, _, _, _, _ = sealed_on_device(algo, form, sptr3, n, chunk, header=False, offset=5)
        blob2 = host(out2, 5)
        assert np.array_equal(blob2[:h1.container_len], blobs[form]), form
        decode_back(optr2, h1.container_len, data, header=None)
        # sealing twice: refused from the caller's header, and from the one on the device
        with pytest.raises(EncodeError):
            container.seal_device(sptr, n, optr, cap, header=h1)
        with pytest.raises(EncodeError):
            container.seal_device(sptr, n, optr, cap, header=None)
        assert np.array_equal(host(out)[:h1.container_len], blobs[form]), "a refused seal wrote to the container"
        if form == "slotted":
            # pack_device carries the trailer along: byte for byte encode_device + seal_device
            pcap = container.container_bound(algo, n, chunk) + container.seal_overhead(n, chunk)
            packed, pptr = zeros(pcap)
            ph = container.pack_device(optr, h1.container_len, pptr, pcap, header=h1)
            assert ph.flags == h1.flags & ~container.FLAG_SLOTTED
            assert np.array_equal(host(packed)[:ph.container_len], blobs["packed"]) and ph.container_len == blobs["packed"].size
            packed2, pptr2 = zeros(pcap)
            container.pack_device(optr2, h1.container_len, pptr2, pcap, header=None, want_header=False)
            assert np.array_equal(host(packed2)[:ph.container_len], blobs["packed"])


def test_seal_paged():
    n, chunk = 8 << 20, 1 << 20
    data = datagen.by_kind("rep", n, seed=23)
    src, sptr = to_device(data)
    out, optr, cap, h0, before, h1 = sealed_on_device("chameleon", "paged", sptr, n, chunk)
    assert h0.flags & container.FLAG_PAGED and h0.container_len % 16 == 0
    blob = host(out)
    check_sealed("chameleon", data, chunk, h0, before, h1, blob)
    decode_back(optr, h1.container_len, data, header=h1)
    out2, optr2, _, _, _, _ = sealed_on_device("chameleon", "paged", sptr, n, chunk, header=False)
    h2 = container.parse_header(host(out2))
    assert h2.flags == h1.flags                                        # (pages are handed out in the order the work-groups ask: the bytes may differ)
    assert container.chunk_checksums(host(out2)[:h2.container_len]) == chunk_sums(data, chunk)
    decode_back(optr2, h2.container_len, data, header=None)
    with pytest.raises(EncodeError):                                   # a paged container is wire-ready as it stands, sealed or not
        container.pack_device(optr, h1.container_len, zeros(cap)[1], cap, header=h1)


@pytest.mark.parametrize("form", ["packed", "slotted"])
@pytest.mark.parametrize("name", ["b", "a"])
def test_pack_of_a_sealed_cpu_built_container_places_trailer_gap_and_padding(name, form):
    """the CPU-built containers of tests/unpage_cases.py (b: 4 chunks, a trailer of exactly 16 bytes; a: 7 chunks, 4 bytes of padding behind it), sealed, in
    the packed form and in worst-case slots: pack_device writes the model's sealed packed container, whole, and nothing behind it"""
    import torch
    import slice_cpu
    import unpage_cases as uc
    _, n, chunk, _ = uc.CASES[name]
    nc, _, _, base, _ = uc.geometry(n, chunk)
    want = uc.sealed(uc.packed(name), name)
    blob = uc.packed(name)
    if form == "slotted":
        ss, stride = uc.streams(name), slice_cpu.up(slice_cpu.safe_size(0, chunk), 256)
        blob = np.zeros(base + (nc - 1) * stride + len(ss[-1]), dtype=np.uint8)
        blob[:base] = uc.packed(name)[:base]
        for i, s in enumerate(ss):
            blob[base + i * stride:base + i * stride + len(s)] = np.frombuffer(s, dtype=np.uint8)
        h = container.parse_header(blob[:32].tobytes())
        h.flags |= container.FLAG_SLOTTED
        h.container_len = blob.size
        blob[:32] = np.frombuffer(bytes(h), dtype=np.uint8)
    blob = uc.sealed(blob, name)
    src, sptr = to_device(blob)
    cap = container.container_bound("chameleon", n, chunk) + container.seal_overhead(n, chunk)
    out = torch.full((cap + 256,), 0xA5, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    hdr = container.pack_device(sptr, blob.size, out.data_ptr(), cap)
    got = host(out)
    assert bytes(hdr) == want[:32].tobytes() and hdr.flags == container.FLAG_BLOCK_INDEX | container.FLAG_CHECKSUM
    assert np.array_equal(got[:want.size], want), int(np.flatnonzero(got[:want.size] != want)[0])
    assert (got[want.size:] == 0xA5).all()


@pytest.mark.parametrize("algo", ALGOS)
def test_seal_capacity_one_byte_short(algo):
    """A capacity one byte below the sealed container_len: refused from the caller's header at once, and by the device otherwise; the container stays unsealed."""
    kind, n, chunk = SEAL_SHAPES[2]
    data = datagen.by_kind(kind, n, seed=23)
    src, sptr = to_device(data)
    cap = container.container_bound(algo, n, chunk) + container.seal_overhead(n, chunk)
    out, optr = zeros(cap)
    h0 = container.encode_device(algo, sptr, n, optr, cap, chunk)
    before = host(out).copy()
    sealed_len = (h0.container_len + 15) // 16 * 16 + trailer_bytes(h0.n_chunks)
    for header in (h0, None):
        with pytest.raises(EncodeError) as e:
            container.seal_device(sptr, n, optr, sealed_len - 1, header=header)
        assert f"error {_lib.ERR_CAPACITY}" in str(e.value), str(e.value)
        assert np.array_equal(host(out), before), "a refused seal wrote to the container"
        with pytest.raises(EncodeError) as e:                          # an input that is not the container's
            container.seal_device(sptr, n - 1, optr, cap, header=header)
        assert f"error {_lib.ERR_ARGUMENT}" in str(e.value), str(e.value)
        assert np.array_equal(host(out), before), "a refused seal wrote to the container"
    container.seal_device(sptr, n, optr, sealed_len - 1, header=None, want_header=False)      # asynchronous: nothing reported, nothing sealed
    assert np.array_equal(host(out), before)
    h1 = container.seal_device(sptr, n, optr, sealed_len, header=None)                         # exactly enough
    assert h1.container_len == sealed_len and container.chunk_checksums(host(out)[:sealed_len]) == chunk_sums(data, chunk)


def test_zero_length_input_seals_to_the_flag():
    h0 = _lib.Header(0x31434844, 0, 1, 0, 65536, 0, 0, 32)                # the container of an empty input: its header
    out, optr = to_device(np.frombuffer(bytes(h0), dtype=np.uint8), tail=32)
    h1 = container.seal_device(0, 0, optr, 64, header=None)
    assert (h1.flags, h1.container_len, h1.n_chunks) == (h0.flags | 8, 32, 0)
    assert container.chunk_checksums(host(out)[:32]) == []


# ------------------------------------------------------------------------------------------------------------------------------------------
# 3. unsealed containers are untouched
# ------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("algo", ALGOS)
def test_unsealed_containers_are_untouched(algo):
    """An unsealed round trip gives the same bytes through the same kernels, in the same order, whether or not a seal and a verify of another container
    ran in between on the same workspace and error word."""
    n, chunk = 900_001, 65536
    data = datagen.by_kind("mixed", n, seed=29)
    other = datagen.by_kind("prose", 300_000, seed=30)
    src, sptr = to_device(data)
    cap = container.container_bound(algo, n, chunk)

    def round_trip():
        out, optr = zeros(cap)
        container.last_timings()
        container.set_profiling(True)
        try:
            h = container.encode_device(algo, sptr, n, optr, cap, chunk)
            back, bptr = zeros(n)
            assert container.decode_device(optr, h.container_len, bptr, n, header=h) == n
            names = [name for name, _ in container.last_timings()]
        finally:
            container.set_profiling(False)
        return host(out)[:h.container_len].copy(), host(back).copy(), names, h.flags

    blob_a, back_a, names_a, flags = round_trip()
    assert not flags & container.FLAG_CHECKSUM and np.array_equal(back_a, data)
    if SESSION_VARIANT == 0:
        assert names_a == [f"{algo}_encode_chunks", "layout_encode", "compact", "layout_decode", f"{algo}_decode_chunks"], names_a
    # a seal and a verify (one that fails, too) of another container
    osrc, osptr = to_device(other)
    out, optr, ocap, h0, before, h1 = sealed_on_device(algo, "packed", osptr, other.size, chunk)
    decode_back(optr, h1.container_len, other, header=h1)
    out[h1.container_len - trailer_bytes(h1.n_chunks)] ^= 1
    with pytest.raises(ChecksumError):
        decode_back(optr, h1.container_len, other, header=h1)
    blob_b, back_b, names_b, _ = round_trip()
    assert np.array_equal(blob_a, blob_b) and np.array_equal(back_b, data) and names_a == names_b


# ------------------------------------------------------------------------------------------------------------------------------------------
# 4. corruption: the reason for the feature
# ------------------------------------------------------------------------------------------------------------------------------------------
CHUNK = 65536
VICTIM = 2          # the chunk whose stream is damaged.  (Chunk 1 of this input leaves out 3 of Lion's 16 positions on prose, counted with the CPU oracle; chunks 0, 2 and
                    # 3 leave out at most 2 for every algorithm and kind, like the single-chunk recipe this test is modelled on.)


def payload_offset(blob, i):
    """where chunk i's stream starts in a host-resident PACKED container"""
    h = container.parse_header(blob)
    off = (32 + 4 * h.n_chunks + 15) // 16 * 16
    if h.flags & container.FLAG_BLOCK_INDEX:
        off = (off + (h.total_len + 255) // 256 + 15) // 16 * 16
    for k in range(i):
        off = (off + int.from_bytes(blob[32 + 4 * k:36 + 4 * k].tobytes(), "little") + 15) // 16 * 16
    return off


def silently_wrong(algo, stream, part):
    """the 16 positions of the recipe, and which of them the reference decodes to wrong bytes of the right length"""
    counted = []
    for k in range(16):
        pos = len(stream) * (2 * k + 1) // 32
        bad = bytearray(stream)
        bad[pos] ^= 0x10
        out = pyoracle.decode(algo, bytes(bad), CHUNK)
        if len(out) == CHUNK and out != part.tobytes():
            counted.append(pos)
    return counted


@pytest.mark.parametrize("kind", ["random", "prose"])
@pytest.mark.parametrize("algo", ALGOS)
def test_flipped_payload_bits_are_checksum_errors(algo, kind):
    n = 4 * CHUNK
    data = datagen.by_kind(kind, n, seed=3)
    src, sptr = to_device(data)
    sealed, sp, cap, h0, before, h1 = sealed_on_device(algo, "packed", sptr, n, CHUNK)
    plain, pp = to_device(before[:h0.container_len])
    blob = host(sealed)[:h1.container_len].copy()
    stream = container.chunk_payloads(blob)[1][VICTIM]
    part = data[VICTIM * CHUNK:(VICTIM + 1) * CHUNK]
    assert stream == pyoracle.encode(algo, part)
    counted = silently_wrong(algo, stream, part)
    print(f"{algo} {kind}: {len(counted)} of 16 positions decode silently wrong in the reference")
    assert 16 - len(counted) <= 2, counted
    at = payload_offset(blob, VICTIM)
    assert blob[at:at + len(stream)].tobytes() == stream
    back, bptr = zeros(n)
    outcomes = {"checksum": 0, "format": 0}
    for pos in counted:
        plain[at + pos] ^= 0x10
        sealed[at + pos] ^= 0x10
        host(plain, 0, 1)                                              # (torch's writes before the library's stream reads)
        try:
            unsealed_ok = container.decode_device(pp, h0.container_len, bptr, n, header=h0) == n
            assert not np.array_equal(host(back), data), pos        # wrong bytes of the right length, and OK: what the feature is for
        except ChecksumError:
            raise AssertionError("an unsealed container raised a checksum error")
        except DecodeError:
            unsealed_ok = False
        with pytest.raises(DecodeError) as e:
            container.decode_device(sp, h1.container_len, bptr, n, header=h1)
        if unsealed_ok:
            assert e.type is ChecksumError, (pos, str(e.value))
            assert f"error {_lib.ERR_CHECKSUM}" in str(e.value) and "checksum" in str(e.value)
        outcomes["checksum" if e.type is ChecksumError else "format"] += 1
        plain[at + pos] ^= 0x10
        sealed[at + pos] ^= 0x10
    print(f"{algo} {kind}: {outcomes}")
    if algo != "chameleon":                                             # (Chameleon's index validation may fire first)
        assert outcomes["format"] == 0
    # the undamaged containers still decode
    host(sealed, 0, 1)
    assert container.decode_device(sp, h1.container_len, bptr, n, header=h1) == n and np.array_equal(host(back), data)


@pytest.mark.parametrize("algo", ALGOS)
def test_trailer_damage(algo):
    import torch
    n = 4 * CHUNK
    data = datagen.by_kind("prose", n, seed=3)
    src, sptr = to_device(data)
    sealed, sp, cap, h0, before, h1 = sealed_on_device(algo, "packed", sptr, n, CHUNK)
    t = h1.container_len - trailer_bytes(4)
    # one flipped bit in trailer entry 2
    sealed[t + 4 * 2 + 1] ^= 0x04
    host(sealed, 0, 1)
    out = Region(n + 100, 0)
    got = container.chunk_checksums(host(sealed)[:h1.container_len])
    assert [a == b for a, b in zip(got, chunk_sums(data, CHUNK))] == [True, True, False, True]
    with pytest.raises(ChecksumError):
        container.decode_device(sp, h1.container_len, out.ptr, n + 100, header=h1)
    out.check("decode of a container with a damaged trailer")
    # asynchronous: nothing is reported, exactly like format errors
    assert container.decode_device(sp, h1.container_len, out.ptr, n + 100, header=h1, sync=False) is None
    torch.cuda.synchronize()
    sealed[t + 4 * 2 + 1] ^= 0x04
    host(sealed, 0, 1)
    # container_size cut by 16: the header's container_len does not fit — a format error, and nothing is written
    fresh = Region(n + 100, 0)
    for header in (h1, None):
        with pytest.raises(DecodeError) as e:
            container.decode_device(sp, h1.container_len - 16, fresh.ptr, n + 100, header=header)
        assert e.type is DecodeError and f"error {_lib.ERR_FORMAT}" in str(e.value)
        fresh.untouched("decode of a sealed container cut by 16")
    # a size table that reaches into the trailer is a format error too: the trailer is not payload
    blob = host(sealed)[:h1.container_len].copy()
    last = int.from_bytes(blob[32 + 12:36 + 12].tobytes(), "little")
    grown = last + (h1.container_len - h0.container_len)
    sealed[32 + 12:32 + 16] = torch.from_numpy(np.frombuffer(grown.to_bytes(4, "little"), dtype=np.uint8).copy()).cuda()
    host(sealed, 0, 1)
    with pytest.raises(DecodeError) as e:
        container.decode_device(sp, h1.container_len, fresh.ptr, n + 100, header=h1)
    assert e.type is DecodeError
    fresh.check("decode with a size table that reaches into the trailer")


# ------------------------------------------------------------------------------------------------------------------------------------------
# 5. host pointers
# ------------------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture
def variant():
    yield lambda v: container.set_kernel_variant(v | SESSION_VARIANT)
    container.set_kernel_variant(SESSION_VARIANT)


@pytest.mark.parametrize("algo", ALGOS)
def test_host_pointers(algo, variant):
    n, chunk = 600_000, CHUNK
    data = datagen.by_kind("prose", n, seed=31)
    src, sptr = to_device(data)
    out, optr, cap, h0, before, h1 = sealed_on_device(algo, "packed", sptr, n, chunk)
    want = host(out)[:h1.container_len].copy()
    bound = container.container_bound(algo, n, chunk) + container.seal_overhead(n, chunk)
    for kv in ((0, 256, 512) if algo == "chameleon" else (0,)):
        variant(kv)
        buf = np.zeros(bound, dtype=np.uint8)
        m = container.encode_sealed(algo, data, buf, chunk)
        assert m == want.size and np.array_equal(buf[:m], want), kv
        assert container.decoded_size(buf[:m]) == n
        back = np.zeros(n + 100, dtype=np.uint8)
        assert container.decode(buf[:m], back) == n and np.array_equal(back[:n], data) and not back[n:].any(), kv
        with pytest.raises(EncodeError):
            container.encode_sealed(algo, data, np.zeros(m - 1, dtype=np.uint8), chunk)
        # a damaged trailer, and a payload byte the reference decodes to wrong bytes
        bad = buf[:m].copy()
        bad[m - trailer_bytes(h1.n_chunks) + 4] ^= 0x80
        with pytest.raises(ChecksumError):
            container.decode(bad, back)
        assert "checksum" in _lib.last_error()
        stream = container.chunk_payloads(want)[1][VICTIM]
        part = data[VICTIM * chunk:(VICTIM + 1) * chunk]
        pos = silently_wrong(algo, stream, part)[0]
        bad = buf[:m].copy()
        bad[payload_offset(want, VICTIM) + pos] ^= 0x10
        with pytest.raises(DecodeError) as e:
            container.decode(bad, back)
        if algo != "chameleon":
            assert e.type is ChecksumError and "checksum" in _lib.last_error()
    # the unsealed host call is what it was
    variant(0)
    plain = np.zeros(bound, dtype=np.uint8)
    k = container.encode(algo, data, plain, chunk)
    assert k == h0.container_len and np.array_equal(plain[:k], before[:k]) and container.chunk_checksums(plain[:k]) is None


# ------------------------------------------------------------------------------------------------------------------------------------------
# 6. DHCM: sealed blobs travel whole
# ------------------------------------------------------------------------------------------------------------------------------------------
def test_sealed_blobs_in_a_multi_rank_container():
    import torch
    algo, chunk = "chameleon", CHUNK
    parts = [datagen.by_kind("prose", 4 * CHUNK, seed=3), datagen.by_kind("mixed", 3 * CHUNK + 123, seed=4)]
    blobs = []
    for d in parts:
        src, sptr = to_device(d)
        out, optr, cap, h0, before, h1 = sealed_on_device(algo, "packed", sptr, d.size, chunk)
        blobs.append(host(out)[:h1.container_len].copy())
    front, rows, total = parallel.multi_layout([b.size for b in blobs], [d.size for d in parts], 0, chunk)
    whole = np.zeros(total, dtype=np.uint8)
    whole[:len(front)] = np.frombuffer(front, dtype=np.uint8)
    for b, (off, ln, _) in zip(blobs, rows):
        whole[off:off + ln] = b
    dev = torch.from_numpy(whole).cuda()
    out = torch.zeros(sum(d.size for d in parts), dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    assert parallel.decode_multi_device(dev, out) == out.numel()
    assert np.array_equal(host(out), np.concatenate(parts))
    stream = container.chunk_payloads(blobs[0])[1][VICTIM]
    pos = silently_wrong(algo, stream, parts[0][VICTIM * CHUNK:(VICTIM + 1) * CHUNK])[0]
    dev[rows[0][0] + payload_offset(blobs[0], VICTIM) + pos] ^= 0x10
    torch.cuda.synchronize()
    with pytest.raises(DecodeError):
        parallel.decode_multi_device(dev, out)
