"""Buffer contracts of the device and host entry points (include/density_hip.h): pointers at any offset, capacities exactly at the documented
bounds and one byte below, caller workspaces of exactly the documented size with garbage in them.

Every buffer is a region `front guard | payload | back guard` (Region / HostRegion below): the guards hold a fixed non-zero pattern, the payload
poison (never zeros), the library gets `base + offset`, and after the call both guards must be unchanged — a write in front of the pointer or past
the capacity lands in a guard (the back guard is at least what a wrong kernel could write past the capacity plus 64 KiB), not outside the
allocation.  Decode outputs keep their poison in [decoded length, capacity): the reference writes only what it decodes.

The library picks kernels by alignment (rotor_encode.hip / rotor_decode.hip: rotor_encode_eligible / rotor_decode_eligible, chameleon.hip: the 16-wave pipelines,
exchange_stages.hip: stage_encode_eligible, decode_passes.hip: decode_pass_eligible, api.hip: the paged decoder, api_stream.hip: the segmented
stream encode), so the offsets below put each call on both sides of each gate; 4, 8 and 12 pass every `% 4` gate at addresses that are not
16-byte aligned.  Where a counter says which path served a call (density_hip_decode_pass_count, density_hip_stage_stats under variant 64,
density_hip_stream_stats), the tests assert that the misaligned case took the fallback and the aligned one did not.

A library call with a NULL stream runs on the library's own stream, not torch's: buffers filled with torch are synchronised first."""
import ctypes
import os

import numpy as np
import pytest

import datagen
from density_amd import BY_NAME, _lib, container
from density_amd.codec import DecodeError
from oracle import pyoracle

pytestmark = pytest.mark.gpu

FRONT = 4096                      # front guard in front of the largest offset
BACK = 64 << 10                   # back guard beyond what a call may write
PAIRS = [(0, 0), (1, 0), (0, 1), (2, 2), (3, 5), (4, 12), (8, 4), (12, 3)]      # (data offset, container / stream offset)
KINDS = ["prose", "mixed", "zeros", "random"]
CONTAINER_CASES = [("chameleon", (4 << 20) + 4321, 1 << 20), ("chameleon", (4 << 20) + 4321, 64 << 10),
                   ("cheetah", (2 << 20) + 777, 256 << 10), ("lion", (2 << 20) + 777, 256 << 10)]
STREAM_SIZES = {"chameleon": (5 << 20) + 3, "cheetah": 300_001, "lion": 300_001}
SESSION_VARIANT = int(os.environ.get("DENSITY_TEST_VARIANT", "0") or 0)
COUNTERS = SESSION_VARIANT == 0    # the path counters describe the default kernel family


def L():
    return _lib.lib()


def guard_pattern(n, salt):
    """Fixed, non-zero, position-dependent: a shifted copy of it does not match itself."""
    i = np.arange(n, dtype=np.uint32)
    return (((i * 37 + salt) ^ (i >> 8)) % 255 + 1).astype(np.uint8)


def poison(n, seed=0xA5):
    return np.random.default_rng(seed).integers(0, 256, size=n, dtype=np.uint8) | np.uint8(1)   # (never a zero byte)


class Region:
    """A device buffer `front guard | payload | back guard`; `ptr` is the payload's address (FRONT + offset into the allocation)."""

    def __init__(self, size, offset=0, fill=None, back=BACK, seed=0xA5):
        import torch
        self.size, self.offset, self.lead = size, offset, FRONT + offset
        self.host = np.concatenate([guard_pattern(self.lead, 11), poison(size, seed) if fill is None else np.asarray(fill, dtype=np.uint8),
                                    guard_pattern(back, 29)])
        assert self.host.size == self.lead + size + back
        self.buf = torch.from_numpy(self.host).cuda()
        torch.cuda.synchronize()
        self.ptr = self.buf.data_ptr() + self.lead

    def payload(self, n=None):
        return self.buf[self.lead:self.lead + (self.size if n is None else n)].cpu().numpy()

    def check(self, what=""):
        got = self.buf.cpu().numpy()
        assert np.array_equal(got[:self.lead], self.host[:self.lead]), f"{what}: bytes in front of the pointer written"
        assert np.array_equal(got[self.lead + self.size:], self.host[self.lead + self.size:]), f"{what}: bytes past the capacity written"
        return got[self.lead:self.lead + self.size]

    def untouched(self, what=""):
        assert np.array_equal(self.check(what), self.host[self.lead:self.lead + self.size]), f"{what}: output written by a failing call"

    def repoison(self, seed):
        import torch
        self.host[self.lead:self.lead + self.size] = poison(self.size, seed)
        self.buf.copy_(torch.from_numpy(self.host))
        torch.cuda.synchronize()


class HostRegion:
    """The same on the host: a numpy slice `buf[lead:lead + size]` of a larger guarded array."""

    def __init__(self, size, offset, fill=None, back=BACK, seed=0x5A):
        self.size, self.lead = size, FRONT + offset
        self.base = np.concatenate([guard_pattern(self.lead, 13), poison(size, seed) if fill is None else np.asarray(fill, dtype=np.uint8),
                                    guard_pattern(back, 31)])
        self.expect = self.base.copy()
        self.view = self.base[self.lead:self.lead + size]
        assert self.view.__array_interface__["data"][0] % 16 == (self.base.__array_interface__["data"][0] + self.lead) % 16

    def check(self, what=""):
        assert np.array_equal(self.base[:self.lead], self.expect[:self.lead]), f"{what}: bytes in front of the slice written"
        assert np.array_equal(self.base[self.lead + self.size:], self.expect[self.lead + self.size:]), f"{what}: bytes past the slice written"
        return self.view

    def untouched(self, what=""):
        assert np.array_equal(self.check(what), self.expect[self.lead:self.lead + self.size]), f"{what}: output written by a failing call"


# ---- raw calls: the return code itself, not just "it raised" ----
ENCODERS = {"packed": ("density_hip_encode_device", container.container_bound), "slotted": ("density_hip_encode_device_slotted", container.container_bound_slotted),
            "paged": ("density_hip_encode_device_paged", container.container_bound_paged)}


def encode_rc(form, algo, d_in, n, d_out, cap, chunk, ws=(0, 0), stream=0):
    hdr = _lib.Header()
    rc = getattr(L(), ENCODERS[form][0])(_lib.ALGO_IDS[algo], d_in, n, d_out, cap, chunk, ws[0], ws[1], stream, ctypes.byref(hdr))
    return rc, hdr


def decode_rc(d_cont, size, d_out, cap, ws=(0, 0), stream=0):
    got = ctypes.c_size_t(0)
    rc = L().density_hip_decode_device(d_cont, size, None, d_out, cap, ws[0], ws[1], stream, ctypes.byref(got))
    return rc, got.value


def pack_rc(d_cont, size, d_out, cap):
    hdr = _lib.Header()
    rc = L().density_hip_pack_device(d_cont, size, None, d_out, cap, 0, 0, 0, ctypes.byref(hdr))
    return rc, hdr


def stream_rc(op, algo, d_in, n, d_out, cap):
    got = ctypes.c_size_t(0)
    rc = getattr(L(), f"density_hip_stream_{op}_device")(_lib.ALGO_IDS[algo], d_in, n, d_out, cap, 0, ctypes.byref(got))
    return rc, got.value


def stage_stats():
    a = (ctypes.c_uint64 * 2)()
    L().density_hip_stage_stats(a)
    return list(a)


def stream_stats():
    a = (ctypes.c_uint64 * 4)()
    L().density_hip_stream_stats(a)
    return list(a)


@pytest.fixture
def variant():
    """set_kernel_variant for one test; the session's variant afterwards."""
    def set_(v):
        container.set_kernel_variant(v | SESSION_VARIANT)
    yield set_
    container.set_kernel_variant(SESSION_VARIANT)


def _data(kind, n, seed=3):
    return datagen.by_kind(kind, n, seed=seed)


def _chunk_streams(algo, data, chunk):
    return [pyoracle.encode(algo, data[i:i + chunk]) for i in range(0, data.size, chunk)]


def _paged_layout_ok(algo, n, chunk, d_in_offset):
    """api.hip::run_encode_container: the paged form needs what it is for (Chameleon, chunks of 1 MiB .. 4 MiB, two and more) and a 4-byte aligned input."""
    return algo == "chameleon" and chunk >= (1 << 20) and n > chunk and d_in_offset % 4 == 0 and not (SESSION_VARIANT & 5)


# ------------------------------------------------------------------------------------------------------------------------------------------
# c. the reference's nine symbols and the host container calls on numpy slices at odd offsets
# ------------------------------------------------------------------------------------------------------------------------------------------
HOST_SIZES = {"chameleon": (2 << 20) + 5, "cheetah": 300_001, "lion": 300_001}


@pytest.mark.parametrize("off", [3, 12])
def test_long_host_stream_pipelined_on_slices(off, variant):
    """One Chameleon stream above the pipelining threshold (api_stream.hip::kPipeMinStream, 32 MiB) encoded with output_size = the safe size (the
    pipelined encode: below it the staged path is taken) and decoded with 100 bytes to spare, both on numpy slices at an odd offset; the same
    under variant 512 (never pipelined)."""
    n = (33 << 20) + 7
    data = datagen.rep_text(n, period=1_000_003, seed=61)
    want = np.frombuffer(pyoracle.encode("chameleon", data), dtype=np.uint8)
    safe = L().chameleon_safe_encode_buffer_size(n)
    addr = lambda r: r.view.__array_interface__["data"][0]
    for kv in (0, 512):
        variant(kv)
        src = HostRegion(n, off, fill=data)
        out = HostRegion(safe, 16 - off)
        got = L().chameleon_encode(addr(src), n, addr(out), safe)
        assert got == want.size and np.array_equal(out.check("long encode")[:got], want), kv
        src.check("long encode input")
        back = HostRegion(n + 100, off)
        assert L().chameleon_decode(addr(out), got, addr(back), n + 100) == n
        res = back.check("long decode")
        assert np.array_equal(res[:n], data) and np.array_equal(res[n:], back.expect[back.lead + n:back.lead + n + 100]), kv


@pytest.mark.parametrize("kv", [0, 256, 512])
def test_host_chameleon_containers_on_slices(kv, variant):
    """Chameleon, whose host container calls pipeline (under variant 256 at any size): see _host_containers."""
    _host_containers("chameleon", (4 << 20) + 4321, 64 << 10, kv, variant)


@pytest.mark.parametrize("algo", ["cheetah", "lion"])
@pytest.mark.parametrize("kv", [0, 512])
def test_host_containers_on_slices(algo, kv, variant):
    """Cheetah and Lion (staged: host buffers of a MiB and more, which the library pins in place for the copy): see _host_containers."""
    _host_containers(algo, (3 << 20) + 777, 256 << 10, kv, variant)


def _host_containers(algo, n, chunk, kv, variant):
    """container.encode / decode / decoded_size on numpy slices at offsets 1, 3, 4 and 12 under kernel variants 0, 256 (pipelined whatever the
    size: the caller's unaligned ranges pinned in place) and 512 (never pipelined): the container is the aligned call's, the decode the input
    with the 100 bytes behind it untouched; an output one byte short of the container's total_len is an error."""
    variant(kv)
    data = _data("prose", n, seed=51)
    bound = container.container_bound(algo, n, chunk)
    ref = np.zeros(bound, dtype=np.uint8)
    m = container.encode(algo, data, ref, chunk)
    assert container.chunk_payloads(ref[:m])[1] == _chunk_streams(algo, data, chunk)
    for off in (1, 3, 4, 12):
        src = HostRegion(n, off, fill=data)
        out = HostRegion(bound, 16 - off)
        assert container.encode(algo, src.view, out.view, chunk) == m
        assert np.array_equal(out.check("encode")[:m], ref[:m]), off
        blob = HostRegion(m, off, fill=ref[:m])
        assert container.decoded_size(blob.view) == n
        back = HostRegion(n + 100, (off * 7) % 16)
        assert container.decode(blob.view, back.view) == n
        res = back.check("decode")
        assert np.array_equal(res[:n], data) and np.array_equal(res[n:], back.expect[back.lead + n:back.lead + n + 100]), off
        short = HostRegion(n - 1, off)
        with pytest.raises(DecodeError):
            container.decode(blob.view, short.view)
        short.untouched("decode at total_len - 1")
        blob.check("decode input")


@pytest.mark.parametrize("algo", ["chameleon", "cheetah", "lion"])
def test_reference_symbols_on_host_slices(algo, variant):
    """{algo}_encode with output_size = the oracle's exact length (succeeds: host_stream_codec in api_stream.hip checks what was produced), that length - 1 (0, the
    buffer untouched) and the safe size; {algo}_decode with n - 1 (0), n and n + 100 (n, the 100 bytes behind untouched) — input and output
    numpy slices at offsets 1, 3, 4 and 12 of guarded arrays."""
    for kv in (0, 512):
        variant(kv)
        _reference_symbols(algo)


def _reference_symbols(algo):
    n = HOST_SIZES[algo]
    data = _data("mixed", n, seed=41)
    want = np.frombuffer(pyoracle.encode(algo, data), dtype=np.uint8)
    codec = BY_NAME[algo]
    safe = codec.safe_encode_buffer_size(n)
    enc, dec = getattr(L(), f"{algo}_encode"), getattr(L(), f"{algo}_decode")
    addr = lambda r: r.view.__array_interface__["data"][0]
    for off in (1, 3, 4, 12):
        src = HostRegion(n, off, fill=data)
        for size in (want.size, want.size - 1, safe):
            out = HostRegion(size, (off * 5) % 16)
            got = enc(addr(src), n, addr(out), size)
            where = f"{algo}_encode +{off}, output_size {size}"
            if size < want.size:
                assert got == 0, where
                out.untouched(where)
            else:
                assert got == want.size and np.array_equal(out.check(where)[:got], want), where
            src.check(where)
        stream = HostRegion(want.size, off, fill=want)
        for size in (n - 1, n, n + 100):
            back = HostRegion(size, (off * 3) % 16)
            got = dec(addr(stream), want.size, addr(back), size)
            where = f"{algo}_decode +{off}, output_size {size}"
            if size < n:
                assert got == 0, where
                back.check(where)
            else:
                res = back.check(where)
                assert got == n and np.array_equal(res[:n], data), where
                assert np.array_equal(res[n:], back.expect[back.lead + n:back.lead + size]), f"{where}: bytes behind the stream's length written"


# ------------------------------------------------------------------------------------------------------------------------------------------
# a. misaligned device pointers: containers
# ------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("algo,n,chunk", CONTAINER_CASES)
def test_misaligned_device_containers(algo, n, chunk, kind, variant):
    """encode_device / _slotted / _paged, pack_device and decode_device with the data and the container at the offsets of PAIRS: every packed and
    slotted container is byte for byte the aligned call's, every paged one holds the oracle's chunk streams (and is paged exactly when its input is
    4-byte aligned), every decode is the input with the poison behind it intact, no guard is touched."""
    if algo != "chameleon" and COUNTERS:
        variant(64)                                                   # stage_stats: the chunks the exchange passes take
    data = _data(kind, n)
    want = _chunk_streams(algo, data, chunk)
    n_chunks = len(want)
    ref = {}
    for form in ("packed", "slotted"):
        src = Region(n, 0, fill=data)
        cap = ENCODERS[form][1](algo, n, chunk)
        out = Region(cap, 0)
        rc, hdr = encode_rc(form, algo, src.ptr, n, out.ptr, cap, chunk)
        assert rc == _lib.OK, (form, rc, _lib.last_error())
        ref[form] = out.check(form)[:hdr.container_len].copy()
        _, payloads = container.chunk_payloads(ref[form])
        assert payloads == want, f"aligned {form} container is not the oracle's streams"
    for io, oo in PAIRS:
        src = Region(n, io, fill=data)
        for form in ("packed", "slotted", "paged"):
            cap = ENCODERS[form][1](algo, n, chunk)
            out = Region(cap, oo)
            s0 = stage_stats()
            rc, hdr = encode_rc(form, algo, src.ptr, n, out.ptr, cap, chunk)
            s1 = stage_stats()
            where = f"{form} encode, data +{io}, container +{oo}"
            assert rc == _lib.OK, (where, rc, _lib.last_error())
            blob = out.check(where)[:hdr.container_len].copy()
            if algo != "chameleon" and COUNTERS:
                taken = s1[0] - s0[0]
                assert taken == (n_chunks if io % 4 == 0 else 0), (where, "exchange passes", taken)      # exchange_stages.hip: d_in % 4
            if form == "paged":
                paged = bool(hdr.flags & container.FLAG_PAGED)
                assert paged == _paged_layout_ok(algo, n, chunk, io), (where, hdr.flags)            # settle_form in api.hip: a misaligned input comes out slotted
                if not paged:
                    assert hdr.flags & container.FLAG_SLOTTED and np.array_equal(blob, ref["slotted"]), where
                _, payloads = container.chunk_payloads(blob)
                assert payloads == want, where
            else:
                assert np.array_equal(blob, ref[form]), f"{where}: not the aligned call's container"
            # decode in place (the container at +oo: index, payloads and page base misaligned with it) to an output at +io
            back = Region(n + 100, io, seed=7)
            c0 = L().density_hip_decode_pass_count()
            rc, got = decode_rc(out.ptr, hdr.container_len, back.ptr, n + 100)
            c1 = L().density_hip_decode_pass_count()
            where = f"decode of the {form} container at +{oo} to +{io}"
            if form == "paged" and hdr.flags & container.FLAG_PAGED:
                pages_base = _pages_base(blob)
                if io % 4 or (oo + pages_base) % 4 or (oo + _index_at(hdr)) % 4:             # run_decode_container in api.hip: the paged decoder reads pages in place, 4-byte aligned
                    assert rc == _lib.ERR_UNSUPPORTED, (where, rc)
                    back.untouched(where)
                    continue
            assert rc == _lib.OK and got == n, (where, rc, got, _lib.last_error())
            res = back.check(where)
            assert np.array_equal(res[:n], data), where
            assert np.array_equal(res[n:], back.host[back.lead + n:back.lead + n + 100]), f"{where}: [decoded length, capacity) written"
            if algo == "cheetah" and COUNTERS:
                assert c1 - c0 == (1 if io % 4 == 0 and oo % 2 == 0 else 0), (where, "decode passes", c1 - c0)   # decode_pass_eligible: d_out % 4, d_in % 2
            if form == "slotted" and hdr.flags & container.FLAG_SLOTTED:
                # pack the slotted container at +oo into an output at +io: the aligned packed container
                pcap = container.container_bound(algo, n, chunk)
                packed = Region(pcap, io, seed=9)
                rc, phdr = pack_rc(out.ptr, hdr.container_len, packed.ptr, pcap)
                assert rc == _lib.OK, (f"pack +{oo} -> +{io}", rc, _lib.last_error())
                assert np.array_equal(packed.check("pack")[:phdr.container_len], ref["packed"]), f"pack +{oo} -> +{io}"


def _index_at(hdr):
    return (32 + 4 * hdr.n_chunks + 15) // 16 * 16


def _pages_base(blob):
    h = container.parse_header(blob)
    off = (_index_at(h) + (h.total_len + 255) // 256 + 15) // 16 * 16
    ppc = int(L().density_hip_paged_pages_per_chunk(h.chunk_size))
    return (off + 16 * (ppc + 1) * h.n_chunks + 255) // 256 * 256


@pytest.mark.parametrize("io,oo", [(16, 0), (4, 4), (12, 8), (3, 1)])
def test_misaligned_chameleon_pipelines(io, oo, variant):
    """Kernel variant 4 (the 16-wave role pipelines, chameleon.hip:1300 / 1330): their encoder takes 16-byte aligned inputs only, their decoder
    16-byte aligned containers and 4-byte aligned outputs; everything else goes to the one-wavefront kernels.  Same containers either way."""
    n, chunk = (1 << 20) + 4321, 64 << 10
    data = _data("mixed", n, seed=8)
    want = _chunk_streams("chameleon", data, chunk)
    variant(4)
    cap = container.container_bound("chameleon", n, chunk)
    src, out = Region(n, io, fill=data), Region(cap, oo)
    rc, hdr = encode_rc("packed", "chameleon", src.ptr, n, out.ptr, cap, chunk)
    assert rc == _lib.OK
    blob = out.check("encode")[:hdr.container_len]
    assert container.chunk_payloads(blob)[1] == want
    back = Region(n + 100, io, seed=4)
    rc, got = decode_rc(out.ptr, hdr.container_len, back.ptr, n + 100)
    assert rc == _lib.OK and got == n
    res = back.check("decode")
    assert np.array_equal(res[:n], data) and np.array_equal(res[n:], back.host[back.lead + n:back.lead + n + 100])


# ------------------------------------------------------------------------------------------------------------------------------------------
# a. misaligned device pointers: single reference streams
# ------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("algo", ["chameleon", "cheetah", "lion"])
def test_misaligned_device_streams(algo, kind):
    """stream_encode_device / stream_decode_device at the offsets of PAIRS: the oracle's stream, the input back, poison and guards intact.
    Chameleon's segmented encode takes 4-byte aligned inputs only (run_stream_encode in api_stream.hip), its segmented decode 4-byte aligned outputs; Cheetah's
    decode passes 4-byte aligned outputs."""
    n = STREAM_SIZES[algo]
    data = _data(kind, n, seed=5)
    want = np.frombuffer(pyoracle.encode(algo, data), dtype=np.uint8)
    safe = BY_NAME[algo].safe_encode_buffer_size(n)
    for io, oo in PAIRS:
        src, out = Region(n, io, fill=data), Region(safe, oo)
        st0 = stream_stats()
        rc, m = stream_rc("encode", algo, src.ptr, n, out.ptr, safe)
        st1 = stream_stats()
        where = f"stream encode +{io} -> +{oo}"
        assert rc == _lib.OK and m == want.size, (where, rc, m, _lib.last_error())
        assert np.array_equal(out.check(where)[:m], want), where
        if algo == "chameleon" and COUNTERS:
            assert st1[0] - st0[0] == (1 if io % 4 == 0 else 0), (where, "segmented encodes", st1[0] - st0[0])
        back = Region(n + 100, io, seed=6)
        c0, st0 = L().density_hip_decode_pass_count(), stream_stats()
        rc, got = stream_rc("decode", algo, out.ptr, m, back.ptr, n + 100)
        c1, st1 = L().density_hip_decode_pass_count(), stream_stats()
        where = f"stream decode +{oo} -> +{io}"
        assert rc == _lib.OK and got == n, (where, rc, got, _lib.last_error())
        res = back.check(where)
        assert np.array_equal(res[:n], data), where
        assert np.array_equal(res[n:], back.host[back.lead + n:back.lead + n + 100]), f"{where}: [decoded length, capacity) written"
        if COUNTERS and algo == "cheetah":
            assert c1 - c0 == (1 if io % 4 == 0 and oo % 2 == 0 else 0), (where, "decode passes")
        if COUNTERS and algo == "chameleon" and kind == "prose":                     # (a calm stream: what the segmented decode is for)
            assert (st1[2] - st0[2], st1[3] - st0[3]) == ((1, 0) if io % 4 == 0 else (0, 1)), (where, "segmented / sequential decodes")
    # the stream itself at the offsets 1, 2, 4, 12 (decode from a file buffer at any offset), the output aligned
    for so in (1, 2, 4, 12):
        s = Region(want.size, so, fill=want)
        back = Region(n, 0, seed=so)
        rc, got = stream_rc("decode", algo, s.ptr, want.size, back.ptr, n)
        assert rc == _lib.OK and got == n and np.array_equal(back.check(f"stream at +{so}"), data), so


# ------------------------------------------------------------------------------------------------------------------------------------------
# b. exact capacities
# ------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("algo,n,chunk", [CONTAINER_CASES[0], CONTAINER_CASES[2], CONTAINER_CASES[3]])
def test_exact_container_capacities(algo, n, chunk):
    """At exactly the bound every device container call succeeds; one byte below it returns ERR_CAPACITY with the output (header included) and
    the guards untouched."""
    data = _data("prose", n, seed=12)
    src = Region(n, 0, fill=data)
    made = {}
    for form in ("packed", "slotted", "paged"):
        bound = ENCODERS[form][1](algo, n, chunk)
        out = Region(bound - 1, 0)
        rc, _ = encode_rc(form, algo, src.ptr, n, out.ptr, bound - 1, chunk)
        assert rc == _lib.ERR_CAPACITY, (form, rc)
        out.untouched(f"{form} encode at bound - 1")
        out = Region(bound, 0)
        rc, hdr = encode_rc(form, algo, src.ptr, n, out.ptr, bound, chunk)
        assert rc == _lib.OK, (form, rc, _lib.last_error())
        out.check(f"{form} encode at the bound")
        made[form] = (out, hdr)
    out, hdr = made["slotted"]
    if hdr.flags & container.FLAG_SLOTTED:
        bound = container.container_bound(algo, n, chunk)
        short = Region(bound - 1, 0)
        assert pack_rc(out.ptr, hdr.container_len, short.ptr, bound - 1)[0] == _lib.ERR_CAPACITY
        short.untouched("pack at bound - 1")
        exact = Region(bound, 0)
        rc, phdr = pack_rc(out.ptr, hdr.container_len, exact.ptr, bound)
        assert rc == _lib.OK
        assert np.array_equal(exact.check("pack at the bound")[:phdr.container_len], made["packed"][0].payload(phdr.container_len))
    for form, (out, hdr) in made.items():
        short = Region(n - 1, 0)
        assert decode_rc(out.ptr, hdr.container_len, short.ptr, n - 1)[0] == _lib.ERR_CAPACITY, form
        short.untouched(f"decode of {form} at total_len - 1")
        exact = Region(n, 0)
        assert decode_rc(out.ptr, hdr.container_len, exact.ptr, n) == (_lib.OK, n), form
        assert np.array_equal(exact.check(f"decode of {form} at total_len"), data)


@pytest.mark.parametrize("algo", ["chameleon", "cheetah", "lion"])
def test_exact_stream_capacities(algo):
    """stream_encode_device: safe_encode_buffer_size succeeds, one byte less is ERR_CAPACITY with nothing written.  stream_decode_device: n
    succeeds; n - 1, n - 256 and n // 2 are errors that write nothing at or past the capacity (Chameleon: the segmented decode; Cheetah: the
    decode passes; Lion: the one-wave decoder)."""
    n = STREAM_SIZES[algo]
    data = _data("prose", n, seed=13)
    want = np.frombuffer(pyoracle.encode(algo, data), dtype=np.uint8)
    safe = BY_NAME[algo].safe_encode_buffer_size(n)
    src = Region(n, 0, fill=data)
    short = Region(safe - 1, 0)
    assert stream_rc("encode", algo, src.ptr, n, short.ptr, safe - 1)[0] == _lib.ERR_CAPACITY
    short.untouched("stream encode at safe - 1")
    out = Region(safe, 0)
    rc, m = stream_rc("encode", algo, src.ptr, n, out.ptr, safe)
    assert rc == _lib.OK and np.array_equal(out.check("stream encode at safe")[:m], want)
    for cap in (n - 1, n - 256, n // 2):
        back = Region(cap, 0, back=n - cap + BACK, seed=cap & 0xff)
        c0 = L().density_hip_decode_pass_count()
        rc, got = stream_rc("decode", algo, out.ptr, m, back.ptr, cap)
        assert rc != _lib.OK, (cap, got)
        back.check(f"stream decode at capacity {cap}")
        if algo == "cheetah" and COUNTERS and cap == n - 1:
            assert L().density_hip_decode_pass_count() == c0 + 1, "the decode passes were to see the short capacity"
    exact = Region(n, 0, seed=3)
    assert stream_rc("decode", algo, out.ptr, m, exact.ptr, n) == (_lib.OK, n)
    assert np.array_equal(exact.check("stream decode at n"), data)


# ------------------------------------------------------------------------------------------------------------------------------------------
# d. caller workspaces
# ------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("algo,n,chunk", [CONTAINER_CASES[1], CONTAINER_CASES[2], CONTAINER_CASES[3]])
def test_exact_dirty_workspaces(algo, n, chunk):
    """A workspace of exactly density_hip_encode_workspace_size / density_hip_decode_workspace_size_for bytes, poisoned before the first call and
    guarded behind, serves two calls back to back (the second on the first one's leftovers); one byte less is ERR_CAPACITY (a Cheetah decode
    instead leaves the decode passes to the one-wave decoder: DecodePlan::pass in api_internal.hpp)."""
    data = _data("mixed", n, seed=21)
    want = _chunk_streams(algo, data, chunk)
    src = Region(n, 0, fill=data)
    ews = int(L().density_hip_encode_workspace_size(_lib.ALGO_IDS[algo], n, chunk))
    dws = int(L().density_hip_decode_workspace_size_for(_lib.ALGO_IDS[algo], n, chunk))
    cap = container.container_bound_slotted(algo, n, chunk)
    small = Region(ews - 1, 0)
    out = Region(cap, 0)
    assert encode_rc("slotted", algo, src.ptr, n, out.ptr, cap, chunk, ws=(small.ptr, ews - 1))[0] == _lib.ERR_CAPACITY
    out.untouched("encode with workspace - 1")
    ws = Region(ews, 0, seed=0xEE)
    blobs = []
    for form in ("slotted", "packed", "packed"):
        out = Region(container.container_bound_slotted(algo, n, chunk), 0, seed=len(blobs))
        rc, hdr = encode_rc(form, algo, src.ptr, n, out.ptr, out.size, chunk, ws=(ws.ptr, ews))
        assert rc == _lib.OK, (form, rc, _lib.last_error())
        ws.check("encode workspace")
        blob = out.check(form)[:hdr.container_len].copy()
        assert container.chunk_payloads(blob)[1] == want, form
        blobs.append((out, hdr))
    dw = Region(dws, 0, seed=0xDD)
    for k, (out, hdr) in enumerate(blobs):
        if k == 1:
            dw.repoison(0xDC)
        back = Region(n, 0, seed=k)
        c0 = L().density_hip_decode_pass_count()
        assert decode_rc(out.ptr, hdr.container_len, back.ptr, n, ws=(dw.ptr, dws)) == (_lib.OK, n)
        dw.check("decode workspace")
        assert np.array_equal(back.check("decode"), data)
        if COUNTERS:
            assert L().density_hip_decode_pass_count() - c0 == (1 if algo == "cheetah" else 0)
    out, hdr = blobs[1]
    less = Region(dws - 1, 0, seed=0xCC)
    back = Region(n, 0)
    c0 = L().density_hip_decode_pass_count()
    rc, got = decode_rc(out.ptr, hdr.container_len, back.ptr, n, ws=(less.ptr, dws - 1))
    if algo == "cheetah":
        assert (rc, got) == (_lib.OK, n) and np.array_equal(back.check("decode, workspace - 1"), data)
        assert L().density_hip_decode_pass_count() == c0, "a workspace below decode_workspace_size_for: no decode passes"
        bare = int(L().density_hip_decode_workspace_size(hdr.n_chunks))
        mini = Region(bare, 0, seed=0xBB)
        back = Region(n, 0, seed=1)
        assert decode_rc(out.ptr, hdr.container_len, back.ptr, n, ws=(mini.ptr, bare)) == (_lib.OK, n)
        mini.check("decode_workspace_size workspace")
        assert np.array_equal(back.check("decode on decode_workspace_size"), data)
        # the passes whenever the workspace also holds their scratch (DecodePlan::pass in api_internal.hpp): decode_workspace_size() is sized for Lion's tables,
        # which for a few chunks exceeds what Cheetah's passes need
        assert L().density_hip_decode_pass_count() - c0 == (1 if bare >= dws else 0), (bare, dws)
        # chunks of 1 MiB: there decode_workspace_size() cannot hold the passes' scratch, and the one-wave decoder serves the call
        cap1 = container.container_bound(algo, n, 1 << 20)
        out1 = Region(cap1, 0, seed=0x11)
        rc, h1 = encode_rc("packed", algo, src.ptr, n, out1.ptr, cap1, 1 << 20)
        assert rc == _lib.OK
        bare1 = int(L().density_hip_decode_workspace_size(h1.n_chunks))
        assert bare1 < int(L().density_hip_decode_workspace_size_for(_lib.ALGO_IDS[algo], n, 1 << 20))
        mini1, back1 = Region(bare1, 0, seed=0xBA), Region(n, 0, seed=2)
        c0 = L().density_hip_decode_pass_count()
        assert decode_rc(out1.ptr, h1.container_len, back1.ptr, n, ws=(mini1.ptr, bare1)) == (_lib.OK, n)
        mini1.check("decode_workspace_size workspace, 1 MiB chunks")
        assert np.array_equal(back1.check("decode on decode_workspace_size, 1 MiB chunks"), data)
        assert L().density_hip_decode_pass_count() == c0, "the one-wave fallback (include/density_hip.h) was to serve it"
    else:
        assert rc == _lib.ERR_CAPACITY, rc
        back.untouched("decode, workspace - 1")
    less.check("workspace - 1")


@pytest.mark.parametrize("algo,n,chunk", [CONTAINER_CASES[0], CONTAINER_CASES[2], CONTAINER_CASES[3]])
def test_two_async_calls_with_own_workspaces(algo, n, chunk):
    """Two asynchronous encodes (no header: nothing synchronises) on two torch streams, each with its own workspace and output, enqueued before
    either is waited for; then two asynchronous decodes likewise.  Only the NULL-workspace path forbids the overlap (include/density_hip.h)."""
    import torch
    datas = [_data("prose", n, seed=31), _data("mixed", n, seed=32)]
    ews = int(L().density_hip_encode_workspace_size(_lib.ALGO_IDS[algo], n, chunk))
    dws = int(L().density_hip_decode_workspace_size_for(_lib.ALGO_IDS[algo], n, chunk))
    cap = container.container_bound(algo, n, chunk)
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    srcs = [Region(n, 4 * k, fill=d) for k, d in enumerate(datas)]
    outs = [Region(cap, 8 * k, seed=k) for k in range(2)]
    wss = [Region(ews, 0, seed=0x40 + k) for k in range(2)]
    for k in range(2):
        assert container.encode_device(algo, srcs[k].ptr, n, outs[k].ptr, cap, chunk, stream=streams[k].cuda_stream, workspace=(wss[k].ptr, ews), want_header=False) is None
    for s in streams:
        s.synchronize()
    hdrs = []
    for k in range(2):
        blob = outs[k].check("async encode")
        hdr = container.parse_header(blob)
        hdrs.append(hdr)
        assert container.chunk_payloads(blob[:hdr.container_len])[1] == _chunk_streams(algo, datas[k], chunk), k
        wss[k].check("async encode workspace")
    dwss = [Region(dws, 0, seed=0x50 + k) for k in range(2)]
    backs = [Region(n, 4 - 4 * k, seed=0x60 + k) for k in range(2)]
    for k in range(2):
        container.decode_device(outs[k].ptr, hdrs[k].container_len, backs[k].ptr, n, header=hdrs[k], stream=streams[k].cuda_stream,
                                workspace=(dwss[k].ptr, dws), sync=False)
    for s in streams:
        s.synchronize()
    for k in range(2):
        assert np.array_equal(backs[k].check("async decode"), datas[k]), k
        dwss[k].check("async decode workspace")
