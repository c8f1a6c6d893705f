"""density_hip_unpage_device: a PAGED container to the packed wire form on the device.  The expected bytes come from the CPU — the oracle's chunk streams
in paged containers built by tests/paged_cpu.py and brought to the packed form by container.unpage (itself held to the oracle in tests/test_unpage_cpu.py) —
and, for containers the GPU wrote, from density_hip_encode_device (held to the oracle in tests/test_gpu_chameleon.py and others)."""
import ctypes

import numpy as np
import pytest

import datagen
import unpage_cases as uc

pytestmark = pytest.mark.gpu

FILL, GUARD = 0xA5, 256


def _stream():
    """The stream argument of a library call: its own stream (0), once everything torch has queued for the call's buffers is through — a null stream
    argument is the library's own non-blocking stream, which is not ordered behind torch's fills and copies."""
    import torch
    torch.cuda.synchronize()
    return 0


def _bound(blob):
    """The capacity the call asks for, from the blob's own header."""
    from density_amd import container
    h = container.parse_header(bytes(blob[:32]))
    cap = container.container_bound("chameleon", h.total_len, h.chunk_size)
    return cap + (container.seal_overhead(h.total_len, h.chunk_size) if h.flags & container.FLAG_CHECKSUM else 0)


def _buffers(blob, in_off=0, out_off=0, cap=None):
    """The blob on the device at byte offset in_off of its allocation; an output of `cap` bytes at byte offset out_off, pre-filled, GUARD bytes behind it."""
    import torch
    cap = _bound(blob) if cap is None else cap
    d = torch.zeros(in_off + blob.size, dtype=torch.uint8, device="cuda")
    d[in_off:] = torch.from_numpy(np.array(blob)).cuda()
    out = torch.full((out_off + cap + GUARD,), FILL, dtype=torch.uint8, device="cuda")
    return d, out, cap


def _unpage(blob, in_off=0, out_off=0):
    """(header, the whole output allocation from out_off on as numpy, capacity) of one synchronous call on torch's stream"""
    from density_amd import container
    d, out, cap = _buffers(blob, in_off, out_off)
    hdr = container.unpage_device(d.data_ptr() + in_off, blob.size, out.data_ptr() + out_off, cap, stream=_stream())
    return hdr, out.cpu().numpy()[out_off:], cap


def _rc(blob, cap=None):
    """(return code, output allocation as numpy, capacity) of the raw call with a header_out"""
    import torch
    from density_amd import _lib
    d, out, cap = _buffers(blob, cap=cap)
    hdr = _lib.Header()
    rc = _lib.lib().density_hip_unpage_device(d.data_ptr(), blob.size, None, out.data_ptr(), cap, 0, 0, _stream(), ctypes.byref(hdr))
    torch.cuda.synchronize()
    return rc, out.cpu().numpy(), cap


def _check_output(got, hdr, want, cap):
    assert hdr.container_len == want.size
    assert bytes(hdr) == want[:32].tobytes()
    assert np.array_equal(got[:want.size], want), int(np.flatnonzero(got[:want.size] != want)[0])
    assert (got[want.size:] == FILL).all(), "bytes at and beyond container_len keep the fill, the guards behind the capacity too"
    assert got.size == cap + GUARD


@pytest.mark.parametrize("name,shuffled", uc.ORDERS)
def test_cpu_built_paged_containers_unpage_to_the_packed_form(name, shuffled):
    import torch
    from density_amd import container
    blob = uc.paged(name, shuffled)
    want = container.unpage(blob)
    hdr, got, cap = _unpage(blob)
    _check_output(got, hdr, want, cap)
    # ... and the result is a container like any other: it decodes to the input
    n = uc.data(name).size
    d = torch.from_numpy(got[:want.size].copy()).cuda()
    back = torch.zeros(n, dtype=torch.uint8, device="cuda")
    assert container.decode_device(d.data_ptr(), want.size, back.data_ptr(), n, stream=_stream()) == n
    assert np.array_equal(back.cpu().numpy(), uc.data(name))


@pytest.mark.parametrize("name,shuffled", [("a", True), ("b", False), ("g", False)])
def test_sealed_cpu_built_paged_containers_keep_their_trailer(name, shuffled):
    from density_amd import container
    blob = uc.sealed(uc.paged(name, shuffled), name)
    want = container.unpage(blob)
    assert np.array_equal(want, uc.sealed(uc.packed(name), name))
    hdr, got, cap = _unpage(blob)
    assert hdr.flags == container.FLAG_BLOCK_INDEX | container.FLAG_CHECKSUM
    _check_output(got, hdr, want, cap)


@pytest.mark.parametrize("in_off,out_off", [(1, 0), (0, 1), (3, 5), (12, 3)])
def test_both_buffers_at_any_byte_alignment(in_off, out_off):
    from density_amd import container
    blob = uc.paged("a")
    hdr, got, cap = _unpage(blob, in_off, out_off)
    _check_output(got, hdr, container.unpage(blob), cap)


def _gpu_input(kind):
    if kind == "rep-text":
        return datagen.rep_text(8 << 20), 1 << 20
    return datagen.by_kind("mixed", (6 << 20) + 12345, seed=11), 1 << 20


def _encode(fn, x, n, chunk, seal):
    """A container of device tensor x by encode call `fn`, sealed behind it or not: (tensor cut to container_len, header)"""
    import torch
    from density_amd import container
    bound = container.container_bound_paged if fn is container.encode_device_paged else container.container_bound
    cap = bound("chameleon", n, chunk) + container.seal_overhead(n, chunk)
    cont = torch.zeros(cap, dtype=torch.uint8, device="cuda")
    hdr = fn("chameleon", x.data_ptr(), n, cont.data_ptr(), cap, chunk, stream=_stream())
    if seal:
        hdr = container.seal_device(x.data_ptr(), n, cont.data_ptr(), cap, header=hdr, stream=_stream())
    return cont[:hdr.container_len], hdr


@pytest.mark.parametrize("seal", [False, True])
@pytest.mark.parametrize("kind", ["rep-text", "mixed"])
def test_gpu_written_paged_containers_unpage_to_what_encode_device_writes(kind, seal):
    import torch
    from density_amd import container
    host, chunk = _gpu_input(kind)
    n = host.size
    x = torch.from_numpy(host).cuda()
    packed, hp = _encode(container.encode_device, x, n, chunk, seal)
    want = packed.cpu().numpy()
    results = []
    for _ in range(2):                                                              # two separate paged encodes: their page order is their own
        paged, h = _encode(container.encode_device_paged, x, n, chunk, seal)
        assert h.flags & container.FLAG_PAGED and bool(h.flags & container.FLAG_CHECKSUM) == seal
        cap = container.container_bound("chameleon", n, chunk) + (container.seal_overhead(n, chunk) if seal else 0)
        out = torch.full((cap + GUARD,), FILL, dtype=torch.uint8, device="cuda")
        hdr = container.unpage_device(paged.data_ptr(), h.container_len, out.data_ptr(), cap, header=h, stream=_stream())
        got = out.cpu().numpy()
        _check_output(got, hdr, want, cap)
        assert bytes(hdr) == bytes(hp)
        results.append(got)
    assert np.array_equal(results[0], results[1]), "the packed form is deterministic, whatever order the pages were taken in"
    back = torch.zeros(n, dtype=torch.uint8, device="cuda")
    d = torch.from_numpy(results[0][:want.size].copy()).cuda()
    assert container.decode_device(d.data_ptr(), want.size, back.data_ptr(), n, stream=_stream()) == n     # (sealed: the decode verifies the trailer)
    assert torch.equal(back, x)


def test_asynchronous_form_on_a_callers_stream_and_workspace():
    import torch
    from density_amd import _lib, container
    blob = uc.paged("a", True)
    want = container.unpage(blob)
    d, out, cap = _buffers(blob)
    h = container.parse_header(bytes(blob[:32]))
    ws_size = int(_lib.lib().density_hip_decode_workspace_size(h.n_chunks))
    ws = torch.empty(ws_size, dtype=torch.uint8, device="cuda")
    s = torch.cuda.Stream()
    torch.cuda.synchronize()                                                        # (the buffers were filled on torch's current stream)
    container.set_profiling(True)
    try:
        container.last_timings()
        assert container.unpage_device(d.data_ptr(), blob.size, out.data_ptr(), cap, header=h, stream=s.cuda_stream, workspace=(ws.data_ptr(), ws_size),
                                       want_header=False) is None
        s.synchronize()
        names = [name for name, _ in container.last_timings()]
    finally:
        container.set_profiling(False)
    assert "unpage" in names and "layout_encode" in names and "move_trailer" not in names
    got = out.cpu().numpy()
    _check_output(got, container.parse_header(got[:32].tobytes()), want, cap)


def test_packed_and_slotted_containers_are_refused_with_nothing_written():
    import torch
    from density_amd import _lib, container
    rc, got, cap = _rc(uc.packed("a"))
    assert rc == _lib.ERR_ARGUMENT and (got == FILL).all()
    host = datagen.by_kind("mixed", 3 * 65536 + 77, seed=7)
    x = torch.from_numpy(host).cuda()
    scap = container.container_bound_slotted("chameleon", host.size, 65536)
    cont = torch.zeros(scap, dtype=torch.uint8, device="cuda")
    hs = container.encode_device_slotted("chameleon", x.data_ptr(), host.size, cont.data_ptr(), scap, 65536, stream=_stream())
    assert hs.flags & container.FLAG_SLOTTED
    rc, got, cap = _rc(cont[:hs.container_len].cpu().numpy())
    assert rc == _lib.ERR_ARGUMENT and (got == FILL).all()


def test_a_capacity_below_the_bound_is_refused_on_the_host():
    from density_amd import _lib
    for blob in (uc.paged("a"), uc.sealed(uc.paged("a"), "a")):
        rc, got, cap = _rc(blob, cap=_bound(blob) - 1)
        assert rc == _lib.ERR_CAPACITY and (got == FILL).all()
        rc, got, cap = _rc(blob)
        assert rc == _lib.OK


@pytest.mark.parametrize("what", list(uc.format_mutations()))
def test_a_directory_the_call_cannot_follow_is_a_format_error(what):
    """An answer, not a crash: the directory check refuses it before anything reads through the directory, and no chunk's payload is written."""
    from density_amd import _lib
    blob = uc.format_mutations()[what]
    _, n, chunk, _ = uc.CASES["a"]
    payload_at = uc.geometry(n, chunk)[3]                                           # (the packed payloads start where the paged directory does)
    rc, got, cap = _rc(blob)
    assert rc == _lib.ERR_FORMAT, (rc, _lib.last_error())
    assert (got[payload_at:] == FILL).all()
    rc, got, cap = _rc(uc.paged("a"))                                               # (the library is fine afterwards)
    assert rc == _lib.OK
