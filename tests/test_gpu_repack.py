"""density_hip_pack_device and density_hip_unpage_device are the whole-window slice: the three calls run one driver (run_slice_container in api.hip), so
their outputs are held to each other byte for byte — header, every byte below container_len, nothing behind it — and to what does not go through that
driver: density_hip_encode_device (+ density_hip_seal_device) of the input for the library's own containers, the models of tests/slice_cpu.py and
tests/unpage_cases.py for the CPU-built ones.  Outputs are pre-filled so that stale bytes cannot pass.

A library call with a NULL stream runs on the library's own stream, not torch's: buffers filled with torch are synchronised first."""
import ctypes

import numpy as np
import pytest

import slice_cpu
import test_gpu_slice as ts
import unpage_cases as uc
import verdict_cases as vc
from density_amd import _lib, container

pytestmark = pytest.mark.gpu

FILL, GUARD = ts.FILL, ts.GUARD


def _call(blob):
    """the call that brings this container to the packed form whole"""
    paged = container.parse_header(bytes(blob[:32])).flags & container.FLAG_PAGED
    return container.unpage_device if paged else container.pack_device


def _repack(blob, header=True):
    """(header, the output allocation as numpy, capacity) of one synchronous pack_device / unpage_device at the capacity the call asks for"""
    h = container.parse_header(bytes(blob[:32]))
    cap = container.slice_bound(h, 0, h.n_chunks)                                  # == container_bound() (+ seal_overhead()): the whole window's bound
    d, out = ts._buffers(blob, cap=cap)
    hdr = _call(blob)(d.data_ptr(), blob.size, out.data_ptr(), cap, header=h if header else None, stream=ts._stream())
    return hdr, out.cpu().numpy(), cap


def _same_as_the_whole_slice(blob, want):
    """pack / unpage of `blob` == slice_device(blob, 0, n_chunks) == `want`: headers, bytes up to container_len, the fill behind it"""
    n = container.parse_header(bytes(blob[:32])).n_chunks
    hdr, got, cap = _repack(blob)
    ts._check_output(got, hdr, want, cap)
    hdr_s, got_s, cap_s = ts._slice(blob, 0, n)
    assert cap_s == cap and bytes(hdr_s) == bytes(hdr)
    assert np.array_equal(got_s, got), "the same bytes, and the same fill behind them"
    return hdr


@pytest.mark.parametrize("seal", [False, True])
@pytest.mark.parametrize("algo,form", list(vc.SHAPES))
def test_the_librarys_own_containers_repack_to_the_whole_slice_and_to_what_encode_device_writes(algo, form, seal):
    data, chunk, sealed_blob, plain = ts._own(algo, form)
    blob = sealed_blob if seal else plain
    made = ts._encoded(algo, data, chunk, seal)
    hdr = _same_as_the_whole_slice(blob, made)
    assert hdr.flags & ~container.FLAG_BLOCK_INDEX == (container.FLAG_CHECKSUM if seal else 0)
    assert np.array_equal(slice_cpu.slice_container(blob, 0, hdr.n_chunks), made)


@pytest.mark.parametrize("name,form,seal", ts.CPU_SOURCES)
def test_cpu_built_containers_repack_to_the_whole_slice_and_to_the_models_bytes(name, form, seal):
    blob = ts._cpu_blob(name, form, seal)
    want = uc.sealed(uc.packed(name), name) if seal else uc.packed(name)
    hdr = _same_as_the_whole_slice(blob, want)
    assert hdr.flags == container.FLAG_BLOCK_INDEX | (container.FLAG_CHECKSUM if seal else 0)
    assert np.array_equal(slice_cpu.slice_container(blob, 0, hdr.n_chunks), want)


def test_the_header_may_be_read_back_from_the_device():
    for algo, form in [("lion", "slotted"), ("chameleon", "paged")]:
        data, chunk, blob, _ = ts._own(algo, form)
        hdr, got, cap = _repack(blob, header=False)
        ts._check_output(got, hdr, ts._encoded(algo, data, chunk, True), cap)


def test_a_container_of_no_chunks_packs_to_its_header():
    """the window [0, 0): no part for the driver, the front matter alone"""
    h0 = _lib.Header(0x31434844, 0, 1, 0, 65536, 0, 0, 32)                         # the container of an empty input: its header
    blob = np.frombuffer(bytes(h0), dtype=np.uint8)
    cap = container.container_bound("chameleon", 0, 65536)
    assert cap >= 32
    d, out = ts._buffers(blob, cap=cap)
    hdr = container.pack_device(d.data_ptr(), blob.size, out.data_ptr(), cap, stream=ts._stream())
    ts._check_output(out.cpu().numpy(), hdr, blob, cap)


def test_pack_of_a_packed_container_refuses_a_size_table_entry_above_its_chunks_worst_case():
    """The layout kernel of the windows judges every entry of the window, so the whole-window pack of a PACKED source does too.  The mutation is that of
    test_gpu_slice.py::test_size_table_faults_of_packed_and_slotted_windows (its smaller value), once on the container as it is — the streams behind the
    entry then run past its end — and once on the container with room behind its last stream, so that every stream the table describes stays inside
    container_len: the one case in which the call, before it shared the slice's driver, copied the entry along.  No container of the library has one."""
    import torch
    _, _, _, packed = ts._own("cheetah", "packed")
    h = container.parse_header(packed)
    base, k, value = ts._payload_at(packed, 0, h.n_chunks), 3, slice_cpu.safe_size(1, h.chunk_size) + 1
    assert uc.get32(packed, 32 + 4 * k) < value
    bad = packed.copy()
    uc.put32(bad, 32 + 4 * k, value)
    roomy = np.concatenate([bad, np.zeros(slice_cpu.up(value, 16), dtype=np.uint8)])
    uc.put32(roomy, 24, roomy.size)                                                 # container_len (its low word)
    assert container.parse_header(roomy).container_len == roomy.size
    cap = container.slice_bound(h, 0, h.n_chunks)
    for blob in (bad, roomy):
        hb = container.parse_header(blob)
        for want_header, rc_want in ((True, _lib.ERR_FORMAT), (False, _lib.OK)):   # (without header_out the call does not wait for the device's verdict)
            d, out = ts._buffers(blob, cap=cap)
            hdr = _lib.Header()
            rc = _lib.lib().density_hip_pack_device(d.data_ptr(), blob.size, ctypes.byref(hb), out.data_ptr(), cap, 0, 0, ts._stream(), ctypes.byref(hdr) if want_header else None)
            torch.cuda.synchronize()
            assert rc == rc_want, (rc, _lib.last_error())
            assert (out.cpu().numpy()[base:] == FILL).all(), "no payload byte is written"


def test_profiling_marks_of_a_sealed_pack_and_a_sealed_unpage():
    import torch
    for (algo, form), marks in ((("cheetah", "slotted"), ["layout_encode", "compact", "move_trailer"]), (("chameleon", "paged"), ["layout_encode", "unpage", "move_trailer"])):
        data, chunk, blob, _ = ts._own(algo, form)
        h = container.parse_header(blob)
        cap = container.slice_bound(h, 0, h.n_chunks)
        d, out = ts._buffers(blob, cap=cap)
        torch.cuda.synchronize()
        container.set_profiling(True)
        try:
            container.last_timings()
            _call(blob)(d.data_ptr(), blob.size, out.data_ptr(), cap, header=h, stream=ts._stream())
            names = [name for name, _ in container.last_timings()]
        finally:
            container.set_profiling(False)
        assert names == marks
        got = out.cpu().numpy()
        ts._check_output(got, container.parse_header(got[:32].tobytes()), ts._encoded(algo, data, chunk, True), cap)
