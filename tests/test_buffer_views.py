"""The Python bindings hand the library one address and one length per buffer (density_amd/codec.py: _ro / _rw).  Those two describe a buffer
only if it is C-contiguous: a strided view's first `nbytes` bytes are not its elements, and a reversed view's address is its LAST element, so
the library would write `nbytes` bytes past the end of the base array.  Such views are refused with TypeError before any library call (no GPU
needed); contiguous slices at any offset are accepted, at their own address."""
import numpy as np
import pytest

from density_amd import BY_NAME, container
from density_amd.codec import _ro, _rw


def _base():
    return np.arange(4096, dtype=np.uint8)


def _bad_views():
    a = _base()
    return {"step2": a[::2], "reversed": a[::-1], "fortran2d": np.asfortranarray(a.reshape(64, 64)),
            "columns": a.reshape(64, 64)[:, :32], "memoryview_step2": memoryview(a)[::2]}


BAD = sorted(_bad_views())


def _good():
    return _base()[3:3 + 1024]


@pytest.mark.parametrize("algo", sorted(BY_NAME))
@pytest.mark.parametrize("view", BAD)
@pytest.mark.parametrize("side", ["input", "output"])
@pytest.mark.parametrize("op", ["encode", "decode"])
def test_codec_refuses_non_contiguous_buffers(algo, view, side, op):
    bad = _bad_views()[view]
    args = (bad, np.zeros(8192, dtype=np.uint8)) if side == "input" else (_good(), bad)
    with pytest.raises(TypeError, match="C-contiguous"):
        getattr(BY_NAME[algo], op)(*args)


@pytest.mark.parametrize("view", BAD)
@pytest.mark.parametrize("side", ["input", "output"])
def test_container_encode_refuses_non_contiguous_buffers(view, side):
    bad = _bad_views()[view]
    args = (bad, np.zeros(16384, dtype=np.uint8)) if side == "input" else (_good(), bad)
    with pytest.raises(TypeError, match="C-contiguous"):
        container.encode("chameleon", *args)


@pytest.mark.parametrize("view", BAD)
@pytest.mark.parametrize("side", ["input", "output"])
def test_container_decode_refuses_non_contiguous_buffers(view, side):
    bad = _bad_views()[view]
    args = (bad, np.zeros(16384, dtype=np.uint8)) if side == "input" else (_good(), bad)
    with pytest.raises(TypeError, match="C-contiguous"):
        container.decode(*args)


@pytest.mark.parametrize("view", BAD)
def test_container_decoded_size_refuses_non_contiguous_buffers(view):
    with pytest.raises(TypeError, match="C-contiguous"):
        container.decoded_size(_bad_views()[view])


def test_read_only_output_is_still_refused():
    a = _base()
    a.flags.writeable = False
    with pytest.raises(TypeError, match="read-only"):
        _rw(a)
    with pytest.raises(TypeError, match="read-only"):
        _rw(b"abc")


@pytest.mark.parametrize("offset", [1, 3, 4, 12])
def test_contiguous_slices_at_odd_offsets_are_accepted_at_their_own_address(offset):
    a = _base()
    base = a.__array_interface__["data"][0]
    for view in (a[offset:], a[offset:offset + 100], a.reshape(64, 64)[1:][:, :].reshape(-1)[offset:]):
        want = view.__array_interface__["data"][0]
        assert _ro(view)[:2] == (want, view.nbytes)
        assert _rw(view)[:2] == (want, view.nbytes)
    assert _ro(a[offset:])[0] == base + offset
    # 2-D C-ordered row blocks, one-element strides of size-1 axes, other item sizes: one run of bytes each
    rows = a.reshape(64, 64)[offset:offset + 4]
    assert _ro(rows)[:2] == (base + 64 * offset, 256)
    col = a[offset:offset + 64].reshape(64, 1)
    assert _ro(col)[:2] == (base + offset, 64)
    words = a.view(np.uint32)[offset:]
    assert _rw(words)[:2] == (base + 4 * offset, words.nbytes)
    # the buffer protocol: bytes (copied: read-only), bytearray and memoryview slices (in place)
    assert _ro(b"x" * (offset + 5))[1] == offset + 5
    ba = bytearray(64)
    assert _rw(memoryview(ba)[offset:])[1] == 64 - offset
    assert _ro(memoryview(a)[offset:])[1] == a.nbytes - offset
