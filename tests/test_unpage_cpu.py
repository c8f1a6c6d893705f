"""container.unpage: a paged container to the packed wire form on the HOST — the CPU reader's tool and the executable statement of what
density_hip_unpage_device writes (tests/test_gpu_unpage.py holds the device call against it).  Every expectation here comes from the oracle's chunk streams
laid out by the header's rules (tests/unpage_cases.py), with the pages in chunk order and shuffled."""
import numpy as np
import pytest

import unpage_cases as uc
from density_amd import container


@pytest.mark.parametrize("name,shuffled", uc.ORDERS)
def test_unpage_is_the_packed_container_of_the_oracles_streams(name, shuffled):
    blob = uc.paged(name, shuffled)
    got = container.unpage(blob)
    want = uc.packed(name)
    assert got.dtype == np.uint8 and got.size == want.size
    assert np.array_equal(got, want), int(np.flatnonzero(got != want)[0])
    hdr, streams = container.chunk_payloads(got)
    assert hdr.flags == container.FLAG_BLOCK_INDEX and hdr.container_len == got.size
    assert tuple(streams) == uc.streams(name)
    assert np.array_equal(container.unpage(bytes(blob)), want)                     # bytes in, the same array out


@pytest.mark.parametrize("name,shuffled", [("a", False), ("a", True), ("d", False), ("g", False)])
def test_a_sealed_paged_container_keeps_its_trailer(name, shuffled):
    got = container.unpage(uc.sealed(uc.paged(name, shuffled), name))
    want = uc.sealed(uc.packed(name), name)
    assert np.array_equal(got, want)
    hdr = container.parse_header(got[:32].tobytes())
    assert hdr.flags == container.FLAG_BLOCK_INDEX | container.FLAG_CHECKSUM and hdr.container_len == got.size
    assert container.chunk_checksums(got) == container.chunk_checksums(want)


@pytest.mark.parametrize("what", list(uc.format_mutations()))
def test_a_directory_that_cannot_be_followed_raises(what):
    with pytest.raises(ValueError):
        container.unpage(uc.format_mutations()[what])


def test_what_is_not_a_paged_container_raises():
    with pytest.raises(ValueError):
        container.unpage(uc.packed("a"))
    with pytest.raises(ValueError):
        container.unpage(b"\0" * 16)
    cut = uc.paged("a")[:-1]                                                        # shorter than its container_len
    with pytest.raises(ValueError):
        container.unpage(cut)
