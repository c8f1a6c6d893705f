"""Verdicts and salvage, what can be checked without a device: the two calls and two constants as the header, the Python binding and the Rust shim declare
them, the exception's new attribute, the multi-rank reader's refusal of a wrong `out`, and the condition tests/test_gpu_verdicts.py rests on — the
candidate positions hold a flip that the reference decodes silently, for Cheetah and Lion, on the very inputs that test uses."""
import os
import re

import numpy as np
import pytest

import verdict_cases as vc
from density_amd import ChecksumError, DecodeError, _lib, parallel

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CALLS = ["density_hip_decode_device_verdicts", "density_hip_decode_verdicts"]
CONSTANTS = {"DENSITY_HIP_CHUNK_DAMAGED": 1, "DENSITY_HIP_SALVAGE_BLANK": 1}


def test_header_binding_and_rust_shim_declare_the_same():
    header = open(os.path.join(ROOT, "include", "density_hip.h")).read()
    rust = open(os.path.join(ROOT, "bindings", "rust", "src", "lib.rs")).read()
    for name in CALLS:
        assert re.search(r"^(int|size_t) %s\(" % name, header, flags=re.M), name
        assert re.search(r"pub fn %s\(" % name, rust), name
        assert name in _lib.SYMBOLS and hasattr(_lib.lib(), name)
    for name, value in CONSTANTS.items():
        assert re.search(r"^#define %s %du\b" % (name, value), header, flags=re.M), name
        assert re.search(r"pub const %s: u32 = %d;" % (name, value), rust), name
    assert (_lib.CHUNK_DAMAGED, _lib.SALVAGE_BLANK) == (1, 1)
    # argument for argument: the header's parameter list against the shim's
    for name in CALLS:
        c_args = re.search(r"%s\(([^;]*)\);" % name, re.sub(r"/\*.*?\*/", "", header, flags=re.S)).group(1).split(",")
        rust_args = re.search(r"pub fn %s\(([^;]*)\) ->" % name, rust, flags=re.S).group(1).split(",")
        assert [a.split()[-1].lstrip("*") for a in c_args] == [a.split(":")[0].strip() for a in rust_args], name
        assert len(c_args) == len(_lib.SYMBOLS[name][1])


def test_checksum_error_names_its_chunks():
    assert ChecksumError().damaged_chunks == ()
    e = ChecksumError("checksum mismatch", damaged_chunks=[3, 5])
    assert e.damaged_chunks == (3, 5) and str(e) == "checksum mismatch" and isinstance(e, DecodeError)


def test_multi_rank_reader_refuses_a_wrong_out():
    """before it touches a device: host tensors reach the check"""
    import torch
    front, rows, total = parallel.multi_layout([64, 96], [1000, 500], 0, 65536)
    blob = torch.zeros(total, dtype=torch.uint8)
    blob[:len(front)] = torch.frombuffer(bytearray(front), dtype=torch.uint8)
    for wrong in (torch.zeros(1499, dtype=torch.uint8), torch.zeros(1500, dtype=torch.int8), torch.zeros(3000, dtype=torch.uint8)[::2]):
        for salvage in (False, True):
            with pytest.raises(ValueError):
                parallel.decode_multi_device(blob, wrong, salvage=salvage)


@pytest.mark.parametrize("kind", vc.KINDS)
@pytest.mark.parametrize("algo", ["cheetah", "lion"])
def test_candidates_hold_a_silent_flip(algo, kind):
    n, chunk = vc.SHAPES[(algo, "packed")]
    assert vc.SHAPES[(algo, "slotted")] == (n, chunk)
    for k in vc.victims(algo, "packed"):
        pos, found = vc.silent_position(algo, kind, n, chunk, k)
        print(f"{algo} {kind} chunk {k}: {found} of {vc.CANDIDATES} candidates decode silently wrong in the reference")
        assert found >= 1 and pos is not None


@pytest.mark.parametrize("kind", vc.KINDS)
def test_chameleon_position_is_a_plain_quad(kind):
    """the flip leaves the record structure alone: the reference decodes the damaged stream to the full length, and only quads of that chunk differ"""
    from oracle import pyoracle
    for form in ("paged", "packed"):
        n, chunk = vc.SHAPES[("chameleon", form)]
        for k in vc.victims("chameleon", form):
            pos, found = vc.silent_position("chameleon", kind, n, chunk, k)
            part = vc._input(kind, n)[k * chunk:(k + 1) * chunk]
            stream = bytearray(pyoracle.encode("chameleon", part))
            assert found == 1 and 8 <= pos < len(stream)
            stream[pos] ^= vc.FLIP
            out = np.frombuffer(pyoracle.decode("chameleon", bytes(stream), part.size), dtype=np.uint8)
            assert out.size == part.size and not np.array_equal(out, part)
