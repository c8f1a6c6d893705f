"""Lion's decoders (density_amd/csrc/serial_codec.hip: lion_decode_pair — a parser wave and a table wave per stream, a ring of steps in LDS between
them, a repair walk where a predicted quad read a row that an earlier quad of the same step has since moved —, lion_decode_wave, kernel variant
32768, and one lane per stream, variant 16) against the oracle, the way tests/test_gpu_decode_passes.py holds Cheetah's: containers ASSEMBLED ON
THE CPU from oracle streams, so nothing the GPU encoder does can mask a decoder fault, on inputs built for the decoder's own structures
(tests/datagen.py LION_KINDS: Markov chains whose prediction rows keep moving, dictionary slots whose two entries keep swapping, copy mode
switching at every record of a step; tests/test_lion_inputs.py holds them to the oracle's flag histogram on the CPU).  On valid input the three
decoders return the input; on anything else they agree with each other outcome for outcome, and with the oracle wherever it decodes all bytes."""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

import datagen
from density_amd import DecodeError, Lion, container
from oracle import pyoracle
from test_gpu_decode_passes import cpu_container
from test_lion_inputs import GPU_KINDS, lion_blocks

pytestmark = pytest.mark.gpu
ALGO = "lion"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DECODERS = {"pair": 0, "wave": 32768, "lane": 16}
NEW_KINDS = list(datagen.LION_KINDS)
KINDS = NEW_KINDS + ["prose", "mixed", "random", "zeros", "binaryish"]
assert KINDS == GPU_KINDS                                                                 # the kinds whose histogram the CPU test holds to the floor


@functools.lru_cache(maxsize=None)
def _big(kind):
    d = datagen.by_kind(kind, (2 << 20) + 77, seed=23)
    d.setflags(write=False)
    return d


def make(kind, n):
    """The first n bytes of one 2 MiB input per kind (stretches: made for n, so that its random tail is this input's tail)."""
    if kind == "stretches":
        return datagen.stretches(n, 23, body=_markov_body())
    return _big(kind)[:n].copy()


@functools.lru_cache(maxsize=None)
def _markov_body():
    d = datagen.markov((2 << 20) + 77, 23, 64, 5)
    d.setflags(write=False)
    return d


def on_three(fn):
    """fn() on the three decoders -> its outcome, ('ok', value) or ('error',); the three must agree."""
    res = {}
    try:
        for name, variant in DECODERS.items():
            container.set_kernel_variant(variant)
            try:
                res[name] = ("ok", fn())
            except DecodeError:
                res[name] = ("error",)
    finally:
        container.set_kernel_variant(0)
    same = res["pair"] == res["wave"] == res["lane"]
    assert same, {k: (v[0], len(v[1]) if len(v) > 1 else 0, _first_difference(v, res["lane"])) for k, v in res.items()}
    return res["pair"]


def _first_difference(a, b):
    if len(a) < 2 or len(b) < 2:
        return None
    x, y = np.frombuffer(a[1], dtype=np.uint8), np.frombuffer(b[1], dtype=np.uint8)
    m = min(x.size, y.size)
    d = np.flatnonzero(x[:m] != y[:m])
    return int(d[0]) if d.size else (None if x.size == y.size else m)


def decode_container(raw, n, extra=0):
    def run():
        out = np.zeros(max(n + extra, 1), dtype=np.uint8)
        m = container.decode(raw, out)
        return out[:m].tobytes()
    return run


def decode_stream(enc, cap):
    enc = np.frombuffer(bytes(enc), dtype=np.uint8)

    def run():
        out = np.zeros(max(cap, 1), dtype=np.uint8)
        m = Lion.decode(enc, out)
        return out[:m].tobytes()
    return run


def shipped_chunk():
    """the chunk size the library picks for Lion at the flagship size (100 MB)"""
    from density_amd import _lib
    c = int(_lib.lib().density_hip_auto_chunk_for(_lib.ALGO_IDS[ALGO], 100_000_000))
    assert c >= 65536 and c % 4096 == 0
    return c


def expect_input(res, data, what):
    assert res[0] == "ok", (what, "a valid stream came back as an error")
    ok = res[1] == data.tobytes()
    assert ok, (what, len(res[1]), data.size, _first_difference(res, ("ok", data.tobytes())))


@pytest.mark.parametrize("kind", KINDS)
def test_cpu_built_containers(kind):
    """Packed DHC1 containers from oracle streams, chunks of 4 KiB, 64 KiB, the shipped chunk and 1 MiB, each with a ragged last chunk."""
    auto = shipped_chunk()
    for n, chunk in [(24 * 4096 + 77, 4096), (6 * 65536 + 1234, 65536), (5 * auto + 4321, auto), (2 * (1 << 20) + 77, 1 << 20)]:
        data = make(kind, n)
        raw, streams = cpu_container(data, chunk, ALGO, 2)
        assert len(streams) == -(-n // chunk) and n % chunk
        expect_input(on_three(decode_container(raw, n)), data, (kind, n, chunk))


SLOTS_SCRIPT = r'''
import os, sys
sys.path.insert(0, os.environ["ROOT"]); sys.path.insert(0, os.path.join(os.environ["ROOT"], "tests"))
from density_amd import _lib
_lib.use_debug_build()
import test_gpu_lion_decode as t
kind, n, chunk = sys.argv[1], int(sys.argv[2]), int(sys.argv[3])
data = t.make(kind, n)
raw, streams = t.cpu_container(data, chunk, t.ALGO, 2)
for rep in range(2):
    t.expect_input(t.on_three(t.decode_container(raw, n)), data, (kind, n, chunk, rep))
print("ok", len(streams))
'''


@pytest.mark.parametrize("kind,n,chunk,slots", [("markov16", 1_500_000, 65536, 3), ("weave", 1_500_000, 65536, 3), ("stretches", 700_001, 32768, 2), ("pools24", 1_000_000, 131072, 1)])
def test_cpu_built_containers_with_more_chunks_than_table_slots(kind, n, chunk, slots):
    """A work-group takes its chunks one after the other and clears its tables in between (tests/test_gpu_few_slots.py: the debug build's
    DENSITY_HIP_SERIAL_SLOTS, in a process of its own): rows and slots that the chunk before left full."""
    env = dict(os.environ, DENSITY_HIP_SERIAL_SLOTS=str(slots), ROOT=ROOT)
    r = subprocess.run([sys.executable, "-c", SLOTS_SCRIPT, kind, str(n), str(chunk)], env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and r.stdout.strip().endswith("ok %d" % -(-n // chunk)), (r.stdout[-2000:], r.stderr[-3000:])


@pytest.mark.parametrize("kind", KINDS)
def test_one_reference_stream(kind):
    """`lion_decode` (the reference's symbol: ONE stream, host pointers) and the device-pointer form, 1.5 MB per kind; an output buffer of exactly
    the data's size, and a larger one."""
    import torch
    n = 1_500_003
    data = make(kind, n)
    enc = pyoracle.encode(ALGO, data)
    expect_input(on_three(decode_stream(enc, n)), data, (kind, "host"))
    x = torch.from_numpy(np.frombuffer(enc, dtype=np.uint8).copy()).cuda()

    def device():
        out = torch.zeros(n + 100_000, dtype=torch.uint8, device="cuda")
        m = container.stream_decode_device(ALGO, x.data_ptr(), x.numel(), out.data_ptr(), out.numel())
        assert not bool(out[m:].any()), "bytes written behind the data"
        return out[:m].cpu().numpy().tobytes()
    expect_input(on_three(device), data, (kind, "device, larger buffer"))


def test_a_long_copy_run_is_no_false_alarm():
    """One MiB of incompressible bytes inside Markov data: the table wave has nothing to do for thousands of records while the parser copies, and
    the pair decoder's spin watchdog (error bit 16) must not take that wait for a hang."""
    n = 1_700_000
    data = datagen.stretches(n, 29, long_run=1 << 20)
    enc, st = pyoracle.encode_stats(ALGO, data)
    assert st["copy_blocks"] > (1 << 20) // 64 // 2
    expect_input(on_three(decode_stream(enc, n)), data, "stream")
    raw, _ = cpu_container(data, 1 << 20, ALGO, 2)
    expect_input(on_three(decode_container(raw, n)), data, "container")


@pytest.mark.parametrize("kind", ["markov16", "stretches"])
@pytest.mark.parametrize("n0", [5 * 1024 + 3, 65536 - 160])
def test_step_and_tail_boundaries(kind, n0):
    """Every length n0 .. n0 + 320: all residues of the 256-byte step, the 64-byte record, the 72-byte look-ahead of the hot loop and the tail of
    fewer than four bytes, into a buffer of exactly n bytes and of n + 1."""
    wrong = []
    for k in range(321):
        n = n0 + k
        data = make(kind, n)
        enc = pyoracle.encode(ALGO, data)
        for cap in (n, n + 1):
            res = on_three(decode_stream(enc, cap))
            if res != ("ok", data.tobytes()):
                wrong.append((n, cap, res[0], len(res[1]) if len(res) > 1 else 0))
    assert not wrong, wrong[:20]


def stage_stats():
    import ctypes
    from density_amd import _lib
    a = (ctypes.c_uint64 * 2)()
    _lib.lib().density_hip_stage_stats(a)
    return list(a)


@pytest.mark.parametrize("kind", NEW_KINDS)
def test_round_trip_through_the_gpu_encoder(kind):
    """The encoder's exchange passes have not seen these inputs either: every chunk stream == the oracle's (chunks of 256 KiB: the passes take
    every chunk, and keep those in which the oracle copies no block), one long stream through `lion_encode`, and the three decoders on what the
    GPU wrote."""
    chunk = 262144
    n = 5 * chunk + 3 * 4096 + 1001
    data = make(kind, n)
    cont = np.zeros(container.container_bound(ALGO, n, chunk), dtype=np.uint8)
    try:
        container.set_kernel_variant(64)                                                  # audit: count the chunks kept / handed back
        s0 = stage_stats()
        cn = container.encode(ALGO, data, cont, chunk)
        s1 = stage_stats()
        out = np.zeros(Lion.safe_encode_buffer_size(n), dtype=np.uint8)
        m = Lion.encode(data, out)
    finally:
        container.set_kernel_variant(0)
    hdr, payloads = container.chunk_payloads(cont[:cn])
    assert hdr.n_chunks == 6
    copies = 0
    for i, p in enumerate(payloads):
        want, st = pyoracle.encode_stats(ALGO, data[i * chunk:(i + 1) * chunk])
        assert p == want, (kind, i)
        copies += st["copy_blocks"]
    assert s1[0] - s0[0] == hdr.n_chunks and 0 <= s1[1] - s0[1] <= hdr.n_chunks
    if copies == 0:
        assert s1[1] - s0[1] == 0
    assert out[:m].tobytes() == pyoracle.encode(ALGO, data), kind
    expect_input(on_three(decode_container(cont[:cn], n)), data, (kind, "container"))


def corrupt_cases(raw, streams, n, chunk, seed):
    """48 seeded corruptions of a CPU-built container's payloads: a flipped byte, eight random bytes, a flipped bit inside a record's signature."""
    base = (32 + 4 * len(streams) + 15) // 16 * 16
    offs, o = [], base
    for s in streams:
        offs.append(o)
        o = (o + len(s) + 15) // 16 * 16
    sigs = [offs[k] + at for k, s in enumerate(streams) for kind, at in lion_blocks(s, min(chunk, n - k * chunk)) if kind == "r"]
    rng = np.random.default_rng(seed)
    for t in range(48):
        bad = raw.copy()
        mode = t % 3
        if mode == 0:
            at = base + int(rng.integers(0, len(raw) - base)); bad[at] ^= int(rng.integers(1, 256))
        elif mode == 1:
            at = base + int(rng.integers(0, len(raw) - base - 8)); bad[at:at + 8] = rng.integers(0, 256, size=8, dtype=np.uint8)
        else:
            at = sigs[int(rng.integers(0, len(sigs)))] + int(rng.integers(0, 6)); bad[at] ^= 1 << int(rng.integers(0, 8))
        yield t, bad, offs


def oracle_container_decode(bad, streams, offs, n, chunk):
    return b"".join(pyoracle.decode(ALGO, bytes(bad[offs[k]:offs[k] + len(s)]), min(chunk, n - k * chunk)) for k, s in enumerate(streams))


CORRUPT_N, CORRUPT_CHUNK, CORRUPT_SEED = 4 * 65536 + 555, 65536, 331         # (the seed: on the CPU the oracle decodes all n bytes in 18 to 38 of the 48 cases of every kind)


@pytest.mark.parametrize("kind", NEW_KINDS)
def test_corrupt_streams_decode_like_the_oracle(kind):
    """What no encoder writes: predictions out of rows nothing has written, MAP flags on empty slots, garbage items, a record whose signature says
    another length than the encoder gave it.  The three decoders end the same way, and where the oracle decodes all n bytes of the same container,
    with those bytes, never with an error.  (Input validation on a fixed list: every case stays inside the container's and the output's documented sizes.)"""
    n, chunk = CORRUPT_N, CORRUPT_CHUNK
    data = make(kind, n)
    raw, streams = cpu_container(data, chunk, ALGO, 2)
    compared = 0
    for t, bad, offs in corrupt_cases(raw, streams, n, chunk, CORRUPT_SEED):
        res = on_three(decode_container(bad, n))
        want = oracle_container_decode(bad, streams, offs, n, chunk)
        if len(want) == n:                                                        # (where the oracle itself stops short the container decode is an error or differs by design)
            assert res[0] == "ok", (kind, t, "the oracle decodes this container")
            same = res[1] == want
            assert same, (kind, t, _first_difference(res, ("ok", want)))
            compared += 1
    assert compared >= 16, compared


@pytest.mark.parametrize("kind", NEW_KINDS)
def test_truncated_streams_end_like_the_oracle(kind):
    """tests/test_gpu_cheetah_lion.py::test_errors_are_reported on the new kinds: a truncated stream ends exactly like the oracle's decode of it —
    the same bytes, or an error where the oracle returns 0 (the reference panics there: io/read_buffer.rs:22) — on all three decoders."""
    wrong = []
    for n in (3000, 70_000):
        data = make(kind, n)
        enc = pyoracle.encode(ALGO, data)
        with pytest.raises(DecodeError):
            Lion.decode(enc, np.zeros(n - 100, dtype=np.uint8))
        for cut in (1, 2, 3, 5, 9, 100, 257, 1000):
            want = pyoracle.decode(ALGO, enc[:-cut], n)
            res = on_three(decode_stream(enc[:-cut], n))
            got = res[1] if res[0] == "ok" else b""
            if got != want:
                wrong.append((kind, n, cut, len(got), len(want)))
    assert not wrong, wrong
