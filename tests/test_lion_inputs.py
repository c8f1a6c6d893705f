"""The inputs of tests/test_gpu_lion_decode.py, held to what they are for, on the CPU: over the kinds that file decodes every one of Lion's
eight flags (PLAIN, PRED_A..PRED_E, MAP_A, MAP_B) is at least 5 % of the coded quads of at least one kind (the oracle's histogram) — a floor
for the inputs, not a measurement: on text PRED_C..E and MAP_B are 1 % each, and those are the flags that move an entry inside a prediction
row —, `stretches` switches copy mode on behind a step's first, second, third and fourth record and within the last 300 bytes, and the C
oracle agrees with the independent Python model on every new kind (they are inputs neither has seen)."""
import numpy as np
import pytest

import datagen
from oracle import pymodel, pyoracle

NEW_KINDS = list(datagen.LION_KINDS)
GPU_KINDS = NEW_KINDS + ["prose", "mixed", "random", "zeros", "binaryish"]        # test_gpu_lion_decode.KINDS (checked there)
FLAGS = ["PLAIN", "PRED_A", "PRED_B", "PRED_C", "PRED_D", "PRED_E", "MAP_A", "MAP_B"]


def test_every_lion_flag_is_common_in_some_kind():
    best = {}
    for kind in GPU_KINDS:
        _, st = pyoracle.encode_stats("lion", datagen.by_kind(kind, 300_000, seed=3))
        total = sum(st["flags"])
        assert 16 * (st["coded_blocks"] - 1) < total <= 16 * st["coded_blocks"]
        for name, c in zip(FLAGS, st["flags"]):
            if c / total > best.get(name, (0.0, ""))[0]:
                best[name] = (c / total, kind)
    print(best)
    assert all(best.get(name, (0.0, ""))[0] >= 0.05 for name in FLAGS), best


def test_slot_pools_land_in_their_slots():
    rng = np.random.default_rng(1)
    for slot in (1, 77, 65535):
        q = datagen.slot_quads(slot, 3, rng)
        assert len(set(int(x) for x in q)) == 3 and all(pymodel.h16(int(x)) == slot for x in q)


def lion_blocks(enc, n):
    """('c' raw copy | 'r' coded record, offset in the stream) for each 64-byte block of the input, from the stream alone (codec.rs:82-126: the
    decoder's view)."""
    g, blocks, ipos = pymodel.Guard(), [], 0
    for pos in range(0, n, 64):
        take = min(64, n - pos)
        if g.next_is_copy():
            blocks.append(("c", ipos))
            ipos += take
            g.decay()
            continue
        sig = int.from_bytes(enc[ipos:ipos + 6], "little")
        flags = [(sig >> (3 * k)) & 7 for k in range(take // 4)]
        size = 6 + sum(4 if f == 0 else 2 if f >= 6 else 0 for f in flags) + take % 4
        blocks.append(("r", ipos))
        ipos += size
        g.update(size >= 64)
    assert ipos == len(enc)
    return blocks


def block_kinds(enc, n):
    return [k for k, _ in lion_blocks(enc, n)]


def test_stretches_switch_copy_mode_at_every_record_of_a_step():
    n = 300_000
    data = datagen.by_kind("stretches", n, seed=3)
    enc, st = pyoracle.encode_stats("lion", data)
    assert st["copy_blocks"] > 0 and st["coded_blocks"] > 0
    kinds = block_kinds(enc, n)
    assert kinds.count("c") == st["copy_blocks"]
    # a decoder step: up to four coded records in a row, counted from the last copy block (density_amd/csrc/serial_codec.hip, lion_decode_*)
    on_after, run = [0, 0, 0, 0], 0
    for k in kinds:
        if k == "c":
            if run:
                on_after[(run - 1) % 4] += 1
            run = 0
        else:
            run += 1
    print(on_after)
    assert min(on_after) >= 8, on_after
    assert "c" in kinds[-(300 // 64):] and "r" in kinds[-(300 // 64):], kinds[-6:]
    # ... and at the sizes the boundary test of the GPU file walks through, copy mode is on near the end of every one of them
    for m in (4096 + 77, 65536 + 131):
        d = datagen.by_kind("stretches", m, seed=3)
        kinds = block_kinds(pyoracle.encode("lion", d), m)
        assert "c" in kinds[-5:], (m, kinds[-8:])
    long = datagen.stretches(1_600_000, 3, long_run=1 << 20)
    _, st = pyoracle.encode_stats("lion", long)
    assert st["copy_blocks"] > (1 << 20) // 64 // 2 and st["coded_blocks"] > (1 << 20) // 64 // 4


@pytest.mark.parametrize("kind", NEW_KINDS)
def test_oracle_matches_independent_model_on_the_new_kinds(kind):
    for n in (40_000, 4099):
        data = bytes(datagen.by_kind(kind, n, seed=12))
        enc_c, st = pyoracle.encode_stats("lion", data)
        enc_py, copied = pymodel.encode("lion", data)
        assert enc_c == enc_py, (kind, n)
        assert st["copy_blocks"] == copied
        assert pymodel.decode("lion", enc_c) == data
        assert pyoracle.decode("lion", enc_py, n) == data
