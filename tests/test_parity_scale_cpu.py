"""The inputs of test_gpu_parity_scale.py (parity_scale_cases.py), held to what that file assumes of them, and the host arithmetic of the parity calls at its
chunk and group counts — without a device.  The conditions on the inputs are met by the oracle alone: every chunk a device test names as a victim has a
position where one flipped bit decodes, in the reference, to the full length and to other bytes."""
import numpy as np

import parity2_cpu
import parity_cpu
import parity_scale_cases as sc
import parity_update_cases as pc
import verdict_cases as vc
from density_amd import _lib, container
from oracle import pyoracle
from test_parity_update_cpu import fields, header_of, update_header


def test_shapes_reach_the_thresholds_they_are_named_for():
    assert sc.MAX_GRID == 2048 and sc.BLOCK == 256 and sc.MAX_MEMBERS == parity2_cpu.MAX_MEMBERS == 255
    n, (groups,) = sc.SHAPES["WIDE"]
    assert groups > sc.MAX_GRID and -(-groups // sc.BLOCK) == 9 and n == 3 * groups + 1
    assert [len(sc.members("WIDE", groups, g)) for g in (0, 1, groups - 1)] == [4, 3, 3]
    n, (few, more) = sc.SHAPES["DEEP"]
    assert [len(sc.members("DEEP", few, g)) for g in range(few)] == [2101, 2100] and -(-2101 // sc.BLOCK) == 9
    assert sorted({len(sc.members("DEEP", more, g)) for g in range(more)}) == [262, 263]
    n, (groups,) = sc.SHAPES["FIELD"]
    assert {len(sc.members("FIELD", groups, g)) for g in range(groups)} == {sc.MAX_MEMBERS}
    for shape in sc.SHAPES:
        b = sc.built(shape)
        h = b.header
        assert (h.n_chunks, h.total_len, h.chunk_size) == (sc.n_chunks(shape), sc.total(shape), sc.CHUNK) and h.n_chunks > sc.SCAN_TILE
        assert h.flags == container.FLAG_BLOCK_INDEX | container.FLAG_CHECKSUM and h.container_len == b.blob.size
        assert sc.total(shape) % sc.CHUNK == sc.RAGGED and -(-h.n_chunks // sc.BLOCK) >= 9


def test_the_input_has_no_zero_runs_and_the_containers_are_the_oracles_streams():
    src = sc._source()
    assert not (src.reshape(-1, 4) == 0).all(axis=1).any(), "a quad of zeros"
    assert len(np.unique(src[sc.PROSE_PIECE:sc.PROSE_PIECE + sc.RANDOM_PIECE])) > 150 and src[:sc.PROSE_PIECE].max() < 128
    for shape in sc.SHAPES:
        b = sc.built(shape)
        h, streams = container.chunk_payloads(b.blob)
        assert tuple(streams) == b.streams
        assert container.chunk_checksums(b.blob) == [container.checksum32(b.chunk(k)) for k in range(h.n_chunks)]
        for k in (0, 1, 1023, 1024, h.n_chunks - 2, h.n_chunks - 1):
            assert int(b.stream_at[k]) == vc.stream_byte_at(b.blob, k, 0), k
            assert pyoracle.decode(sc.ALGO, b.streams[k], b.chunk(k).size) == b.chunk(k).tobytes()


def test_every_named_victim_has_a_silent_position():
    """none skipped, none substituted: the flipped stream decodes in the reference to the full length and to different bytes"""
    seen = 0
    for what, b, victims in sc.every_victim():
        assert len(set(victims)) == len(victims) and victims, what
        for k in victims:
            part, stream = b.chunk(k), bytearray(b.streams[k])
            pos = b.plain_position(k)
            assert 8 <= pos < len(stream), (what, k)
            stream[pos] ^= vc.FLIP
            out = pyoracle.decode(sc.ALGO, bytes(stream), part.size)
            assert len(out) == part.size and out != part.tobytes(), (what, k)
            seen += 1
        bad = b.damage(victims)
        assert sorted(np.flatnonzero(bad != b.blob)) == sorted(b.flip_at(k) for k in victims), what
    assert seen > 4000


def test_losses_are_what_the_device_tests_say_of_them():
    groups = sc.WIDE_GROUPS
    singles, pairs, triples = sc.wide_losses()
    lost_of = {}
    for lost in singles + pairs + triples:
        (g,) = {k % groups for k in lost}
        assert g not in lost_of
        lost_of[g] = lost
    assert all(len(lost_of.get(g, ())) == (g % 4 if g not in (0, sc.WIDE_HANDS_OVER) else 2 if g == 0 else 0) for g in range(groups))
    assert lost_of[0] == (0, 6300) and {k // groups for (k,) in singles} == {0, 1, 2}
    assert sc.wide_losses(triples=False)[:2] == (singles, pairs)
    # groups on both sides of the grid's first trip and of every block of the verify kernel lose one, two and three members
    for losses in (singles, pairs, triples):
        assert {lost[0] % groups // sc.BLOCK for lost in losses} == set(range(9)) and max(lost[0] % groups for lost in losses) >= sc.MAX_GRID
    for groups, lost, back in sc.DEEP_CASES:
        per_group = {}
        for k in lost:
            per_group.setdefault(k % groups, []).append(k)
        assert set(back) == {ks[0] for ks in per_group.values() if len(ks) == 1} and back and max(k // groups for k in back) >= sc.BLOCK
    lanes_and_trips = [[(k // 2 % sc.BLOCK, k // 2 // sc.BLOCK) for k in lost[:2]] for groups, lost, back in sc.DEEP_CASES[1:3]]
    assert lanes_and_trips == [[(3, 0), (3, 4)], [(3, 0), (6, 4)]]


def test_field_pairs_cover_every_distance():
    places = [sc.field_places(p) for p in range(sc.FIELD_GROUPS * sc.FIELD_CALLS)]
    assert all(0 <= a < b <= 254 for a, b in places)
    assert {b - a for a, b in places} == set(range(1, 255)), "a distance is missing"
    assert {(0, 254), (0, 1), (253, 254), (127, 128)} <= set(places)
    assert len({a for a, b in places}) > 64                 # (the first places are spread too)
    last = sc.n_chunks("FIELD") - 1
    for call in range(sc.FIELD_CALLS):
        pairs = sc.field_pairs(call)
        assert [k1 % 64 for k1, k2 in pairs] == [k2 % 64 for k1, k2 in pairs] == list(range(64))
        assert [(k1 // 64, k2 // 64) for k1, k2 in pairs] == places[64 * call:64 * call + 64] and max(k2 for _, k2 in pairs) <= last
    assert sc.field_pairs(3)[63] == (63 + 64 * 253, last)


def test_sizes_are_the_models():
    size1, size2 = _lib.lib().density_hip_parity_size, _lib.lib().density_hip_parity2_size
    for shape, (n, asked) in sc.SHAPES.items():
        for groups in asked + (1, n, n + 5):
            t = sc.total(shape)
            assert size1(t, sc.CHUNK, groups) == parity_cpu.size(t, sc.CHUNK, groups) == 32 + min(groups, n) * 256, (shape, groups)
            assert size2(t, sc.CHUNK, groups) == parity2_cpu.size(t, sc.CHUNK, groups), (shape, groups)
            assert (size2(t, sc.CHUNK, groups) == 0) == (-(-n // min(groups, n)) > 255)
    t = sc.total("DEEP")
    assert size2(t, sc.CHUNK, 16) == 0 == size2(t, sc.CHUNK, 2) and size1(t, sc.CHUNK, 16) == 32 + 16 * 256 and size1(t, sc.CHUNK, 2) == 32 + 2 * 256
    assert size2(sc.total("FIELD"), sc.CHUNK, 64) == 32 + 2 * 64 * 256 and size2(sc.total("FIELD") + 157, sc.CHUNK, 64) == 0
    assert size2(sc.total("WIDE"), sc.CHUNK, 2100) == 32 + 2 * 2100 * 256


def test_update_header_agrees_with_the_rules_written_down_twice():
    taken = refused = 0
    for name, (shape, groups, versions, edit) in {**sc.EDITS, **sc.OTHER_EDITS}.items():
        for version in versions:
            h = header_of(version, sc.total(shape), sc.CHUNK, groups)
            rc, after = update_header(h, edit)
            valid = pc.valid(sc.total(shape), sc.CHUNK, groups, version, edit)
            assert valid or name in sc.OTHER_EDITS, name
            if not valid:
                assert rc == _lib.ERR_ARGUMENT and fields(after) == fields(_lib.ParityHeader()) and _lib.last_error(), (name, version)
                refused += 1
                continue
            assert rc == _lib.OK, (name, version, _lib.last_error())
            new_total = sc.total(shape) - edit[1] + edit[2]
            want = header_of(version, new_total, sc.CHUNK, h.n_groups)
            assert fields(after) == fields(want), (name, version)
            if name in sc.EDITS:
                assert fields(after) == fields(container.parse_parity_header(sc.edited_blob(name, version))), (name, version)
            taken += 1
    assert taken == 13 + 3 and refused == 2 + 2 + 1
    assert not pc.valid(sc.total("FIELD"), sc.CHUNK, 64, 2, sc.OTHER_EDITS["field_256th_member"][3]) and pc.valid(sc.total("FIELD"), sc.CHUNK, 64, 1, sc.OTHER_EDITS["field_256th_member"][3])


def wrecked(b, lost):
    out = b.data.copy()
    for i, k in enumerate(lost):
        out[k * sc.CHUNK:(k + 1) * sc.CHUNK] = 0xEE - 0x11 * (i % 8)
    return out


def test_the_models_rebuild_what_the_device_tests_expect_back():
    """from the intact input, the lost chunks overwritten: version 1 and version 2's P row give a group's only lost chunk, both rows a pair"""
    b = sc.built("WIDE")
    singles, pairs, triples = sc.wide_losses()
    lost = singles[::25] + pairs[::25] + pairs[:1]
    out = wrecked(b, sc.flat(lost))
    v1, v2 = sc.model_blob("WIDE", 1, sc.WIDE_GROUPS), sc.model_blob("WIDE", 2, sc.WIDE_GROUPS)
    for ks in lost:
        if len(ks) == 1:
            assert np.array_equal(parity_cpu.rebuild(v1, out, ks[0]), b.chunk(ks[0])) and np.array_equal(parity2_cpu.rebuild_one(v2, out, ks[0]), b.chunk(ks[0]))
        else:
            d1, d2 = parity2_cpu.rebuild_two(v2, out, *ks)
            assert np.array_equal(d1, b.chunk(ks[0])) and np.array_equal(d2, b.chunk(ks[1])), ks
    assert b.chunk(6300).size == sc.RAGGED
    b = sc.built("DEEP")
    for groups, lost, back in sc.DEEP_CASES:
        out = wrecked(b, lost)
        for k in back:
            assert np.array_equal(parity_cpu.rebuild(sc.model_blob("DEEP", 1, groups), out, k), b.chunk(k)), (groups, k)
    b = sc.built("FIELD")
    v2 = sc.model_blob("FIELD", 2, sc.FIELD_GROUPS)
    by_places = {(k1 // 64, k2 // 64): (k1, k2) for call in range(sc.FIELD_CALLS) for k1, k2 in sc.field_pairs(call)}
    named = [by_places[p] for p in ((0, 254), (253, 254), (0, 1), (127, 128))]
    assert named[1][1] == sc.n_chunks("FIELD") - 1
    for call in range(sc.FIELD_CALLS):
        pairs = sc.field_pairs(call)
        out = wrecked(b, sc.flat(pairs))
        for k1, k2 in pairs[::8] + [p for p in named if p in pairs]:
            d1, d2 = parity2_cpu.rebuild_two(v2, out, k1, k2)
            assert np.array_equal(d1, b.chunk(k1)) and np.array_equal(d2, b.chunk(k2)), (k1, k2)
    for name, pair in sc.END_TO_END.items():
        b = sc.built_edited(name)
        d1, d2 = parity2_cpu.rebuild_two(sc.edited_blob(name, 2), wrecked(b, pair), *pair)
        assert np.array_equal(d1, b.chunk(pair[0])) and np.array_equal(d2, b.chunk(pair[1])), name
        assert np.array_equal(b.data, sc.edited(name)[0]) and not np.array_equal(b.chunk(pair[1]), sc.built(sc.EDITS[name][0]).data[pair[1] * sc.CHUNK:(pair[1] + 1) * sc.CHUNK])


def test_pair_constants_over_the_whole_field():
    """for every pair of places a < b: c1 * (1 ^ 2^(b-a)) = 2^(b-a) and c2 * (2^a ^ 2^b) = 1 — the model's own arithmetic, wherever a pair may stand"""
    times = lambda c, v: int(parity2_cpu.times(c, [v])[0])
    count = 0
    for a in range(sc.MAX_MEMBERS):
        for b in range(a + 1, sc.MAX_MEMBERS):
            c1, c2 = sc.pair_constants(a, b)
            assert times(c1, 1 ^ parity2_cpu.pow2(b - a)) == parity2_cpu.pow2(b - a), (a, b)
            assert times(c2, parity2_cpu.pow2(a) ^ parity2_cpu.pow2(b)) == 1, (a, b)
            count += 1
    assert count == 255 * 254 // 2
