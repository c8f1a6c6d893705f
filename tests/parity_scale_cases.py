"""What the parity tests at scale (test_parity_scale_cpu.py without a device, test_gpu_parity_scale.py on one) share: inputs of thousands of 256-byte chunks, their
sealed packed Chameleon containers assembled HERE from the oracle's chunk streams (slice_cpu.assemble, as tests/test_gpu_slice.py does for its many-chunk case),
the victims of every recover decode, and the edits of every update.  The shapes are chosen by the trip counts of the kernels in density_amd/csrc/parity.hip
and of the sealed decode in front of them — see MAX_GRID, BLOCK and MAX_MEMBERS.  Test infrastructure: it calls the oracle and the numpy models
(parity_cpu.py, parity2_cpu.py), never the library's device calls.  Everything is built once per session and handed out read-only.

The input alternates pieces of prose and of random bytes and has no runs of zeros: every chunk is encoded on its own, so its first quad meets an empty
dictionary and is PLAIN — every chunk has a position where one flipped bit is silent damage (a chunk of zeros has none) —, and the random pieces put every
bit pattern through the field's products."""
import functools

import numpy as np

import datagen
import paged_cpu
import parity2_cpu
import parity_cpu
import parity_update_cases as pc
import slice_cpu
import verdict_cases as vc
from density_amd import container
from oracle import pyoracle

ALGO = "chameleon"
CHUNK = 256            # the smallest chunk size the library takes
RAGGED = 100           # the last chunk of every shape: its 16-byte slots end bytewise
MAX_GRID = 2048        # parity.hip: kParMaxGroups — parity_rows_, recover_plan_, recover_rebuild_, recover_sum_ and parity_update_kernel are launched with at most
                       # so many work-groups and take what is left of their units (n_groups x tiles) in a grid-stride loop
BLOCK = 256            # parity.hip: recover_verify_kernel (a thread per GROUP, blocks of 256) and kParThreads, the lanes that share out a group's members in
                       # recover_plan_kernel; checksum.hip: checksum_verdict_kernel (a thread per CHUNK, blocks of 256)
MAX_MEMBERS = 255      # parity.hip: pair_word / gf_pow2 — a version-2 group has the places 0 .. 254, the powers of 2 the field has
SCAN_TILE = 1024       # container.hip: kScanThreads — the chunks layout_decode_kernel's one work-group scans per trip, the carry going on to the next

# name: (chunks, the group counts asked for)
SHAPES = {
    "WIDE": (3 * 2100 + 1, (2100,)),       # units = 2100 > MAX_GRID in every bulk kernel and in the plan; 9 blocks of recover_verify_kernel; groups of 3, group 0 of 4
    "DEEP": (4201, (2, 16)),               # version 1 only: 2101 / 2100 members (nine trips of the plan kernel's lane loop), and 263 / 262 members
    "FIELD": (64 * MAX_MEMBERS, (64,)),    # version 2 at its limit: 255 members in every group
}
PROSE_PIECE, RANDOM_PIECE = 700, 500       # (1200 is no multiple of the chunk size: the pieces meet the chunk boundaries at 75 different phases)


def n_chunks(shape):
    return SHAPES[shape][0]


def total(shape):
    return (n_chunks(shape) - 1) * CHUNK + RAGGED


def _frozen(a):
    a.setflags(write=False)
    return a


@functools.lru_cache(maxsize=None)
def _source():
    """as many whole chunks as the largest shape has"""
    n = max(c for c, _ in SHAPES.values()) * CHUNK
    periods = -(-n // (PROSE_PIECE + RANDOM_PIECE))
    text = datagen.prose(periods * PROSE_PIECE, seed=29).reshape(periods, PROSE_PIECE)
    noise = datagen.random_bytes(periods * RANDOM_PIECE, seed=31).reshape(periods, RANDOM_PIECE)
    return _frozen(np.concatenate([text, noise], axis=1).reshape(-1)[:n].copy())


@functools.lru_cache(maxsize=None)
def _whole_streams():
    src = _source()
    return tuple(pyoracle.encode(ALGO, src[i:i + CHUNK]) for i in range(0, src.size, CHUNK))


@functools.lru_cache(maxsize=None)
def data(shape):
    return _frozen(_source()[:total(shape)].copy())


class Built:
    """An input, the oracle's stream of each of its chunks, and the sealed packed container of them: header, size table, block index, the streams at 16-byte
    boundaries, and the trailer of container.checksum32 per INPUT chunk (unpage_cases.sealed writes the same)."""

    def __init__(self, data, streams):
        n = -(-data.size // CHUNK)
        assert len(streams) == n
        index = b"".join(bytes(b for b, _ in paged_cpu.walk_records(s, min(CHUNK, data.size - i * CHUNK))) for i, s in enumerate(streams))
        sums = [container.checksum32(data[i:i + CHUNK]) for i in range(0, data.size, CHUNK)]
        self.data, self.streams = data, streams
        self.blob = _frozen(slice_cpu.assemble(0, CHUNK, data.size, streams, index, sums))
        self.header = container.parse_header(self.blob)
        sizes = np.array([len(s) for s in streams], dtype=np.int64)
        first = vc.front_matter(self.header)[1]
        self.stream_at = first + np.concatenate(([0], np.cumsum((sizes + 15) // 16 * 16)[:-1]))      # (what vc.stream_byte_at adds up chunk by chunk)
        self._positions = {}

    def chunk(self, k):
        return self.data[k * CHUNK:(k + 1) * CHUNK]

    def plain_position(self, k):
        """the stream offset of chunk k's first PLAIN quad"""
        if k not in self._positions:
            self._positions[k] = vc.chameleon_plain_position(self.streams[k], self.chunk(k).size, from_block=0)
        return self._positions[k]

    def flip_at(self, k):
        """the container offset of chunk k's silent flip"""
        pos = self.plain_position(k)
        at = int(self.stream_at[k]) + pos
        assert self.blob[at] == self.streams[k][pos]
        return at

    def damage(self, victims):
        """the container with one silent flip (vc.FLIP) in the stream of every chunk of `victims`"""
        victims = list(victims)
        assert len(set(victims)) == len(victims)
        bad = self.blob.copy()
        for k in victims:
            bad[self.flip_at(k)] ^= vc.FLIP
        return bad


@functools.lru_cache(maxsize=None)
def built(shape):
    d = data(shape)
    return Built(d, _whole_streams()[:n_chunks(shape) - 1] + (pyoracle.encode(ALGO, d[-RAGGED:]),))


def sealed(shape):
    return built(shape).blob


def damage(shape, victims):
    return built(shape).damage(victims)


@functools.lru_cache(maxsize=None)
def model_blob(shape, version, groups):
    return _frozen(pc.model(version).blob(data(shape), CHUNK, groups))


def members(shape, groups, g):
    return list(range(g, n_chunks(shape), groups))


# ------------------------------------------------------------------------------------------------------------------------------------------
# the decode in front of recovery: 300 victims, every block of 256 chunks has some, the first and the (ragged) last chunk among them

def spread(shape, count=300):
    n = n_chunks(shape)
    victims = sorted({i * (n - 1) // (count - 1) for i in range(count)})
    assert len(victims) == count and victims[0] == 0 and victims[-1] == n - 1
    assert {k // BLOCK for k in victims} == set(range(-(-n // BLOCK))), "a block of the verdict kernel without a victim"
    assert any(k >= SCAN_TILE for k in victims)
    return victims


# ------------------------------------------------------------------------------------------------------------------------------------------
# WIDE: 2100 groups; group g is intact (g % 4 == 0), has lost one member (1), two (2) or all three (3)

WIDE_GROUPS = 2100
PLACE_PAIRS = [(0, 1), (0, 2), (1, 2)]
WIDE_HANDS_OVER = 2098      # this group's pair goes to group 0 instead: chunk 0 with the ragged chunk 6300, places 0 and 3 of the one group of four


def wide_losses(triples=True):
    """(singles, pairs, triples): lists of chunk tuples.  A single stands at place 0, 1, 2 in turn, a pair at each of the three place pairs in turn."""
    chunk_of = lambda g, place: g + place * WIDE_GROUPS
    singles, pairs, threes = [], [(0, n_chunks("WIDE") - 1)], []
    for g in range(WIDE_GROUPS):
        turn = (g // 4) % 3
        if g % 4 == 1:
            singles.append((chunk_of(g, turn),))
        elif g % 4 == 2 and g != WIDE_HANDS_OVER:
            pairs.append(tuple(chunk_of(g, place) for place in PLACE_PAIRS[turn]))
        elif g % 4 == 3 and triples:
            threes.append(tuple(chunk_of(g, place) for place in range(3)))
    assert len(singles) == len(pairs) == 525 and len(threes) == (525 if triples else 0)
    assert {k % WIDE_GROUPS for k in pairs[0]} == {0} and {tuple(k // WIDE_GROUPS for k in p) for p in pairs[1:]} == set(PLACE_PAIRS)
    assert max(k % WIDE_GROUPS for lost in singles + pairs + threes for k in lost) >= MAX_GRID, "no victim group behind the grid's first trip"
    return singles, pairs, threes


def flat(*lists):
    return [k for losses in lists for lost in losses for k in lost]


# ------------------------------------------------------------------------------------------------------------------------------------------
# DEEP: version 1, groups of thousands (2 groups) and of 263 / 262 (16 groups).  (groups, the chunks lost, those of them that come back) — a chunk
# is group + place * groups; with 2 groups a lane of the plan kernel takes the places lane, lane + 256, ...: place 1027 is lane 3 in its trip 4

def _deep(groups, *group_places):
    return tuple(g + place * groups for g, place in group_places)


DEEP_CASES = [
    (2, _deep(2, (0, 1500), (1, 2050)), _deep(2, (0, 1500), (1, 2050))),                       # one of each group, behind the first 256 places
    (2, _deep(2, (0, 3), (0, 1027), (1, 2050)), _deep(2, (1, 2050))),                          # two of group 0 in ONE lane, trips 0 and 4: lost; group 1's comes back
    (2, _deep(2, (0, 3), (0, 1030), (1, 2050)), _deep(2, (1, 2050))),                          # ... in the lanes 3 and 6, trips 0 and 4
    (2, _deep(2, (0, 2100), (1, 2099)), _deep(2, (0, 2100), (1, 2099))),                       # the last member of each group: the ragged chunk, trip 8
    (16, _deep(16, (8, 262), (3, 262), (15, 261)), _deep(16, (8, 262), (3, 262), (15, 261))),  # place 262 (lane 6, trip 1): the ragged chunk 4200, chunk 4195
    (16, _deep(16, (0, 3), (0, 260), (8, 262)), _deep(16, (8, 262))),                          # two of group 0 in the lanes 3 and 4, trips 0 and 1
]
assert DEEP_CASES[0][1] == (3000, 4101) and DEEP_CASES[1][1][:2] == (6, 2054) and DEEP_CASES[3][1][0] == 4200 == DEEP_CASES[4][1][0]


# ------------------------------------------------------------------------------------------------------------------------------------------
# FIELD: four recover decodes, a pair in each of the 64 groups.  The rule: pair p = 64 * call + group has the distance d = p + 1 and the first place
# a = 37 * p mod (255 - d), p < 254 — every distance 1 .. 254 once, (0, 1) at p = 0, (0, 254) at p = 253 —; p = 254 is (127, 128) and p = 255, in group 63, is
# (253, 254): its later member is the ragged last chunk.

FIELD_GROUPS, FIELD_CALLS = 64, 4


def field_places(p):
    if p >= 254:
        return (127, 128) if p == 254 else (253, 254)
    d = p + 1
    a = 37 * p % (MAX_MEMBERS - d)
    return a, a + d


def field_pairs(call):
    """the 64 pairs of chunks of decode `call`"""
    return [tuple(g + place * FIELD_GROUPS for place in field_places(FIELD_GROUPS * call + g)) for g in range(FIELD_GROUPS)]


# ------------------------------------------------------------------------------------------------------------------------------------------
# updates.  name: (shape, groups asked for, versions, (offset, old_size, new_size)) — the new bytes are pc.new_bytes(new_size)

def _edits():
    w, d, f = total("WIDE"), total("DEEP"), total("FIELD")
    span = (6290 * CHUNK + 9) - (10 * CHUNK + 7)
    last_row = (MAX_MEMBERS - 1) * FIELD_GROUPS * CHUNK
    edits = {
        "wide_span": ("WIDE", WIDE_GROUPS, (1, 2), (10 * CHUNK + 7, span, span)),          # 6281 chunks: every group touched (more than MAX_GRID), up to three members
        "wide_append": ("WIDE", WIDE_GROUPS, (1, 2), (w, 0, 2500 * CHUNK + 33)),           # onto the ragged chunk: 2501 chunks touched
        "wide_truncate": ("WIDE", WIDE_GROUPS, (1, 2), (2100 * CHUNK, w - 2100 * CHUNK, 0)),   # down to exactly n_groups chunks
        "deep_whole": ("DEEP", 2, (1,), (0, d, d)),                                        # 2101 / 2100 touched members a unit
        "field_whole": ("FIELD", FIELD_GROUPS, (1, 2), (0, f, f)),                         # 255 touched members: the update's whole Horner chain
        "field_last_row": ("FIELD", FIELD_GROUPS, (1, 2), (last_row, f - last_row, f - last_row)),   # the last 64 chunks: first / n_groups = 254, the largest power
        "field_small": ("FIELD", FIELD_GROUPS, (1, 2), (16000 * CHUNK + 50, 11, 11)),
    }
    refused = {
        "wide_below_its_groups": ("WIDE", WIDE_GROUPS, (1, 2), (2099 * CHUNK, w - 2099 * CHUNK, 0)),
        "wide_neither_shape": ("WIDE", WIDE_GROUPS, (1, 2), (10 * CHUNK, 5, 6)),
        "field_256th_member": ("FIELD", FIELD_GROUPS, (1, 2), (f, 0, CHUNK - RAGGED + 1)),           # version 2 refuses, version 1 takes it
        "field_fills_its_last_chunk": ("FIELD", FIELD_GROUPS, (1, 2), (f, 0, CHUNK - RAGGED)),       # ... and this one both take
    }
    return edits, refused


EDITS, OTHER_EDITS = _edits()
# the updated blob in use: (edit, the pair of one group lost from a container of the EDITED input)
END_TO_END = {"wide_append": (6300, 8400),       # the chunk that was ragged (place 3 of group 0) and an appended one (place 4)
              "field_small": (0, 16000)}         # places 0 and 250 of group 0: the edited chunk


@functools.lru_cache(maxsize=None)
def edited(name):
    """(the input after edit `name`, the new bytes)"""
    shape, groups, versions, edit = EDITS[name]
    new = pc.new_bytes(edit[2])
    return _frozen(pc.edited(data(shape), edit, new)), _frozen(new)


@functools.lru_cache(maxsize=None)
def edited_blob(name, version):
    """the model's blob of the edited input, with the n_groups of the blob it was updated from"""
    shape, groups, versions, edit = EDITS[name]
    return _frozen(pc.model(version).blob(edited(name)[0], CHUNK, parity_cpu.geometry(total(shape), CHUNK, groups)[1]))


@functools.lru_cache(maxsize=None)
def built_edited(name):
    """Built of the edited input: the streams of the chunks the edit leaves alone are the old ones"""
    shape, groups, versions, (offset, old_size, new_size) = EDITS[name]
    after, old = edited(name)[0], built(shape).streams
    first = offset // CHUNK
    behind = -(-(offset + old_size) // CHUNK) if old_size == new_size else len(old)            # (an edit of the tail: everything from `first` on is new)
    streams = tuple(old[i] if i < first or (i >= behind and i < len(old)) else pyoracle.encode(ALGO, after[i * CHUNK:(i + 1) * CHUNK]) for i in range(-(-after.size // CHUNK)))
    return Built(after, streams)


# ------------------------------------------------------------------------------------------------------------------------------------------
# every chunk a test names as a victim: [(what, Built, chunks)]

def every_victim():
    out = [(f"{shape} spread", built(shape), spread(shape)) for shape in SHAPES]
    out.append(("WIDE losses", built("WIDE"), flat(*wide_losses())))
    out += [(f"DEEP {groups} groups {lost}", built("DEEP"), list(lost)) for groups, lost, _ in DEEP_CASES]
    out += [(f"FIELD call {call}", built("FIELD"), flat(field_pairs(call))) for call in range(FIELD_CALLS)]
    out += [(f"after {name}", built_edited(name), list(pair)) for name, pair in END_TO_END.items()]
    return out


def pair_constants(a, b):
    """(c1, c2) of the solve for the places a < b, as parity2_cpu.rebuild_two computes them"""
    over_d = parity2_cpu.inverse(parity2_cpu.pow2(b - a) ^ 1)
    return int(parity2_cpu.times(over_d, [parity2_cpu.pow2(b - a)])[0]), int(parity2_cpu.times(over_d, [parity2_cpu.pow2(255 - a)])[0])
