"""What the parity-update tests (test_parity_update_cpu.py without a device, test_gpu_parity_update.py on one) share: the shapes, the edits, the edited input and
the blob it should have — the numpy models parity_cpu.py / parity2_cpu.py run on the edited input.  Test infrastructure: it never calls the library.

An edit is (offset, old_size, new_size): input bytes [offset, offset + old_size) are replaced by new_size new bytes.  It is a same-size edit (old_size == new_size,
anywhere inside the input), an edit of the tail (offset + old_size == total: append, truncation, a tail of another length), or both."""
import functools

import numpy as np

import datagen
import parity2_cpu
import parity_cpu

ROW_TILE = 16384      # parity.hip: kParTile, what a work-group takes of a row per trip
CHUNK = 65536
TOTAL = 5 * CHUNK + 777
GROUPS = [1, 2, 3, 6]
# chunk sizes at the row tile and 256 either side of it: three chunks and 1001 bytes, two groups
TILE_SHAPES = [(3 * c + 1001, c, 2) for c in (ROW_TILE - 256, ROW_TILE, ROW_TILE + 256)]
LONG = (255 * 256, 256, 1)          # the longest Q chain: 255 members in one group


def model(version):
    return parity_cpu if version == 1 else parity2_cpu


@functools.lru_cache(maxsize=None)
def input_of(total):
    data = datagen.by_kind("mixed", max(total, 1), seed=43)[:total]
    data.setflags(write=False)
    return data


def new_bytes(size, seed=7):
    """the bytes an edit writes: every bit pattern, so that every term of the field's products is exercised"""
    return np.random.default_rng(seed + size).integers(0, 256, size=size, dtype=np.uint8)


def edited(data, edit, new):
    offset, old_size, new_size = edit
    assert new.size == new_size and offset + old_size <= data.size and (old_size == new_size or offset + old_size == data.size)
    return np.concatenate([data[:offset], new, data[offset + old_size:]])


def valid(total, chunk, groups, version, edit):
    """the header file's rules, written down a second time: is the edit one the update takes for the blob of `total` bytes with `groups` groups asked for"""
    offset, old_size, new_size = edit
    n_chunks, n_groups, row_bytes = parity_cpu.geometry(total, chunk, groups)
    same, tail = old_size == new_size and offset + old_size <= total, offset + old_size == total
    if not (same or tail):
        return False
    after = total if same else offset + new_size
    n_after = -(-after // chunk)
    if n_after >= 1 << 32 or n_after < n_groups or (n_after and not n_groups) or (min(chunk, after) + 15) // 16 * 16 != row_bytes:
        return False
    return version == 1 or n_groups == 0 or -(-n_after // n_groups) <= 255


def same_size_edits(total, chunk):
    """(offset, size, size): every whole chunk (the ragged last at its true length), ranges inside chunk 1 — within one 16-byte slot, across a slot boundary,
    across a tile boundary where the chunk has one —, a range across two chunks, ranges over three chunks (two touched members of a group with two groups: chunks
    1 and 3 from place 0, chunks 2 and 4 from place 1) where the input has them"""
    n_chunks = -(-total // chunk)
    edits = [(k * chunk, min(chunk, total - k * chunk)) for k in range(n_chunks)]
    edits += [(chunk + 16 * 5 + 2, 11), (chunk + 16 * 7 + 10, 20), (chunk - 5, 11)]
    if chunk > ROW_TILE:
        edits.append((chunk + ROW_TILE - 7, 30))
    if n_chunks >= 4:
        edits.append((chunk + 100, 2 * chunk + 50 - 100))
    if n_chunks >= 5:
        edits.append((2 * chunk + 9, 2 * chunk + 1000))
    return [(at, size, size) for at, size in edits]


def tail_edits(total, chunk, n_groups):
    """(base total, edit) of the tail edits: the base is `total`, but for the append that starts at a chunk boundary"""
    whole = total - total % chunk
    edits = [(whole, (whole, 0, total - whole)),                              # append at a chunk boundary
             (total, (total, 0, 1000)),                                       # ... onto the ragged chunk without crossing it
             (total, (total, 0, 5 * chunk + 100)),                            # ... of five chunks and more: with two groups they wrap more than once
             (total, (total - 777, 777, 0)),                                  # truncate by 777, by a chunk more, down to exactly n_groups chunks
             (total, (total - 777 - chunk, 777 + chunk, 0)),
             (total, (n_groups * chunk, total - n_groups * chunk, 0)),
             (total, (total - 1000, 1000, 70_000))]                           # a tail of 1000 replaced by 70 000
    return [(base, edit) for base, edit in edits if edit[0] >= 0 and edit[1] >= 0]


def blobs(version, data, chunk, groups, edit, new):
    """(the model's blob of the input, the model's blob of the edited input with the FIRST blob's n_groups, the edited input)"""
    after = edited(data, edit, new)
    m = model(version)
    return m.blob(data, chunk, groups), m.blob(after, chunk, parity_cpu.geometry(data.size, chunk, groups)[1]), after
