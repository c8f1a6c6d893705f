"""Recovery records at chunk and group counts beyond one trip of their kernels (density_amd/csrc/parity.hip), and the sealed decode in front of them at the same
counts.  Every kernel there is a loop meant to go round more than once — a grid-stride loop over n_groups x tiles units behind a grid of at most 2048
work-groups, a lane loop over a group's members, a thread per group in blocks of 256, a walk along up to 254 powers of 2 — and the other parity files never
send one round twice.  The shapes of parity_scale_cases.py do:

    WIDE   6301 chunks of 256 bytes, 2100 groups of 3 (one of 4)     units = 2100 > 2048: the second trip of rows, plan, rebuild, sum and update; 9 blocks of verify
    DEEP   4201 chunks, 2 groups (2101 / 2100 members) and 16        version 1: nine trips of the plan's lane loop, members behind place 255
    FIELD  16320 chunks, 64 groups of 255                            version 2 at its limit: every distance 1 .. 254 between a pair, the longest Horner chains

The containers are assembled on the CPU from the oracle's streams, so nothing here depends on an encoder.  The blobs handed to the decoder and to the update
are the numpy MODELS' (parity_cpu.py, parity2_cpu.py); the device's own blob is held to the model separately; no two kernels are checked against each other.
The recover decode is held against ground truth, the input, with the contract and the helpers of test_gpu_parity.py; test_parity_scale_cpu.py holds the inputs
to what is assumed of them here (every victim has a silent position in the reference) without a device."""
import numpy as np
import pytest

import parity_scale_cases as sc
import test_gpu_parity as v1_file
import test_gpu_parity2 as v2_file
import test_gpu_verdicts as verdict_file
from density_amd import _lib, container
from test_gpu_checksum import to_device
from test_gpu_parity import DAMAGED, OK, POISON, RECOVERED, check_contract, recover_decode
from test_gpu_parity_update import fields, update

pytestmark = pytest.mark.gpu

# (blank, offset of the output in its buffer, offset of the blob in its): both ways, and once with every rebuilt 256-byte chunk beginning and ending bytewise
PLACEMENTS = [(False, 0, 0), (True, 0, 0), (False, 3, 5)]
# the blob each shape's intact container is decoded with: (version, groups asked for)
BLOB_OF = {"WIDE": (2, sc.WIDE_GROUPS), "DEEP": (1, 2), "FIELD": (2, sc.FIELD_GROUPS)}


def expected(n, recovered=(), damaged=()):
    want = np.full(n, OK, dtype=np.int64)
    want[np.array(list(recovered), dtype=np.intp)] = RECOVERED
    want[np.array(list(damaged), dtype=np.intp)] = DAMAGED
    return want


def same_verdicts(verdicts, want):
    assert np.array_equal(np.asarray(verdicts, dtype=np.int64), want), np.flatnonzero(np.asarray(verdicts, dtype=np.int64) != want)[:8]


def recover_and_check(b, bad, parity, recovered, damaged, blank, offset=0, parity_offset=0, plain=None):
    """one recover decode of `bad` (made from b's container): the exact verdict vector, the exact counts, the return code, the contract; where nothing stays
    damaged the output is the input; without blanking a chunk left damaged holds what the plain verdict decode `plain` left there"""
    n = b.header.n_chunks
    rc, n_damaged, n_recovered, got, verdicts = recover_decode(bad, parity, b.data.size, blank, header=b.header, offset=offset, parity_offset=parity_offset)
    same_verdicts(verdicts, expected(n, recovered, damaged))
    assert (rc, n_damaged, n_recovered) == (_lib.ERR_CHECKSUM if damaged else _lib.OK, len(damaged), len(recovered)), (rc, n_damaged, n_recovered)
    assert check_contract(b.data, sc.CHUNK, got, verdicts, blank) == (set(damaged), set(recovered))
    if not damaged:
        assert np.array_equal(got, b.data), np.flatnonzero(got != b.data)[:8]
    elif not blank and plain is not None:
        for k in damaged:
            assert np.array_equal(got[k * sc.CHUNK:(k + 1) * sc.CHUNK], plain[k * sc.CHUNK:(k + 1) * sc.CHUNK]), f"chunk {k}: an unrecoverable chunk was written"
    return got


# ------------------------------------------------------------------------------------------------------------------------------------------
# a. the decode in front of recovery: layout_decode_kernel's scan beyond 1024 chunks, checksum_verdict_kernel's blocks of 256 chunks and the count they add up

@pytest.mark.parametrize("shape", list(sc.SHAPES))
def test_intact_containers_decode_verify_and_need_no_recovery(shape):
    b = sc.built(shape)
    for blank in (False, True):
        rc, damaged, got, verdicts = verdict_file.verdict_decode(b.blob, b.data.size, blank, header=b.header)
        assert (rc, damaged) == (_lib.OK, 0) and not verdicts.any()
        assert np.array_equal(got, b.data), np.flatnonzero(got != b.data)[:8]
    version, groups = BLOB_OF[shape]
    for blank, offset, parity_offset in PLACEMENTS:
        recover_and_check(b, b.blob, sc.model_blob(shape, version, groups), (), (), blank, offset, parity_offset)


@pytest.mark.parametrize("shape", list(sc.SHAPES))
def test_three_hundred_silent_flips_are_named_exactly(shape):
    b, victims = sc.built(shape), sc.spread(shape)
    bad = b.damage(victims)
    for blank in (False, True):
        rc, damaged, got, verdicts = verdict_file.verdict_decode(bad, b.data.size, blank, header=b.header)
        same_verdicts(verdicts, expected(b.header.n_chunks, damaged=victims))
        assert (rc, damaged) == (_lib.ERR_CHECKSUM, 300), (rc, damaged)
        assert verdict_file.check_contract(b.data, sc.CHUNK, got, verdicts, blank) == set(victims)


# ------------------------------------------------------------------------------------------------------------------------------------------
# b. the blobs

@pytest.mark.parametrize("shape,version,groups", [("WIDE", 1, sc.WIDE_GROUPS), ("WIDE", 2, sc.WIDE_GROUPS), ("DEEP", 1, 2), ("DEEP", 1, 16), ("FIELD", 1, sc.FIELD_GROUPS),
                                                  ("FIELD", 2, sc.FIELD_GROUPS)])
def test_blobs_are_the_models(shape, version, groups):
    want = sc.model_blob(shape, version, groups)
    assert want.size == 32 + version * groups * sc.CHUNK and want[4] == version
    device_blob = (v1_file if version == 1 else v2_file).device_blob
    for in_offset, out_offset in ((0, 0), (7, 9)):
        got = device_blob(sc.data(shape), sc.CHUNK, groups, in_offset, out_offset)         # (checks the guard bytes around the blob)
        assert np.array_equal(got, want), (in_offset, out_offset, np.flatnonzero(got != want)[:8])


def test_groups_of_more_than_255_have_no_version_2_blob():
    import torch
    d = sc.data("DEEP")
    src, sptr = to_device(np.array(d))
    room = container.parity_size(d.size, sc.CHUNK, 16) * 2
    out = torch.full((room,), POISON, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    for groups in (2, 16):
        assert container.parity2_size(d.size, sc.CHUNK, groups) == 0
        assert _lib.lib().density_hip_parity2_device(sptr, d.size, sc.CHUNK, groups, out.data_ptr(), room, 0) == _lib.ERR_ARGUMENT
    torch.cuda.synchronize()
    assert (out.cpu().numpy() == POISON).all(), "a refused call wrote"


# ------------------------------------------------------------------------------------------------------------------------------------------
# c. recovery

@pytest.mark.parametrize("version", [2, 1])
def test_wide_groups_that_lost_one_two_and_three_members(version):
    """525 groups each have lost one member, two, and all three — on both sides of the grid's first trip and in every block of the verify kernel.  Version 2 gives
    the singles and the pairs back, version 1 the singles; what cannot come back is left as the decoder made it, counted, and named."""
    b = sc.built("WIDE")
    parity = sc.model_blob("WIDE", version, sc.WIDE_GROUPS)
    singles, pairs, triples = sc.wide_losses()
    back = sc.flat(singles, pairs) if version == 2 else sc.flat(singles)
    lost = sc.flat(triples) if version == 2 else sc.flat(pairs, triples)
    assert (len(back), len(lost)) == ((525 + 2 * 525, 3 * 525) if version == 2 else (525, 5 * 525))
    bad = b.damage(sc.flat(singles, pairs, triples))
    plain = verdict_file.verdict_decode(bad, b.data.size, False, header=b.header)[2]
    for blank, offset, parity_offset in PLACEMENTS:
        recover_and_check(b, bad, parity, back, lost, blank, offset, parity_offset, plain=plain)
    assert f"{len(lost)} of 6301 chunks damaged, {len(back)} recovered" in _lib.last_error(), _lib.last_error()
    # the same damage without the triples (version 1: and without the pairs): everything comes back
    fewer = b.damage(back)
    for blank, offset, parity_offset in PLACEMENTS:
        recover_and_check(b, fewer, parity, back, (), blank, offset, parity_offset)
    assert _lib.last_error() == ""


@pytest.mark.parametrize("case", range(len(sc.DEEP_CASES)))
def test_deep_groups(case):
    """version 1, groups of 2101 / 2100 and of 263 / 262 members: a single loss far behind the plan kernel's first trip comes back; two losses of one group — in one
    lane's two trips, in two lanes' — are counted as two and left, and the other group's single still comes back"""
    groups, lost, back = sc.DEEP_CASES[case]
    b = sc.built("DEEP")
    bad = b.damage(lost)
    plain = verdict_file.verdict_decode(bad, b.data.size, False, header=b.header)[2]
    for blank, offset, parity_offset in PLACEMENTS:
        recover_and_check(b, bad, sc.model_blob("DEEP", 1, groups), back, sorted(set(lost) - set(back)), blank, offset, parity_offset, plain=plain)


@pytest.mark.parametrize("call", range(sc.FIELD_CALLS))
def test_field_pairs_at_every_distance(call):
    """64 pairs a decode, one in each group of 255 (parity_scale_cases.field_places: the rule, held to cover every distance in test_parity_scale_cpu.py)"""
    b = sc.built("FIELD")
    pairs = sc.field_pairs(call)
    bad = b.damage(sc.flat(pairs))
    parity = sc.model_blob("FIELD", 2, sc.FIELD_GROUPS)
    for blank, offset, parity_offset in PLACEMENTS if call == sc.FIELD_CALLS - 1 else PLACEMENTS[:2]:      # (the last call has the pair with the ragged chunk)
        got = recover_and_check(b, bad, parity, sc.flat(pairs), (), blank, offset, parity_offset)
        assert np.array_equal(got, b.data)
    assert len(sc.flat(pairs)) == 128 and _lib.last_error() == ""


@pytest.mark.parametrize("version", [2, 1])
def test_asynchronous_form_counts_across_the_blocks(version):
    """Both out-pointers NULL, the caller's workspace at its advertised size with 0xA5 behind it: the counts the nine blocks of recover_verify_kernel and the 25 of
    checksum_verdict_kernel add up lie in the workspace's second and third word"""
    import torch
    b = sc.built("WIDE")
    parity = sc.model_blob("WIDE", version, sc.WIDE_GROUPS)
    singles, pairs, triples = sc.wide_losses()
    back = sc.flat(singles, pairs) if version == 2 else sc.flat(singles)
    lost = sc.flat(triples) if version == 2 else sc.flat(pairs, triples)
    need = int(_lib.lib().density_hip_decode_workspace_size_for(_lib.ALGO_IDS[sc.ALGO], b.data.size, sc.CHUNK))
    assert need > 0
    ws = torch.zeros(need + 64, dtype=torch.uint8, device="cuda")
    ws[need:] = POISON
    rc, damaged, recovered, got, verdicts = recover_decode(b.damage(sc.flat(singles, pairs, triples)), parity, b.data.size, True, header=b.header,
                                                           parity_header=container.parse_parity_header(parity), workspace=(ws.data_ptr(), need), sync=False, parity_offset=3)
    same_verdicts(verdicts, expected(b.header.n_chunks, back, lost))
    assert check_contract(b.data, sc.CHUNK, got, verdicts, True) == (set(lost), set(back))
    words = ws[:12].cpu().numpy().view(np.uint32)
    assert (int(words[1]), int(words[2])) == (len(lost), len(back)), words
    assert (ws[need:].cpu().numpy() == POISON).all(), "bytes behind the workspace written"


# ------------------------------------------------------------------------------------------------------------------------------------------
# d. the update

def updated(name, version):
    """the model's blob of the input, updated on the device by edit `name`: held to the model's blob of the edited input (update() checks the guards)"""
    shape, groups, versions, edit = sc.EDITS[name]
    after, new = sc.edited(name)
    want = sc.edited_blob(name, version)
    old = np.array(sc.data(shape)[edit[0]:edit[0] + edit[1]])
    got, hdr = update(np.array(sc.model_blob(shape, version, groups)), edit[0], old, np.array(new))
    assert got.size == want.size and np.array_equal(got, want), (name, version, np.flatnonzero(got != want)[:8])
    assert fields(hdr) == fields(container.parse_parity_header(want)) and hdr.total_len == after.size
    return got


@pytest.mark.parametrize("name,version", [(name, version) for name, case in sc.EDITS.items() for version in case[2]])
def test_updates_are_the_models_blob_of_the_edited_input(name, version):
    updated(name, version)


@pytest.mark.parametrize("name", list(sc.END_TO_END))
def test_updated_blob_recovers_a_pair_of_the_edited_input(name):
    """the end-to-end use: the version-2 blob kept by the update alone gives back two chunks of one group of a container of the EDITED input — an edited (an
    appended) chunk among them —, which the blob of the old input does not"""
    b, pair = sc.built_edited(name), sc.END_TO_END[name]
    shape, groups = sc.EDITS[name][:2]
    blob = updated(name, 2)
    bad = b.damage(pair)
    for blank in (False, True):
        recover_and_check(b, bad, blob, pair, (), blank)
    if b.data.size == sc.data(shape).size:                  # (a same-size edit: the stale blob is still a blob of this container's geometry)
        rc, damaged, recovered, got, verdicts = recover_decode(bad, sc.model_blob(shape, 2, groups), b.data.size, True, header=b.header)
        assert (rc, damaged) == (_lib.ERR_CHECKSUM, 1) and verdicts[pair[1]] == DAMAGED, "the stale blob gave the edited chunk back"
