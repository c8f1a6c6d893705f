"""What a join is, stated in numpy from the header's layout alone (include/density_hip.h): the chunk windows of several host-resident containers, of any
form, sealed or not, as the ONE packed container of those chunk streams in order.  Built on tests/slice_cpu.py (chunk_streams, assemble).  Test
infrastructure — the expectation tests/test_gpu_join.py holds density_hip_join_device to, itself held to the oracle in tests/test_join_cpu.py — and never
the code under test."""
import numpy as np

import slice_cpu
from slice_cpu import CHECKSUM, INDEX, up


def window_len(blob, first, count):
    """the input bytes chunks [first, first + count) of `blob` cover"""
    _, _, chunk, n, total, _ = slice_cpu.header_of(blob)
    assert first + count <= n
    return min(total, (first + count) * chunk) - first * chunk


def join_containers(parts):
    """parts = [(blob, first_chunk, chunk_count), ...] -> the packed container of their chunk streams, uint8 array of container_len bytes.  Parts with
    chunk_count == 0 are skipped.  Asserts what the call refuses: parts that differ in algorithm, chunk size, block index or seal, and a ragged chunk in
    front of the output's last."""
    live = [(np.ascontiguousarray(b, dtype=np.uint8).reshape(-1), f, c) for b, f, c in parts if c]
    assert live
    algo, flags, chunk = slice_cpu.header_of(live[0][0])[:3]
    common = flags & (INDEX | CHECKSUM)
    streams, index, sums, total = [], b"", [], 0
    for src, first, count in live:
        a, fl, ch, n, tot, clen = slice_cpu.header_of(src)
        assert (a, ch, fl & (INDEX | CHECKSUM)) == (algo, chunk, common) and count >= 1 and first + count <= n and clen <= src.size
        assert total % chunk == 0, "a ragged chunk may only be the output's last"
        length = window_len(src, first, count)
        streams += slice_cpu.chunk_streams(src, range(first, first + count))
        if common & INDEX:
            ix0 = up(32 + 4 * n, 16)
            index += src[ix0 + first * chunk // 256:][:(length + 255) // 256].tobytes()
        if common & CHECKSUM:
            t = clen - up(4 * n, 16)
            sums += src[t + 4 * first:t + 4 * (first + count)].view("<u4").tolist()
        total += length
    return slice_cpu.assemble(algo, chunk, total, streams, index if common & INDEX else None, sums if common & CHECKSUM else None)
