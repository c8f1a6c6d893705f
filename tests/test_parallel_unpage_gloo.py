"""world_size-2 gloo test (CPU) of the single-container stitch over PAGED local containers: parallel.concat_to_rank0 brings a paged local container to
the packed form first (CPU tensors: container.unpage) and then stitches as ever.  The local containers are built on the CPU from oracle streams
(tests/paged_cpu.py); the stitched container must be the one-process packed container of the whole input."""
import os
import sys
import tempfile

import torch
import torch.distributed as dist
import torch.multiprocessing as mp

import datagen
from density_amd import parallel


def _worker(rank, world, initfile, total, chunk, ret):
    import paged_cpu
    from density_amd import container
    from test_parallel_gloo import cpu_container, cpu_decode_container
    dist.init_process_group("gloo", init_method=f"file://{initfile}", rank=rank, world_size=world)
    try:
        data = datagen.mixed(total, seed=5)
        c0, c1, b0, b1 = parallel.shard_chunks(total, chunk, rank, world)
        blob = paged_cpu.build(data[b0:b1], chunk)
        assert container.parse_header(blob[:32].tobytes()).flags & container.FLAG_PAGED
        local = torch.frombuffer(bytearray(blob.tobytes()), dtype=torch.uint8)
        merged = parallel.concat_to_rank0(local, chunk)
        if rank == 0:
            raw = bytes(merged.numpy())
            ret["equal_to_single_process_container"] = raw == cpu_container(data, chunk, True)
            ret["round_trip"] = cpu_decode_container(raw) == data.tobytes()
        else:
            assert merged is None
    finally:
        dist.destroy_process_group()


def test_two_rank_concat_of_paged_local_containers_matches_single_process():
    total, chunk, world = 5 * 65536 + 4321, 65536, 2
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    with tempfile.TemporaryDirectory() as d:
        mgr = mp.Manager()
        ret = mgr.dict()
        mp.spawn(_worker, args=(world, os.path.join(d, "init"), total, chunk, ret), nprocs=world, join=True)
        assert ret["equal_to_single_process_container"], "stitched container differs from the one-process packed container"
        assert ret["round_trip"]
