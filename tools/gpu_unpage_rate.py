"""What bringing a PAGED container to the packed wire form costs (density_hip_unpage_device) against the yardstick that moves the same bytes: density_hip_pack_device
on the SLOTTED container of the same input (compact_kernel: E bytes read, E bytes written).  Pack, unpage and slice share one driver: the two calls differ
in their gather kernel alone, layout and trailer are the same kernels.  One process, same box: 1 GiB of rep-text in automatic 4 MiB
chunks, both paths warmed up, 20 timed repetitions each with HIP events, alternating the two; min / median / max of each and the ratio of the medians.
python tools/gpu_unpage_rate.py [out=profiles/unpage_rate.txt]"""
import os, statistics, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import torch, datagen
from density_amd import _lib, container
out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "unpage_rate.txt")
lines = []
def say(text):
    print(text, flush=True); lines.append(text)
stream = torch.cuda.Stream()                                  # a stream of torch's: a null stream argument would be the library's own, which torch's events do not see
torch.cuda.set_stream(stream)
s = stream.cuda_stream
say(_lib.lib().density_hip_version().decode())
n, chunk = 1 << 30, 0
x = torch.from_numpy(datagen.rep_text(n)).cuda()
def encoded(fn, bound):
    cap = bound("chameleon", n, chunk)
    cont = torch.empty(cap, dtype=torch.uint8, device="cuda")
    return cont, fn("chameleon", x.data_ptr(), n, cont.data_ptr(), cap, chunk, stream=s)
slotted, hs = encoded(container.encode_device_slotted, container.container_bound_slotted)
paged, hp = encoded(container.encode_device_paged, container.container_bound_paged)
assert hs.flags & container.FLAG_SLOTTED and hp.flags & container.FLAG_PAGED, (hs.flags, hp.flags)
cap = container.container_bound("chameleon", n, chunk)
ws_size = int(_lib.lib().density_hip_decode_workspace_size(hs.n_chunks))
ws = torch.empty(ws_size, dtype=torch.uint8, device="cuda")
out_pack = torch.empty(cap, dtype=torch.uint8, device="cuda"); out_unpage = torch.empty(cap, dtype=torch.uint8, device="cuda")
paths = {
    "pack_device(slotted)": lambda: container.pack_device(slotted.data_ptr(), hs.container_len, out_pack.data_ptr(), cap, header=hs, stream=s, workspace=(ws.data_ptr(), ws_size), want_header=False),
    "unpage_device(paged)": lambda: container.unpage_device(paged.data_ptr(), hp.container_len, out_unpage.data_ptr(), cap, header=hp, stream=s, workspace=(ws.data_ptr(), ws_size), want_header=False),
}
for _ in range(5):
    for fn in paths.values(): fn()
torch.cuda.synchronize()
E = container.parse_header(bytes(out_pack[:32].cpu().numpy())).container_len
same = bool(torch.equal(out_pack[:E], out_unpage[:E]))
times = {k: [] for k in paths}
for _ in range(20):
    for k, fn in paths.items():
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(); fn(); b.record(); b.synchronize()
        times[k].append(a.elapsed_time(b))
say(f"{n} B of rep-text in {hs.chunk_size} B chunks ({hs.n_chunks}); slotted {hs.container_len} B, paged {hp.container_len} B, packed E = {E} B; the two outputs identical: {same}")
for k, t in times.items():
    say(f"{k}: min {min(t):.4f} ms, median {statistics.median(t):.4f} ms, max {max(t):.4f} ms ({2 * E / statistics.median(t) / 1e6:.0f} GB/s of 2E)")
ratio = statistics.median(times["unpage_device(paged)"]) / statistics.median(times["pack_device(slotted)"])
say(f"ratio of the medians unpage / pack: {ratio:.3f} (expectation: at most 1.25)")
# the kernels' own share, by the library's profiling marks (10 calls each)
container.set_profiling(True); container.last_timings()
for k, fn in paths.items():
    for _ in range(10): fn()
    torch.cuda.synchronize()
    t = {}
    for nm, ms in container.last_timings(): t[nm] = t.get(nm, 0.0) + ms / 10
    say(f"{k} marks [ms]: " + ", ".join(f"{a} {b:.4f}" for a, b in t.items()))
container.set_profiling(False)
os.makedirs(os.path.dirname(out_path), exist_ok=True)
open(out_path, "w").write("\n".join(lines) + "\n")
