"""What a slice costs (density_hip_slice_device) against the calls that move the same container whole: density_hip_pack_device on the PACKED container and
density_hip_unpage_device on the PAGED one.  Since pack, unpage and slice share one driver these are the SAME kernels as the slice of the window [0, n) — the
window layout, then one run of run_gather_kernel (packed) or unpage_kernel over the whole directory (paged) — under other marks, so the whole-window ratios
say what the box's repeatability is, no more (profiles/slice_rate.txt is from before: the pack was a device copy then).  One process, same box: 1 GiB of
rep-text in automatic 4 MiB chunks; per form the whole window [0, n) — the same bytes as the yardstick — and the middle half [n/4, n/4 + n/2); everything
warmed up, 20 timed repetitions each with HIP events, the paths alternating; min / median / max of each, the ratio of the medians full window / yardstick,
and the marks of the library's own profiling.  A report, not a gate.
python tools/gpu_slice_rate.py [out=profiles/slice_rate.txt]"""
import os, statistics, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import torch, datagen
from density_amd import _lib, container
out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "slice_rate.txt")
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
packed, hk = encoded(container.encode_device, container.container_bound)
paged, hp = encoded(container.encode_device_paged, container.container_bound_paged)
assert not hk.flags & (container.FLAG_SLOTTED | container.FLAG_PAGED) and hp.flags & container.FLAG_PAGED, (hk.flags, hp.flags)
nc = hk.n_chunks
cap = container.container_bound("chameleon", n, chunk)
ws_size = int(_lib.lib().density_hip_decode_workspace_size(nc))
ws = torch.empty(ws_size, dtype=torch.uint8, device="cuda")
outs = {k: torch.empty(cap, dtype=torch.uint8, device="cuda") for k in ("pack", "unpage", "slice packed", "slice paged")}
half = (nc // 4, nc // 2)
kw = dict(stream=s, workspace=(ws.data_ptr(), ws_size), want_header=False)
def slicer(cont, h, window, out):
    return lambda: container.slice_device(cont.data_ptr(), h.container_len, window[0], window[1], out.data_ptr(), cap, header=h, **kw)
paths = {
    "pack_device(packed)": lambda: container.pack_device(packed.data_ptr(), hk.container_len, outs["pack"].data_ptr(), cap, header=hk, **kw),
    "slice_device(packed, [0, n))": slicer(packed, hk, (0, nc), outs["slice packed"]),
    "unpage_device(paged)": lambda: container.unpage_device(paged.data_ptr(), hp.container_len, outs["unpage"].data_ptr(), cap, header=hp, **kw),
    "slice_device(paged, [0, n))": slicer(paged, hp, (0, nc), outs["slice paged"]),
    "slice_device(packed, middle half)": slicer(packed, hk, half, outs["slice packed"]),
    "slice_device(paged, middle half)": slicer(paged, hp, half, outs["slice paged"]),
}
def length_of(out):
    return container.parse_header(bytes(out[:32].cpu().numpy())).container_len
moved = {}
for k, fn in paths.items():                                   # (in this order: the full windows are compared before the halves overwrite their outputs)
    for _ in range(5): fn()
    torch.cuda.synchronize()
    moved[k] = length_of(outs["pack" if k.startswith("pack") else "unpage" if k.startswith("unpage") else "slice packed" if "packed" in k else "slice paged"])
    if k == "slice_device(paged, [0, n))":
        E = moved["pack_device(packed)"]
        same = all(bool(torch.equal(outs["pack"][:E], outs[o][:E])) for o in ("unpage", "slice packed", "slice paged"))
times = {k: [] for k in paths}
for _ in range(20):
    for k, fn in paths.items():
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(); fn(); b.record(); b.synchronize()
        times[k].append(a.elapsed_time(b))
say(f"{n} B of rep-text in {hk.chunk_size} B chunks ({nc}); packed E = {E} B, paged {hp.container_len} B; the four whole outputs identical: {same}; middle half: chunks [{half[0]}, {half[0] + half[1]})")
for k, t in times.items():
    say(f"{k}: min {min(t):.4f} ms, median {statistics.median(t):.4f} ms, max {max(t):.4f} ms; {moved[k]} B written ({2 * moved[k] / statistics.median(t) / 1e6:.0f} GB/s read + written)")
med = {k: statistics.median(t) for k, t in times.items()}
say(f"ratio of the medians slice [0, n) / pack_device, packed: {med['slice_device(packed, [0, n))'] / med['pack_device(packed)']:.3f} (the same bytes: expectation about 1)")
say(f"ratio of the medians slice [0, n) / unpage_device, paged: {med['slice_device(paged, [0, n))'] / med['unpage_device(paged)']:.3f} (the same bytes: expectation about 1)")
say(f"middle half / whole window: packed {med['slice_device(packed, middle half)'] / med['slice_device(packed, [0, n))']:.3f}, paged {med['slice_device(paged, middle half)'] / med['slice_device(paged, [0, n))']:.3f} (half the bytes)")
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
