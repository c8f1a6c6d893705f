"""What verdicts and salvage cost (include/density_hip.h: density_hip_decode_device_verdicts), on one box, in one process, same buffers, the sealed paged
1 GiB container of the headline (4 MiB chunks):
  * intact container: the verdict call (no blanking, and with it) against density_hip_decode_device of a BASELINE library — another build of
    libdensity_hip.so given on the command line (the commit before this feature), or, without one, this library's own density_hip_decode_device, whose code
    the feature does not touch — 20 repetitions each, interleaved, HIP events around every call: medians and the spread of each;
  * blanking: the "blank_chunks" mark with one damaged chunk and with all 256 (a trailer entry flipped per damaged chunk), beside hipMemsetAsync over the
    same 1 GiB in the same run, the reference for a fill.
One GPU process, no retry: run it under a time limit of its own.
python tools/gpu_verdicts_rate.py [out=profiles/verdicts_rate.txt] [baseline=path/to/another/libdensity_hip.so]"""
import ctypes, os, statistics, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import torch, datagen
from density_amd import _lib, container
out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "verdicts_rate.txt")
baseline_path = sys.argv[2] if len(sys.argv) > 2 else None
lines = []
def say(text):
    print(text, flush=True); lines.append(text)
def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record(); fn(); b.record(); b.synchronize()
    return a.elapsed_time(b)
def spread(t):
    return f"median {statistics.median(t):.4f} ms (min {min(t):.4f}, max {max(t):.4f})"
side = torch.cuda.Stream()                                 # (a stream of its own: the default stream's handle is NULL, which the library reads as ITS stream, not the events')
torch.cuda.set_stream(side)
s = side.cuda_stream
assert s != 0
L = _lib.lib()
say(L.density_hip_version().decode())
if baseline_path:
    B = ctypes.CDLL(baseline_path)
    B.density_hip_version.restype = ctypes.c_char_p
    B.density_hip_decode_device.restype, B.density_hip_decode_device.argtypes = _lib.SYMBOLS["density_hip_decode_device"]
    say(f"baseline: {B.density_hip_version().decode()} ({os.path.basename(baseline_path)})")
else:
    B = L
    say("baseline: this library's own density_hip_decode_device")
n, chunk = 1 << 30, 4 << 20
big = torch.from_numpy(datagen.rep_text(n)).cuda()
cap = container.container_bound_paged("chameleon", n, chunk) + container.seal_overhead(n, chunk)
cont = torch.empty(cap, dtype=torch.uint8, device="cuda"); back = torch.empty(n, dtype=torch.uint8, device="cuda")
hdr = container.encode_device_paged("chameleon", big.data_ptr(), n, cont.data_ptr(), cap, chunk, stream=s)
sealed = container.seal_device(big.data_ptr(), n, cont.data_ptr(), cap, header=hdr, stream=s)
assert sealed.flags & container.FLAG_PAGED and sealed.flags & container.FLAG_CHECKSUM
nc = sealed.n_chunks
verdicts = torch.zeros(nc, dtype=torch.int32, device="cuda")
def base():
    assert B.density_hip_decode_device(cont.data_ptr(), sealed.container_len, ctypes.byref(sealed), back.data_ptr(), n, None, 0, s, None) == 0
def verdict(blank):
    return lambda: container.decode_device_verdicts(cont.data_ptr(), sealed.container_len, back.data_ptr(), n, verdicts.data_ptr(), header=sealed, stream=s, blank=blank, sync=False)
legs = {"decode_device (baseline)": base, "decode_device_verdicts": verdict(False), "decode_device_verdicts + blank": verdict(True)}
for _ in range(5):
    for fn in legs.values(): fn()
torch.cuda.synchronize()
times = {k: [] for k in legs}
for _ in range(20):                                        # interleaved: whatever drifts, drifts for all three
    for k, fn in legs.items(): times[k].append(timed(fn))
for k, t in times.items():
    say(f"intact, 1 GiB paged, {nc} chunks: {k}: {spread(t)}")
d = statistics.median(times["decode_device_verdicts"]) - statistics.median(times["decode_device (baseline)"])
say(f"difference of the medians, verdicts - baseline: {d:+.4f} ms; the baseline's own spread: {max(times['decode_device (baseline)']) - min(times['decode_device (baseline)']):.4f} ms")
rc, damaged = container.decode_device_verdicts(cont.data_ptr(), sealed.container_len, back.data_ptr(), n, verdicts.data_ptr(), header=sealed, stream=s)
say(f"intact: return code {rc}, damaged {damaged}, round trip == input: {bool(torch.equal(back, big))}")
# blanking: by the library's marks
def marks(fn, steps=10):
    for _ in range(3): fn()
    torch.cuda.synchronize(); container.set_profiling(True); container.last_timings()
    for _ in range(steps): fn()
    torch.cuda.synchronize()
    t = {}
    for nm, ms in container.last_timings(): t.setdefault(nm, []).append(ms)
    container.set_profiling(False)
    return t
fmt = lambda t: ", ".join(f"{k} {statistics.median(v):.4f}" for k, v in t.items())
say(f"intact, marks [ms, median of 10]: {fmt(marks(verdict(True)))}")
trailer = sealed.container_len - (4 * nc + 15) // 16 * 16
for what, hit in (("one chunk damaged", [nc // 2]), (f"all {nc} chunks damaged", list(range(nc)))):
    for i in hit: cont[trailer + 4 * i] ^= 1
    torch.cuda.synchronize()
    t = marks(verdict(True))
    rc, damaged = container.decode_device_verdicts(cont.data_ptr(), sealed.container_len, back.data_ptr(), n, verdicts.data_ptr(), header=sealed, stream=s)
    zeros = sum(int(not back[i * chunk:(i + 1) * chunk].any()) for i in hit)
    say(f"{what} (trailer entries flipped): return code {rc}, damaged {damaged}, blanked regions all zero: {zeros} of {len(hit)}; marks [ms, median of 10]: {fmt(t)}   "
        f"blank_chunks: {spread(t['blank_chunks'])}, {len(hit) * chunk / statistics.median(t['blank_chunks']) / 1e6:.0f} GB/s")
    for i in hit: cont[trailer + 4 * i] ^= 1
    torch.cuda.synchronize()
hip = ctypes.CDLL("libamdhip64.so")
hip.hipMemsetAsync.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_size_t, ctypes.c_void_p]
def fill():
    assert hip.hipMemsetAsync(back.data_ptr(), 0, n, s) == 0
for _ in range(5): fill()
t = [timed(fill) for _ in range(20)]
say(f"hipMemsetAsync over 1 GiB: {spread(t)}, {n / statistics.median(t) / 1e6:.0f} GB/s")
os.makedirs(os.path.dirname(out_path), exist_ok=True)
open(out_path, "w").write("\n".join(lines) + "\n")
