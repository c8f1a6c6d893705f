"""What the content checksum of a sealed container costs (include/density_hip.h: DENSITY_HIP_FLAG_CHECKSUM), on one box, same buffers:
  * the sum kernel over 1 GiB (4 MiB chunks) and 100 MB (384 KiB chunks) against torch.sum over the same buffer viewed as int32 — a read-only reduction
    by the vendor stack, the yardstick — HIP events around every call, the median of 20 after warm-up;
  * seal behind a paged encode and verify inside a paged decode at 1 GiB, by the library's profiling marks, beside the kernels they ride on (the encode and
    decode kernels' own times are the unsealed calls': they run first and do not know of the seal).
python tools/gpu_checksum_rate.py [out=profiles/checksum_rate.txt]"""
import os, statistics, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import torch, datagen
from density_amd import _lib, container
out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "checksum_rate.txt")
lines = []
def say(text):
    print(text, flush=True); lines.append(text)
def median_ms(fn, runs=20, warm=5):
    for _ in range(warm): fn()
    torch.cuda.synchronize()
    t = []
    for _ in range(runs):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(); fn(); b.record(); b.synchronize()
        t.append(a.elapsed_time(b))
    return statistics.median(t), min(t), max(t)
s = torch.cuda.current_stream().cuda_stream
say(_lib.lib().density_hip_version().decode())
big = torch.from_numpy(datagen.rep_text(1 << 30)).cuda()
for n, chunk in ((1 << 30, 4 << 20), (100_000_000, 384 << 10)):
    x = big[:n]
    sums = torch.zeros(-(-n // chunk), dtype=torch.int32, device="cuda")
    words = x[:n // 4 * 4].view(torch.int32)
    for rep in range(2):                                  # twice, alternating: the spread between the passes says what a difference is worth
        ours = median_ms(lambda: container.checksum_device(x.data_ptr(), n, chunk, sums.data_ptr(), stream=s))
        ref = median_ms(lambda: torch.sum(words))
        say(f"{n} B in {chunk} B chunks, pass {rep}: checksum_device {ours[0]:.4f} ms (min {ours[1]:.4f}, max {ours[2]:.4f}; {n / ours[0] / 1e6:.0f} GB/s)   "
            f"torch.sum(int32) {ref[0]:.4f} ms (min {ref[1]:.4f}, max {ref[2]:.4f}; {n / ref[0] / 1e6:.0f} GB/s)   ratio {ours[0] / ref[0]:.3f}")
# beside the container calls: paged encode + seal, paged decode + verify, 1 GiB
n, chunk = 1 << 30, 4 << 20
cap = container.container_bound_paged("chameleon", n, chunk) + container.seal_overhead(n, chunk)
cont = torch.empty(cap, dtype=torch.uint8, device="cuda"); back = torch.empty(n, dtype=torch.uint8, device="cuda")
def marks(fn, steps=10):
    for _ in range(10): fn()
    torch.cuda.synchronize(); container.set_profiling(True); container.last_timings()
    for _ in range(steps): fn()
    torch.cuda.synchronize()
    t = {}
    for nm, ms in container.last_timings(): t[nm] = t.get(nm, 0.0) + ms / steps
    container.set_profiling(False)
    return t
def encode_and_seal():
    container.encode_device_paged("chameleon", big.data_ptr(), n, cont.data_ptr(), cap, chunk, stream=s, want_header=False)
    container.seal_device(big.data_ptr(), n, cont.data_ptr(), cap, header=None, stream=s, want_header=False)
te = marks(encode_and_seal)
hdr = container.encode_device_paged("chameleon", big.data_ptr(), n, cont.data_ptr(), cap, chunk, stream=s)
tu = marks(lambda: container.decode_device(cont.data_ptr(), hdr.container_len, back.data_ptr(), n, header=hdr, stream=s, sync=False))
sealed = container.seal_device(big.data_ptr(), n, cont.data_ptr(), cap, header=hdr, stream=s)
td = marks(lambda: container.decode_device(cont.data_ptr(), sealed.container_len, back.data_ptr(), n, header=sealed, stream=s, sync=False))
ok = container.decode_device(cont.data_ptr(), sealed.container_len, back.data_ptr(), n, header=sealed, stream=s) == n and bool(torch.equal(back, big))
fmt = lambda t: ", ".join(f"{k} {v:.4f}" for k, v in t.items())
say(f"1 GiB paged, flags {sealed.flags}: encode + seal [ms] {fmt(te)}")
say(f"1 GiB paged: decode, unsealed [ms] {fmt(tu)}")
say(f"1 GiB paged: decode + verify [ms] {fmt(td)}   round trip == input: {ok}")
os.makedirs(os.path.dirname(out_path), exist_ok=True)
open(out_path, "w").write("\n".join(lines) + "\n")
