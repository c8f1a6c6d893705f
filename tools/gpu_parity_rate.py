"""What recovery records cost (include/density_hip.h: the parity blob "DHP1"), on one box, same buffers:
  * density_hip_parity_device over 1 GiB (4 MiB chunks, 16 groups) beside density_hip_checksum_device over the same buffer — the same traffic shape: the
    input read once, little written — HIP events around every call, the median of 20 after warm-up, the two alternating twice;
  * the recover decode of a sealed paged container of that input, by the library's profiling marks: intact, and with one chunk reported damaged (its trailer
    entry flipped, so the rebuild runs — over the 15 other members of its group — and the chunk stays damaged) with the blob the first part made.
python tools/gpu_parity_rate.py [out=profiles/parity_rate.txt]"""
import os, statistics, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import torch, datagen
from density_amd import _lib, container
out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "parity_rate.txt")
lines = []
def say(text):
    print(text, flush=True); lines.append(text)
def median_ms(fn, runs=20, warm=5):
    for _ in range(warm): fn()
    torch.cuda.synchronize()
    t = []
    for _ in range(runs):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(st); fn(); b.record(st); b.synchronize()
        t.append(a.elapsed_time(b))
    return statistics.median(t), min(t), max(t)
st = torch.cuda.Stream()                                  # (a stream of our own: the library takes a NULL stream — torch's default — for its internal one, which no event here would see)
s = st.cuda_stream
say(_lib.lib().density_hip_version().decode())
n, chunk, groups = 1 << 30, 4 << 20, 16
big = torch.from_numpy(datagen.rep_text(n)).cuda()
nc = -(-n // chunk)
sums = torch.zeros(nc, dtype=torch.int32, device="cuda")
psize = container.parity_size(n, chunk, groups)
parity = torch.zeros(psize, dtype=torch.uint8, device="cuda")
for rep in range(2):                                      # twice, alternating: the spread between the passes says what a difference is worth
    ours = median_ms(lambda: container.parity_device(big.data_ptr(), n, chunk, groups, parity.data_ptr(), psize, stream=s))
    ref = median_ms(lambda: container.checksum_device(big.data_ptr(), n, chunk, sums.data_ptr(), stream=s))
    say(f"{n} B in {chunk} B chunks, {groups} groups ({psize} B of parity), pass {rep}: parity_device {ours[0]:.4f} ms (min {ours[1]:.4f}, max {ours[2]:.4f}; "
        f"{(n + psize) / ours[0] / 1e6:.0f} GB/s read + written)   checksum_device {ref[0]:.4f} ms (min {ref[1]:.4f}, max {ref[2]:.4f}; {n / ref[0] / 1e6:.0f} GB/s)   "
        f"ratio {ours[0] / ref[0]:.3f}")
# the blob against the definition, on the device: row 0 is the XOR of chunks 0, 16, 32, ...
torch.cuda.synchronize()
want = torch.zeros(chunk, dtype=torch.uint8, device="cuda")
for i in range(0, nc, groups): want ^= big[i * chunk:(i + 1) * chunk]
torch.cuda.synchronize()
say(f"row 0 == XOR of its {nc // groups} chunks: {bool(torch.equal(parity[32:32 + chunk], want))}")
# beside the decode it follows: a sealed paged container of the same input
cap = container.container_bound_paged("chameleon", n, chunk) + container.seal_overhead(n, chunk)
cont = torch.empty(cap, dtype=torch.uint8, device="cuda"); back = torch.empty(n, dtype=torch.uint8, device="cuda")
verdicts = torch.zeros(nc, dtype=torch.int32, device="cuda")
hdr = container.encode_device_paged("chameleon", big.data_ptr(), n, cont.data_ptr(), cap, chunk, stream=s)
sealed = container.seal_device(big.data_ptr(), n, cont.data_ptr(), cap, header=hdr, stream=s)
ph = container.parse_parity_header(parity[:32].cpu().numpy())
def marks(fn, steps=10):
    for _ in range(5): fn()
    torch.cuda.synchronize(); container.set_profiling(True); container.last_timings()
    for _ in range(steps): fn()
    torch.cuda.synchronize()
    t = {}
    for nm, ms in container.last_timings(): t[nm] = t.get(nm, 0.0) + ms / steps
    container.set_profiling(False)
    return t
fmt = lambda t: ", ".join(f"{k} {v:.4f}" for k, v in t.items())
def recover(sync):
    return container.decode_device_recover(cont.data_ptr(), sealed.container_len, parity.data_ptr(), psize, back.data_ptr(), n, verdicts.data_ptr(), header=sealed,
                                           parity_header=ph, stream=s, blank=False, sync=sync)
t = marks(lambda: recover(False))
say(f"1 GiB paged, intact: recover decode [ms, mean of 10] {fmt(t)}   {recover(True)}, round trip == input: {bool(torch.equal(back, big))}")
k = 117
at = sealed.container_len - (4 * nc + 15) // 16 * 16 + 4 * k
torch.cuda.synchronize()
cont[at] ^= 0x04
torch.cuda.synchronize()
t = marks(lambda: recover(False))
say(f"1 GiB paged, trailer entry {k} flipped: recover decode [ms, mean of 10] {fmt(t)}   {recover(True)}, verdict {int(verdicts[k])}, "
    f"output == input (the chunk rebuilt to the bytes it had): {bool(torch.equal(back, big))}")
os.makedirs(os.path.dirname(out_path), exist_ok=True)
open(out_path, "w").write("\n".join(lines) + "\n")
