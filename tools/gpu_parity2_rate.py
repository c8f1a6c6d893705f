"""What double parity costs (include/density_hip.h: version 2 of the parity blob "DHP1", P rows and Q rows over GF(2^8)), on one box, same buffers:
  * density_hip_parity2_device over 1 GiB (4 MiB chunks, 16 groups) beside density_hip_parity_device over the same buffer — the same reads, twice the rows
    written: by traffic (1 + 2G/n_chunks) / (1 + G/n_chunks) = 1.059 of the time — HIP events around every call, the median of 20 after warm-up, the two
    alternating twice;
  * the recover decode of a sealed paged container of that input with the version-2 blob, by the library's profiling marks: intact, with one chunk reported
    damaged (its trailer entry flipped: rebuilt from P over the 15 other members of its group, and it stays damaged), and with two of one group (rebuilt by the
    solve over the 14 others, both rows read; both stay damaged).
python tools/gpu_parity2_rate.py [out=profiles/parity2_rate.txt]"""
import os, statistics, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import torch, datagen
from density_amd import _lib, container
out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "parity2_rate.txt")
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
p1size, p2size = container.parity_size(n, chunk, groups), container.parity2_size(n, chunk, groups)
parity1 = torch.zeros(p1size, dtype=torch.uint8, device="cuda")
parity2 = torch.zeros(p2size, dtype=torch.uint8, device="cuda")
for rep in range(2):                                      # twice, alternating: the spread between the passes says what a difference is worth
    ours = median_ms(lambda: container.parity2_device(big.data_ptr(), n, chunk, groups, parity2.data_ptr(), p2size, stream=s))
    ref = median_ms(lambda: container.parity_device(big.data_ptr(), n, chunk, groups, parity1.data_ptr(), p1size, stream=s))
    say(f"{n} B in {chunk} B chunks, {groups} groups, pass {rep}: parity2_device ({p2size} B) {ours[0]:.4f} ms (min {ours[1]:.4f}, max {ours[2]:.4f}; "
        f"{(n + p2size) / ours[0] / 1e6:.0f} GB/s read + written)   parity_device ({p1size} B) {ref[0]:.4f} ms (min {ref[1]:.4f}, max {ref[2]:.4f}; "
        f"{(n + p1size) / ref[0] / 1e6:.0f} GB/s)   ratio {ours[0] / ref[0]:.3f}   by traffic {(n + p2size) / (n + p1size):.3f}")
# the blob against the definition, on the device: the P rows are version 1's; Q row 0 folded by Horner's rule with torch's integer arithmetic
torch.cuda.synchronize()
rows = groups * chunk
say(f"P rows == the version-1 rows: {bool(torch.equal(parity2[32:32 + rows], parity1[32:32 + rows]))}")
want = torch.zeros(chunk, dtype=torch.int32, device="cuda")
for i in reversed(range(0, nc, groups)):
    want = ((want << 1) ^ ((want >> 7) * 0x11D)) ^ big[i * chunk:(i + 1) * chunk].to(torch.int32)
torch.cuda.synchronize()
say(f"Q row 0 == XOR of 2^j times its {nc // groups} chunks: {bool(torch.equal(parity2[32 + rows:32 + rows + chunk], want.to(torch.uint8)))}")
# beside the decode it follows: a sealed paged container of the same input
cap = container.container_bound_paged("chameleon", n, chunk) + container.seal_overhead(n, chunk)
cont = torch.empty(cap, dtype=torch.uint8, device="cuda"); back = torch.empty(n, dtype=torch.uint8, device="cuda")
verdicts = torch.zeros(nc, dtype=torch.int32, device="cuda")
hdr = container.encode_device_paged("chameleon", big.data_ptr(), n, cont.data_ptr(), cap, chunk, stream=s)
sealed = container.seal_device(big.data_ptr(), n, cont.data_ptr(), cap, header=hdr, stream=s)
ph = container.parse_parity_header(parity2[:32].cpu().numpy())
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
    return container.decode_device_recover(cont.data_ptr(), sealed.container_len, parity2.data_ptr(), p2size, back.data_ptr(), n, verdicts.data_ptr(), header=sealed,
                                           parity_header=ph, stream=s, blank=False, sync=sync)
t = marks(lambda: recover(False))
say(f"1 GiB paged, intact: recover decode [ms, mean of 10] {fmt(t)}   {recover(True)}, round trip == input: {bool(torch.equal(back, big))}")
trailer = sealed.container_len - (4 * nc + 15) // 16 * 16
hit = []
for k in (117, 117 + 5 * groups):                         # the second one: of the same group, five places on
    torch.cuda.synchronize()
    cont[trailer + 4 * k] ^= 0x04
    torch.cuda.synchronize()
    hit.append(k)
    t = marks(lambda: recover(False))
    say(f"1 GiB paged, trailer entries {hit} flipped: recover decode [ms, mean of 10] {fmt(t)}   {recover(True)}, verdicts {[int(verdicts[i]) for i in hit]}, "
        f"output == input (the chunks rebuilt to the bytes they had): {bool(torch.equal(back, big))}")
os.makedirs(os.path.dirname(out_path), exist_ok=True)
open(out_path, "w").write("\n".join(lines) + "\n")
