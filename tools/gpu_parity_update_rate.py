"""What keeping a parity blob current costs (include/density_hip.h: density_hip_parity_update_device) beside what a caller did before it existed — a new blob of
the whole edited input —, on one box, same buffers: 1 GiB, 4 MiB chunks, 16 groups, versions 1 and 2 of the blob:
  (a) one chunk replaced: density_hip_parity_update_device with the chunk's old and new bytes.  Bytes moved: old + new + the touched row read and written, once per
      row kind — 16 MiB (24 MiB) against the 1 GiB + blob of (c): by traffic about 1/64 (1/47);
  (b) 64 MiB appended: the new bytes + all sixteen rows read and written, once per row kind;
  (c) density_hip_parity_device / density_hip_parity2_device over the whole edited input: the baseline.
The ratios of bytes are derived, not measured; the times are stated as they come: HIP events around every call, the median of 20 after warm-up.  (Repeated
updates of one blob with the same host header XOR the same delta in and out again: the same work every time.)  Each update is checked once against the blob
the full pass makes of the edited input.
python tools/gpu_parity_update_rate.py [out=profiles/parity_update_rate.txt]"""
import os, statistics, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import torch, datagen
from density_amd import _lib, container
out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "parity_update_rate.txt")
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
say("(the updates' working sets — 16 to 320 MiB, the same buffers every repetition — lie at or near the 256 MiB Infinity Cache, the full pass's 1 GiB does not: the updates' "
    "times are those of a warm cache, and (a) is mostly the launch)")
n, chunk, groups, extra, k = 1 << 30, 4 << 20, 16, 64 << 20, 117
big = torch.from_numpy(datagen.rep_text(n + extra)).cuda()               # the input, and behind it what (b) appends
patch = torch.from_numpy(datagen.rep_text(chunk, seed=99)).cuda()        # chunk k's new bytes
old = big[k * chunk:(k + 1) * chunk].clone()
MIB = float(1 << 20)
for version, size_of, full in ((1, container.parity_size, container.parity_device), (2, container.parity2_size, container.parity2_device)):
    size = size_of(n, chunk, groups)
    assert size == size_of(n + extra, chunk, groups)
    blob, fresh = torch.zeros(size, dtype=torch.uint8, device="cuda"), torch.zeros(size, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    full(big.data_ptr(), n, chunk, groups, blob.data_ptr(), size, stream=s)
    st.synchronize()
    ph = container.parse_parity_header(blob[:32].cpu().numpy())
    replace = lambda: container.parity_update_device(blob.data_ptr(), size, k * chunk, old.data_ptr(), chunk, patch.data_ptr(), chunk, parity_header=ph, stream=s, want_header=False)
    append = lambda: container.parity_update_device(blob.data_ptr(), size, n, 0, 0, big.data_ptr() + n, extra, parity_header=ph, stream=s, want_header=False)
    # each once, against the full pass over the edited input
    replace(); st.synchronize()
    big[k * chunk:(k + 1) * chunk] = patch
    torch.cuda.synchronize()
    full(big.data_ptr(), n, chunk, groups, fresh.data_ptr(), size, stream=s); st.synchronize()
    say(f"version {version}: chunk {k} replaced, updated blob == the blob of the edited input: {bool(torch.equal(blob, fresh))}")
    big[k * chunk:(k + 1) * chunk] = old
    torch.cuda.synchronize()
    replace(); st.synchronize()                                        # (and back: the blob of the input again)
    append(); st.synchronize()
    full(big.data_ptr(), n + extra, chunk, groups, fresh.data_ptr(), size, stream=s); st.synchronize()
    say(f"version {version}: {extra} B appended, updated blob == the blob of the edited input: {bool(torch.equal(blob, fresh))}")
    for rep in range(2):                                               # twice, alternating: the spread between the passes says what a difference is worth
        a = median_ms(replace)
        b = median_ms(append)
        c_a = median_ms(lambda: full(big.data_ptr(), n, chunk, groups, fresh.data_ptr(), size, stream=s))
        c_b = median_ms(lambda: full(big.data_ptr(), n + extra, chunk, groups, fresh.data_ptr(), size, stream=s))
        bytes_a, bytes_b = 2 * chunk + 2 * version * chunk, extra + 2 * version * groups * chunk
        say(f"version {version}, {n} B in {chunk} B chunks, {groups} groups, blob {size} B, pass {rep}:")
        say(f"  (a) replace one chunk: parity_update {a[0]:.4f} ms (min {a[1]:.4f}, max {a[2]:.4f}); expected traffic {bytes_a / MIB:.0f} MiB = old + new + 2 x {version} row(s)")
        say(f"  (c) full pass over {n} B: {c_a[0]:.4f} ms (min {c_a[1]:.4f}, max {c_a[2]:.4f}); traffic {(n + size) / MIB:.0f} MiB; by traffic (a)/(c) = 1/{(n + size) / bytes_a:.1f}, "
            f"measured (a)/(c) = 1/{c_a[0] / a[0]:.1f}")
        say(f"  (b) append {extra} B: parity_update {b[0]:.4f} ms (min {b[1]:.4f}, max {b[2]:.4f}); expected traffic {bytes_b / MIB:.0f} MiB = new + 2 x {version} x {groups} rows")
        say(f"  (c) full pass over {n + extra} B: {c_b[0]:.4f} ms (min {c_b[1]:.4f}, max {c_b[2]:.4f}); traffic {(n + extra + size) / MIB:.0f} MiB; by traffic (b)/(c) = "
            f"1/{(n + extra + size) / bytes_b:.1f}, measured (b)/(c) = 1/{c_b[0] / b[0]:.1f}")
    del blob, fresh
os.makedirs(os.path.dirname(out_path), exist_ok=True)
open(out_path, "w").write("\n".join(lines) + "\n")
