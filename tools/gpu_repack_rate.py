"""The calls that bring a container to the packed form whole, this tree's library against ANOTHER build of the library (the yardstick: the parent commit's
libdensity_hip.so, built elsewhere and named on the command line).  Since pack, unpage and slice share one driver the three calls run the same kernels —
window_layout_kernel, then run_gather_kernel (packed: one run; slotted: a run per chunk) or unpage_kernel (paged) —, where the yardstick's pack ran
layout_decode / layout_encode and a device copy (packed) or compact_kernel (slotted).  One process, both libraries loaded, same box, same buffers: 1 GiB of
rep-text in automatic 4 MiB chunks; density_hip_pack_device of the PACKED and of the SLOTTED container, density_hip_unpage_device of the PAGED one;
everything warmed up; per call 20 timed repetitions of each library with HIP events, the yardstick first and the two alternating (so each follows a run of
the other over the same source); min / median / max of each, the marks of the libraries' own profiling taken the same way, and whether the tree's median
lies within the yardstick's own max - min.  The outputs of the two libraries are compared whole.
python tools/gpu_repack_rate.py path/to/the/other/libdensity_hip.so [out=profiles/repack_rate.txt]"""
import ctypes, os, statistics, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import torch, datagen
from density_amd import _lib, container
other_path = sys.argv[1]
out_path = sys.argv[2] if len(sys.argv) > 2 else os.path.join(ROOT, "profiles", "repack_rate.txt")
lines = []
def say(text):
    print(text, flush=True); lines.append(text)
def load(path):
    L = ctypes.CDLL(path)
    for name, (res, args) in _lib.SYMBOLS.items():
        fn = getattr(L, name)
        fn.restype, fn.argtypes = res, args
    return L
libs = {"parent": load(other_path), "tree": _lib.lib()}
def use(which):                                               # container.* asks _lib.lib() at every call
    _lib._lib = libs[which]
stream = torch.cuda.Stream()                                  # a stream of torch's: a null stream argument would be the library's own, which torch's events do not see
torch.cuda.set_stream(stream)
s = stream.cuda_stream
for which in libs:
    say(f"{which}: {libs[which].density_hip_version().decode()}")
n, chunk = 1 << 30, 0
x = torch.from_numpy(datagen.rep_text(n)).cuda()
def encoded(fn, bound):
    cap = bound("chameleon", n, chunk)
    cont = torch.empty(cap, dtype=torch.uint8, device="cuda")
    return cont, fn("chameleon", x.data_ptr(), n, cont.data_ptr(), cap, chunk, stream=s)
use("tree")
sources = {"packed": encoded(container.encode_device, container.container_bound), "slotted": encoded(container.encode_device_slotted, container.container_bound_slotted),
           "paged": encoded(container.encode_device_paged, container.container_bound_paged)}
assert sources["slotted"][1].flags & container.FLAG_SLOTTED and sources["paged"][1].flags & container.FLAG_PAGED
cap = container.container_bound("chameleon", n, chunk)
ws_size = int(_lib.lib().density_hip_decode_workspace_size(sources["packed"][1].n_chunks))
ws = torch.empty(ws_size, dtype=torch.uint8, device="cuda")
outs = {(which, form): torch.empty(cap, dtype=torch.uint8, device="cuda") for which in libs for form in sources}
def mover(which, form):
    cont, h = sources[form]
    call = container.unpage_device if form == "paged" else container.pack_device
    def fn():
        use(which)
        call(cont.data_ptr(), h.container_len, outs[(which, form)].data_ptr(), cap, header=h, stream=s, workspace=(ws.data_ptr(), ws_size), want_header=False)
    return fn
name = lambda form: ("unpage_device" if form == "paged" else "pack_device") + f"({form})"
paths = {(form, which): mover(which, form) for form in sources for which in libs}      # per form: the parent, then the tree
for fn in paths.values():
    for _ in range(5): fn()
torch.cuda.synchronize()
E = container.parse_header(bytes(outs[("tree", "packed")][:32].cpu().numpy())).container_len
same = all(bool(torch.equal(outs[("tree", "packed")][:E], o[:E])) for o in outs.values())
times = {k: [] for k in paths}
for form in sources:
    for _ in range(20):
        for which in libs:
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record(); paths[(form, which)](); b.record(); b.synchronize()
            times[(form, which)].append(a.elapsed_time(b))
say(f"{n} B of rep-text in {sources['packed'][1].chunk_size} B chunks ({sources['packed'][1].n_chunks}); packed E = {E} B; the six outputs (three calls, two libraries) identical: {same}")
for (form, which), t in times.items():
    say(f"{name(form)}, {which}: min {min(t):.4f} ms, median {statistics.median(t):.4f} ms, max {max(t):.4f} ms ({2 * E / statistics.median(t) / 1e6:.0f} GB/s read + written)")
for form in sources:
    p, t = times[(form, "parent")], times[(form, "tree")]
    d, spread = statistics.median(t) - statistics.median(p), max(p) - min(p)
    say(f"{name(form)}: tree / parent {statistics.median(t) / statistics.median(p):.3f}; median tree - median parent {d:+.4f} ms, the parent's own max - min {spread:.4f} ms: {'within' if d <= spread else 'OUTSIDE'}")
# the kernels' own share, by the libraries' profiling marks: 20 calls each, alternating as above, the median of every mark
marks = {k: {} for k in paths}
for which in libs:
    use(which); container.set_profiling(True); container.last_timings()
for form in sources:
    for _ in range(20):
        for which in libs:
            paths[(form, which)]()
            torch.cuda.synchronize()
            for nm, ms in container.last_timings(): marks[(form, which)].setdefault(nm, []).append(ms)
for which in libs:
    use(which); container.set_profiling(False)
for k, t in marks.items():
    say(f"{name(k[0])}, {k[1]} marks [ms], median (min - max): " + ", ".join(f"{a} {statistics.median(b):.4f} ({min(b):.4f} - {max(b):.4f})" for a, b in t.items()))
for form in sources:
    for mark in marks[(form, "parent")]:
        p, t = marks[(form, "parent")][mark], marks[(form, "tree")][mark]
        d, spread = statistics.median(t) - statistics.median(p), max(p) - min(p)
        say(f"{name(form)} {mark}: median tree - median parent {d:+.4f} ms, the parent's own max - min {spread:.4f} ms: {'within' if d <= spread else 'OUTSIDE'}")
os.makedirs(os.path.dirname(out_path), exist_ok=True)
open(out_path, "w").write("\n".join(lines) + "\n")
