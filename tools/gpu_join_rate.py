"""What a join costs (density_hip_join_device) against the calls that move the same bytes.  1 GiB of rep-text as two halves of 512 MiB, each encoded on its own in
4 MiB Chameleon chunks — packed, and the first also paged, the second also slotted.  Measured, in ONE process and alternating: the join of the two packed
halves, the join of the paged and the slotted half, the replacement of a single chunk of the whole packed container (container.replace_chunks_device), and
beside them density_hip_slice_device of the whole packed container's window [0, n) (the same bytes through the one-source kernels), density_hip_pack_device of
each slotted-or-packed half and density_hip_unpage_device of the paged half (the same halves through the calls that move a container whole: since pack,
unpage and slice share the join's driver these run the join's layout kernel too and, but for the slotted pack's compact_kernel, its gathers).  Everything warmed
up, 20 timed repetitions each with HIP events; min / median / max, bytes written, and the ratios of the medians.  A report, not a gate.

Three steps, each a process of its own under its own `timeout`, the first failure ends the run: "check" (the joins' bytes against density_hip_encode_device of
the whole input), "rates" (the timings above), "marks" (the calls' share by the library's profiling marks).
python tools/gpu_join_rate.py [out=profiles/join_rate.txt]"""
import os, statistics, subprocess, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STEPS = {"check": 300, "rates": 420, "marks": 300}             # seconds each step may take


def drive(out_path):
    lines = []
    for step, limit in STEPS.items():
        child = subprocess.Popen(["timeout", "-k", "10", str(limit), sys.executable, os.path.abspath(__file__), "--step", step], stdout=subprocess.PIPE, text=True)
        for line in child.stdout:                              # passed on as it comes
            sys.stdout.write(line); sys.stdout.flush()
            lines.append(line)
        if child.wait() != 0:
            print(f"step {step} ended with status {child.returncode}: stopping here, nothing written", flush=True)
            return child.returncode
    os.makedirs(os.path.dirname(out_path), exist_ok=True)
    open(out_path, "w").write("".join(lines))
    return 0


def say(text):
    print(text, flush=True)


def setup():
    """the input, its two halves and whole in the forms the steps use, all on one stream of torch's"""
    sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
    import torch, datagen
    from density_amd import _lib, container
    stream = torch.cuda.Stream()                              # a stream of torch's: a null stream argument would be the library's own, which torch's events do not see
    torch.cuda.set_stream(stream)
    s = stream.cuda_stream
    n, chunk = 1 << 30, 4 << 20
    half = n // 2
    x = torch.from_numpy(datagen.rep_text(n)).cuda()

    def encoded(fn, bound, ptr, size):
        cap = bound("chameleon", size, chunk)
        cont = torch.empty(cap, dtype=torch.uint8, device="cuda")
        return cont, fn("chameleon", ptr, size, cont.data_ptr(), cap, chunk, stream=s)
    c = {"whole": encoded(container.encode_device, container.container_bound, x.data_ptr(), n),
         "a packed": encoded(container.encode_device, container.container_bound, x.data_ptr(), half),
         "b packed": encoded(container.encode_device, container.container_bound, x.data_ptr() + half, half),
         "a paged": encoded(container.encode_device_paged, container.container_bound_paged, x.data_ptr(), half),
         "b slotted": encoded(container.encode_device_slotted, container.container_bound_slotted, x.data_ptr() + half, half)}
    assert c["a paged"][1].flags & container.FLAG_PAGED and c["b slotted"][1].flags & container.FLAG_SLOTTED
    # the replacement chunk: chunk k of the input, encoded alone
    k = c["whole"][1].n_chunks // 2
    c["one"] = encoded(container.encode_device, container.container_bound, x.data_ptr() + k * chunk, chunk)
    return torch, _lib, container, s, n, chunk, c, k


def main(step):
    torch, _lib, container, s, n, chunk, c, k = setup()
    whole, hw = c["whole"]
    nc = hw.n_chunks
    cap = container.container_bound("chameleon", n, chunk)
    ws_size = max(int(_lib.lib().density_hip_decode_workspace_size(nc)), container.join_workspace_size(3, nc))
    ws = torch.empty(ws_size, dtype=torch.uint8, device="cuda")
    kw = dict(stream=s, workspace=(ws.data_ptr(), ws_size), want_header=False)
    names = ("join packed", "join mixed", "replace", "slice", "pack a", "pack b", "unpage a")
    outs = {name: torch.empty(cap, dtype=torch.uint8, device="cuda") for name in names}

    def part(key, first=0, count=None):
        t, h = c[key]
        return (t.data_ptr(), h.container_len, h, first, h.n_chunks if count is None else count)

    def mover(fn, key, out):
        t, h = c[key]
        return lambda: fn(t.data_ptr(), h.container_len, outs[out].data_ptr(), cap, header=h, **kw)
    paths = {
        "join_device(a packed, b packed)": ("join packed", lambda: container.join_device([part("a packed"), part("b packed")], outs["join packed"].data_ptr(), cap, **kw)),
        "join_device(a paged, b slotted)": ("join mixed", lambda: container.join_device([part("a paged"), part("b slotted")], outs["join mixed"].data_ptr(), cap, **kw)),
        "slice_device(whole, [0, n))": ("slice", lambda: container.slice_device(whole.data_ptr(), hw.container_len, 0, nc, outs["slice"].data_ptr(), cap, header=hw, **kw)),
        "replace_chunks_device(whole, chunk n/2)": ("replace", lambda: container.replace_chunks_device(whole.data_ptr(), hw.container_len, k, c["one"][0].data_ptr(), c["one"][1].container_len,
                                                                                                   outs["replace"].data_ptr(), cap, header=hw, new_header=c["one"][1], **kw)),
        "pack_device(a packed)": ("pack a", mover(container.pack_device, "a packed", "pack a")),
        "pack_device(b slotted)": ("pack b", mover(container.pack_device, "b slotted", "pack b")),
        "unpage_device(a paged)": ("unpage a", mover(container.unpage_device, "a paged", "unpage a")),
    }

    def length_of(out):
        return container.parse_header(bytes(out[:32].cpu().numpy())).container_len
    for _, fn in paths.values():
        for _ in range(3): fn()
    torch.cuda.synchronize()
    moved = {name: length_of(outs[out]) for name, (out, _) in paths.items()}
    if step == "check":
        say(_lib.lib().density_hip_version().decode())
        E = hw.container_len
        same = {o: bool(torch.equal(whole[:E], outs[o][:E])) for o in ("join packed", "join mixed", "replace", "slice")}
        say(f"{n} B of rep-text in {chunk} B chunks ({nc}), two halves of {n // 2} B; whole packed E = {E} B, a paged {c['a paged'][1].container_len} B, b slotted {c['b slotted'][1].container_len} B")
        say(f"identical to encode_device of the whole input: {same}")
        return 0 if all(same.values()) else 1
    if step == "rates":
        times = {name: [] for name in paths}
        for _ in range(20):
            for name, (_, fn) in paths.items():
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record(); fn(); b.record(); b.synchronize()
                times[name].append(a.elapsed_time(b))
        med = {name: statistics.median(t) for name, t in times.items()}
        for name, t in times.items():
            say(f"{name}: min {min(t):.4f} ms, median {med[name]:.4f} ms, max {max(t):.4f} ms; {moved[name]} B written ({2 * moved[name] / med[name] / 1e6:.0f} GB/s read + written)")
        say(f"ratio of the medians join(a packed, b packed) / slice [0, n): {med['join_device(a packed, b packed)'] / med['slice_device(whole, [0, n))']:.3f} (the same bytes)")
        say(f"ratio of the medians join(a packed, b packed) / (pack a + pack b): {med['join_device(a packed, b packed)'] / (med['pack_device(a packed)'] + med['pack_device(b slotted)']):.3f}")
        say(f"ratio of the medians join(a paged, b slotted) / (unpage a + pack b): {med['join_device(a paged, b slotted)'] / (med['unpage_device(a paged)'] + med['pack_device(b slotted)']):.3f}")
        say(f"ratio of the medians replace one chunk / join(a packed, b packed): {med['replace_chunks_device(whole, chunk n/2)'] / med['join_device(a packed, b packed)']:.3f} (the same bytes, three parts)")
        return 0
    # the kernels' own share, by the library's profiling marks (10 calls each)
    container.set_profiling(True); container.last_timings()
    for name, (_, fn) in paths.items():
        for _ in range(10): fn()
        torch.cuda.synchronize()
        t = {}
        for nm, ms in container.last_timings(): t[nm] = t.get(nm, 0.0) + ms / 10
        say(f"{name} marks [ms]: " + ", ".join(f"{a} {b:.4f}" for a, b in t.items()))
    container.set_profiling(False)
    return 0


if __name__ == "__main__":
    if "--step" in sys.argv:
        sys.exit(main(sys.argv[sys.argv.index("--step") + 1]))
    sys.exit(drive(sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "join_rate.txt")))
