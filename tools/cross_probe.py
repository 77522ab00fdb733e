"""tools/cross_probe.py (GPU box): time of the feature-cross kernels at B = 65 536 -- a 2-key and a 3-key one-hot cross, four crosses in one
launch against four single launches, a ragged 3 x 3 cross -- each beside a plain device copy of the bytes the transform moves
(8 * (keys + 1) per sample for the one-hot form), on the same box in the same run.  Two times per case: "eager" = device events around n
calls through ops (the host's enqueue is part of it), "graph" = the same calls captured once and replayed (the device's time alone)."""
import sys

import torch

sys.path.insert(0, ".")
import dir_amd  # noqa: E402
from dir_amd import ops  # noqa: E402

dir_amd.load_library()
gen = torch.Generator(device="cuda").manual_seed(3)
B = 65536
I64 = torch.iinfo(torch.int64)


def us(fn, n=200):
    for _ in range(10):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / n


def graphed(fn, reps=20):
    """fn captured `reps` times in one graph -> a function replaying it; its time / reps is the device's time per call."""
    fn()
    g, side = torch.cuda.CUDAGraph(), torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        with torch.cuda.graph(g, stream=side):
            for _ in range(reps):
                fn()
    torch.cuda.current_stream().wait_stream(side)
    return g.replay, reps


def report(name, fn, nbytes):
    src = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
    dst = torch.empty_like(src)
    copy = lambda: dst.copy_(src)
    rows = []
    for f in (fn, copy):
        eager = us(f)
        replay, reps = graphed(f)
        rows.append((eager, us(replay, 50) / reps))
    (te, tg), (ce, cg) = rows
    print("%-34s %8.2f MB | eager %6.1f us (copy %6.1f, x%.2f) | graph %6.2f us (copy %6.2f, x%.2f)"
          % (name, nbytes / 1e6, te, ce, te / ce, tg, cg, tg / cg))
    return te, tg


cols = [torch.randint(-(1 << 62), 1 << 62, (B,), generator=gen, device="cuda") for _ in range(8)]
out1 = torch.empty((1, B), dtype=torch.int64, device="cuda")
out4 = torch.empty((4, B), dtype=torch.int64, device="cuda")

report("one-hot, 2 keys", lambda: ops.cross_hash(cols[:2], [([0, 1], 128)], out=out1), 8 * 3 * B)
report("one-hot, 3 keys", lambda: ops.cross_hash(cols[:3], [([0, 1, 2], 128)], out=out1), 8 * 4 * B)
four = [([0, 1], 128), ([1, 2], 1000), ([2, 3, 0], 1 << 20), ([3, 1], 50)]
one = report("4 crosses, one launch (4 sources)", lambda: ops.cross_hash(cols[:4], four, out=out4), 8 * (4 + 4) * B)


def singles():
    for x, c in enumerate(four):
        ops.cross_hash(cols[:4], [c], out=out4[x:x + 1])


sep = report("4 crosses, four launches", singles, 8 * (9 + 4) * B)
print("one launch / four launches: eager x%.2f, graph x%.2f" % (one[0] / sep[0], one[1] / sep[1]))

lens = torch.full((B,), 3, dtype=torch.int64, device="cuda")
offs = torch.cat([torch.zeros(1, dtype=torch.int64, device="cuda"), torch.cumsum(lens, 0)])
ra = (torch.randint(-(1 << 62), 1 << 62, (3 * B,), generator=gen, device="cuda"), offs)
rb = (torch.randint(-(1 << 62), 1 << 62, (3 * B,), generator=gen, device="cuda"), offs)
vals, _ = ops.cross_hash_ragged([ra, rb], 128)
assert vals.numel() == 9 * B
# values 2 x 3 in, offsets 2 x (B+1) in, counts + offsets out, 9 ids out per sample
nbytes = 8 * (6 + 2 + 2 + 9) * B
src = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
dst = torch.empty_like(src)
t = us(lambda: ops.cross_hash_ragged([ra, rb], 128), 100)
tk = us(lambda: ops.cross_hash_ragged([ra, rb], 128, capacity=9 * B, out=vals), 100)
c = us(lambda: dst.copy_(src), 100)
print("%-34s %8.2f MB | eager %6.1f us with the size read-back, %6.1f us with a known capacity (copy %6.1f, x%.2f / x%.2f)"
      % ("ragged 3 x 3 (count, cumsum, fill)", nbytes / 1e6, t, tk, c, t / c, tk / c))
