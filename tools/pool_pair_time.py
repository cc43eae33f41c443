"""times ph_pool_depth_pair against the two depth-only ph_pool_counts launches it replaces, each alone on the GPU, at one part of
the headline step (32 frames, N = 153, 128 x 256, nsplit 8, bf16 planes), alternating in one process with HIP events; checks that
the sums and counts agree bit for bit first.
usage: python tools/pool_pair_time.py [frames = 32] [nsplit = 8] [rounds = 9] [reps per round = 10] [mask density in percent = 50]
(masks of independent random bits; 0 / 100: every lookup of a mask byte's A fragment reads the same table entry)"""
import statistics
import sys

import torch

sys.path.insert(0, ".")
from polyphonicformer_amd import _lib, engine as E

dev = torch.device("cuda:0")
B, ns, rounds, reps, density = (int(a) for a in (sys.argv[1:] + ["32", "8", "9", "10", "50"][len(sys.argv) - 1:]))
N, HW, prec = 153, 128 * 256, _lib.PH_PREC_BF16
Npad = E.n_padded(N)
dp = torch.randint(-2**15, 2**15, (1, B, 256, HW), dtype=torch.int16, device=dev) & 0x3BFF      # finite in bf16
bits = [E.binarize(torch.rand((B, N, 128, 256), device=dev) - (1 - density / 100)) for _ in range(2)]
new = lambda: [(torch.zeros((B, ns, Npad, 512), device=dev), torch.zeros((B, ns, Npad), dtype=torch.int32, device=dev)) for _ in range(2)]
two, one = new(), new()


def run_two():
    for (part, cnt), b in zip(two, bits):
        E.pool_depth_only(dp, b, N, HW, prec, part, cnt)


def run_pair():
    E.pool_depth_pair(dp, bits[0], bits[1], N, HW, prec, one[0][0], one[1][0], one[0][1], one[1][1])


def timed(fn):
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    ev[0].record()
    for _ in range(reps):
        fn()
    ev[1].record()
    torch.cuda.synchronize()
    return ev[0].elapsed_time(ev[1]) * 1e3 / reps


run_two(), run_pair()
torch.cuda.synchronize()
same = all(torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) for a, b in zip(two, one))
print(f"B={B} N={N} HW={HW} nsplit={ns} bf16 planes, {density} % of the mask bits set: sums and counts of both sets bit-identical: {same}")
assert same
t2, t1 = [], []
for _ in range(rounds):
    t2.append(timed(run_two))
    t1.append(timed(run_pair))
m2, m1 = statistics.median(t2), statistics.median(t1)
read = B * 256 * HW * 2 / 1e6
print(f"two depth-only ph_pool_counts launches: median {m2:.1f} us (min {min(t2):.1f}, max {max(t2):.1f}), {2 * read:.0f} MB of features read")
print(f"one ph_pool_depth_pair launch         : median {m1:.1f} us (min {min(t1):.1f}, max {max(t1):.1f}), {read:.0f} MB of features read")
print(f"paired / two = {m1 / m2:.3f}")
