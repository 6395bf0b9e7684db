"""Measurement aid: wall time of cnf2_sweep_place with Q = 16 and Q = 64 candidates (sums only, device outputs) against
cnf2_sweep with dosage rows and cnf2_sweep_accumulate without rows -- the two calls the placement's launches are made of,
neither of which this feature changes -- in the same process on the same box, alternating, best of `repeats`.  Synthetic F2
(synth.make_f2); config 2 of BASELINE: 10 000 individuals x 20 chromosomes x 2 500 SNPs (+1 dummy marker each).  The
candidates are every (M // Q)-th column of the map itself.  Also prints the contraction's arithmetic (2 x 512 flops per
individual x marker x candidate, and what the 16 x 32 tiles of place_rows_kernel issue with their masked edges) and the
bytes of state posteriors a pass writes and reads, from the shapes; the kernels' own times come from a rocprofv3
--kernel-trace --stats run of this script.
usage: python tools/place_timing.py [individuals=10000] [snps_per_chrom=2500] [chroms=20] [repeats=3]"""
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
from cnf2freq_amd import capi, synth

a = [int(x) for x in sys.argv[1:]] + [10000, 2500, 20, 3][len(sys.argv) - 1:]
n, snps, chroms, reps = a[:4]
t0 = time.perf_counter()
ped = synth.make_f2(n, snps, chroms, seed=2)
gen_s = time.perf_counter() - t0
ctx = capi.Context(0)
ctx.upload(ped)
M, dev = ped.n_markers, torch.device("cuda", 0)
QS = (16, 64)
f = torch.empty((n, chroms, 8), dtype=torch.float64, device=dev)
ll = torch.empty((n, chroms), dtype=torch.float64, device=dev)
ll2 = torch.empty_like(ll)
dos = torch.empty((n, M, 3), dtype=torch.float64, device=dev)
ps = torch.empty((max(QS), M), dtype=torch.float64, device=dev)
nz = torch.empty((max(QS), M), dtype=torch.int32, device=dev)
nul = torch.empty(max(QS), dtype=torch.float64, device=dev)
cnt = torch.empty(chroms, dtype=torch.int32, device=dev)
desc = np.ones(ped.n_rec, np.int32)
cand = {}
for Q in QS:
    cols = np.arange(Q) * (M // Q)
    cand[Q] = (np.ascontiguousarray(ped.allele[:, cols]), np.ascontiguousarray(ped.sure[:, cols]))
kernel_ms = {}


def plain():
    ctx.sweep_device(0, n, f.data_ptr(), ll.data_ptr(), dos.data_ptr(), 0)
    ctx.sync()


def acc():
    ctx.sweep_accumulate_keep(desc)          # no rows asked for, accumulators kept in the context: nothing is copied
    ctx.sync()


SWEEP_LIKELIHOODS, OWN_LIKELIHOODS = 1 << 30, 1 << 29     # cnf2_sweep_place's internal A/B flags (cnf2_capi.hip)
f2 = torch.empty_like(f)


def placer(Q, flags=0, fo=None, key=None):
    def run():
        ca, cs = cand[Q]
        ctx.sweep_place_device(ca, cs, None, 0, n, (f if fo is None else fo).data_ptr(), ll2.data_ptr(), None, ps.data_ptr(),
                               nz.data_ptr(), nul.data_ptr(), cnt.data_ptr(), flags)
        ctx.sync()
        kernel_ms[key or Q] = ctx.last_kernel_ms()
    return run


fns = dict(plain=plain, acc=acc)
for Q in QS:
    fns["Q%d" % Q] = placer(Q)
# the two routes to the likelihoods against each other (Q = 16): cnf2_sweep's launches first / the placement sweep's own
fns["sweep_lik"] = placer(QS[0], SWEEP_LIKELIHOODS, f, "sweep_lik")
fns["own_lik"] = placer(QS[0], OWN_LIKELIHOODS, f2, "own_lik")
for fn in fns.values():
    fn()
best = {k: 1e9 for k in fns}
for _ in range(reps):
    for k, fn in fns.items():
        t0 = time.perf_counter()
        fn()
        best[k] = min(best[k], time.perf_counter() - t0)
plain()
fns["Q%d" % QS[-1]]()
assert torch.equal(ll, ll2)
print("%d F2 x %d markers (%d chromosomes; input %.1f s): cnf2_sweep with rows %.3f s, cnf2_sweep_accumulate without rows %.3f s; "
      "cnf2_sweep_place (sums only) %s" % (n, M, chroms, gen_s, best["plain"], best["acc"],
                                          ", ".join("Q = %d %.3f s = %.2f x the sweep with rows (its batched part %.3f s)"
                                                    % (Q, best["Q%d" % Q], best["Q%d" % Q] / best["plain"], kernel_ms[Q] / 1e3) for Q in QS)))
plain()
f_plain = f.clone()
fns["own_lik"]()
print("likelihood routes at Q = %d: cnf2_sweep's launches first %.3f s, the placement sweep's own %.3f s; own factors bit-equal to "
      "cnf2_sweep's: %s (largest difference %.3g)" % (QS[0], best["sweep_lik"], best["own_lik"], torch.equal(f_plain, f2),
                                                     float((f_plain - f2).abs().max())))
lens = np.diff(np.asarray(ped.chromstarts))
tiles = int(sum((L + 15) // 16 for L in lens))
for Q in QS:
    print("Q = %d: contraction %.3g useful flops, %.3g issued in 16 x 32 tiles; state posteriors %.1f GB written and read once"
          % (Q, 2.0 * 512 * n * M * Q, 2.0 * 512 * n * tiles * 16 * ((Q + 31) // 32) * 32, n * M * 4096 / 1e9))
ctx.close()
