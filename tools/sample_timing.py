"""Measurement aid: kernel-inclusive wall time of cnf2_sweep_sample with K = 1, 8 and 64 draws against the plain cnf2_sweep
with dosage rows, cnf2_sweep_crossovers with sums only and cnf2_sweep_viterbi, all with device outputs (CNF2_OUT_DEVICE,
torch tensors), on a synthetic F2 (synth.make_f2).  Config 2 of BASELINE: 10 000 individuals x 20 chromosomes x 2 500 SNPs
(+1 dummy marker each).  Best of `repeats` per call.
usage: python tools/sample_timing.py [individuals=10000] [snps_per_chrom=2500] [chroms=20] [repeats=3]"""
import ctypes as C
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
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
KS = (1, 8, 64)
f = torch.empty((n, chroms, 8), dtype=torch.float64, device=dev)
ll = torch.empty((n, chroms), dtype=torch.float64, device=dev)
ll2 = torch.empty_like(ll)
dos = torch.empty((n, M, 3), dtype=torch.float64, device=dev)
xs = torch.empty((M, 6), dtype=torch.float64, device=dev)
cnt = torch.empty(chroms, dtype=torch.int32, device=dev)
lm = torch.empty((n, chroms, 8), dtype=torch.float64, device=dev)
vst = torch.empty((n, M), dtype=torch.uint8, device=dev)
vsh = torch.empty((n, chroms), dtype=torch.int32, device=dev)
st = torch.empty((n, max(KS), M), dtype=torch.uint8, device=dev)
sh = torch.empty((n, max(KS), chroms), dtype=torch.int32, device=dev)
lp = torch.empty((n, max(KS), chroms), dtype=torch.float64, device=dev)
P = lambda t: C.c_void_p(t.data_ptr())


def plain():
    ctx.sweep_device(0, n, f.data_ptr(), ll.data_ptr(), dos.data_ptr(), 0)
    ctx.sync()


def xo():
    rc = ctx.L.cnf2_sweep_crossovers(ctx.h, 0, n, P(f), P(ll2), None, P(xs), P(cnt), capi.OUT_DEVICE)
    assert rc == 0, ctx.L.cnf2_last_error(ctx.h)
    ctx.sync()


def vit():
    rc = ctx.L.cnf2_sweep_viterbi(ctx.h, 0, n, P(f), P(ll2), P(lm), P(vst), P(vsh), capi.OUT_DEVICE)
    assert rc == 0, ctx.L.cnf2_last_error(ctx.h)
    ctx.sync()


def sampler(K):
    def run():
        rc = ctx.L.cnf2_sweep_sample(ctx.h, 0, n, K, 1, P(f), P(ll2), P(st), P(sh), P(lp), capi.OUT_DEVICE)
        assert rc == 0, ctx.L.cnf2_last_error(ctx.h)
        ctx.sync()
    return run


fns = dict(plain=plain, xo=xo, vit=vit)
for K in KS:
    fns["K%d" % K] = sampler(K)
for fn in fns.values():
    fn()
best = {k: 1e9 for k in fns}
for _ in range(reps):
    for k, fn in fns.items():
        t0 = time.perf_counter()
        fn()
        best[k] = min(best[k], time.perf_counter() - t0)
plain()
fns["K%d" % KS[-1]]()
assert torch.equal(ll, ll2)
print("%d F2 x %d markers (%d chromosomes; input %.1f s): cnf2_sweep with rows %.3f s, cnf2_sweep_crossovers sums only %.3f s,"
      " cnf2_sweep_viterbi %.3f s; cnf2_sweep_sample %s; K = 1 is %.2f x the crossover call, K = %d %.2f x the sweep with rows"
      % (n, M, chroms, gen_s, best["plain"], best["xo"], best["vit"],
         ", ".join("K = %d %.3f s" % (K, best["K%d" % K]) for K in KS), best["K1"] / best["xo"], KS[-1],
         best["K%d" % KS[-1]] / best["plain"]))
ctx.close()
