"""Measurement aid: wall time, ending in a device synchronise, of one multiple-imputation scan (cnf2_qtl_scan_imp) beside what
the library offered for the draws' profiles before it: one cnf2_qtl_scan call per draw on that draw's one-hot origin rows,
expanded on the device from the same state bytes.  Synthetic states (no sweep): n individuals, M markers on chromosomes of
250, K = 2 covariates, one trait and P permutations, D draws; device states, host outputs, a warm context.  The two routes
alternate in one process, `repeats` times, and the best time of each is reported with all of them; the shader clock
(cnf2_clock_probe) is read before and after.  The baseline cannot give the permutations' maxima of the combined profile: its
D x P maxima are per draw.
usage: python tools/qtlimp_timing.py [n=1000] [markers=5000] [draws=16] [permutations=100] [repeats=3]"""
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
from cnf2freq_amd import capi, qtl, synth

a = [int(x) for x in sys.argv[1:6]] + [1000, 5000, 16, 100, 3][len(sys.argv[1:6]):]
n, M, D, P, reps = a
K, T, CHROM = 2, 1, 250
dev = torch.device("cuda", 0)


def paths(n, M, seed, switch=0.02):
    """classes [n][M]: two gametes per individual, each a two-state Markov chain along the markers of a chromosome"""
    u = lambda stream, shape: synth.uniform(seed * 16 + stream, np.arange(int(np.prod(shape)))).reshape(shape)
    flip = u(1, (2, n, M)) < switch
    flip[:, :, ::CHROM] = u(0, (2, n, len(range(0, M, CHROM)))) < 0.5
    g = np.zeros((2, n, M), np.int64)
    for c0 in range(0, M, CHROM):
        g[:, :, c0:c0 + CHROM] = np.cumsum(flip[:, :, c0:c0 + CHROM], axis=2) & 1
    return g[0] + 2 * g[1]


t0 = time.perf_counter()
base = paths(n, M, 2)
state = np.empty((n, D, M), np.uint8)
for d in range(D):
    take = synth.uniform(900 + d, np.arange(n * M)).reshape(n, M) < 0.2
    k = np.where(take, paths(n, M, 100 + d), base)
    state[:, d] = (k & 1) | ((k >> 1) << 3)
cs = np.append(np.arange(0, M, CHROM), M).astype(np.int32)
pos = np.concatenate([np.arange(cs[c + 1] - cs[c], dtype=np.float64) * 0.4 for c in range(len(cs) - 1)])
planted = M // 2
cov = synth.uniform(41, np.arange(n * K)).reshape(n, K) * 2.0 - 1.0
pheno = (0.3 * ((base[:, planted] == 3) * 1.0 - (base[:, planted] == 0)) + 0.3 * cov[:, 0] + synth.uniform(77, np.arange(n)) - 0.5)[:, None]
perm = qtl.permutations(n, P, 5) if P else None
ctx = capi.Context(0)
ctx.upload_map(pos, cs)
d_state = torch.from_numpy(state).to(dev)
print("%d individuals x %d markers on %d chromosomes, T = %d, K = %d, %d permutations, %d draws (input %.1f s); times in s, ending in a synchronise"
      % (n, M, len(cs) - 1, T, K, P, D, time.perf_counter() - t0), flush=True)
print("  bytes of genotype input per call: states %.1f MB; one-hot origin rows %.1f MB per draw, %.1f MB for the %d draws"
      % (state.nbytes / 1e6, n * M * 32 / 1e6, D * n * M * 32 / 1e6, D), flush=True)

out = {}


def sync():
    ctx.sync()
    torch.cuda.synchronize(dev)


def imp_call():
    out["imp"] = ctx.qtl_scan_imp_device(n, D, d_state.data_ptr(), pheno, cov=cov, perm=perm)
    sync()


def single_calls():
    """(whole time, of which the expansion of the rows) of the D single scans"""
    lods, t_exp = [], 0.0
    for d in range(D):
        t1 = time.perf_counter()
        g = d_state[:, d].to(torch.int64)
        rows = torch.nn.functional.one_hot((g & 1) + ((g >> 2) & 2), 4).to(torch.float64).contiguous()
        torch.cuda.synchronize(dev)
        t_exp += time.perf_counter() - t1
        lods.append(ctx.qtl_scan_device(n, rows.data_ptr(), pheno, cov=cov, perm=perm)["lod"])
    sync()
    out["single"] = np.stack(lods)
    return t_exp


imp_call()                      # warm: code objects, the context's buffers
single_calls()
clock0 = ctx.clock_probe()
t_imp, t_single, t_expand = [], [], []
for _ in range(reps):
    t1 = time.perf_counter()
    imp_call()
    t_imp.append(time.perf_counter() - t1)
    t1 = time.perf_counter()
    t_expand.append(single_calls())
    t_single.append(time.perf_counter() - t1)
clock1 = ctx.clock_probe()
fmt = lambda v: " ".join("%.4f" % x for x in v)
print("  cnf2_qtl_scan_imp, one call:          best %.4f (all: %s)" % (min(t_imp), fmt(t_imp)))
print("  %2d cnf2_qtl_scan calls on one-hot rows: best %.4f (all: %s), of which expanding the rows %.4f (all: %s)"
      % (D, min(t_single), fmt(t_single), min(t_expand), fmt(t_expand)))
print("  the one call takes %.3f of the D calls' best time, %.3f of it without the expansion; shader clock %.0f MHz before, %.0f MHz after"
      % (min(t_imp) / min(t_single), min(t_imp) / (min(t_single) - min(t_expand)), clock0, clock1))
m = out["single"].max(axis=0)
combined = m + np.log10((10.0 ** (out["single"] - m)).mean(axis=0))
print("  the one call's LOD against the D profiles combined on the host: %.3g (largest LOD %.2f at marker %d, planted %d)"
      % (np.abs(combined - out["imp"]["lod"]).max(), out["imp"]["lod"].max(), int(np.argmax(out["imp"]["lod"][0])), planted))
mfma = ((M + 15) // 16) * ((T * (1 + P) + 15) // 16) * ((n + 3) // 4) * 2 * D
print("  the product: %.3g v_mfma_f64_16x16x4_f64 = %.3g flop (2048 each) in either route" % (mfma, mfma * 2048.0))
ctx.close()
