"""Measurement aid: wall time, ending in a device synchronise, of one bootstrap scan (cnf2_qtl_scan_boot) beside what the
library offered for the same result before it: one cnf2_qtl_scan_cols call per replicate with sqrt(count) as `scale` and the
host-side scaled x0 and pheno.  Hand-made soft rows (no sweep): n individuals, one chromosome of M markers, one trait, one
covariate, B replicates; device rows, host outputs, a warm context.
  1. the one call: `repeats` runs, their median, with the shader clock (cnf2_clock_probe) before and after
  2. the B column-scan calls, once (`baseline` = 0 skips them, e.g. under a profiler), and the largest difference of the
     two routes' best LODs
  3. the MFMAs the product needs, counted from the shapes, for a rate over the product kernel's time of a profiler run
usage: python tools/qtlboot_timing.py [n=2000] [markers=2500] [replicates=1000] [repeats=5] [baseline=1]"""
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
from cnf2freq_amd import capi, qtl, synth

a = [int(x) for x in sys.argv[1:6]] + [2000, 2500, 1000, 5, 1][len(sys.argv[1:6]):]
n, M, B, reps, baseline = a
K, T = 1, 1
dev = torch.device("cuda", 0)


def soft_rows(n, M, seed):
    """origin[n][M][4]: two gametes per individual, each a two-state Markov chain along the markers, a weight of 0.6 .. 1 on
    the true class and the rest spread over the others"""
    u = lambda stream, shape: synth.uniform(seed * 16 + stream, np.arange(int(np.prod(shape)))).reshape(shape)
    flip = u(1, (2, n, M)) < 0.02
    flip[:, :, 0] = u(0, (2, n)) < 0.5
    g = np.cumsum(flip, axis=2) & 1
    k = g[0] + 2 * g[1]
    w = 0.6 + 0.4 * u(2, (n, M))
    o = np.repeat(((1.0 - w) / 3.0)[:, :, None], 4, axis=2)
    np.put_along_axis(o, k[:, :, None], w[:, :, None], axis=2)
    return o


t0 = time.perf_counter()
origin = soft_rows(n, M, 2)
planted = M // 2
cov = synth.uniform(41, np.arange(n))[:, None] * 2.0 - 1.0
pheno = 0.3 * (origin[:, planted, 3] - origin[:, planted, 0])[:, None] + 0.3 * cov + (synth.uniform(77, np.arange(n))[:, None] - 0.5)
count = qtl.bootstrap_counts(n, B, 5)
ctx = capi.Context(0)
ctx.upload_map(np.arange(M, dtype=np.float64) * 0.05, np.array([0, M], np.int32))
d_o = torch.from_numpy(origin).to(dev)
print("%d individuals x %d markers on one chromosome, T = %d, K = %d, %d replicates (input %.1f s); times in s, ending in a synchronise"
      % (n, M, T, K, B, time.perf_counter() - t0), flush=True)

# ---- 1. the one call
out = None


def one_call():
    global out
    out = ctx.qtl_scan_boot_device(n, d_o.data_ptr(), pheno, count, cov=cov, out=out)
    ctx.sync()


one_call()                      # warm: code objects, the context's buffers
clock0 = ctx.clock_probe()
times = []
for _ in range(reps):
    t0 = time.perf_counter()
    one_call()
    times.append(time.perf_counter() - t0)
clock1 = ctx.clock_probe()
med = float(np.median(times))
print("  cnf2_qtl_scan_boot, one call: median %.4f (all: %s; spread %.1f %%); shader clock %.0f MHz before, %.0f MHz after" % (
    med, " ".join("%.4f" % v for v in times), 100 * (max(times) - min(times)) / min(times), clock0, clock1), flush=True)
iv = qtl.boot_interval(out["boot_arg"][:, 0, 0], np.arange(M) * 0.05)
print("  95 %% interval: markers %d .. %d of %d usable replicates (effect planted at %d)" % (iv["lo"], iv["hi"], iv["V"], planted))

# ---- 3. what the product computes: per tile of 16 markers, group of 16 replicates and 4 individuals one MFMA per feature
feat = 3 + 2 * (K + 1) + 2 * T
mfma = ((M + 15) // 16) * ((B + 15) // 16) * ((n + 3) // 4) * feat
print("  the product: %d features, %.3g v_mfma_f64_16x16x4_f64 = %.3g flop (2048 each); at the call's whole time %.2f Tflop/s" % (
    feat, mfma, mfma * 2048.0, mfma * 2048.0 / med / 1e12), flush=True)

# ---- 2. the route before: one column scan per replicate
if baseline:
    use = np.ones(n, bool)
    y = pheno - pheno.mean(axis=0)
    x0 = np.concatenate([np.ones((n, 1)), cov - cov.mean(axis=0)], axis=1)
    reg = torch.stack([d_o[:, :, 3] - d_o[:, :, 0], d_o[:, :, 1] + d_o[:, :, 2]], dim=2).contiguous()
    best = np.zeros(B)

    def column_scans():
        for b in range(B):
            s = np.sqrt(count[b].astype(np.float64))
            got = ctx.qtl_scan_cols_device(n, M, 2, reg.data_ptr(), x0 * s[:, None], y * s[:, None], scale=s)
            best[b] = got["lod"][0].max()
        ctx.sync()

    ctx.qtl_scan_cols_device(n, M, 2, reg.data_ptr(), x0, y, scale=np.ones(n))          # warm
    ctx.sync()
    t0 = time.perf_counter()
    column_scans()
    t_cols = time.perf_counter() - t0
    print("  %d cnf2_qtl_scan_cols calls with sqrt(count) as scale: %.3f in all, %.2f ms a call; the one call takes %.3f of that" % (
        B, t_cols, 1e3 * t_cols / B, med / t_cols))
    print("  largest difference of the two routes' best LODs: %.3g (largest LOD %.2f)" % (
        np.abs(best - out["boot_max"][:, 0, 0]).max(), best.max()))
ctx.close()
