"""GPU suite: the four QTL scans (cnf2_qtl_scan, cnf2_qtl_scanx, cnf2_qtl_scan2, cnf2_qtl_scan_em) on shifted and rescaled
traits and covariates and on relabelled inputs (tests/qtl_invariance.py).  The model is exactly invariant; the reference of a
transformed problem is the float64 yardstick of the base problem carried over by that invariance (map_reference), and the
comparison is the scan's own, with ATOL unchanged.  Every test also prints how far the outputs are from the same scan's
outputs on the base inputs.  One command-line run: the same cross with the table in other units gives the same files.

The binary-trait scan (cnf2_qtl_scan_binary) follows: a 0/1 trait has no units, so its covariates alone are rescaled and
shifted (nothing changes), the trait is complemented (every effect changes sign, n_ones -> n_used - n_ones) and the inputs
relabelled; the comparison is qtlbin_reference.compare_bin against the mapped base yardstick, and the command line runs once
more with the covariate shifted."""
import numpy as np
import pytest

import qtl_invariance as V
import qtlbin_reference as RB
from cnf2freq_amd import synth
from qtl_reference import CHROM_LENS, chromstarts_of, noise

pytestmark = pytest.mark.gpu

TRANSFORM_IDS = sorted(V.TRANSFORMS)


@pytest.fixture(scope="module")
def capi():
    import __graft_entry__ as g
    g.build()
    from cnf2freq_amd import capi as c
    return c


def map_context(capi, lens=CHROM_LENS):
    """a context that holds a map only: what the scans need"""
    cs = chromstarts_of(lens)
    pos = np.concatenate([np.arange(k, dtype=np.float64) * 2.0 for k in lens])
    ctx = capi.Context(0)
    ctx.upload_map(pos, cs)
    return ctx


_BASE_GOT = {}


def base_outputs(capi, case, scan):
    """the scan's outputs on the base inputs, once per module"""
    if (case, scan) not in _BASE_GOT:
        ctx = map_context(capi)
        _BASE_GOT[case, scan] = V.run(ctx, scan, V.make_base(case))
        ctx.close()
    return _BASE_GOT[case, scan]


def extra_checks(scan, got):
    s = V.SCANS[scan]
    if s["kind"] == "em" and s["tol"] < 0:
        fitted = got["rank"] > 0
        assert np.all(got["iters"][:, fitted] == s["max_iter"]) and np.all(got["status"][:, fitted] == 1)


@pytest.mark.parametrize("name", TRANSFORM_IDS)
@pytest.mark.parametrize("case", V.CASES, ids=V.CASE_IDS)
@pytest.mark.parametrize("scan", list(V.SCANS))
def test_transform(capi, scan, case, name):
    """a scan on transformed inputs against the mapped base reference; where the traits are rescaled also in the base problem's
    units, against the base reference itself (the comparisons are relative to max(1, |figure|): after 2^-100 y the mapped one
    alone would ask nothing of the effects)"""
    tr = V.transform_for(scan, V.TRANSFORMS[name])
    ref, names = V.base_reference(case, scan), V.coef_names(scan)
    if "near" in ref:
        assert ref["near"].mean() <= 0.01                   # on the reference alone: cells at the edge of the stopping rule
    ctx = map_context(capi)
    got = V.run(ctx, scan, V.apply(V.make_base(case), tr))
    ctx.close()
    back = V.unmap(got, tr, names)
    what = "%s %s transform %s" % (scan, case[0], name)
    print(V.errors_line("INVARIANCE " + what + " | against the mapped base reference:", V.errors(back, ref)))
    base_got = base_outputs(capi, case, scan)
    print(V.errors_line("INVARIANCE " + what + " | against the base run:", V.errors(back, base_got)))
    if name in "FG":
        print("INVARIANCE %s | bit-equal to the base run: %s" % (what, V.bit_equal(back, base_got)))
    V.check(scan, got, V.map_reference(ref, tr["alpha"], tr["gamma"], names), what)
    if np.any(tr["alpha"] != 1.0):
        V.check(scan, back, ref, what + " in base units")
    extra_checks(scan, got)


# (with an interactive covariate the exchange of the covariate columns is another model)
RELABELLED = [(scan, name) for scan in V.SCANS for name in V.RELABELLINGS if not (name == "covswap" and V.SCANS[scan].get("interactive"))]


@pytest.mark.parametrize("case", V.CASES, ids=V.CASE_IDS)
@pytest.mark.parametrize("scan,name", RELABELLED)
def test_relabelling(capi, scan, name, case):
    """classes 0 and 3 or 1 and 2 of every origin row exchanged, the covariate columns exchanged, the individuals reordered:
    against the correspondingly mapped base reference"""
    inp, flip = V.relabel(V.make_base(case), name)
    ref, names = V.base_reference(case, scan), V.coef_names(scan)
    ctx = map_context(capi)
    got = V.run(ctx, scan, inp)
    ctx.close()
    what = "%s %s relabelling %s" % (scan, case[0], name)
    want = V.map_reference(ref, names=names, flip=flip)
    print(V.errors_line("INVARIANCE " + what + " | against the mapped base reference:", V.errors(got, want)))
    V.check(scan, got, want, what)
    extra_checks(scan, got)


# ------------------------------------------------------------------------------------------------ the binary-trait scan
BIN_TRANSFORM_IDS = sorted(V.BIN_TRANSFORMS)
BIN_CHANGES = ("complement",) + V.RELABELLINGS
_BIN_BASE_GOT = {}


def bin_base_outputs(capi, case, scan):
    """Context.qtl_scan_binary's outputs on the base inputs, once per module"""
    if (case, scan) not in _BIN_BASE_GOT:
        ctx = map_context(capi)
        _BIN_BASE_GOT[case, scan] = V.bin_run(ctx, scan, V.make_bin_base(case))
        ctx.close()
    return _BIN_BASE_GOT[case, scan]


def bin_check(capi, scan, case, name, inp, how):
    """Context.qtl_scan_binary on the inputs `inp` against the base yardstick carried over by map_bin_reference: RB.compare_bin,
    unchanged, at ATOL.  Prints the figures against the mapped reference and, carried back, against the run on the base inputs."""
    V.assert_bin_conditions(case, scan)          # on the reference alone, before the product runs
    ref, names = V.bin_base_reference(case, scan), V.bin_coef_names(scan)
    want = V.map_bin_reference(ref, names=names, **how)
    ctx = map_context(capi)
    got = V.bin_run(ctx, scan, inp)
    ctx.close()
    what = "%s %s %s" % (scan, case[0], name)
    print(V.errors_line("INVARIANCE " + what + " | against the mapped base reference:", V.bin_errors(got, want)))
    back = V.map_bin_reference(got, names=names, **how)         # (each of the maps is its own inverse)
    print(V.errors_line("INVARIANCE " + what + " | against the base run:", V.bin_errors(back, bin_base_outputs(capi, case, scan))))
    RB.compare_bin(got, want, V.CS, what)
    s = V.BIN_SCANS[scan]
    if s["tol"] < 0:
        fitted = got["rank"] > 0
        assert np.all(got["iters"][:, fitted] == s["max_iter"]) and np.all(got["status"][:, fitted] == 1)
    return got


@pytest.mark.parametrize("name", BIN_TRANSFORM_IDS)
@pytest.mark.parametrize("case", V.CASES, ids=V.CASE_IDS)
@pytest.mark.parametrize("scan", list(V.BIN_SCANS))
def test_bin_transform(capi, scan, case, name):
    """the binary scan on rescaled and shifted covariates: no output changes.  For gamma = 2^+-100 whether the run has the
    bits of the base run is printed, not asserted (the mean that the centring subtracts is itself rounded)."""
    got = bin_check(capi, scan, case, "transform " + name, V.apply(V.make_bin_base(case), V.BIN_TRANSFORMS[name]), {})
    if name in "FG":
        print("INVARIANCE %s %s transform %s | bit-equal to the base run: %s" %
              (scan, case[0], name, V.bin_bit_equal(got, bin_base_outputs(capi, case, scan))))


@pytest.mark.parametrize("change", BIN_CHANGES)
@pytest.mark.parametrize("case", V.CASES, ids=V.CASE_IDS)
@pytest.mark.parametrize("scan", list(V.BIN_SCANS))
def test_bin_complement_and_relabelling(capi, scan, case, change):
    """y -> 1 - y on the used individuals (every effect changes sign, n_ones -> n_used - n_ones), classes 0 and 3 or 1 and 2 of
    every origin row exchanged (a, resp. i changes sign), the covariate columns exchanged, the individuals reordered"""
    base = V.make_bin_base(case)
    if change == "complement":
        inp, how = V.complement(base), dict(complemented=True)
    else:
        inp, flip = V.relabel(base, change)
        how = dict(flip=flip)
    bin_check(capi, scan, case, change, inp, how)


def test_cli_other_units(capi, tmp_path):
    """cnF2freq --qtl and --qtlem on an F2 of 14 on two chromosomes written to files, once with the phenotype table as it is
    and once with trait w + 65536 and covariate age + 16384 (values on a binary grid, written with repr: the text is exact).
    alpha = 1, so every column -- LOD, rank, iterations, thresholds, and the effects, sigma2 and status too -- is the same text."""
    import os
    import subprocess
    from conftest import ROOT
    from test_gpu_qtl2 import write_f2_files
    ped = synth.make_f2(14, 9, 2, seed=3, missing=0.1)
    files, names = write_f2_files(ped, tmp_path)
    n = 14
    g = lambda m: ped.allele[3:, m, :].astype(np.float64).sum(axis=1) - 3.0
    age = V.on_grid(synth.uniform(5, np.arange(n)) * 10.0)
    y = V.on_grid(np.stack([g(4) + noise(n, 1, 2)[:, 0], noise(n, 1, 3)[:, 0] * 4.0 + g(12)], axis=1))
    y[3, 1] = np.nan
    cell = lambda v: "NA" if np.isnan(v) else repr(float(v))
    exe = os.path.join(ROOT, "cnf2freq_amd", "cnF2freq")
    out = {}
    for tag, dw, dage in (("base", 0.0, 0.0), ("shifted", 65536.0, 16384.0)):
        w, a = y[:, 0] + dw, age + dage
        assert np.array_equal(w - dw, y[:, 0]) and np.array_equal(a - dage, age)
        table = ["id w age h"] + ["%s %s %s %s" % (names[i], cell(w[i]), cell(a[i]), cell(y[i, 1])) for i in range(n)]
        ph = tmp_path / ("pheno_%s.txt" % tag)
        ph.write_text("\n".join(table) + "\n")
        cmd = [exe, "--mapfile", files[0], "--pedfile", files[1], "--genfile", files[2], "--quiet", "--count", "1", "--phenofile", str(ph),
               "--qtl-covariates", "age", "--qtl-permutations", "5", "--qtl-seed", "4", "--output", str(tmp_path / (tag + ".out")),
               "--qtl", str(tmp_path / (tag + "_q.txt")), "--qtlem", str(tmp_path / (tag + "_qe.txt")),
               "--qtl-em-iterations", "300", "--qtl-em-tol", "1e-7"]
        subprocess.run(cmd, capture_output=True, text=True, timeout=600, check=True, cwd=str(tmp_path))
        out[tag] = [open(str(tmp_path / (tag + suffix))).read().split("\n") for suffix in ("_q.txt", "_qe.txt")]
    for which, (b, s) in zip(("--qtl", "--qtlem"), zip(out["base"], out["shifted"])):
        differ = [(x, z) for x, z in zip(b, s) if x != z]
        print("INVARIANCE cli %s: %d lines, %d differ%s" % (which, len(b), len(differ), "".join("\n  %s\n  %s" % d for d in differ[:5])))
        assert len(b) == len(s) > 20
        assert which == "--qtl" or any(ln.startswith("threshold\tlod") for ln in b)
        assert not differ, which


def test_cli_qtlbin_other_units(capi, tmp_path):
    """cnF2freq --qtlbin on the F2 of 14 of test_gpu_qtlbin.test_cli_qtlbin (two 0/1 traits, one with a missing value of its
    own, the covariate age, 5 permutations), once with the table as it is and once with age + 16384 (values on the binary grid,
    written with repr: the text is exact).  The two --qtlbin files are the same text, line for line."""
    import os
    import subprocess
    from conftest import ROOT
    from test_gpu_qtl2 import write_f2_files
    ped = synth.make_f2(14, 9, 2, seed=3, missing=0.1)
    files, names = write_f2_files(ped, tmp_path)
    n = 14
    g = lambda m: ped.allele[3:, m, :].astype(np.float64).sum(axis=1) - 3.0
    age = V.on_grid(synth.uniform(5, np.arange(n)) * 10.0)
    y = RB.bernoulli(np.stack([0.8 * g(4), 0.8 * g(12) + 0.3], axis=1), 2)
    y[3, 1] = np.nan
    cell = lambda v: "NA" if np.isnan(v) else repr(float(v))
    exe = os.path.join(ROOT, "cnf2freq_amd", "cnF2freq")
    out = {}
    for tag, dage in (("base", 0.0), ("shifted", 16384.0)):
        a = age + dage
        assert np.array_equal(a - dage, age)
        table = ["id b age h"] + ["%s %d %s %s" % (names[i], int(y[i, 0]), cell(a[i]), cell(y[i, 1])) for i in range(n)]
        ph = tmp_path / ("pheno_%s.txt" % tag)
        ph.write_text("\n".join(table) + "\n")
        cmd = [exe, "--mapfile", files[0], "--pedfile", files[1], "--genfile", files[2], "--quiet", "--count", "1", "--phenofile", str(ph),
               "--qtl-covariates", "age", "--qtl-permutations", "5", "--qtl-seed", "4", "--output", str(tmp_path / (tag + ".out")),
               "--qtlbin", str(tmp_path / (tag + "_qb.txt")), "--qtl-binary-iterations", "30", "--qtl-binary-tol", "1e-6"]
        subprocess.run(cmd, capture_output=True, text=True, timeout=600, check=True, cwd=str(tmp_path))
        out[tag] = open(str(tmp_path / (tag + "_qb.txt"))).read().split("\n")
    b, s = out["base"], out["shifted"]
    differ = [(x, z) for x, z in zip(b, s) if x != z]
    print("INVARIANCE cli --qtlbin: %d lines, %d differ%s" % (len(b), len(differ), "".join("\n  %s\n  %s" % d for d in differ[:5])))
    assert len(b) == len(s) > 2 * ped.n_markers
    assert sum(ln.startswith("threshold\tlod") for ln in b) == 2 and sum(ln.startswith("trait\t") for ln in b) == 2
    # (the scan did fit: some marker of the base file reports a LOD above 0.5, as test_cli_qtlbin asks of the same cross)
    assert max(float(ln.split("\t")[4]) for ln in b if ln[:1].isdigit()) > 0.5
    assert not differ
