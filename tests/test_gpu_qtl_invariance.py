"""GPU suite: the four QTL scans (cnf2_qtl_scan, cnf2_qtl_scanx, cnf2_qtl_scan2, cnf2_qtl_scan_em) on shifted and rescaled
traits and covariates and on relabelled inputs (tests/qtl_invariance.py).  The model is exactly invariant; the reference of a
transformed problem is the float64 yardstick of the base problem carried over by that invariance (map_reference), and the
comparison is the scan's own, with ATOL unchanged.  Every test also prints how far the outputs are from the same scan's
outputs on the base inputs.  One command-line run: the same cross with the table in other units gives the same files.

The binary-trait scan (cnf2_qtl_scan_binary) follows: a 0/1 trait has no units, so its covariates alone are rescaled and
shifted (nothing changes), the trait is complemented (every effect changes sign, n_ones -> n_used - n_ones) and the inputs
relabelled; the comparison is qtlbin_reference.compare_bin against the mapped base yardstick, and the command line runs once
more with the covariate shifted.

The cofactor scan (cnf2_qtl_scan_cof), the bootstrap scan (cnf2_qtl_scan_boot) and the polygenic scan (qtl.scan_lmm on
cnf2_kinship_sums and cnf2_qtl_scan_cols) follow, each under the same eight transforms and four relabellings against the base
problem's yardstick carried over by its own map, with the scan's own comparison at ATOL; then the kinship sums and the column
scan by themselves, and the command line's --qtlcof and --qtlboot files in other units."""
import numpy as np
import pytest

import qtl_invariance as V
import qtlbin_reference as RB
import qtlboot_reference as RO
import qtlcof_reference as RC
import qtllmm_reference as RL
from cnf2freq_amd import qtl, synth
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


CLI_BOOT_SEED = 4               # the --qtl-seed of test_cli_newer_scans_other_units (its docstring says how it was picked)


def cli_newer_scans_table(ped):
    """(w and h [n][2], age [n]) of the F2 of 14 of test_gpu_qtlcof.test_cli_qtlcof, every value on the binary grid"""
    n = 14
    g = lambda m: ped.allele[3:, m, :].astype(np.float64).sum(axis=1) - 3.0
    age = V.on_grid(synth.uniform(5, np.arange(n)) * 10.0)
    y = V.on_grid(np.stack([g(4) + 0.5 * g(12) + noise(n, 1, 2)[:, 0], noise(n, 1, 3)[:, 0] * 4.0 + g(12)], axis=1))
    y[3, 1] = np.nan                             # the second trait has its own pattern of missing values, and its own draws
    return y, age


def cli_boot_gaps(capi, files, ped, y, age, seed, replicates=40, chrom=1):
    """[T] the smallest gap between the best and the second best LOD of a replicate, by qtlboot_reference.reference_boot on the
    sweep's rows of the files (host.Run.from_files), with the counts `cnF2freq --qtlboot` draws per pattern of missing values"""
    from cnf2freq_amd import host
    n, M, cs = len(y), ped.n_markers, np.asarray(ped.chromstarts)
    r = host.Run.from_files(*files)
    r.postmarkerdata()
    ctx = capi.Context.borrowed(r.context(), M, cs, n)
    origin = qtl.origin_rows(ctx).cpu().numpy()
    ctx.close()
    r.close()
    gaps = []
    for t in range(y.shape[1]):
        u = np.isfinite(y[:, t])
        count = qtl.bootstrap_counts(n, replicates, seed, use=u)
        ref = RO.reference_boot(origin, cs, y[:, [t]], count, u, age[:, None], False, chrom, chrom + 1)
        gaps.append(float(ref["gap"].min()))
    return gaps


def test_cli_newer_scans_other_units(capi, tmp_path):
    """cnF2freq --qtlcof (cofactors 12,4 with a window, 5 permutations) and --qtlboot (chromosome 2, 40 replicates) on the F2 of
    14 of test_cli_qtlcof, once with the phenotype table as it is and once with trait w + 65536 and covariate age + 16384
    (values on the binary grid, written with repr: the text is exact).  Both files are the same text, line for line.  For the
    bootstrap file that asks that no replicate's choice of marker is a tie, which is asserted first on the reference alone:
    every gap of reference_boot on the base table is at least ARG_GAP.  --qtl-seed 4, the seed of test_cli_qtlcof and
    test_cli_qtlboot, was the first one tried and has it."""
    import os
    import subprocess
    from conftest import ROOT
    from test_gpu_qtl2 import write_f2_files
    ped = synth.make_f2(14, 9, 2, seed=3, missing=0.1)
    files, names = write_f2_files(ped, tmp_path)
    n, cs = 14, np.asarray(ped.chromstarts)
    y, age = cli_newer_scans_table(ped)
    gaps = cli_boot_gaps(capi, files, ped, y, age, CLI_BOOT_SEED)
    print("INVARIANCE cli --qtlboot: the smallest gap of a replicate per trait, on the reference: %s" % gaps)
    assert min(gaps) >= RO.ARG_GAP
    window = 0.3 * float(ped.pos[cs[1] - 1] - ped.pos[0])
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
               "--qtl-covariates", "age", "--qtl-permutations", "5", "--qtl-seed", str(CLI_BOOT_SEED), "--output", str(tmp_path / (tag + ".out")),
               "--qtlcof", str(tmp_path / (tag + "_qc.txt")), "--qtl-cofactors", "12,4", "--qtl-window", repr(window),
               "--qtlboot", str(tmp_path / (tag + "_qb.txt")), "--qtl-boot-chrom", "2", "--qtl-boot-replicates", "40"]
        subprocess.run(cmd, capture_output=True, text=True, timeout=600, check=True, cwd=str(tmp_path))
        out[tag] = [open(str(tmp_path / (tag + suffix))).read().split("\n") for suffix in ("_qc.txt", "_qb.txt")]
    for which, least, (b, s) in zip(("--qtlcof", "--qtlboot"), (2 * ped.n_markers, int(cs[2] - cs[1])), zip(out["base"], out["shifted"])):
        differ = [(x, z) for x, z in zip(b, s) if x != z]
        print("INVARIANCE cli %s: %d lines, %d differ%s" % (which, len(b), len(differ), "".join("\n  %s\n  %s" % d for d in differ[:5])))
        assert len(b) == len(s) > least
        assert not differ, which
    assert sum(ln.startswith("threshold\tlod") for ln in out["base"][0]) == 2
    # (the scans did fit: a conditional LOD above 0.5, as test_cli_qtlcof asks, and an interval from usable replicates)
    assert max(float(ln.split("\t")[6]) for ln in out["base"][0] if ln[:1].isdigit()) > 0.5
    assert all(int(ln.split("\t")[7]) > 0 for ln in out["base"][1][:2])


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


# ------------------------------------------------------------------------------------------------ the cofactor scan
COF_SCAN_IDS = list(V.COF_SCANS)
_COF_BASE_GOT = {}


def cof_base_outputs(capi, case, scan, config=V.COF):
    """Context.qtl_scan_cof's outputs on the base inputs, once per module"""
    if (case, scan, config) not in _COF_BASE_GOT:
        ctx = map_context(capi)
        _COF_BASE_GOT[case, scan, config] = V.cof_run(ctx, scan, V.make_base(case), config)
        ctx.close()
    return _COF_BASE_GOT[case, scan, config]


def cof_check(capi, scan, case, name, inp, tr, flip, config=V.COF):
    """Context.qtl_scan_cof on the inputs `inp` against the base yardstick carried over by map_cof_reference: compare_cof,
    unchanged (share 0.99, strict, ATOL); where the traits are rescaled also in base units"""
    ref = V.cof_base_reference(case, scan, config)
    assert RC.compared_markers(ref, V.CS, share=0.99, strict=True).mean() >= 0.99      # on the reference alone, before the product runs
    ctx = map_context(capi)
    got = V.cof_run(ctx, scan, inp, config)
    ctx.close()
    back = V.map_cof_reference(got, 1.0 / tr["alpha"], flip)
    base_got = cof_base_outputs(capi, case, scan, config)
    what = "%s %s %s" % (scan, case[0], name)
    print(V.errors_line("INVARIANCE " + what + " | against the mapped base reference:", V.cof_errors(back, ref)))
    print(V.errors_line("INVARIANCE " + what + " | against the base run:", V.cof_errors(back, base_got)))
    if name[-1] in "FG":
        print("INVARIANCE %s | bit-equal to the base run: %s" % (what, V.cof_bit_equal(back, base_got)))
    RC.compare_cof(got, V.map_cof_reference(ref, tr["alpha"], flip), V.CS, what, share=0.99, strict=True)
    if np.any(tr["alpha"] != 1.0):
        RC.compare_cof(V.map_cof_reference(got, 1.0 / tr["alpha"]), ref, V.CS, what + " in base units", share=0.99, strict=True)
    return got


@pytest.mark.parametrize("name", TRANSFORM_IDS)
@pytest.mark.parametrize("case", V.CASES, ids=V.CASE_IDS)
@pytest.mark.parametrize("scan", COF_SCAN_IDS)
def test_cof_transform(capi, scan, case, name):
    """the cofactor scan (cofactors 22 and 60, +-3 markers left out) on transformed traits and covariates"""
    tr = V.TRANSFORMS[name]
    cof_check(capi, scan, case, "transform " + name, V.apply(V.make_base(case), tr), tr, ())


@pytest.mark.parametrize("name", V.RELABELLINGS)
@pytest.mark.parametrize("case", V.CASES, ids=V.CASE_IDS)
@pytest.mark.parametrize("scan", COF_SCAN_IDS)
def test_cof_relabelling(capi, scan, case, name):
    """classes 0 and 3 (a changes sign) or 1 and 2 (nothing does) exchanged, the covariate columns exchanged, the individuals
    reordered"""
    inp, flip = V.relabel(V.make_base(case), name)
    cof_check(capi, scan, case, "relabelling " + name, inp, V.IDENTITY, flip)


@pytest.mark.parametrize("name", ["B", "D", "reorder"])
@pytest.mark.parametrize("case", V.CASES, ids=V.CASE_IDS)
@pytest.mark.parametrize("scan", COF_SCAN_IDS)
def test_cof_three_cofactors(capi, scan, case, name):
    """three cofactors (7, 43, 70; +-2 markers) under the two largest shifts and the reordering: in n67-skip the individuals
    that chromosome 3 skips are in the fits of the other chromosomes, so n_used differs by chromosome"""
    base = V.make_base(case)
    if name == "reorder":
        inp, flip = V.relabel(base, name)
        got = cof_check(capi, scan, case, "three cofactors relabelling " + name, inp, V.IDENTITY, flip, V.COF3)
    else:
        got = cof_check(capi, scan, case, "three cofactors transform " + name, V.apply(base, V.TRANSFORMS[name]), V.TRANSFORMS[name], (), V.COF3)
    n = case[1]
    assert list(got["n_used"]) == ([n - 2] * 6 if case[3] else [n, n, n, n - 2, n, n])


# ------------------------------------------------------------------------------------------------ the bootstrap scan
BOOT_SCAN_IDS = list(V.BOOT_SCANS)
_BOOT_BASE_GOT = {}


def boot_base_outputs(capi, case, scan):
    """Context.qtl_scan_boot's outputs on the base inputs, once per module"""
    if (case, scan) not in _BOOT_BASE_GOT:
        ctx = map_context(capi)
        _BOOT_BASE_GOT[case, scan] = V.boot_run(ctx, scan, V.make_boot_base(case))
        ctx.close()
    return _BOOT_BASE_GOT[case, scan]


def boot_check(capi, scan, case, name, inp):
    """Context.qtl_scan_boot on the inputs `inp` against the base yardstick itself (the map is the identity):
    qtlboot_reference.compare, unchanged, on the cells of conditions(base reference, K = 2)"""
    ref, compared = V.boot_base_reference(case, scan)            # (asserts the conditions, on the reference alone, before the product runs)
    ctx = map_context(capi)
    got = V.boot_run(ctx, scan, inp)
    ctx.close()
    base_got = boot_base_outputs(capi, case, scan)
    what = "%s %s %s" % (scan, case[0], name)
    print(V.errors_line("INVARIANCE " + what + " | against the base reference:", V.boot_errors(got, ref, compared)))
    print(V.errors_line("INVARIANCE " + what + " | against the base run:", V.boot_errors(got, base_got)))
    if name[-1] in "FG":
        print("INVARIANCE %s | bit-equal to the base run: %s" % (what, V.boot_bit_equal(got, base_got)))
    RO.compare(got, ref, compared, what)
    return got


@pytest.mark.parametrize("name", TRANSFORM_IDS)
@pytest.mark.parametrize("case", V.CASES, ids=V.CASE_IDS)
@pytest.mark.parametrize("scan", BOOT_SCAN_IDS)
def test_boot_transform(capi, scan, case, name):
    """the bootstrap scan (21 replicates, all six chromosomes, with the profile) on transformed traits and covariates: no
    output changes"""
    boot_check(capi, scan, case, "transform " + name, V.apply(V.make_boot_base(case), V.TRANSFORMS[name]))


@pytest.mark.parametrize("name", V.RELABELLINGS)
@pytest.mark.parametrize("case", V.CASES, ids=V.CASE_IDS)
@pytest.mark.parametrize("scan", BOOT_SCAN_IDS)
def test_boot_relabelling(capi, scan, case, name):
    """classes exchanged, covariate columns exchanged, the individuals reordered with their counts: no output changes"""
    boot_check(capi, scan, case, "relabelling " + name, V.boot_relabel(V.make_boot_base(case), name))


@pytest.mark.parametrize("case", V.CASES, ids=V.CASE_IDS)
@pytest.mark.parametrize("scan", BOOT_SCAN_IDS)
def test_boot_replicates_reversed(capi, scan, case):
    """the replicates in reverse order, count[::-1]: every output reversed along B, bit for bit (replicate tiles change no bit)"""
    base = V.make_boot_base(case)
    ctx = map_context(capi)
    got = V.boot_run(ctx, scan, dict(base, count=np.ascontiguousarray(base["count"][::-1])))
    ctx.close()
    base_got = boot_base_outputs(capi, case, scan)
    for key in V.BOOT_KEYS:
        same = V.same_bits(got[key], base_got[key][::-1])
        print("INVARIANCE %s %s replicates-reversed | %s bit-equal to the reversed base run: %s" % (scan, case[0], key, same))
        assert same, key


# ------------------------------------------------------------------------------------------------ the polygenic scan
LMM_SCAN_IDS = list(V.LMM_SCANS)
_LMM_BASE_GOT = {}


def lmm_call(capi, scan, inp, permutations=None, kinship=None, record=None):
    """qtl.scan_lmm on the inputs `inp` through a context that holds the map and the number of individuals; with `record` (a
    list) every permuted call of Context.qtl_scan_cols_device is recorded with the columns the product handed to it"""
    import torch
    from test_gpu_qtllmm import device_array
    ctx = map_context(capi)
    ctx.n_ind = inp["origin"].shape[0]
    rows = torch.from_numpy(inp["origin"]).cuda()
    plain = ctx.qtl_scan_cols_device

    def recording(nk, n_mark, ne, d_reg, x0, y, scale=None, perm=None):
        if perm is not None:
            record.append(dict(reg=device_array(capi, d_reg, (nk, n_mark, ne)), x0=x0.copy(), pheno=y.copy(), scale=scale.copy(), perm=perm.copy()))
        return plain(nk, n_mark, ne, d_reg, x0, y, scale=scale, perm=perm)
    if record is not None:
        ctx.qtl_scan_cols_device = recording
    got = V.lmm_run(ctx, scan, inp, rows, permutations=permutations, kinship=kinship)
    ctx.qtl_scan_cols_device = plain
    ctx.close()
    return got


def lmm_base_outputs(capi, case, scan):
    """qtl.scan_lmm's outputs on the base inputs, once per module"""
    if (case, scan) not in _LMM_BASE_GOT:
        _LMM_BASE_GOT[case, scan] = lmm_call(capi, scan, V.make_base(case))
    return _LMM_BASE_GOT[case, scan]


def lmm_check(capi, scan, case, name, inp, tr, flip, permutations=None, kinship=None):
    """qtl.scan_lmm on the inputs `inp` against the Cholesky yardstick of the BASE problem -- at the given h2, or at the h2 this
    run returned -- carried over by map_lmm_reference: compare_lmm at ATOL with at least 0.9 of the cells compared, sigma2,
    n_used; the estimated h2 within 1e-4 of the base problem's grid; perm_max against cols_reference on the very columns the
    product permuted"""
    s = V.LMM_SCANS[scan]
    C = len(CHROM_LENS)
    if s["h2"] is not None:
        assert V.lmm_base_reference(case, scan)["compared"].mean() >= 0.9           # on the reference alone, before the product runs
    else:
        grid = [V.lmm_grid_h2(case, t) for t in range(V.T)]                        # (asserts a single local maximum)
    calls = []
    got = lmm_call(capi, scan, inp, permutations, kinship, record=calls)
    base_got = lmm_base_outputs(capi, case, scan)
    what = "%s %s %s" % (scan, case[0], name)
    if s["h2"] is not None:
        ref = V.lmm_base_reference(case, scan)
        assert np.array_equal(got["h2"], V.lmm_given_h2(scan))
    else:
        for t in range(V.T):
            print("INVARIANCE %s | trait %d: h2 %.10f, the base grid's maximum at %.4f, from the base run's h2 %.3g" %
                  (what, t, got["h2"][t, 0], grid[t], abs(got["h2"][t, 0] - base_got["h2"][t, 0])))
            assert np.all(got["h2"][t] == got["h2"][t, 0]) and np.all(got["sigma2"][t] == got["sigma2"][t, 0])
            assert abs(got["h2"][t, 0] - grid[t]) <= V.LMM_H2_BOUND
        ref = V.lmm_reference(V.make_base(case), V.lmm_base_kinship(case, False), got["h2"])
        assert ref["compared"].mean() >= 0.9
    back = V.map_lmm_reference(got, 1.0 / tr["alpha"], flip)
    print(V.errors_line("INVARIANCE " + what + " | against the mapped base reference:", V.lmm_errors(back, ref)))
    print(V.errors_line("INVARIANCE " + what + " | against the base run:", V.lmm_errors(back, base_got)))
    if name[-1] in "FG":
        print("INVARIANCE %s | bit-equal to the base run: %s" % (what, V.lmm_bit_equal(back, base_got)))
    V.lmm_check(got, V.map_lmm_reference(ref, tr["alpha"], flip), what)
    if np.any(tr["alpha"] != 1.0):
        V.lmm_check(V.map_lmm_reference(got, 1.0 / tr["alpha"]), ref, what + " in base units")
    P = s["permutations"] if permutations is None else permutations
    if not P:
        assert got["perm_max"] is None and not calls
        return got
    # the permutations: the maxima of a least-squares scan over the very columns the product permuted (a pattern runs through
    # its chromosomes, and within a chromosome through its traits)
    assert got["perm_max"].shape == (P, V.T, C) and len(calls) == V.T * C
    nk = int(V.lmm_keep(inp).sum())
    worst = 0.0
    for k, call in enumerate(calls):
        c, t = k // V.T, k % V.T
        assert call["reg"].shape == (nk, CHROM_LENS[c], 2) and np.array_equal(call["perm"], qtl.permutations(nk, P, V.LMM_SEED))
        want = RL.cols_reference(call["reg"], call["x0"], call["pheno"], call["scale"], call["perm"])
        worst = max(worst, np.abs(got["perm_max"][:, t, c] - want["perm_max"][:, 0]).max())
    print("INVARIANCE %s | perm_max against cols_reference on the permuted columns: %.3g" % (what, worst))
    assert worst <= RL.ATOL
    return got


@pytest.mark.parametrize("name", TRANSFORM_IDS)
@pytest.mark.parametrize("case", V.CASES, ids=V.CASE_IDS)
@pytest.mark.parametrize("scan", LMM_SCAN_IDS)
def test_lmm_transform(capi, scan, case, name):
    """the polygenic scan -- h2 = (0.3, 0.8) with a chromosome left out of the kinship and 3 permutations; h2 estimated by REML
    with the genome's kinship -- on transformed traits and covariates"""
    tr = V.TRANSFORMS[name]
    lmm_check(capi, scan, case, "transform " + name, V.apply(V.make_base(case), tr), tr, ())


@pytest.mark.parametrize("name", V.RELABELLINGS)
@pytest.mark.parametrize("case", V.CASES, ids=V.CASE_IDS)
@pytest.mark.parametrize("scan", LMM_SCAN_IDS)
def test_lmm_relabelling(capi, scan, case, name):
    """classes 0 and 3 (a changes sign, a_i a_j does not) or 1 and 2 (nothing changes) exchanged, the covariate columns
    exchanged, the individuals reordered.  The reordering runs without permutations (scan_lmm draws its own), once with the
    kinship computed from the reordered rows and once with the reordered base kinship K[s][:, s] passed as [C][n][n]."""
    inp, flip = V.relabel(V.make_base(case), name)
    if name != "reorder":
        lmm_check(capi, scan, case, "relabelling " + name, inp, V.IDENTITY, flip)
        return
    s = V.order_of(case[1])
    K = V.lmm_base_kinship(case, V.LMM_SCANS[scan]["loco"])
    lmm_check(capi, scan, case, "relabelling reorder, kinship from the rows", inp, V.IDENTITY, flip, permutations=0)
    lmm_check(capi, scan, case, "relabelling reorder, kinship K[s][:, s] given", inp, V.IDENTITY, flip, permutations=0,
              kinship=np.ascontiguousarray(K[:, s][:, :, s]))


@pytest.mark.parametrize("case", V.CASES, ids=V.CASE_IDS)
def test_lmm_estimated_h2(capi, case):
    """the base problem itself: the estimated h2 within 1e-4, the grid's step, of the maximum of the Cholesky-route REML
    likelihood on the grid, for both traits; the same with the genome's kinship handed over as one [n][n] matrix"""
    base = V.make_base(case)
    lmm_check(capi, "lmm-est", case, "base", base, V.IDENTITY, ())
    lmm_check(capi, "lmm-est", case, "base, kinship given", base, V.IDENTITY, (), kinship=V.lmm_base_kinship(case, False)[0])


# ------------------------------------------------------------------------------------------------ kinship sums, the column scan
@pytest.mark.parametrize("case", V.CASES, ids=V.CASE_IDS)
def test_kinship_relabelling(capi, case):
    """Context.kinship_sums on the base rows over three chromosome ranges: the same bits with classes 0 and 3 or 1 and 2
    exchanged; under the reordering S' = S[s][:, s] within ATOL, and S' equal to its transpose to the bit"""
    ctx = map_context(capi)
    V.check_kinship_relabellings(ctx.kinship_sums, case, "Context.kinship_sums")
    ctx.close()


def test_cols_units(capi):
    """Context.qtl_scan_cols, whose model centres nothing and adds no intercept, on the traits times 2^+-100 (coef times alpha,
    rss0 times alpha^2), on x0 @ diag(2^3, 2^-5) and on reg 2^7 with scale / 2^7 (nothing changes), on reg 2^7 alone (coef /
    2^7) and on reordered individuals: cols_compare, unchanged, against cols_reference of the base, also in base units"""
    inp, ref = V.cols_base()
    RL.cols_compared(ref)                        # the conditions of the comparison, on the reference, before anything runs
    ctx = capi.Context(0)
    base_got = ctx.qtl_scan_cols(inp["reg"], inp["x0"], inp["pheno"], scale=inp["scale"], perm=inp["perm"])
    RL.cols_compare(base_got, ref, "cols base")
    keys = ("lod", "coef", "rss0", "perm_max")
    for name, p, alpha, divisor in V.cols_problems():
        got = ctx.qtl_scan_cols(p["reg"], p["x0"], p["pheno"], scale=p["scale"], perm=p["perm"])
        back = V.map_cols(got, 1.0 / alpha, 1.0 / divisor)
        what = "cols " + name
        print(V.errors_line("INVARIANCE " + what + " | against the mapped base reference:", V.errors(back, ref, keys, ("rank",))))
        print(V.errors_line("INVARIANCE " + what + " | against the base run:", V.errors(back, base_got, keys, ("rank",))))
        print("INVARIANCE %s | bit-equal to the base run: %s" % (what, V.bit_equal(back, base_got, keys + ("rank",))))
        RL.cols_compare(got, V.map_cols(ref, alpha, divisor), what)
        if alpha != 1.0 or divisor != 1.0:
            RL.cols_compare(back, ref, what + " in base units")
    ctx.close()
