"""CPU suite: the host side of the within-family scan (cnf2h_qtlfam_marker, cnf2h_qtl_families of include/cnf2host.h;
families and fam_fstat of cnf2freq_amd/qtl.py).  The serial fit of one marker through cnf2freq_amd/csrc/cnf2_qtlfam.h -- the
header the kernels use -- against the dense least-squares design of tests/qtlfam_reference.py."""
import numpy as np
import pytest

from cnf2freq_amd import qtl, synth
from qtl_reference import CHROM_LENS, chromstarts_of
from qtlfam_reference import ATOL, CASES, compare, compared_markers, make_case, reference_scan


@pytest.fixture(scope="module")
def host():
    import __graft_entry__ as g
    g.build()
    from cnf2freq_amd import host as h
    h.load()
    return h


def serial_scan(host, origin, cs, side, grp, cell, F, pheno, use=None, cov=None):
    """cnf2h_qtlfam_marker at every marker, assembled as cnf2_qtl_scan_fam reports: traits and covariates minus their means
    over the used individuals, the chromosome's mask from its first marker"""
    n, M, _ = origin.shape
    C = len(cs) - 1
    used = (np.ones(n, bool) if use is None else np.asarray(use) != 0) & (np.asarray(grp) >= 0)
    y = np.where(used[:, None], pheno, 0.0)
    y = np.where(used[:, None], y - y[used].mean(axis=0), 0.0)
    z = None
    if cov is not None:
        z = np.where(used[:, None], cov, 0.0)
        z = np.where(used[:, None], z - z[used].mean(axis=0), 0.0)
    T = y.shape[1]
    out = dict(lod=np.zeros((T, M)), df=np.zeros(M, np.int32), slope=np.zeros((T, M, F)), rss0=np.zeros((T, C)),
               n_used=np.zeros(C, np.int32), n_cells=np.zeros(C, np.int32))
    for c in range(C):
        mask = used & (origin[:, cs[c]] != 0.0).any(axis=1)
        for m in range(cs[c], cs[c + 1]):
            r = host.qtlfam_marker(origin[:, m], side, grp, F, y, cell=cell, cov=z, c=mask)
            out["lod"][:, m], out["df"][m], out["slope"][:, m] = r["lod"], r["df"], r["slope"]
            out["rss0"][:, c], out["n_used"][c], out["n_cells"][c] = r["rss0"], r["n_used"], r["n_cells"]
    return out


@pytest.mark.parametrize("T,P,K,side,fine,mask,skipped", CASES)
def test_marker_against_reference(host, T, P, K, side, fine, mask, skipped):
    origin, grp, cell, F, pheno, cov, use, _ = make_case(T, 0, K, side, fine, mask, skipped)
    cs = chromstarts_of(CHROM_LENS)
    ref = reference_scan(origin, cs, side, grp, cell, F, pheno, use, cov)
    got = serial_scan(host, origin, cs, side, grp, cell, F, pheno, use, cov)
    got["perm_max"] = None
    compare(got, ref, cs, "T %d K %d side %d fine %d" % (T, K, side, fine))
    # a family of one member is never fitted; with skipped individuals one family is emptied and one loses its slope
    assert not ref["fitted"][:, 0].any() and np.isnan(got["slope"][:, :, 0]).all()
    if skipped:
        on = slice(cs[3], cs[4])
        assert not ref["fitted"][on, 1].any() and not ref["fitted"][on, 2].any() and ref["fitted"][: cs[3], 2].all()


def test_families_outbred3(host):
    ped = synth.make_outbred3(3, 4, 5, 1, seed=5)
    for side in (0, 1):
        grp, cell, F = qtl.families(ped, side)
        assert F == 3 and list(grp) == [0] * 4 + [1] * 4 + [2] * 4 and list(cell) == list(grp)
        assert grp.dtype == np.int32 and cell.dtype == np.int32


def test_families_one_sire_two_dams(host):
    """records: 0-3 grandparents of the sire and of dam A, 4 the sire, 5 dam A, 6 dam B (a founder: no recorded parents),
    7 a second sire without recorded parents, 8-12 the offspring"""
    par = np.full((13, 2), -1, np.int32)
    par[4], par[5] = (0, 1), (2, 3)
    par[8], par[9], par[10], par[11], par[12] = (4, 5), (4, 6), (4, 5), (7, 5), (4, 6)
    dous = np.arange(8, 13, dtype=np.int32)
    g0, c0, f0 = host.qtl_families(par, dous, 0)
    assert f0 == 1 and list(g0) == [0, 0, 0, -1, 0] and list(c0) == [0, 1, 0, -1, 1]      # one sire, two cells
    g1, c1, f1 = host.qtl_families(par, dous, 1)
    assert f1 == 1 and list(g1) == [0, -1, 0, 0, -1] and list(c1) == [0, -1, 0, 1, -1]     # dam B's bit has no meaning
    with pytest.raises(ValueError):
        host.qtl_families(par, dous, 2)
    with pytest.raises(ValueError):
        host.qtl_families(par, np.array([13], np.int32), 0)


def test_fam_fstat_hand_numbers():
    """n_c = 20, 4 cells, K = 1, df = 3: the residual df is 20 - 4 - 1 - 3 = 12.  lod = 10 log10(2) is RSS0 / RSS1 = 2, so
    F = ((RSS0 - RSS1) / 3) / (RSS1 / 12) = 4"""
    lod = np.array([[10.0 * np.log10(2.0), 0.0, 1.0]])
    df = np.array([3, 0, 3], np.int32)
    F, d1, d2 = qtl.fam_fstat(lod, df, np.array([20]), np.array([4]), 1, chromstarts=np.array([0, 3]))
    assert list(d1[0]) == [3, 0, 3] and list(d2[0]) == [12, 0, 12]
    assert abs(F[0, 0] - 4.0) <= 1e-12 and np.isnan(F[0, 1])
    assert abs(F[0, 2] - (10.0 ** 0.1 - 1.0) * 12 / 3) <= 1e-12
    # per-marker n_used / n_cells, as scan_fam's [T][C] rows are expanded, give the same
    F2, _, _ = qtl.fam_fstat(lod, df, np.full(3, 20), np.full(3, 4), 1)
    assert np.array_equal(F, F2, equal_nan=True)


def test_refusals(host):
    origin, grp, cell, F, pheno, cov, use, _ = make_case(1, 0, 1, 0, True, False, False)
    o, y = origin[:, 0], pheno - pheno.mean(axis=0)
    ok = host.qtlfam_marker(o, 0, grp, F, y, cell=cell, cov=cov)
    assert ok["df"] > 0
    split = cell.copy()
    split[np.flatnonzero(grp == 3)[0]] = cell[np.flatnonzero(grp == 5)[0]]        # a cell with members of two groups
    for kw in (dict(side=2), dict(grp=np.where(grp == 6, F, grp)), dict(cell=split), dict(cell=np.where(grp == 2, -1, cell)),
               dict(cov=np.zeros((len(grp), 9))), dict(n_fam=0)):
        a = dict(side=0, grp=grp, n_fam=F, cell=cell, cov=cov)
        a.update(kw)
        with pytest.raises(ValueError):
            host.qtlfam_marker(o, a["side"], a["grp"], a["n_fam"], y, cell=a["cell"], cov=a["cov"])
