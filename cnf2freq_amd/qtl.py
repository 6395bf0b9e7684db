"""QTL scans on the origin rows: Context.qtl_scan / Context.sweep_qtl (cnf2_qtl_scan, cnf2_sweep_qtl) and how to read them.

The scan is Haley-Knott regression of phenotypes on a = P(BB) - P(AA) and d = P(AB) + P(BA) at every marker (the model:
include/cnf2hip.h); it runs on the GPU for the observed phenotypes and for every permuted one.  This module makes the
permutations, the residuals that are permuted when there are covariates (Freedman-Lane), turns the permutations' maxima into
thresholds and reads peaks with their LOD-drop support intervals off a profile.  Nothing here scans.

The pair scan (Context.qtl_scan2, cnf2_qtl_scan2) asks the next two questions -- is there a second locus, do two loci
interact -- for every pair of selected markers: scan2, thresholds2 and pair_summary are its counterparts here.

The extended scan (Context.qtl_scanx, cnf2_qtl_scanx) asks of every marker whether its effect depends on the parent it came
from (imprinting) and on a covariate (QTL x covariate interaction): scanx, coef_names and thresholdsx.

The maximum-likelihood scan (Context.qtl_scan_em, cnf2_qtl_scan_em) fits the normal mixture over the origin classes by EM
(interval mapping) where Haley-Knott regresses on their expectations: scan_em; thresholds and peaks read it as they read scan.

The binary-trait scan (Context.qtl_scan_binary, cnf2_qtl_scan_binary) fits a logistic regression of a 0/1 trait per marker:
scan_binary, read by thresholds and peaks in the same way.

The survival-trait scan (Context.qtl_scan_surv, cnf2_qtl_scan_surv) fits Cox's proportional hazards regression of a
time-to-event trait with censoring per marker: scan_surv, read by thresholds and peaks in the same way.

The variance-QTL scan (Context.qtl_scan_var, cnf2_qtl_scan_var) fits a mean part and a log-variance part per marker and gives
a joint, a mean and a variance LOD: scan_var, read by thresholds_var and peaks_var.

The cofactor scan (Context.qtl_scan_cof, cnf2_qtl_scan_cof) is composite interval mapping: every marker fitted together with
the loci found before, each left out inside its own window.  scan_cof with cofactor_windows asks whether there is a further
QTL, fit_multi (read_multi) reads the multiple-QTL model -- full LOD, drop-one LODs, effects -- off one call, and
forward_select builds the model a locus at a time against permutation thresholds.

The polygenic scan (Context.kinship_sums, Context.qtl_scan_cols; cnf2_kinship_sums, cnf2_qtl_scan_cols) drops the assumption
that individuals are independent given the tested locus: kinship makes the realised kinship from the origin rows (also
leaving one chromosome out), est_herit estimates the heritability, and scan_lmm scans the linear mixed model on columns
rotated by the kinship's eigenvectors; thresholds and peaks read it as they read scan.

The bootstrap scan (Context.qtl_scan_boot, cnf2_qtl_scan_boot) says where a QTL sits: bootstrap_counts draws the individuals
with replacement, scan_boot scans a chromosome again for every replicate in one call, and boot_interval turns the
replicates' best markers into a confidence interval of the position.  bayes_interval is the credible interval read off one
profile (the 10^LOD posterior); peaks keeps its LOD-drop interval.

The multi-trait scan (Context.qtl_scan_mv, cnf2_qtl_scan_mv) asks whether a locus moves several correlated traits jointly
(Wilks' lambda of multivariate Haley-Knott regression): scan_mv; thresholds and peaks read its one joint profile.

The multiple-imputation scan (Context.qtl_scan_imp, cnf2_qtl_scan_imp) fits scan's model to hard genotypes sampled from the
posterior and combines the draws on the likelihood scale: sample_states, sampled_classes and scan_imp; thresholds and peaks
read it as they read scan.

The within-family scan (Context.qtl_scan_fam, cnf2_qtl_scan_fam) drops the assumption that the founder lines are fixed for
different QTL alleles, which an outbred cross does not meet: every F1 parent on a side gets its own mean and its own
substitution effect on the bit of the origin rows that says which of its two alleles an offspring received (the nested
half-sib model of Knott, Elsen and Haley 1996).  families makes the slope groups and mean cells from a pedigree, scan_fam
scans one side or both with permutations inside the cells, and fam_fstat turns a profile into F statistics: the number of
fitted families varies along the map, so a bare LOD is not comparable between markers without it.  thresholds and peaks read
a side's profile as they read scan."""
import numpy as np

from . import synth


def permutations(n, P, seed, use=None, strata=None):
    """perm[P][n] (int32): permutation p gives individual i the phenotype of perm[p][i].  Within every stratum the used
    individuals, in ascending order idx[0..k), are ordered by the key synth.splitmix64(seed, p * n + i) with a stable
    argsort: perm[p][idx[j]] = idx[order[j]].  Unused individuals map to themselves.  No sequential generator enters, so
    the same lines in another language give the same arrays (cnf2h_qtl_permutations of the host library, which
    `cnF2freq --qtl` uses)."""
    use = np.ones(n, bool) if use is None else np.asarray(use) != 0
    strata = np.zeros(n, np.int64) if strata is None else np.asarray(strata)
    if use.shape != (n,) or strata.shape != (n,):
        raise ValueError("use and strata must be [n]")
    perm = np.tile(np.arange(n, dtype=np.int32), (P, 1))
    groups = [np.flatnonzero(use & (strata == s)) for s in np.unique(strata[use])] if use.any() else []
    for p in range(P):
        keys = synth.splitmix64(seed, np.uint64(p) * np.uint64(n) + np.arange(n, dtype=np.uint64))
        for idx in groups:
            perm[p, idx] = idx[np.argsort(keys[idx], kind="stable")]
    return perm


_permutations = permutations      # (scan's argument of the same name is a count)


def null_residuals(pheno, cov=None, use=None):
    """[n][T]: the residuals of every phenotype column on the null design [1, cov] over the used individuals (0 for the
    others).  With covariates a permutation test permutes these, not the raw values (Freedman and Lane 1983); without,
    the two give the same LODs."""
    y = np.asarray(pheno, np.float64)
    y = y[:, None] if y.ndim == 1 else y
    n = y.shape[0]
    use = np.ones(n, bool) if use is None else np.asarray(use) != 0
    X = np.ones((n, 1))
    if cov is not None:
        z = np.asarray(cov, np.float64)
        X = np.concatenate([X, z[:, None] if z.ndim == 1 else z], axis=1)
    res = np.zeros_like(y)
    if use.any():
        # (the columns minus their means over the used individuals: the residuals do not depend on offsets, the sums do)
        Xu, yu = X[use], y[use] - y[use].mean(axis=0)
        Xu[:, 1:] -= Xu[:, 1:].mean(axis=0)
        beta = np.linalg.lstsq(Xu, yu, rcond=None)[0]
        res[use] = yu - Xu @ beta
    return res


def origin_rows(ctx):
    """One origin sweep of the context's pedigree with the rows left on its GPU: a torch tensor [n][M][4] that scan and scan2
    take as `rows`, so that both run from one sweep."""
    import torch
    n, M, C = ctx.n_ind, ctx.n_markers, ctx.n_chrom
    dev = torch.device("cuda", ctx.device)          # the context's GPU, whatever torch's current one is
    t = lambda *shape, dtype=torch.float64: torch.zeros(shape, dtype=dtype, device=dev)
    d_f, d_l, d_o, d_s, d_c = t(n, C, 8), t(n, C), t(n, M, 4), t(M, 4), t(C, dtype=torch.int32)
    ctx.sweep_origins_device(0, n, d_f.data_ptr(), d_l.data_ptr(), d_o.data_ptr(), None, d_s.data_ptr(), d_c.data_ptr())
    ctx.sync()
    return d_o


def select_every(chromstarts, every=1):
    """sel: every `every`-th marker of each chromosome, from its first (what `cnF2freq --qtl2-every` selects)"""
    cs = np.asarray(chromstarts, np.int64)
    return np.concatenate([np.arange(cs[c], cs[c + 1], every) for c in range(len(cs) - 1)]).astype(np.int32)


def _patterns(y, use):
    """The columns of y[n][T] grouped by their pattern of missing (not finite) values, a pattern at the place of its first
    column: (cols, u) per pattern, u the individuals of use[n] that the pattern does not miss."""
    missing = ~np.isfinite(y)
    patterns = {}
    for k in range(y.shape[1]):
        patterns.setdefault(missing[:, k].tobytes(), []).append(k)
    for cols in patterns.values():
        yield cols, use & ~missing[:, cols[0]]


def pair_rows(ctx, sel):
    """One pair sweep of the context's pedigree for the markers sel[L] with the rows left on its GPU: a torch tensor
    [n][n_pairs][16] that scan2(linked=True) takes as `joint`."""
    import torch
    n, C = ctx.n_ind, ctx.n_chrom
    NP = len(ctx.linked_pairs(sel))
    dev = torch.device("cuda", ctx.device)
    t = lambda *shape, dtype=torch.float64: torch.zeros(shape, dtype=dtype, device=dev)
    d_f, d_l, d_j, d_s, d_c = t(n, C, 8), t(n, C), t(n, max(NP, 1), 16), t(max(NP, 1), 16), t(C, dtype=torch.int32)
    if NP:
        ctx.sweep_pairs_device(0, n, sel, d_f.data_ptr(), d_l.data_ptr(), d_j.data_ptr(), d_s.data_ptr(), d_c.data_ptr())
        ctx.sync()
    return d_j


def scan2(ctx, pheno, sel, cov=None, use=None, permutations=0, seed=0, additive=False, rows=None, linked=False, joint=None):
    """The pair scan of a whole cross on the context's uploaded pedigree, for every pair of the markers sel[L]: one origin
    sweep with the rows left on the device (or `rows`, the tensor origin_rows returned, e.g. the one a preceding scan used),
    then per pattern of missing phenotypes (NaN) one observed scan with the pattern's own `use`, and with permutations > 0
    one more on the permuted residuals of the null model, as scan does.  A dict: lod_add[T][L][L], lod_full[T][L][L],
    rank_add[T][L][L], rank_full[T][L][L], n_used[T][C][C], perm_max[P][T][3] or None (the maxima of lod_add, lod_full and
    lod_full - lod_add: thresholds2).
    linked=True: one pair sweep for sel as well, its rows left on the device (or `joint`, the tensor pair_rows returned), and
    the linked scan (cnf2_qtl_scan2_linked): the full model is fitted on the pairs of one chromosome too, and perm_max's
    second and third maxima run over all pairs.  The default is the scan without it, to the bit."""
    y = np.asarray(pheno, np.float64)
    y = y[:, None] if y.ndim == 1 else y
    n, T = y.shape
    if n != ctx.n_ind:
        raise ValueError("pheno must have a row per analysed individual (%d)" % ctx.n_ind)
    sel = np.ascontiguousarray(sel, np.int32)
    L, C = len(sel), ctx.n_chrom
    use = np.ones(n, bool) if use is None else np.asarray(use) != 0
    d_o = origin_rows(ctx) if rows is None else rows
    d_j = (pair_rows(ctx, sel) if joint is None else joint) if linked else None
    if linked:
        call = lambda ys, **kw: ctx.qtl_scan2_linked_device(n, d_o.data_ptr(), d_j.data_ptr(), sel, ys, cov=cov, additive=additive, **kw)
    else:
        call = lambda ys, **kw: ctx.qtl_scan2_device(n, d_o.data_ptr(), sel, ys, cov=cov, additive=additive, **kw)
    out = dict(lod_add=np.zeros((T, L, L)), lod_full=np.zeros((T, L, L)), rank_add=np.zeros((T, L, L), np.int32),
               rank_full=np.zeros((T, L, L), np.int32), n_used=np.zeros((T, C, C), np.int32),
               perm_max=np.zeros((permutations, T, 3)) if permutations else None)
    for cols, u in _patterns(y, use):
        yk = np.where(u[:, None], y[:, cols], 0.0)
        got = call(yk, use=u)
        for key in ("lod_add", "lod_full", "rank_add", "rank_full", "n_used"):
            out[key][cols] = got[key]
        if permutations:
            perm = _permutations(n, permutations, seed, use=u)
            res = null_residuals(yk, cov, u)
            out["perm_max"][:, cols] = call(res, use=u, perm=perm)["perm_max"]
    return out


def thresholds2(perm_max, alpha=(0.05, 0.01)):
    """From perm_max[P][T][3] of a pair scan: add, full and int, each [len(alpha)][T] -- the genome-wide thresholds of the
    largest additive-pair LOD, the largest full LOD and the largest lod_full - lod_add, by the order statistic of
    thresholds()."""
    pm = np.asarray(perm_max, np.float64)
    if pm.ndim != 3 or pm.shape[0] == 0 or pm.shape[2] != 3:
        raise ValueError("perm_max must be [P][T][3] with P >= 1")
    srt = np.sort(pm, axis=0)
    idx = [quantile_index(pm.shape[0], a) for a in alpha]
    return dict(alpha=tuple(alpha), add=srt[idx, :, 0], full=srt[idx, :, 1], int=srt[idx, :, 2])


def pair_summary(lod_add, lod_full, sel, chromstarts):
    """The usual summary of a two-dimensional scan.  Per trait and chromosome pair c1 <= c2 that holds a pair of selected
    loci, a dict: trait, chrom1, chrom2; add = (marker 1, marker 2) of the best additive pair and lod_add its LOD; and for
    c1 != c2 full = the best full pair, lod_full its LOD, lod_add_at_full the additive LOD there, and
    lod_int = lod_full - lod_add, the best full against the best additive model of the chromosome pair.  On one chromosome
    the plain scan fits only the additive model -- full is None and lod_full, lod_add_at_full, lod_int are NaN -- and the
    linked scan (scan2(linked=True)) the full one too: where its lod_full is there, the entry is filled like any other.  The
    first pair in (j, k) order wins a tie."""
    la, lf = np.asarray(lod_add, np.float64), np.asarray(lod_full, np.float64)
    la, lf = (la[None] if la.ndim == 2 else la), (lf[None] if lf.ndim == 2 else lf)
    sel = np.asarray(sel, np.int64)
    L = len(sel)
    if la.shape[1:] != (L, L) or lf.shape != la.shape:
        raise ValueError("lod_add and lod_full must be [T][L][L] with L = len(sel)")
    cs = np.asarray(chromstarts, np.int64)
    sc = np.searchsorted(cs, sel, side="right") - 1
    found = []
    for t in range(la.shape[0]):
        for c1 in range(len(cs) - 1):
            for c2 in range(c1, len(cs) - 1):
                jj, kk = np.flatnonzero(sc == c1), np.flatnonzero(sc == c2)
                pairs = [(j, k) for j in jj for k in kk if j < k]
                if not pairs:
                    continue
                pj, pk = np.array(pairs).T
                ia = int(np.argmax(la[t, pj, pk]))
                r = dict(trait=t, chrom1=c1, chrom2=c2, add=(int(sel[pj[ia]]), int(sel[pk[ia]])), lod_add=float(la[t, pj[ia], pk[ia]]),
                         full=None, lod_full=np.nan, lod_add_at_full=np.nan, lod_int=np.nan)
                if c1 != c2 or not np.isnan(lf[t, pj, pk]).any():
                    i = int(np.argmax(lf[t, pj, pk]))
                    r.update(full=(int(sel[pj[i]]), int(sel[pk[i]])), lod_full=float(lf[t, pj[i], pk[i]]),
                             lod_add_at_full=float(la[t, pj[i], pk[i]]))
                    r["lod_int"] = r["lod_full"] - r["lod_add"]
                found.append(r)
    return found


def scan(ctx, pheno, cov=None, use=None, permutations=0, seed=0, additive=False, rows=None):
    """The scan of a whole cross on the context's uploaded pedigree: one origin sweep with the rows left on the device, then
    per pattern of missing phenotypes (NaN) one observed scan with the pattern's own `use`, and with permutations > 0 one
    more on the permuted residuals of the null model.  A dict: lod[T][M], coef[T][M][2], rank[T][M] (the design, and with
    it the rank, depends on who is used), n_used[T][C], perm_max[P][T][C] or None.  rows: the tensor of origin_rows, instead
    of a sweep of this call's own (scan and scan2 of one cross from one sweep)."""
    y = np.asarray(pheno, np.float64)
    y = y[:, None] if y.ndim == 1 else y
    n, T = y.shape
    if n != ctx.n_ind:
        raise ValueError("pheno must have a row per analysed individual (%d)" % ctx.n_ind)
    use = np.ones(n, bool) if use is None else np.asarray(use) != 0
    M, C = ctx.n_markers, ctx.n_chrom
    d_o = origin_rows(ctx) if rows is None else rows
    out = dict(lod=np.zeros((T, M)), coef=np.full((T, M, 2), np.nan), rank=np.zeros((T, M), np.int32),
               n_used=np.zeros((T, C), np.int32), perm_max=np.zeros((permutations, T, C)) if permutations else None)
    for cols, u in _patterns(y, use):
        yk = np.where(u[:, None], y[:, cols], 0.0)
        got = ctx.qtl_scan_device(n, d_o.data_ptr(), yk, cov=cov, use=u, additive=additive)
        out["lod"][cols], out["coef"][cols] = got["lod"], got["coef"]
        out["rank"][cols], out["n_used"][cols] = got["rank"], got["n_used"]
        if permutations:
            perm = _permutations(n, permutations, seed, use=u)
            res = null_residuals(yk, cov, u)
            out["perm_max"][:, cols] = ctx.qtl_scan_device(n, d_o.data_ptr(), res, cov=cov, use=u, perm=perm,
                                                           additive=additive)["perm_max"]
    return out


def families(ped, side):
    """(grp[n], cell[n], F) of the analysed individuals of a pedigree (anything with par[R][2] and dous[n]: a
    synth.Pedigree, a Context after upload) for the within-family scan: grp the F1 parent on the side (0 or "first": par[.][0],
    1 or "second": par[.][1]) and cell the pair of parents, both numbered from 0 in ascending order of the records; -1 where
    that parent is missing or has no recorded parents, so that its bit of the origin rows has no meaning.  F the parents
    counted.  (cnf2h_qtl_families of the host library, which `cnF2freq --qtlfam` uses.)"""
    from . import host
    return host.qtl_families(ped.par, ped.dous, _side(side))


def _side(side):
    if side in (0, 1):
        return int(side)
    if side in ("first", "second"):
        return 0 if side == "first" else 1
    raise ValueError("side must be 0, 1, 'first', 'second' or 'both'")


def cell_residuals(pheno, cell, cov=None, use=None):
    """null_residuals of the within-family scan's null model: a mean per cell[n] and the covariates, over the used
    individuals (0 for the others).  These are what scan_fam permutes inside the cells."""
    y = np.asarray(pheno, np.float64)
    y = y[:, None] if y.ndim == 1 else y
    n = y.shape[0]
    use = np.ones(n, bool) if use is None else np.asarray(use) != 0
    cell = np.asarray(cell)
    res = np.zeros_like(y)
    if use.any():
        ids = np.unique(cell[use])
        X = (cell[use][:, None] == ids[None, :]).astype(np.float64)
        if cov is not None:
            z = np.asarray(cov, np.float64).reshape(n, -1)[use]
            X = np.concatenate([X, z - z.mean(axis=0)], axis=1)
        yu = y[use] - y[use].mean(axis=0)
        res[use] = yu - X @ np.linalg.lstsq(X, yu, rcond=None)[0]
    return res


def scan_fam(ctx, pheno, side="both", grp=None, cell=None, cov=None, use=None, permutations=0, seed=0, rows=None, slopes=False):
    """The within-family scan of a whole cross on the context's uploaded pedigree: one origin sweep with the rows left on the
    device (or `rows`, the tensor of origin_rows), then per pattern of missing phenotypes (NaN) one observed scan with the
    pattern's own `use`, and with permutations > 0 one more on the residuals of the cell-centred null model (cell_residuals),
    permuted inside the cells (permutations(..., strata=cell)).  grp / cell: the slope groups and mean cells (None: families
    of the uploaded pedigree -- the parent on the side and the pair of parents).  A dict: lod[T][M], df[T][M] (the design, and
    with it df, depends on who is used), slope[T][M][F] with slopes, rss0[T][C], n_used[T][C], n_cells[T][C], n_fam,
    perm_max[P][T][C] or None.  side "both": two calls, {"first": dict, "second": dict}; grp and cell are then pairs."""
    if side == "both":
        pair = lambda a: (None, None) if a is None else a
        d_o = origin_rows(ctx) if rows is None else rows
        return {name: scan_fam(ctx, pheno, name, pair(grp)[k], pair(cell)[k], cov, use, permutations, seed, d_o, slopes)
                for k, name in enumerate(("first", "second"))}
    side = _side(side)
    y = np.asarray(pheno, np.float64)
    y = y[:, None] if y.ndim == 1 else y
    n, T = y.shape
    if n != ctx.n_ind:
        raise ValueError("pheno must have a row per analysed individual (%d)" % ctx.n_ind)
    if grp is None:
        grp, fam_cell, F = families(ctx, side)
        cell = fam_cell if cell is None else cell
    else:
        grp = np.asarray(grp, np.int32)
        F = int(grp.max()) + 1 if (grp >= 0).any() else 1
    cell = grp if cell is None else np.asarray(cell, np.int32)
    use = (np.ones(n, bool) if use is None else np.asarray(use) != 0) & (grp >= 0)
    M, C = ctx.n_markers, ctx.n_chrom
    d_o = origin_rows(ctx) if rows is None else rows
    out = dict(lod=np.zeros((T, M)), df=np.zeros((T, M), np.int32), slope=np.full((T, M, F), np.nan) if slopes else None,
               rss0=np.zeros((T, C)), n_used=np.zeros((T, C), np.int32), n_cells=np.zeros((T, C), np.int32), n_fam=F,
               perm_max=np.zeros((permutations, T, C)) if permutations else None)
    call = lambda ys, u, **kw: ctx.qtl_scan_fam_device(n, d_o.data_ptr(), side, grp, F, ys, cell=cell, cov=cov, use=u, **kw)
    for cols, u in _patterns(y, use):
        yk = np.where(u[:, None], y[:, cols], 0.0)
        got = call(yk, u, slopes=slopes)
        out["lod"][cols], out["df"][cols], out["rss0"][cols] = got["lod"], got["df"], got["rss0"]
        out["n_used"][cols], out["n_cells"][cols] = got["n_used"], got["n_cells"]
        if slopes:
            out["slope"][cols] = got["slope"]
        if permutations:
            perm = _permutations(n, permutations, seed, use=u, strata=cell)
            out["perm_max"][:, cols] = call(cell_residuals(yk, cell, cov, u), u, perm=perm)["perm_max"]
    return out


def descent_rows(ctx):
    """One descent sweep of the context's pedigree with the rows left on its GPU: a torch tensor [n][M][8] that scan_hap takes
    as `rows`."""
    import torch
    n, M, C = ctx.n_ind, ctx.n_markers, ctx.n_chrom
    dev = torch.device("cuda", ctx.device)
    t = lambda *shape, dtype=torch.float64: torch.zeros(shape, dtype=dtype, device=dev)
    d_f, d_l, d_d, d_c = t(n, C, 8), t(n, C), t(n, M, 8), t(C, dtype=torch.int32)
    ctx.sweep_descent_device(0, n, d_f.data_ptr(), d_l.data_ptr(), d_d.data_ptr(), d_c.data_ptr())
    ctx.sync()
    return d_d


def scan_hap(ctx, ped, pheno, cov=None, by="haplotype", use=None, permutations=0, seed=0, rows=None, col=None, n_columns=None,
             coef=True):
    """The founder-haplotype scan of a whole cross on the context's uploaded pedigree `ped` (anything with par[R][2] and dous[n]):
    one descent sweep with the rows left on the device (or `rows`, the tensor of descent_rows), the column map
    origins.descent_columns(ped.par, ped.dous, by) -- "haplotype": an effect per founder haplotype, "founder": per founder, "line":
    per position in the parents' entries -- or col[n][8] with n_columns, then per pattern of missing phenotypes (NaN) one observed
    scan with the pattern's own `use`, and with permutations > 0 one more on the permuted residuals of the null model, as scan
    does.  A dict: lod[T][M], df[T][M] (the design, and with it df, depends on who is used), coef[T][M][H] with coef (NaN for a
    dropped column), rss0[T][C], n_used[T][C], col, n_columns, perm_max[P][T][C] or None."""
    from . import origins
    y = np.asarray(pheno, np.float64)
    y = y[:, None] if y.ndim == 1 else y
    n, T = y.shape
    if n != ctx.n_ind:
        raise ValueError("pheno must have a row per analysed individual (%d)" % ctx.n_ind)
    if col is None:
        col, grand = origins.descent_columns(ped.par, ped.dous, by)
        H = {"haplotype": 2 * len(grand), "founder": len(grand), "line": 2}[by]
    else:
        col = np.ascontiguousarray(col, np.int32)
        H = int(col.max()) + 1 if n_columns is None else int(n_columns)
    H = max(H, 1)
    use = np.ones(n, bool) if use is None else np.asarray(use) != 0
    M, C = ctx.n_markers, ctx.n_chrom
    d_d = descent_rows(ctx) if rows is None else rows
    out = dict(lod=np.zeros((T, M)), df=np.zeros((T, M), np.int32), coef=np.full((T, M, H), np.nan) if coef else None,
               rss0=np.zeros((T, C)), n_used=np.zeros((T, C), np.int32), col=col, n_columns=H,
               perm_max=np.zeros((permutations, T, C)) if permutations else None)
    call = lambda ys, u, **kw: ctx.qtl_scan_hap_device(n, d_d.data_ptr(), col, H, ys, cov=cov, use=u, **kw)
    for cols, u in _patterns(y, use):
        yk = np.where(u[:, None], y[:, cols], 0.0)
        got = call(yk, u, coef=coef)
        out["lod"][cols], out["df"][cols], out["rss0"][cols], out["n_used"][cols] = got["lod"], got["df"], got["rss0"], got["n_used"]
        if coef:
            out["coef"][cols] = got["coef"]
        if permutations:
            in_model = u & (col >= 0).all(axis=1)
            perm = _permutations(n, permutations, seed, use=in_model)
            out["perm_max"][:, cols] = call(null_residuals(yk, cov, in_model), in_model, perm=perm, coef=False)["perm_max"]
    return out


def scan_vc(ctx, ped, pheno, cov=None, by="haplotype", use=None, permutations=0, seed=0, rows=None, col=None, n_columns=None,
            blup=True):
    """The variance-component scan of a whole cross on the context's uploaded pedigree `ped`, in the shape of scan_hap: random
    effects of the founder haplotypes (up to 64 columns), one variance component per locus (cnf2_qtl_scan_vc).  One descent sweep
    with the rows left on the device (or `rows`), the column map of `by` or col[n][8] with n_columns, then per pattern of missing
    phenotypes (NaN) one observed scan with the pattern's own `use`, and with permutations > 0 one more on the permuted
    residuals of the null model.  A dict: lod[T][M], h[T][M] the locus' share of the variance, sigma2_e[T][M],
    sigma2_u[T][M] = h / (1 - h) sigma2_e, blup[T][M][H] with blup (the predicted founder-allele effects, 0 where the LOD is 0),
    rank[T][M] and eval[T][M][H] (the design, and with it both, depends on who is used), rss0[T][C], n_used[T][C], col,
    n_columns, perm_max[P][T][C] or None.  thresholds and peaks read it as they read scan."""
    from . import origins
    y = np.asarray(pheno, np.float64)
    y = y[:, None] if y.ndim == 1 else y
    n, T = y.shape
    if n != ctx.n_ind:
        raise ValueError("pheno must have a row per analysed individual (%d)" % ctx.n_ind)
    if col is None:
        col, grand = origins.descent_columns(ped.par, ped.dous, by)
        H = {"haplotype": 2 * len(grand), "founder": len(grand), "line": 2}[by]
    else:
        col = np.ascontiguousarray(col, np.int32)
        H = int(col.max()) + 1 if n_columns is None else int(n_columns)
    H = max(H, 1)
    use = np.ones(n, bool) if use is None else np.asarray(use) != 0
    M, C = ctx.n_markers, ctx.n_chrom
    d_d = descent_rows(ctx) if rows is None else rows
    out = dict(lod=np.zeros((T, M)), h=np.zeros((T, M)), sigma2_e=np.zeros((T, M)), sigma2_u=np.zeros((T, M)),
               blup=np.zeros((T, M, H)) if blup else None, rank=np.zeros((T, M), np.int32), eval=np.zeros((T, M, H)),
               rss0=np.zeros((T, C)), n_used=np.zeros((T, C), np.int32), col=col, n_columns=H,
               perm_max=np.zeros((permutations, T, C)) if permutations else None)
    call = lambda ys, u, **kw: ctx.qtl_scan_vc_device(n, d_d.data_ptr(), col, H, ys, cov=cov, use=u, **kw)
    for cols, u in _patterns(y, use):
        yk = np.where(u[:, None], y[:, cols], 0.0)
        got = call(yk, u, blup=blup)
        out["lod"][cols], out["h"][cols], out["sigma2_e"][cols] = got["lod"], got["h"], got["sigma2"]
        out["sigma2_u"][cols] = got["h"] / (1.0 - got["h"]) * got["sigma2"]
        out["rank"][cols], out["eval"][cols], out["rss0"][cols], out["n_used"][cols] = got["rank"], got["eval"], got["rss0"], got["n_used"]
        if blup:
            out["blup"][cols] = got["blup"]
        if permutations:
            in_model = u & (col >= 0).all(axis=1)
            perm = _permutations(n, permutations, seed, use=in_model)
            out["perm_max"][:, cols] = call(null_residuals(yk, cov, in_model), in_model, perm=perm, blup=False, evals=False)["perm_max"]
    return out


def hap_fstat(lod, df, n_used, K, chromstarts=None):
    """(F, df1, df2) of a founder-haplotype profile: lod[T][M] and df[M] or [T][M] of scan_hap, n_used per marker or, with
    chromstarts, per chromosome.  df1 = df, df2 = n_c - 1 - K - df: fam_fstat with the intercept as the one cell.  df varies
    along the map, so a bare LOD is not comparable between markers without it."""
    return fam_fstat(lod, df, n_used, np.ones_like(np.asarray(n_used)), K, chromstarts)


def fam_fstat(lod, df, n_used, n_cells, K, chromstarts=None):
    """(F, df1, df2) of a within-family profile: lod[T][M] and df[M] or [T][M] of scan_fam, n_used and n_cells per marker
    (anything that broadcasts against lod) or, with chromstarts, per chromosome ([C] or [T][C]).  RSS0 / RSS1 = 10^(2 lod /
    n_c), df1 = df, df2 = n_c - n_cells - K - df and F = (RSS0 / RSS1 - 1) df2 / df1: under the null an F(df1, df2) variate
    at every marker, whatever its number of fitted families.  NaN, with df2 = 0, where nothing is fitted."""
    lod = np.asarray(lod, np.float64)
    df1 = np.broadcast_to(np.asarray(df), lod.shape).astype(np.int64)
    if chromstarts is not None:
        reps = np.diff(np.asarray(chromstarts, np.int64))
        n_used, n_cells = np.repeat(np.asarray(n_used), reps, axis=-1), np.repeat(np.asarray(n_cells), reps, axis=-1)
    n_c = np.broadcast_to(np.asarray(n_used), lod.shape).astype(np.int64)
    df2 = np.where(df1 > 0, n_c - np.broadcast_to(np.asarray(n_cells), lod.shape) - K - df1, 0)
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = 10.0 ** (2.0 * lod / np.maximum(n_c, 1))
        F = np.where(df1 > 0, (ratio - 1.0) * df2 / np.maximum(df1, 1), np.nan)
    return F, df1, df2


def sampled_classes(state):
    """The origin class k = bit0 + 2 bit3 of sampled states below 64 (uint8, any shape) -- the class whose probability is
    origin[k] of sweep_origins; 255 (skipped) stays 255.  A value in 64 .. 254 is no state: ValueError."""
    g = np.asarray(state)
    if g.dtype != np.uint8:
        raise ValueError("states are uint8")
    if ((g >= 64) & (g != 255)).any():
        raise ValueError("a state is in 64 .. 254")
    return np.where(g == 255, 255, (g & 1) + ((g >> 2) & 2)).astype(np.uint8)


def sample_states(ctx, draws, seed=0):
    """One sampling sweep of the context's pedigree with the states left on its GPU: a torch tensor [n][draws][M] (uint8) that
    scan_imp takes as `states`, as origin_rows is to scan."""
    import torch
    n, M, C = ctx.n_ind, ctx.n_markers, ctx.n_chrom
    dev = torch.device("cuda", ctx.device)
    d_f = torch.zeros((n, C, 8), dtype=torch.float64, device=dev)
    d_l = torch.zeros((n, C), dtype=torch.float64, device=dev)
    d_s = torch.zeros((n, draws, M), dtype=torch.uint8, device=dev)
    d_h = torch.zeros((n, draws, C), dtype=torch.int32, device=dev)
    ctx.sweep_sample_device(0, n, draws, seed, d_f.data_ptr(), d_l.data_ptr(), d_s.data_ptr(), d_h.data_ptr())
    ctx.sync()
    return d_s


def scan_imp(ctx, pheno, draws=16, seed=0, cov=None, use=None, permutations=0, perm_seed=0, additive=False, states=None,
             draw_lods=False):
    """The multiple-imputation scan of a whole cross on the context's uploaded pedigree (Context.qtl_scan_imp_device,
    cnf2_qtl_scan_imp): `draws` inheritance paths per individual sampled from the posterior (seed; or `states`, the tensor
    of sample_states), the model of scan fitted to the hard genotypes of every draw, and the draws combined on the likelihood
    scale -- the remedy where the origin rows are soft and Haley-Knott regression misjudges the residual variance.  NaN is a
    missing phenotype; per pattern of missing values one observed scan with the pattern's own `use`, and with permutations
    > 0 one more on the permuted residuals of the null model (perm_seed), whose maxima are taken over the combined profile.
    A dict as scan's -- lod[T][M], coef[T][M][2], rank[T][M], n_used[T][C], perm_max[P][T][C] or None -- plus
    draw_lod[draws][T][M] with draw_lods (else None); thresholds and peaks read it as they read scan's.  Positions between
    markers need blank columns in the uploaded map (origins.with_positions), so that the sampler visits them."""
    y = np.asarray(pheno, np.float64)
    y = y[:, None] if y.ndim == 1 else y
    if y.ndim != 2 or y.shape[0] != ctx.n_ind:
        raise ValueError("pheno must have a row per analysed individual (%d)" % ctx.n_ind)
    n, T = y.shape
    M, C = ctx.n_markers, ctx.n_chrom
    if permutations < 0:
        raise ValueError("permutations must not be negative")
    use = np.ones(n, bool) if use is None else np.asarray(use) != 0
    if use.shape != (n,):
        raise ValueError("use must be [n]")
    if states is None:
        if not 1 <= int(draws) <= 1024:
            raise ValueError("draws must be 1 .. 1024")
        states = sample_states(ctx, int(draws), seed)
    if tuple(states.shape[::2]) != (n, M) or len(states.shape) != 3 or not 1 <= states.shape[1] <= 1024:
        raise ValueError("states must be [%d][draws][%d] with 1 .. 1024 draws" % (n, M))
    D = int(states.shape[1])
    out = dict(lod=np.zeros((T, M)), coef=np.full((T, M, 2), np.nan), rank=np.zeros((T, M), np.int32),
               n_used=np.zeros((T, C), np.int32), perm_max=np.zeros((permutations, T, C)) if permutations else None,
               draw_lod=np.zeros((D, T, M)) if draw_lods else None)
    for cols, u in _patterns(y, use):
        yk = np.where(u[:, None], y[:, cols], 0.0)
        got = ctx.qtl_scan_imp_device(n, D, states.data_ptr(), yk, cov=cov, use=u, additive=additive, draw_lods=draw_lods)
        out["lod"][cols], out["coef"][cols] = got["lod"], got["coef"]
        out["rank"][cols], out["n_used"][cols] = got["rank"], got["n_used"]
        if draw_lods:
            out["draw_lod"][:, cols] = got["draw_lod"]
        if permutations:
            perm = _permutations(n, permutations, perm_seed, use=u)
            res = null_residuals(yk, cov, u)
            out["perm_max"][:, cols] = ctx.qtl_scan_imp_device(n, D, states.data_ptr(), res, cov=cov, use=u, perm=perm,
                                                               additive=additive)["perm_max"]
    return out


def scan_mv(ctx, pheno, cov=None, use=None, permutations=0, seed=0, additive=False, rows=None):
    """The multi-trait scan of a whole cross on the context's uploaded pedigree (Context.qtl_scan_mv_device,
    cnf2_qtl_scan_mv): is there a locus that moves the T <= 16 traits of pheno[n][T] jointly?  Complete cases only: an
    individual with any trait that is not finite leaves `use`.  One origin sweep with the rows left on the device (or `rows`,
    the tensor of origin_rows), the observed scan, and with permutations > 0 one more, on the permuted residuals of the null
    model where there are covariates (a permutation moves all traits of an individual together).  A dict: lod[M] the joint
    LOD, rank[M], trait_rank[C] the traits kept, n_used[C], and perm_max[P][1][C] or None -- shaped so that thresholds and
    peaks read it as they read scan's."""
    y = np.asarray(pheno, np.float64)
    y = y[:, None] if y.ndim == 1 else y
    n = y.shape[0]
    if n != ctx.n_ind:
        raise ValueError("pheno must have a row per analysed individual (%d)" % ctx.n_ind)
    u = (np.ones(n, bool) if use is None else np.asarray(use) != 0) & np.isfinite(y).all(axis=1)
    d_o = origin_rows(ctx) if rows is None else rows
    yk = np.where(u[:, None], y, 0.0)
    got = ctx.qtl_scan_mv_device(n, d_o.data_ptr(), yk, cov=cov, use=u, additive=additive)
    out = dict(lod=got["lod"], rank=got["rank"], trait_rank=got["trait_rank"], n_used=got["n_used"], perm_max=None)
    if permutations:
        perm = _permutations(n, permutations, seed, use=u)
        res = yk if cov is None else null_residuals(yk, cov, u)
        out["perm_max"] = ctx.qtl_scan_mv_device(n, d_o.data_ptr(), res, cov=cov, use=u, perm=perm,
                                                 additive=additive)["perm_max"][:, None, :]
    return out


def coef_names(interactive=0, imprint=False, additive=False, cov_names=None):
    """The names of scanx's coef entries in their order: the main effects "a", "d" (unless additive), "i" (with imprint),
    then for every interactive covariate the same effects as "a:z1", ...; cov_names replaces z1, z2, ..."""
    eff = ["a"] + ([] if additive else ["d"]) + (["i"] if imprint else [])
    zs = ["z%d" % (k + 1) for k in range(interactive)] if cov_names is None else list(cov_names)[:interactive]
    if len(zs) != interactive:
        raise ValueError("cov_names must name every interactive covariate")
    return tuple(eff + ["%s:%s" % (e, z) for z in zs for e in eff])


def scanx(ctx, pheno, cov=None, interactive=0, imprint=False, use=None, permutations=0, seed=0, additive=False, rows=None):
    """The extended scan of a whole cross on the context's uploaded pedigree: as scan -- one origin sweep with the rows left on
    the device (or `rows`, the tensor of origin_rows), per pattern of missing phenotypes (NaN) one observed scan with the
    pattern's own `use`, and with permutations > 0 one more on the permuted residuals of the null model -- with the nested
    models Mendelian (a, d), imprinting (+ i, with imprint) and interaction (+ the products with the first `interactive`
    columns of cov).  A dict: lod[T][M][3], lod_imprint = lod[..., 1] - lod[..., 0], lod_interaction = lod[..., 2] -
    lod[..., 1] (both [T][M]), coef[T][M][len(coef_names)], coef_names, rank[T][M][3], n_used[T][C],
    perm_max[P][T][C][5] or None (thresholdsx)."""
    y = np.asarray(pheno, np.float64)
    y = y[:, None] if y.ndim == 1 else y
    n, T = y.shape
    if n != ctx.n_ind:
        raise ValueError("pheno must have a row per analysed individual (%d)" % ctx.n_ind)
    K = 0 if cov is None else np.asarray(cov).reshape(n, -1).shape[1]
    if not 0 <= interactive <= K:
        raise ValueError("interactive must be 0 .. %d, the number of covariates" % K)
    use = np.ones(n, bool) if use is None else np.asarray(use) != 0
    M, C = ctx.n_markers, ctx.n_chrom
    names = coef_names(interactive, imprint, additive)
    d_o = origin_rows(ctx) if rows is None else rows
    out = dict(lod=np.zeros((T, M, 3)), coef=np.full((T, M, len(names)), np.nan), coef_names=names,
               rank=np.zeros((T, M, 3), np.int32), n_used=np.zeros((T, C), np.int32),
               perm_max=np.zeros((permutations, T, C, 5)) if permutations else None)
    kw = dict(cov=cov, interactive=interactive, imprint=imprint, additive=additive)
    for cols, u in _patterns(y, use):
        yk = np.where(u[:, None], y[:, cols], 0.0)
        got = ctx.qtl_scanx_device(n, d_o.data_ptr(), yk, use=u, **kw)
        out["lod"][cols], out["coef"][cols] = got["lod"], got["coef"]
        out["rank"][cols], out["n_used"][cols] = got["rank"], got["n_used"]
        if permutations:
            perm = _permutations(n, permutations, seed, use=u)
            res = null_residuals(yk, cov, u)
            out["perm_max"][:, cols] = ctx.qtl_scanx_device(n, d_o.data_ptr(), res, use=u, perm=perm, **kw)["perm_max"]
    out["lod_imprint"] = out["lod"][..., 1] - out["lod"][..., 0]
    out["lod_interaction"] = out["lod"][..., 2] - out["lod"][..., 1]
    return out


def _fit_columns(ctx, a, what):
    """a as float64 [n][T] (a vector is one column) with a row per analysed individual"""
    a = np.asarray(a, np.float64)
    a = a[:, None] if a.ndim == 1 else a
    n, T = a.shape
    if n != ctx.n_ind:
        raise ValueError("%s must have a row per analysed individual (%d)" % (what, ctx.n_ind))
    return a


def _fit_iterations(max_iter, most, tol):
    if not 1 <= int(max_iter) <= most:
        raise ValueError("max_iter must be 1 .. %d" % most)
    if not np.isfinite(tol):
        raise ValueError("tol must be finite")


def _fit_scan(ctx, call, ys, use, rows, permutations, seed, strata, kw, coef=("coef",), marker=(), chrom=(), fits=(),
              residuals=False):
    """What scan_em, scan_binary, scan_surv and scan_var share.  call: the context's method of the scan on device rows, kw
    its keyword arguments; ys: its column arrays [n][T], the first one's missing values giving the patterns.  The dict:
    lod[T][M], the arrays of `coef` [T][M][len(coef_names)], coef_names, those of `marker` [T][M], iters, status, rank[T][M],
    those of `chrom` (key, dtype) [T][C], n_used[T][C], perm_max[P][T][C] or None; lod, iters, status and perm_max with the
    axes `fits` behind.  Per pattern one call on the pattern's own `use`, copied back by key.  Its permutations (within
    `strata`) go with that call, which permutes the raw values -- or with residuals, in a second call on the null model's
    residuals."""
    n, T = ys[0].shape
    M, C, P = ctx.n_markers, ctx.n_chrom, permutations
    names = coef_names(0, kw["imprint"], kw["additive"])
    use = np.ones(n, bool) if use is None else np.asarray(use) != 0
    d_o = origin_rows(ctx) if rows is None else rows
    out = dict(lod=np.zeros((T, M) + fits))
    out.update((key, np.full((T, M, len(names)), np.nan)) for key in coef)
    out["coef_names"] = names
    out.update((key, np.full((T, M), np.nan)) for key in marker)
    out.update(iters=np.zeros((T, M) + fits, np.int32), status=np.zeros((T, M) + fits, np.int32), rank=np.zeros((T, M), np.int32))
    out.update((key, np.zeros((T, C), dtype)) for key, dtype in chrom)
    out.update(n_used=np.zeros((T, C), np.int32), perm_max=np.zeros((P, T, C) + fits) if P else None)
    keys = [key for key in out if key not in ("coef_names", "perm_max")]
    for cols, u in _patterns(ys[0], use):
        yk = [np.where(u[:, None], a[:, cols], 0.0) for a in ys]
        perm = _permutations(n, P, seed, use=u, strata=strata) if P else None
        got = call(n, d_o.data_ptr(), *yk, use=u, perm=None if residuals else perm, **kw)
        for key in keys:
            out[key][cols] = got[key]
        if P:
            if residuals:
                got = call(n, d_o.data_ptr(), null_residuals(yk[0], kw["cov"], u), use=u, perm=perm, **kw)
            out["perm_max"][:, cols] = got["perm_max"]
    return out


def scan_em(ctx, pheno, cov=None, imprint=False, use=None, permutations=0, seed=0, additive=False, max_iter=1000, tol=1e-6,
            rows=None):
    """The maximum-likelihood scan of a whole cross on the context's uploaded pedigree: as scan -- one origin sweep with the
    rows left on the device (or `rows`, the tensor of origin_rows), per pattern of missing phenotypes (NaN) one observed scan
    with the pattern's own `use`, and with permutations > 0 one more on the permuted residuals of the null model -- with
    every (marker, trait) fitted by EM from the null start until the log-likelihood gains less than tol LOD or max_iter
    iterations are done.  A dict: lod[T][M], coef[T][M][len(coef_names)], coef_names ("a", "d" unless additive, "i" with
    imprint), sigma2[T][M], iters[T][M], status[T][M] (0 = stopped by tol, 1 = by max_iter, 2 = breakdown), rank[T][M],
    n_used[T][C], perm_max[P][T][C] or None (thresholds)."""
    y = _fit_columns(ctx, pheno, "pheno")
    _fit_iterations(max_iter, 10000, tol)
    kw = dict(cov=cov, imprint=imprint, additive=additive, max_iter=max_iter, tol=tol)
    return _fit_scan(ctx, ctx.qtl_scan_em_device, (y,), use, rows, permutations, seed, None, kw, marker=("sigma2",), residuals=True)


def scan_binary(ctx, pheno, cov=None, imprint=False, use=None, permutations=0, seed=0, strata=None, additive=False, max_iter=50,
                tol=1e-7, rows=None):
    """The binary-trait scan of a whole cross on the context's uploaded pedigree: as scan_em -- one origin sweep with the rows
    left on the device (or `rows`, the tensor of origin_rows) and per pattern of missing phenotypes (NaN) one observed scan
    with the pattern's own `use` -- with every (marker, trait) a logistic regression of the 0/1 trait on the covariates and
    the effects a, d (unless additive), i (with imprint), fitted by Newton's method from the null fit until the log-likelihood
    gains less than tol LOD or max_iter iterations are done.  A finite phenotype other than 0 or 1 raises ValueError.
    With permutations > 0 the raw 0/1 values are permuted (the residuals of Freedman and Lane do not exist for this model),
    within the strata of `strata` (qtl.permutations): with covariates the permutations are valid only within strata of the
    covariates, which the caller supplies.  A dict: lod[T][M], coef[T][M][len(coef_names)], coef_names, iters[T][M],
    status[T][M] (0 = stopped by tol, 1 = by max_iter, 2 = breakdown, e.g. a separated marker), rank[T][M], ll0[T][C] (the
    null model's log-likelihood, 0 where the trait is not scanned on the chromosome), n_ones[T][C], n_used[T][C],
    perm_max[P][T][C] or None (thresholds)."""
    y = _fit_columns(ctx, pheno, "pheno")
    _fit_iterations(max_iter, 1000, tol)
    if not np.all(~np.isfinite(y) | (y == 0.0) | (y == 1.0)):
        raise ValueError("a binary trait is 0 or 1 (NaN where it is missing)")
    kw = dict(cov=cov, imprint=imprint, additive=additive, max_iter=max_iter, tol=tol)
    return _fit_scan(ctx, ctx.qtl_scan_binary_device, (y,), use, rows, permutations, seed, strata, kw,
                     chrom=(("ll0", np.float64), ("n_ones", np.int32)))


def scan_surv(ctx, time, status, cov=None, imprint=False, use=None, permutations=0, seed=0, strata=None, additive=False,
              max_iter=50, tol=1e-7, rows=None):
    """The survival-trait scan of a whole cross on the context's uploaded pedigree: as scan_binary -- one origin sweep with the
    rows left on the device (or `rows`, the tensor of origin_rows) and per pattern of missing times (NaN) one scan with the
    pattern's own `use` -- with every (marker, trait) Cox's proportional hazards regression of (time, status) on the
    covariates and the effects a, d (unless additive), i (with imprint), the effects on the log hazard, fitted by Newton's
    method on Breslow's partial likelihood from the null fit until it gains less than tol LOD or max_iter iterations are
    done.  status is 1 where the event was observed at `time` and 0 where the individual was censored then; where the time
    is not missing any other status raises ValueError.  With permutations > 0 the raw pairs (time, status) are permuted
    together, within the strata of `strata` (qtl.permutations): with covariates the permutations are valid only within
    strata of the covariates, which the caller supplies.  A dict: lod[T][M], coef[T][M][len(coef_names)], coef_names,
    iters[T][M], status[T][M] (0 = stopped by tol, 1 = by max_iter, 2 = breakdown, e.g. a monotone likelihood), rank[T][M],
    ll0[T][C] (the null model's log partial likelihood, 0 where the trait is not scanned on the chromosome), n_events[T][C],
    n_used[T][C], perm_max[P][T][C] or None (thresholds)."""
    t = _fit_columns(ctx, time, "time")
    d = np.asarray(status, np.float64)
    d = d[:, None] if d.ndim == 1 else d
    if d.shape != t.shape:
        raise ValueError("status must have the shape of time")
    _fit_iterations(max_iter, 1000, tol)
    if not np.all(~np.isfinite(t) | (d == 0.0) | (d == 1.0)):
        raise ValueError("a status is 1 (event) or 0 (censored) wherever the time is not missing")
    kw = dict(cov=cov, imprint=imprint, additive=additive, max_iter=max_iter, tol=tol)
    return _fit_scan(ctx, ctx.qtl_scan_surv_device, (t, d), use, rows, permutations, seed, strata, kw,
                     chrom=(("ll0", np.float64), ("n_events", np.int32)))


VAR_KEYS = ("joint", "mean", "variance")


def scan_var(ctx, pheno, cov=None, var_covariates=(), imprint=False, use=None, permutations=0, seed=0, strata=None, additive=False,
             max_iter=50, tol=1e-7, rows=None):
    """The variance-QTL scan of a whole cross on the context's uploaded pedigree: as scan_binary -- one origin sweep with the
    rows left on the device (or `rows`, the tensor of origin_rows) and per pattern of missing phenotypes (NaN) one scan with
    the pattern's own `use` -- with every (marker, trait) the double generalised linear model: the trait's mean on the
    covariates and its log variance on the covariates of var_covariates (indices into cov's columns, at most three; they are
    moved to the front of cov in the order given), both on the effects a, d (unless additive), i (with imprint).  Each cell
    is fitted mean-only, variance-only and in full from the null fit, until the log-likelihood gains less than tol LOD or
    max_iter iterations are done.  With permutations > 0 the raw phenotypes are permuted, within the strata of `strata`
    (qtl.permutations): the null of no effect of either kind, which is exact for the joint LOD.  A dict: lod[T][M][3] and its
    slices lod_joint, lod_mean, lod_variance [T][M], coef_mean and coef_var[T][M][len(coef_names)] of the full fit (coef_var
    on the log-variance scale), coef_names, iters and status[T][M][3] by fit (mean-only, variance-only, full; 0 = stopped by
    tol, 1 = by max_iter, 2 = breakdown), rank[T][M], ll0[T][C], n_used[T][C], perm_max[P][T][C][3] or None
    (thresholds_var)."""
    y = _fit_columns(ctx, pheno, "pheno")
    _fit_iterations(max_iter, 1000, tol)
    z = None if cov is None else np.asarray(cov, np.float64).reshape(y.shape[0], -1)
    K = 0 if z is None else z.shape[1]
    vc = [int(k) for k in var_covariates]
    if len(vc) > 3 or len(set(vc)) != len(vc) or any(not 0 <= k < K for k in vc):
        raise ValueError("var_covariates must be at most three different columns of cov")
    if vc:
        z = z[:, vc + [k for k in range(K) if k not in vc]]
    kw = dict(cov=z, n_var=len(vc), imprint=imprint, additive=additive, max_iter=max_iter, tol=tol)
    out = _fit_scan(ctx, ctx.qtl_scan_var_device, (y,), use, rows, permutations, seed, strata, kw, coef=("coef_mean", "coef_var"),
                    chrom=(("ll0", np.float64),), fits=(3,))
    for s, key in enumerate(VAR_KEYS):
        out["lod_" + key] = out["lod"][..., s]
    return out


def cofactor_windows(cof, pos, chromstarts, window=0.0):
    """(excl_lo[Q], excl_hi[Q]) (int32) for scan_cof: per cofactor the markers of its chromosome within `window` map units
    of it, as the first and the last of them.  window = 0 gives the cofactor alone (and whatever shares its position)."""
    cof = np.asarray(cof, np.int64).reshape(-1)
    pos = np.asarray(pos, np.float64)
    cs = np.asarray(chromstarts, np.int64)
    if window < 0:
        raise ValueError("window must not be negative")
    if cof.size and (cof.min() < 0 or cof.max() >= len(pos)):
        raise ValueError("a cofactor is off the map")
    lo, hi = np.zeros(len(cof), np.int32), np.zeros(len(cof), np.int32)
    for q, m in enumerate(cof):
        c = int(np.searchsorted(cs, m, side="right") - 1)
        near = np.flatnonzero(np.abs(pos[cs[c]:cs[c + 1]] - pos[m]) <= window) + cs[c]
        lo[q], hi[q] = near.min(), near.max()
    return lo, hi


def cofactor_columns(rows, cof, additive=False):
    """[n][ne Q] (numpy): the regressors a = o[3] - o[0] and d = o[1] + o[2] (a only with additive) of the markers cof, from
    the origin rows -- a torch tensor on the device (origin_rows) or an array [n][M][4]"""
    cof = [int(m) for m in np.asarray(cof, np.int64).reshape(-1)]
    o = rows[:, cof, :]
    o = np.asarray(o.cpu().numpy() if hasattr(o, "cpu") else o, np.float64)
    a, d = o[:, :, 3] - o[:, :, 0], o[:, :, 1] + o[:, :, 2]
    return a if additive else np.stack([a, d], axis=2).reshape(o.shape[0], -1)


def scan_cof(ctx, pheno, cof, excl=None, cov=None, use=None, permutations=0, seed=0, additive=False, rows=None):
    """The cofactor scan (composite interval mapping) of a whole cross on the context's uploaded pedigree: as scan -- one
    origin sweep with the rows left on the device (or `rows`, the tensor of origin_rows), per pattern of missing phenotypes
    (NaN) one observed scan with the pattern's own `use` -- with the markers cof[Q] (strictly ascending) as cofactors, each
    left out of the design at the markers excl[0][q] .. excl[1][q] (cofactor_windows; None: at its own marker only).  With
    permutations > 0 one more scan on the permuted Freedman-Lane residuals of the null model [1, cov, every cofactor's
    columns] (the columns are fetched from the device rows).  A dict: lod[T][M] (conditional on the cofactors), lod_base[T][M],
    coef[T][M][len(coef_names)], coef_names, rank[T][M], rank_cof[T][M], n_used[T][C], perm_max[P][T][C] or None (the maxima
    over the markers in no range: thresholds), cof, excl_lo, excl_hi, and candidate[M]: the marker lies in no range."""
    y = np.asarray(pheno, np.float64)
    y = y[:, None] if y.ndim == 1 else y
    n, T = y.shape
    if n != ctx.n_ind:
        raise ValueError("pheno must have a row per analysed individual (%d)" % ctx.n_ind)
    use = np.ones(n, bool) if use is None else np.asarray(use) != 0
    M, C = ctx.n_markers, ctx.n_chrom
    cof = np.ascontiguousarray([] if cof is None else cof, np.int32).reshape(-1)
    lo, hi = (cof.copy(), cof.copy()) if excl is None else (np.ascontiguousarray(e, np.int32).reshape(-1) for e in excl)
    names = coef_names(0, False, additive)
    d_o = origin_rows(ctx) if rows is None else rows
    mk = np.arange(M)
    candidate = ~np.any((lo[:, None] <= mk[None, :]) & (mk[None, :] <= hi[:, None]), axis=0) if len(cof) else np.ones(M, bool)
    out = dict(lod=np.zeros((T, M)), lod_base=np.zeros((T, M)), coef=np.full((T, M, len(names)), np.nan), coef_names=names,
               rank=np.zeros((T, M), np.int32), rank_cof=np.zeros((T, M), np.int32), n_used=np.zeros((T, C), np.int32),
               perm_max=np.zeros((permutations, T, C)) if permutations else None, cof=cof, excl_lo=lo, excl_hi=hi,
               candidate=candidate)
    kw = dict(excl=(lo, hi), cov=cov, additive=additive)
    null_cov = None
    if permutations:
        z = None if cov is None else np.asarray(cov, np.float64).reshape(n, -1)
        parts = ([] if z is None else [z]) + ([cofactor_columns(d_o, cof, additive)] if len(cof) else [])
        null_cov = np.concatenate(parts, axis=1) if parts else None
    for cols, u in _patterns(y, use):
        yk = np.where(u[:, None], y[:, cols], 0.0)
        got = ctx.qtl_scan_cof_device(n, d_o.data_ptr(), yk, cof, use=u, **kw)
        for key in ("lod", "lod_base", "coef", "rank", "rank_cof", "n_used"):
            out[key][cols] = got[key]
        if permutations:
            perm = _permutations(n, permutations, seed, use=u)
            res = null_residuals(yk, null_cov, u)
            out["perm_max"][:, cols] = ctx.qtl_scan_cof_device(n, d_o.data_ptr(), res, cof, use=u, perm=perm, **kw)["perm_max"]
    return out


def read_multi(out, loci, chromstarts):
    """A multiple-QTL fit read off a cofactor scan `out` (scan_cof's dict, or arrays of its shapes) that had `loci` as its
    cofactors, each left out at its own marker only.  At a cofactor's marker the tested marker stands in for it, so per trait:
    lod_full[T] = lod_base + lod there (the same at every locus; the first is reported), drop_one[T][Q] = lod at locus q,
    coef[T][Q][ne] its effects in the full model, n[T][Q] the individuals of its chromosome's fit, and the shares of the
    phenotypic variance 1 - 10^(-2 LOD / n): var_full[T], var_drop[T][Q].  The loci are reported in the order given."""
    loci = np.asarray(loci, np.int64).reshape(-1)
    if loci.size == 0:
        raise ValueError("a multiple-QTL fit needs at least one locus")
    cs = np.asarray(chromstarts, np.int64)
    lod, base, coef = np.asarray(out["lod"], np.float64), np.asarray(out["lod_base"], np.float64), np.asarray(out["coef"], np.float64)
    n_used = np.asarray(out["n_used"])
    n_used = n_used[None, :] if n_used.ndim == 1 else n_used
    chrom = np.searchsorted(cs, loci, side="right") - 1
    nq = np.maximum(n_used[:, chrom], 1).astype(np.float64)
    drop = lod[:, loci]
    full = (base[:, loci] + drop)[:, 0]
    share = lambda l, k: 1.0 - 10.0 ** (-2.0 * l / k)
    return dict(loci=loci.copy(), lod_full=full, drop_one=drop, coef=coef[:, loci], n=n_used[:, chrom],
                var_full=share(full, nq[:, 0]), var_drop=share(drop, nq))


def fit_multi(ctx, pheno, loci, cov=None, use=None, additive=False, rows=None, scanner=None, chromstarts=None):
    """The multiple-QTL model of the markers `loci` (any order, no repeats), from one scan_cof call with every locus left
    out at its own marker only: read_multi's dict -- per trait the full model's LOD, per locus the drop-one LOD, the effects
    and the shares of variance.  scanner and chromstarts: what forward_select takes."""
    loci = np.asarray(loci, np.int64).reshape(-1)
    srt = np.sort(loci).astype(np.int32)
    if scanner is None:
        scanner = _cof_scanner(ctx, pheno, cov, use, additive, rows)
    return read_multi(scanner(srt, (srt, srt), 0, 0), loci, ctx.chromstarts if chromstarts is None else chromstarts)


def _cof_scanner(ctx, pheno, cov, use, additive, rows):
    """scanner(cof, excl, permutations, seed) -> scan_cof's dict, on one set of origin rows for every call"""
    d_o = origin_rows(ctx) if rows is None else rows
    return lambda cof, excl, permutations, seed: scan_cof(ctx, pheno, cof, excl=excl, cov=cov, use=use, permutations=permutations,
                                                          seed=seed, additive=additive, rows=d_o)


def forward_select(ctx, pheno, max_loci, window, pos, alpha=0.05, permutations=100, seed=0, cov=None, use=None, additive=False,
                   rows=None, scanner=None, chromstarts=None):
    """Forward selection of QTL for ONE trait (pheno[n] or [n][1]).  Each step is a scan_cof with the loci found so far as
    cofactors, left out within `window` map units of themselves (cofactor_windows on pos), and `permutations` permutations;
    the candidates are the markers in no range.  The best candidate (the first wins a tie) joins the model when its
    conditional LOD exceeds that step's genome-wide threshold, thresholds(perm_max, (alpha,)); otherwise, or with max_loci
    loci, or when one more locus would make the design wider than 15 columns, the selection stops.  One origin sweep (or
    `rows`) serves every step.  A dict: loci (in order of entry), lod and threshold (their entry LODs and thresholds),
    stopped (marker, lod, threshold of the candidate that did not enter; None when none was looked at) and fit (fit_multi
    of the loci; None without loci).  scanner(cof, excl, permutations, seed) replaces scan_cof (a reference of the tests)."""
    y = np.asarray(pheno, np.float64)
    if y.ndim == 2 and y.shape[1] != 1:
        raise ValueError("forward_select works on one trait")
    if permutations < 1:
        raise ValueError("forward_select needs permutations for its thresholds")
    cs = np.asarray(ctx.chromstarts if chromstarts is None else chromstarts, np.int64)
    pos = np.asarray(pos, np.float64)
    K = 0 if cov is None else np.asarray(cov).reshape(len(y), -1).shape[1]
    ne = 1 if additive else 2
    if scanner is None:
        scanner = _cof_scanner(ctx, y, cov, use, additive, rows)
    loci, lods, thrs, stopped = [], [], [], None
    while len(loci) < max_loci and 1 + K + ne * (len(loci) + 2) <= 15:
        cof = np.sort(np.asarray(loci, np.int32))
        out = scanner(cof, cofactor_windows(cof, pos, cs, window), permutations, seed)
        cand = np.flatnonzero(out["candidate"])
        if cand.size == 0:
            break
        best = int(cand[np.argmax(out["lod"][0, cand])])
        lod, thr = float(out["lod"][0, best]), float(thresholds(out["perm_max"], (alpha,))["genome"][0, 0])
        if not lod > thr:
            stopped = dict(marker=best, lod=lod, threshold=thr)
            break
        loci.append(best)
        lods.append(lod)
        thrs.append(thr)
    fit = None
    if loci:
        srt = np.sort(np.asarray(loci, np.int32))
        fit = read_multi(scanner(srt, (srt, srt), 0, 0), loci, cs)
    return dict(loci=loci, lod=lods, threshold=thrs, stopped=stopped, fit=fit)


THRESHOLDSX_KEYS = ("lod0", "lod1", "lod2", "imprint", "interaction")


def thresholdsx(perm_max, alpha=(0.05, 0.01)):
    """From perm_max[P][T][C][5] of the extended scan: per statistic -- lod0, lod1, lod2 (the three nested LODs), imprint
    (lod[1] - lod[0]) and interaction (lod[2] - lod[1]) -- the dict thresholds() gives for it: genome[len(alpha)][T] and
    chromosome[len(alpha)][T][C], by the same order statistic."""
    pm = np.asarray(perm_max, np.float64)
    if pm.ndim != 4 or pm.shape[0] == 0 or pm.shape[3] != 5:
        raise ValueError("perm_max must be [P][T][C][5] with P >= 1")
    out = dict(alpha=tuple(alpha))
    for s, key in enumerate(THRESHOLDSX_KEYS):
        th = thresholds(pm[..., s], alpha)
        out[key] = dict(genome=th["genome"], chromosome=th["chromosome"])
    return out


def thresholds_var(perm_max, alpha=(0.05, 0.01)):
    """From perm_max[P][T][C][3] of the variance-QTL scan: per LOD -- joint, mean, variance -- the dict thresholds() gives for
    it, as thresholdsx does for its statistics.  The permutations are of the phenotype: the null of no effect of either kind,
    exact for the joint LOD and conservative in neither direction for the other two."""
    pm = np.asarray(perm_max, np.float64)
    if pm.ndim != 4 or pm.shape[0] == 0 or pm.shape[3] != 3:
        raise ValueError("perm_max must be [P][T][C][3] with P >= 1")
    out = dict(alpha=tuple(alpha))
    for s, key in enumerate(VAR_KEYS):
        th = thresholds(pm[..., s], alpha)
        out[key] = dict(genome=th["genome"], chromosome=th["chromosome"])
    return out


def peaks_var(out, pos, chromstarts, threshold, drop=1.5):
    """peaks() on each of scan_var's three profiles: a dict joint / mean / variance of its lists.  threshold is a number,
    one per trait, or a dict by those keys (e.g. the genome row of thresholds_var at one alpha)."""
    lod = np.asarray(out["lod"], np.float64)
    if lod.ndim != 3 or lod.shape[2] != 3:
        raise ValueError("out must be scan_var's result: lod[T][M][3]")
    thr = (lambda key: threshold[key]) if isinstance(threshold, dict) else (lambda key: threshold)
    return {key: peaks(lod[..., s], pos, chromstarts, thr(key), drop) for s, key in enumerate(VAR_KEYS)}


def quantile_index(P, alpha):
    """index into P ascending values of the (1 - alpha) threshold: the smallest value that at most alpha P values exceed"""
    return min(P - 1, max(0, int(np.ceil((1.0 - alpha) * P)) - 1))


def thresholds(perm_max, alpha=(0.05, 0.01)):
    """From perm_max[P][T][C]: genome[len(alpha)][T], the thresholds of the maximum over the whole map, and
    chromosome[len(alpha)][T][C], those of one chromosome scanned alone.  A threshold is the order statistic number
    ceil((1 - alpha) P) of the P maxima: at most alpha P permutations exceed it (the conservative convention)."""
    pm = np.asarray(perm_max, np.float64)
    if pm.ndim != 3 or pm.shape[0] == 0:
        raise ValueError("perm_max must be [P][T][C] with P >= 1")
    P = pm.shape[0]
    genome_sorted = np.sort(pm.max(axis=2), axis=0)
    chrom_sorted = np.sort(pm, axis=0)
    idx = [quantile_index(P, a) for a in alpha]
    return dict(alpha=tuple(alpha), genome=genome_sorted[idx], chromosome=chrom_sorted[idx])


def peaks(lod, pos, chromstarts, threshold, drop=1.5, coef=None):
    """Per trait and chromosome the marker with the largest LOD, where that is above the threshold (a number or one per
    trait): a list of dicts with trait, chrom, marker, lod, the LOD-drop support interval lo .. hi (the markers around the
    peak, without a gap, whose LOD is within `drop` of it; pos_lo, pos_hi their positions) and, with coef[T][M][2], the
    effects at the peak.  The first marker wins a tie."""
    lod = np.asarray(lod, np.float64)
    lod = lod[None, :] if lod.ndim == 1 else lod
    T, M = lod.shape
    cs = np.asarray(chromstarts, np.int64)
    pos = np.asarray(pos, np.float64)
    thr = np.broadcast_to(np.asarray(threshold, np.float64), (T,))
    found = []
    for t in range(T):
        for c in range(len(cs) - 1):
            seg = lod[t, cs[c]:cs[c + 1]]
            k = int(np.argmax(seg))
            if not seg[k] > thr[t]:
                continue
            lo = hi = k
            while lo > 0 and seg[lo - 1] >= seg[k] - drop:
                lo -= 1
            while hi + 1 < len(seg) and seg[hi + 1] >= seg[k] - drop:
                hi += 1
            m = int(cs[c]) + k
            p = dict(trait=t, chrom=c, marker=m, lod=float(seg[k]), lo=int(cs[c]) + lo, hi=int(cs[c]) + hi,
                     pos=float(pos[m]), pos_lo=float(pos[cs[c] + lo]), pos_hi=float(pos[cs[c] + hi]))
            if coef is not None:
                p["additive"], p["dominance"] = (float(v) for v in np.asarray(coef)[t, m])
            found.append(p)
    return found


# ------------------------------------------------------------------------------------------------
# Where a QTL sits: the bootstrap of the scan and the posterior of the position
# ------------------------------------------------------------------------------------------------
def bootstrap_counts(n, B, seed, use=None, strata=None):
    """count[B][n] (int32): how often replicate b draws individual i, for Context.qtl_scan_boot.  Within every stratum the k
    used individuals, in ascending order, are idx[0..k); draw j of replicate b -- one per used individual j -- picks
    idx[floor(u * k)] of j's stratum with u = synth.uniform(seed, b * n + j), the keys of permutations().  Every row sums to
    the used individuals of each stratum and unused individuals get 0.  No sequential generator enters, so the same lines
    in another language give the same arrays (cnf2h_qtl_bootstrap_counts of the host library, which `cnF2freq --qtlboot`
    uses)."""
    use = np.ones(n, bool) if use is None else np.asarray(use) != 0
    strata = np.zeros(n, np.int64) if strata is None else np.asarray(strata)
    if use.shape != (n,) or strata.shape != (n,):
        raise ValueError("use and strata must be [n]")
    count = np.zeros((B, n), np.int32)
    groups = [np.flatnonzero(use & (strata == s)) for s in np.unique(strata[use])] if use.any() else []
    for b in range(B):
        u = synth.uniform(seed, np.uint64(b) * np.uint64(n) + np.arange(n, dtype=np.uint64))
        for idx in groups:
            k = len(idx)
            pick = idx[np.minimum(k - 1, np.floor(u[idx] * k).astype(np.int64))]
            count[b] += np.bincount(pick, minlength=n).astype(np.int32)
    return count


def scan_boot(ctx, pheno, chrom, replicates=1000, seed=0, cov=None, use=None, strata=None, additive=False, rows=None,
              profile=False):
    """The non-parametric bootstrap of the scan on the context's uploaded pedigree (Visscher, Thompson and Haley 1996): the
    individuals are drawn with replacement (bootstrap_counts, within strata if given), chromosome `chrom` -- or the range
    (chrom_begin, chrom_end) -- is scanned again for every replicate, and the replicates' best markers are returned for
    boot_interval.  One origin sweep with the rows left on the device (or `rows`, the tensor of origin_rows), then per pattern
    of missing phenotypes (NaN) one Context.qtl_scan_boot_device call that draws among the pattern's own individuals.  A
    dict: boot_max[B][T][C'], boot_arg[B][T][C'] (global marker indices; -1 where a replicate cannot be fitted),
    n_boot[B][T][C'], count[T][B][n], and with profile boot_lod[B][T][M'] (else None)."""
    y = np.asarray(pheno, np.float64)
    y = y[:, None] if y.ndim == 1 else y
    n, T = y.shape
    if n != ctx.n_ind:
        raise ValueError("pheno must have a row per analysed individual (%d)" % ctx.n_ind)
    c0, c1 = (chrom, chrom + 1) if np.ndim(chrom) == 0 else (int(chrom[0]), int(chrom[1]))
    if not 0 <= c0 < c1 <= ctx.n_chrom:
        raise ValueError("the chromosome range must be non-empty and within 0 .. %d" % ctx.n_chrom)
    use = np.ones(n, bool) if use is None else np.asarray(use) != 0
    B, Cn = replicates, c1 - c0
    Mn = int(ctx.chromstarts[c1] - ctx.chromstarts[c0])
    d_o = origin_rows(ctx) if rows is None else rows
    out = dict(boot_max=np.zeros((B, T, Cn)), boot_arg=np.full((B, T, Cn), -1, np.int32), n_boot=np.zeros((B, T, Cn), np.int32),
               count=np.zeros((T, B, n), np.int32), boot_lod=np.zeros((B, T, Mn)) if profile else None)
    for cols, u in _patterns(y, use):
        yk = np.where(u[:, None], y[:, cols], 0.0)
        count = bootstrap_counts(n, B, seed, use=u, strata=strata)
        got = ctx.qtl_scan_boot_device(n, d_o.data_ptr(), yk, count, c0, c1, cov=cov, use=u, additive=additive, profile=profile)
        out["boot_max"][:, cols], out["boot_arg"][:, cols] = got["boot_max"], got["boot_arg"]
        out["n_boot"][:, cols], out["count"][cols] = got["n_boot"][:, None, :], count
        if profile:
            out["boot_lod"][:, cols] = got["boot_lod"]
    return out


def boot_interval(arg, pos, level=0.95):
    """The bootstrap confidence interval of a QTL's position from arg[B], the best marker of every replicate on one
    chromosome (boot_arg of scan_boot for one trait and chromosome).  Replicates with arg = -1 are left out and counted.
    The positions of the V others, sorted, are p_(0) .. p_(V-1); with alpha = 1 - level the interval runs from
    p_(floor(alpha/2 * V)) to p_(ceil((1 - alpha/2) * V) - 1) (the products are taken within 1e-9, so that 0.975 * 200 is
    195).  A dict: pos_lo, pos_hi, lo, hi (their markers; of equal positions the lower marker sorts first), V, left_out,
    and share[len(pos)], the share of the V replicates that chose each marker.  Without a usable replicate the positions
    are NaN and the markers -1."""
    arg = np.asarray(arg, np.int64).ravel()
    pos = np.asarray(pos, np.float64)
    if not 0.0 < level < 1.0:
        raise ValueError("level must lie between 0 and 1")
    if np.any(arg < -1) or np.any(arg >= len(pos)):
        raise ValueError("arg must hold marker indices or -1")
    kept = arg[arg >= 0]
    V = len(kept)
    share = np.bincount(kept, minlength=len(pos)) / max(V, 1)
    r = dict(pos_lo=np.nan, pos_hi=np.nan, lo=-1, hi=-1, V=V, left_out=len(arg) - V, share=share)
    if V:
        order = kept[np.lexsort((kept, pos[kept]))]
        alpha = 1.0 - level
        k_lo = min(V - 1, max(0, int(np.floor(alpha / 2 * V + 1e-9))))
        k_hi = min(V - 1, max(0, int(np.ceil((1.0 - alpha / 2) * V - 1e-9)) - 1))
        lo, hi = int(order[k_lo]), int(order[max(k_hi, k_lo)])
        r.update(pos_lo=float(pos[lo]), pos_hi=float(pos[hi]), lo=lo, hi=hi)
    return r


def bayes_interval(lod, pos, chromstarts, chrom, prob=0.95):
    """The Bayes credible interval of a QTL's position on chromosome `chrom` from one trait's profile lod[M]: the posterior
    of a single QTL under a flat prior along the map is proportional to 10^LOD; every marker stands for the stretch of map
    nearest to it, half of each gap to its neighbours (the markers of a chromosome without length count alike).  Returned is
    the shortest run of neighbouring markers, by map length, that holds at least `prob` -- of equally short runs the one
    with more mass, then the leftmost.  A dict: lo, hi (markers), pos_lo, pos_hi, mass (what the run holds) and
    posterior[markers of the chromosome]."""
    lod = np.asarray(lod, np.float64).ravel()
    pos = np.asarray(pos, np.float64)
    cs = np.asarray(chromstarts, np.int64)
    if not 0 <= chrom < len(cs) - 1 or len(lod) != len(pos):
        raise ValueError("chrom must be a chromosome of the map and lod one value per marker")
    if not 0.0 < prob <= 1.0:
        raise ValueError("prob must lie in (0, 1]")
    f, e = int(cs[chrom]), int(cs[chrom + 1])
    p, l = pos[f:e], lod[f:e]
    L = e - f
    width = np.zeros(L)
    if L > 1:
        gap = np.diff(p)
        width[:-1] += gap / 2
        width[1:] += gap / 2
    if not width.sum() > 0:
        width = np.ones(L)
    post = width * 10.0 ** (l - l.max())
    post = post / post.sum()
    cum = np.concatenate([[0.0], np.cumsum(post)])
    best = None
    for i in range(L):
        for j in range(i, L):
            mass = cum[j + 1] - cum[i]
            if mass >= prob - 1e-12:
                key = (p[j] - p[i], -mass, i)
                if best is None or key < best[0]:
                    best = (key, i, j, mass)
                break
    if best is None:                  # (rounding alone: the whole chromosome holds 1)
        best = (None, 0, L - 1, 1.0)
    _, i, j, mass = best
    return dict(lo=f + i, hi=f + j, pos_lo=float(p[i]), pos_hi=float(p[j]), mass=float(mass), posterior=post)


# ------------------------------------------------------------------------------------------------
# The polygenic (mixed-model) scan: kinship from the origin rows, heritability, the scan on rotated columns
# ------------------------------------------------------------------------------------------------
def kinship(ctx, rows=None, loco=False):
    """The realised line-origin kinship of the analysed individuals from the origin rows (Context.kinship_sums_device,
    cnf2_kinship_sums): K = (1 + S / M) / 2 with S[i][j] the sum over the markers of a_i a_j, a = P(BB) - P(AA) -- R/qtl2's
    allele-probability kinship for two founder lines.  A torch f64 tensor on the context's device: [n][n], or with loco
    [C][n][n], K_-c = (1 + (S - S_c) / (M - M_c)) / 2, the kinship from every chromosome but c (leave one chromosome out: a
    locus under test is then not also in the polygenic term).  rows: the tensor of origin_rows (None: one origin sweep).
    ValueError with loco on a map of one chromosome."""
    import torch
    C = ctx.n_chrom
    if loco and C < 2:
        raise ValueError("leaving one chromosome out needs at least two chromosomes")
    d_o = origin_rows(ctx) if rows is None else rows
    n = d_o.shape[0]
    dev = d_o.device
    cnt = torch.zeros(1, dtype=torch.int32, device=dev)

    def sums(c0, c1):
        s = torch.zeros((n, n), dtype=torch.float64, device=dev)
        ctx.kinship_sums_device(n, d_o.data_ptr(), c0, c1, d_sum=s.data_ptr(), d_n_markers=cnt.data_ptr())
        ctx.sync()
        return s, int(cnt.item())

    S, M = sums(0, C)
    if not loco:
        return (1.0 + S / M) * 0.5
    out = torch.zeros((C, n, n), dtype=torch.float64, device=dev)
    for c in range(C):
        Sc, Mc = sums(c, c + 1)
        out[c] = (1.0 + (S - Sc) / (M - Mc)) * 0.5
    return out


_kinship = kinship      # (scan_lmm's argument of the same name is a matrix)


def _lmm_objective(h2, y, x, lam, reml):
    """(log-likelihood, sigma2, w) of the rotated model at h2: weighted least squares of y on x with w = 1 / (h2 lam + 1 - h2)"""
    w = 1.0 / (h2 * lam + (1.0 - h2))
    sw = np.sqrt(w)
    xs, ys = x * sw[:, None], y * sw
    beta = np.linalg.lstsq(xs, ys, rcond=None)[0]
    rss = float(((ys - xs @ beta) ** 2).sum())
    n, nx = x.shape
    slw = float(np.log(w).sum())
    rss = max(rss, np.finfo(np.float64).tiny)
    if not reml:
        return -(n * np.log(2.0 * np.pi * rss / n) + n - slw) / 2.0, rss / n, w
    df = n - nx
    logdet = np.linalg.slogdet(xs.T @ xs)[1]
    return -(df * np.log(2.0 * np.pi * rss / df) + df - slw + logdet) / 2.0, rss / df, w


def est_herit(y, x0, lam, u, reml=True):
    """(h2, sigma2, loglik): the heritability that maximises the profile log-likelihood of y = x0 b + g + e,
    g ~ N(0, h2 s K), e ~ N(0, (1 - h2) s I), over h2 in [0, 0.999], in the eigen form: K = u diag(lam) u' (eigenvalues
    below 0 count as 0), w_i = 1 / (h2 lam_i + 1 - h2), weighted least squares of u'y on u'x0.  ML maximises
    -(n log(2 pi RSS / n) + n - sum log w) / 2; REML (the default) has n - nx for n and adds log det(x0' u W u' x0) inside
    the bracket.  The search is deterministic: 21 grid points, then golden section in the bracket around the best one down
    to a width of 1e-8.  u None: y and x0 are rotated already.  sigma2 is RSS / n (RSS / (n - nx) with reml)."""
    y = np.asarray(y, np.float64).reshape(-1)
    x = np.asarray(x0, np.float64).reshape(len(y), -1)
    lam = np.maximum(np.asarray(lam, np.float64).reshape(-1), 0.0)
    if u is not None:
        u = np.asarray(u, np.float64)
        y, x = u.T @ y, u.T @ x
    if x.shape[0] <= x.shape[1]:
        raise ValueError("est_herit needs more individuals than columns of x0")
    f = lambda h: _lmm_objective(h, y, x, lam, reml)[0]
    hi = 0.999
    grid = np.linspace(0.0, hi, 21)
    vals = [f(h) for h in grid]
    k = int(np.argmax(vals))
    a, b = grid[max(k - 1, 0)], grid[min(k + 1, 20)]
    g = (np.sqrt(5.0) - 1.0) / 2.0
    c, d = b - g * (b - a), a + g * (b - a)
    fc, fd = f(c), f(d)
    while b - a > 1e-8:
        if fc >= fd:
            b, d, fd = d, c, fc
            c = b - g * (b - a)
            fc = f(c)
        else:
            a, c, fc = c, d, fd
            d = a + g * (b - a)
            fd = f(d)
    cands = [(vals[k], grid[k]), (f(0.5 * (a + b)), 0.5 * (a + b))]
    best = max(cands, key=lambda t: t[0])
    ll, s2, _ = _lmm_objective(best[1], y, x, lam, reml)
    return float(best[1]), float(s2), float(ll)


def _eigh(K):
    """(lam, U) of a symmetric torch matrix on its device; numpy where torch refuses"""
    import torch
    try:
        lam, U = torch.linalg.eigh(K)
        if not bool(torch.isfinite(lam).all()):
            raise RuntimeError("eigh gave values that are not finite")
        return lam, U
    except RuntimeError:
        lam, U = np.linalg.eigh(K.cpu().numpy())
        return torch.from_numpy(lam).to(K.device), torch.from_numpy(U).to(K.device)


def scan_lmm(ctx, pheno, kinship=None, loco=True, cov=None, use=None, permutations=0, seed=0, additive=False, reml=True, h2=None,
             rows=None):
    """The polygenic (mixed-model) scan of a whole cross on the context's uploaded pedigree: y = X0 b + x(m) beta + g + e with
    g ~ N(0, s_g^2 K), what R/qtl2's scan1 with a kinship does.  It runs once per pattern of missing phenotypes (NaN), on the
    individuals that are used, have the phenotype and are skipped on no chromosome.  kinship: None (qtl.kinship of the rows,
    with `loco`), a tensor or array [n][n] (any positive semi-definite matrix, e.g. a pedigree relationship matrix; one
    model for the genome) or [C][n][n] (one per chromosome).  Per pattern, and per chromosome where the kinship is: the kept
    submatrix is eigendecomposed (torch.linalg.eigh on the context's device), the centred phenotypes and [1, centred cov] are
    rotated, per trait h2 is estimated (est_herit; or `h2`, a number or [T], is taken), the chromosome's (a, d) columns are
    rotated by torch matmuls in chunks, and the block is scanned by Context.qtl_scan_cols_device with x0 and y whitened on the
    host and scale = sqrt(w).  With permutations > 0 one more scan per trait runs on the permuted whitened residuals of the
    null model: whitened, they are exchangeable (Freedman-Lane on the whitened model).
    A dict: lod[T][M], coef[T][M][2], rank[T][M], h2[T][C] and sigma2[T][C] (one value repeated where one model serves the
    genome), n_used[T], perm_max[P][T][C] or None: thresholds and peaks read it as they read scan."""
    import torch
    y = np.asarray(pheno, np.float64)
    y = y[:, None] if y.ndim == 1 else y
    n, T = y.shape
    if n != ctx.n_ind:
        raise ValueError("pheno must have a row per analysed individual (%d)" % ctx.n_ind)
    use = np.ones(n, bool) if use is None else np.asarray(use) != 0
    M, C = ctx.n_markers, ctx.n_chrom
    cs = np.asarray(ctx.chromstarts, np.int64)
    z = None if cov is None else np.asarray(cov, np.float64).reshape(n, -1)
    if z is not None and z.shape[1] == 0:
        z = None
    d_o = origin_rows(ctx) if rows is None else rows
    dev = d_o.device
    if kinship is None:
        Kall = _kinship(ctx, rows=d_o, loco=loco and C > 1)
    else:
        Kall = kinship if isinstance(kinship, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(kinship, np.float64))
        Kall = Kall.to(device=dev, dtype=torch.float64)
    per_chrom = Kall.dim() == 3
    if Kall.shape[-2:] != (n, n) or (per_chrom and Kall.shape[0] != C):
        raise ValueError("kinship must be [n][n] or [C][n][n] with n = %d, C = %d" % (n, C))
    h2_given = None if h2 is None else np.broadcast_to(np.asarray(h2, np.float64), (T,))
    if h2_given is not None and not np.all((h2_given >= 0.0) & (h2_given < 1.0)):
        raise ValueError("h2 must lie in [0, 1)")
    ne = 1 if additive else 2
    present = (d_o[:, torch.from_numpy(cs[:-1]).to(dev), :] != 0).any(dim=2).all(dim=1).cpu().numpy()
    out = dict(lod=np.zeros((T, M)), coef=np.full((T, M, 2), np.nan), rank=np.zeros((T, M), np.int32), h2=np.zeros((T, C)),
               sigma2=np.zeros((T, C)), n_used=np.zeros(T, np.int32),
               perm_max=np.zeros((permutations, T, C)) if permutations else None)
    for cols, u in _patterns(y, use & present):
        idx = np.flatnonzero(u)
        nk = len(idx)
        out["n_used"][cols] = nk
        x0 = np.ones((nk, 1)) if z is None else np.concatenate([np.ones((nk, 1)), z[idx] - z[idx].mean(axis=0)], axis=1)
        if nk < x0.shape[1] + 3:
            continue
        yk = y[idx][:, cols] - y[idx][:, cols].mean(axis=0)
        d_idx = torch.from_numpy(idx).to(dev)
        d_yx = torch.from_numpy(np.concatenate([yk, x0], axis=1)).to(dev)
        perm = _permutations(nk, permutations, seed) if permutations else None
        model = None
        for c in range(C):
            if per_chrom or model is None:
                Ksub = (Kall[c] if per_chrom else Kall)[d_idx][:, d_idx]
                lam_t, U = _eigh(0.5 * (Ksub + Ksub.T))
                lam = np.maximum(lam_t.cpu().numpy(), 0.0)
                yx = (U.T @ d_yx).cpu().numpy()
                yr, xr = yx[:, :len(cols)], yx[:, len(cols):]
                fits = []
                for j, t in enumerate(cols):
                    if h2_given is None:
                        h, s2, _ = est_herit(yr[:, j], xr, lam, None, reml)
                    else:
                        h = float(h2_given[t])
                        s2 = _lmm_objective(h, yr[:, j], xr, lam, reml)[1]
                    fits.append((h, s2, np.sqrt(1.0 / (h * lam + (1.0 - h)))))
                model = (U, yr, xr, fits)
            U, yr, xr, fits = model
            m0, m1 = int(cs[c]), int(cs[c + 1])
            R = torch.empty((nk, m1 - m0, ne), dtype=torch.float64, device=dev)
            for b0 in range(m0, m1, 4096):                      # the rotation, in chunks of markers: U' [a, d]
                b1 = min(b0 + 4096, m1)
                o = d_o[d_idx, b0:b1, :]
                reg = o[:, :, 3] - o[:, :, 0]
                reg = reg[:, :, None] if additive else torch.stack([reg, o[:, :, 1] + o[:, :, 2]], dim=2)
                R[:, b0 - m0:b1 - m0, :] = (U.T @ reg.reshape(nk, -1)).reshape(nk, b1 - b0, ne)
            torch.cuda.synchronize(dev)
            for j, t in enumerate(cols):
                h, s2, sw = fits[j]
                out["h2"][t, c], out["sigma2"][t, c] = h, s2
                xs, ys = xr * sw[:, None], yr[:, j] * sw
                got = ctx.qtl_scan_cols_device(nk, m1 - m0, ne, R.data_ptr(), xs, ys, scale=sw)
                out["lod"][t, m0:m1], out["coef"][t, m0:m1], out["rank"][t, m0:m1] = got["lod"][0], got["coef"][0], got["rank"]
                if permutations:
                    res = ys - xs @ np.linalg.lstsq(xs, ys, rcond=None)[0]
                    out["perm_max"][:, t, c] = ctx.qtl_scan_cols_device(nk, m1 - m0, ne, R.data_ptr(), xs, res, scale=sw,
                                                                        perm=perm)["perm_max"][:, 0]
    return out
