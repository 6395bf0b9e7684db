"""ctypes binding of libcnf2host.so (include/cnf2host.h): the host side of a cnF2freq run -- postmarkerdata, the
haplotyping iteration with its device-side updates, dump / deserialize -- driven from arrays.  Same code as the
`cnF2freq` executable; everything numeric goes on to libcnf2hip.so (no CPU compute path here either)."""
import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
# CNF2HOST_LIB: a copy of the host library next to another build of libcnf2hip.so (kernel A/B timing: it binds the libcnf2hip.so of its own directory)
LIB_PATH = os.environ.get("CNF2HOST_LIB") or os.path.join(_HERE, "libcnf2host.so")

SYMBOLS = ["cnf2h_create", "cnf2h_create_on", "cnf2h_create_from_files", "cnf2h_get_dims", "cnf2h_destroy", "cnf2h_last_error", "cnf2h_postmarkerdata", "cnf2h_iteration",
           "cnf2h_dump", "cnf2h_deserialize", "cnf2h_get_state", "cnf2h_set_block", "cnf2h_balanced_block", "cnf2h_set_partition", "cnf2h_get_partition", "cnf2h_set_update_flags", "cnf2h_reserve", "cnf2h_get_timing",
           "cnf2h_set_deterministic", "cnf2h_context", "cnf2h_get_passes", "cnf2h_map_mstep", "cnf2h_write_map",
           "cnf2h_qtl_permutations", "cnf2h_qtl_null_residuals", "cnf2h_qtl2_pair", "cnf2h_qtl2_pair_linked", "cnf2h_qtlx_marker", "cnf2h_qtlx_column",
           "cnf2h_qtlem_fit", "cnf2h_qtlbin_fit", "cnf2h_qtlcof_marker", "cnf2h_kinship_sums", "cnf2h_qtl_cols_marker",
           "cnf2h_qtl_bootstrap_counts", "cnf2h_qtl_boot_marker", "cnf2h_qtl_marker_map", "cnf2h_qtl_column_tile",
           "cnf2h_qtlmv_marker", "cnf2h_qtl_group_tile", "cnf2h_qtlsurv_fit", "cnf2h_qtlvar_fit", "cnf2h_qtlimp_marker",
           "cnf2h_qtlfam_marker", "cnf2h_qtl_families", "cnf2h_descent_columns", "cnf2h_qtlhap_marker", "cnf2h_qtlvc_marker"]

# int fn(void *user, int op, void *buf, size_t count, size_t seg) -- the transport of a multi-process run (cnf2host.h)
EXCHANGE_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_size_t, C.c_size_t)
X_SUM_SEGMENTS, X_SUM_HITS, X_GATHER_SEGMENTS, X_BARRIER, X_BCAST_HOST = 0, 1, 2, 3, 4

_lib = None


def load():
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise RuntimeError("libcnf2host.so is not built: run `make -C cnf2freq_amd/csrc`")
        L = C.CDLL(LIB_PATH)
        vp, i32 = C.c_void_p, C.c_int
        L.cnf2h_create.argtypes = [i32, vp, vp, vp, vp, vp, vp, vp, vp, i32, vp, i32, vp, i32, i32]
        L.cnf2h_create.restype = vp
        L.cnf2h_create_on.argtypes = [i32, i32, vp, vp, vp, vp, vp, vp, vp, vp, i32, vp, i32, vp, i32, i32]
        L.cnf2h_create_on.restype = vp
        L.cnf2h_create_from_files.argtypes = [i32, C.c_char_p, C.c_char_p, C.c_char_p, i32]
        L.cnf2h_create_from_files.restype = vp
        L.cnf2h_get_dims.argtypes = [vp, vp]
        L.cnf2h_set_block.argtypes = [vp, i32, i32]
        L.cnf2h_balanced_block.argtypes = [vp, i32, i32, vp, vp]
        L.cnf2h_set_partition.argtypes = [vp, i32, i32, EXCHANGE_FN, vp]
        L.cnf2h_get_partition.argtypes = [vp, vp, vp]
        L.cnf2h_set_update_flags.argtypes = [vp, C.c_uint32]
        L.cnf2h_reserve.argtypes = [vp]
        L.cnf2h_get_timing.argtypes = [vp, vp]
        L.cnf2h_set_deterministic.argtypes = [vp, i32]
        L.cnf2h_context.argtypes = [vp]
        L.cnf2h_context.restype = vp
        L.cnf2h_get_passes.argtypes = [vp, vp, vp, vp]
        L.cnf2h_destroy.argtypes = [vp]
        L.cnf2h_destroy.restype = None
        L.cnf2h_last_error.restype = C.c_char_p
        L.cnf2h_postmarkerdata.argtypes = [vp, i32]
        L.cnf2h_iteration.argtypes = [vp, C.c_char_p, i32]
        L.cnf2h_dump.argtypes = [vp, C.c_char_p, i32]
        L.cnf2h_deserialize.argtypes = [vp, C.c_char_p]
        L.cnf2h_get_state.argtypes = [vp, vp, vp, vp, vp, vp, vp, vp, vp]
        L.cnf2h_map_mstep.argtypes = [vp, i32, vp, i32, vp, vp, vp, vp]
        L.cnf2h_write_map.argtypes = [C.c_char_p, vp, i32, vp, i32]
        L.cnf2h_qtl_permutations.argtypes = [i32, i32, C.c_uint64, vp, vp, vp]
        L.cnf2h_qtl_null_residuals.argtypes = [i32, i32, vp, i32, vp, vp, vp]
        L.cnf2h_qtl2_pair.argtypes = [vp, i32, vp, vp, i32, i32, i32, i32, vp, vp, vp, vp]
        L.cnf2h_qtl2_pair_linked.argtypes = [i32, vp, vp, vp, vp, i32, vp, i32, vp, i32, vp, vp, vp, vp]
        L.cnf2h_qtlx_marker.argtypes = [vp, i32, vp, vp, i32, i32, i32, i32, i32, vp, vp, vp, vp]
        L.cnf2h_qtlx_column.argtypes = [i32, i32, i32, i32, i32, vp, vp]
        L.cnf2h_qtlcof_marker.argtypes = [vp, i32, vp, vp, i32, i32, i32, C.c_uint32, i32, vp, vp, vp, vp, vp]
        L.cnf2h_qtlem_fit.argtypes = [i32, vp, vp, i32, vp, vp, i32, i32, i32, C.c_double, vp, vp, vp, vp, vp, vp, vp, vp]
        L.cnf2h_qtlbin_fit.argtypes = [i32, vp, vp, i32, vp, vp, i32, i32, i32, C.c_double, vp, vp, vp, vp, vp, vp, vp, vp]
        L.cnf2h_qtlsurv_fit.argtypes = [i32, vp, vp, vp, i32, vp, vp, i32, i32, i32, C.c_double, vp, vp, vp, vp, vp, vp, vp, vp]
        L.cnf2h_qtlvar_fit.argtypes = [i32, vp, vp, i32, vp, i32, vp, i32, i32, i32, C.c_double, vp, vp, vp, vp, vp, vp, vp, vp]
        L.cnf2h_kinship_sums.argtypes = [i32, i32, vp, vp, i32, i32, i32, vp, vp]
        L.cnf2h_qtl_cols_marker.argtypes = [i32, i32, vp, vp, i32, vp, i32, vp, vp, vp, vp, vp]
        L.cnf2h_qtl_bootstrap_counts.argtypes = [i32, i32, C.c_uint64, vp, vp, vp]
        L.cnf2h_qtl_boot_marker.argtypes = [i32, vp, i32, vp, i32, vp, vp, vp, i32, vp, vp, vp, vp, vp]
        L.cnf2h_qtl_marker_map.argtypes = [vp, i32, i32, i32, i32, i32, i32, vp, C.c_int64, vp]
        L.cnf2h_qtl_marker_map.restype = C.c_int64
        L.cnf2h_qtl_column_tile.argtypes = [C.c_int64, C.c_int64, C.c_int64, C.c_int64, i32]
        L.cnf2h_qtl_column_tile.restype = C.c_int64
        L.cnf2h_qtlmv_marker.argtypes = [i32, vp, i32, vp, i32, vp, vp, i32, vp, vp, vp, vp]
        L.cnf2h_qtl_group_tile.argtypes = [C.c_int64, C.c_int64, C.c_int64, C.c_int64, C.c_int64, i32]
        L.cnf2h_qtl_group_tile.restype = C.c_int64
        L.cnf2h_qtlimp_marker.argtypes = [i32, i32, vp, i32, vp, i32, vp, vp, i32, vp, vp, vp, vp, vp, vp]
        L.cnf2h_qtlfam_marker.argtypes = [i32, vp, i32, vp, vp, i32, i32, vp, i32, vp, vp, vp, vp, vp, vp, vp, vp]
        L.cnf2h_qtl_families.argtypes = [i32, vp, i32, vp, i32, vp, vp, vp]
        L.cnf2h_descent_columns.argtypes = [i32, vp, i32, vp, i32, vp, vp]
        L.cnf2h_qtlhap_marker.argtypes = [i32, vp, vp, i32, i32, vp, i32, vp, vp, vp, vp, vp, vp, vp]
        L.cnf2h_qtlvc_marker.argtypes = [i32, vp, vp, i32, i32, vp, i32, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp]
        _lib = L
    return _lib


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def map_mstep(pos, chromstarts, xo_sum, n_contrib, genrec=None):
    """cnf2h_map_mstep (include/cnf2host.h): new marker positions from the summed crossover posteriors of a sweep
    (Context.sweep_crossovers: xo_sum[M][6], n_contrib[n_chrom]).  CPU only."""
    L = load()
    pos = np.ascontiguousarray(pos, np.float64)
    cs = np.ascontiguousarray(chromstarts, np.int32)
    xs = np.ascontiguousarray(xo_sum, np.float64).reshape(len(pos), 6)
    cnt = np.ascontiguousarray(n_contrib, np.int32)
    g = None if genrec is None else np.ascontiguousarray(genrec, np.float64)
    out = np.zeros_like(pos)
    rc = L.cnf2h_map_mstep(_p(pos), len(pos), _p(cs), len(cs) - 1, None if g is None else _p(g), _p(xs), _p(cnt), _p(out))
    if rc != 0:
        raise RuntimeError("cnf2h_map_mstep failed (%d)" % rc)
    return out


def qtl_permutations(n, P, seed, use=None, strata=None):
    """cnf2h_qtl_permutations: perm[P][n] by the rule of cnf2freq_amd.qtl.permutations, as `cnF2freq --qtl` makes them.  CPU only."""
    L = load()
    u = None if use is None else np.ascontiguousarray(np.asarray(use) != 0, np.uint8)
    st = None if strata is None else np.ascontiguousarray(strata, np.int32)
    out = np.zeros((P, n), np.int32)
    rc = L.cnf2h_qtl_permutations(n, P, seed, None if u is None else _p(u), None if st is None else _p(st), _p(out))
    if rc != 0:
        raise RuntimeError("cnf2h_qtl_permutations failed (%d)" % rc)
    return out


def qtl2_pair(gram, xty, yy, n_c, n_cov, additive=False, same_chrom=False):
    """cnf2h_qtl2_pair: the pair scan's factorisation and cells (cnf2_qtl2.h) on a normal matrix gram[16][16], xty[R][16]
    and yy[R].  A dict: usable, rank_add, rank_full, rss0[R], lod_add[R], lod_full[R].  CPU only."""
    L = load()
    g = np.ascontiguousarray(gram, np.float64)
    b = np.ascontiguousarray(xty, np.float64).reshape(-1, 16)
    y2 = np.ascontiguousarray(yy, np.float64).reshape(-1)
    if g.shape != (16, 16) or len(y2) != len(b):
        raise ValueError("gram must be [16][16], xty [R][16] and yy [R]")
    R = len(b)
    rank = np.zeros(3, np.int32)
    out = [np.zeros(R) for _ in range(3)]
    rc = L.cnf2h_qtl2_pair(_p(g), R, _p(b), _p(y2), n_c, n_cov, int(additive), int(same_chrom), _p(rank), *[_p(o) for o in out])
    if rc != 0:
        raise RuntimeError("cnf2h_qtl2_pair failed (%d)" % rc)
    return dict(usable=bool(rank[0]), rank_add=int(rank[1]), rank_full=int(rank[2]), rss0=out[0], lod_add=out[1], lod_full=out[2])


def qtl2_pair_linked(o1, o2, joint, y, cov=None, mask=None, additive=False):
    """cnf2h_qtl2_pair_linked: one pair of loci on one chromosome as cnf2_qtl_scan2_linked fits it -- o1, o2 [n][4] the
    origin rows at the two loci, joint [n][16] the pair's rows of sweep_pairs, y [n][R], cov [n][K], mask [n].  A dict as
    qtl2_pair's.  CPU only."""
    L = load()
    o1, o2 = np.ascontiguousarray(o1, np.float64), np.ascontiguousarray(o2, np.float64)
    J = np.ascontiguousarray(joint, np.float64)
    yv = np.ascontiguousarray(y, np.float64)
    yv = yv[:, None] if yv.ndim == 1 else yv
    n = len(o1)
    if o1.shape != (n, 4) or o2.shape != (n, 4) or J.shape != (n, 16) or len(yv) != n:
        raise ValueError("o1, o2 must be [n][4], joint [n][16] and y [n][R]")
    cv = None if cov is None else np.ascontiguousarray(cov, np.float64).reshape(n, -1)
    mk = None if mask is None else np.ascontiguousarray(np.asarray(mask) != 0, np.uint8)
    R = yv.shape[1]
    rank = np.zeros(3, np.int32)
    out = [np.zeros(R) for _ in range(3)]
    rc = L.cnf2h_qtl2_pair_linked(n, _p(o1), _p(o2), _p(J), None if mk is None else _p(mk), 0 if cv is None else cv.shape[1],
                                  None if cv is None else _p(cv), R, _p(yv), int(additive), _p(rank), *[_p(o) for o in out])
    if rc != 0:
        raise RuntimeError("cnf2h_qtl2_pair_linked failed (%d)" % rc)
    return dict(usable=bool(rank[0]), rank_add=int(rank[1]), rank_full=int(rank[2]), rss0=out[0], lod_add=out[1], lod_full=out[2])


def qtlx_marker(gram, xty, yy, n_c, n_cov, n_int=0, additive=False, imprint=False):
    """cnf2h_qtlx_marker: the extended scan's factorisation and cells (cnf2_qtlx.h) on a normal matrix gram[16][16],
    xty[R][16] and yy[R].  A dict: usable, rank[3], rss0[R], lod[R][3], coef[R][ne (1 + n_int)].  CPU only."""
    L = load()
    g = np.ascontiguousarray(gram, np.float64)
    b = np.ascontiguousarray(xty, np.float64).reshape(-1, 16)
    y2 = np.ascontiguousarray(yy, np.float64).reshape(-1)
    if g.shape != (16, 16) or len(y2) != len(b):
        raise ValueError("gram must be [16][16], xty [R][16] and yy [R]")
    R = len(b)
    ne = 1 + (0 if additive else 1) + (1 if imprint else 0)
    rank = np.zeros(4, np.int32)
    rss0, lod, coef = np.zeros(R), np.zeros((R, 3)), np.zeros((R, ne * (1 + n_int)))
    rc = L.cnf2h_qtlx_marker(_p(g), R, _p(b), _p(y2), n_c, n_cov, n_int, int(additive), int(imprint), _p(rank), _p(rss0), _p(lod),
                             _p(coef))
    if rc != 0:
        raise RuntimeError("cnf2h_qtlx_marker failed (%d)" % rc)
    return dict(usable=bool(rank[0]), rank=rank[1:].copy(), rss0=rss0, lod=lod, coef=coef)


def qtlcof_marker(gram, xty, yy, n_c, n_cov, n_cof, skip=0, additive=False):
    """cnf2h_qtlcof_marker: the cofactor scan's factorisation and cells (cnf2_qtlcof.h) on a normal matrix gram[16][16] of the
    design with all n_cof cofactors, xty[R][16] and yy[R]; bit q of `skip` leaves cofactor q out.  A dict: usable, rank_cof,
    rank, rss0[R], lod_base[R], lod[R], coef[R][ne].  CPU only."""
    L = load()
    g = np.ascontiguousarray(gram, np.float64)
    b = np.ascontiguousarray(xty, np.float64).reshape(-1, 16)
    y2 = np.ascontiguousarray(yy, np.float64).reshape(-1)
    if g.shape != (16, 16) or len(y2) != len(b):
        raise ValueError("gram must be [16][16], xty [R][16] and yy [R]")
    R = len(b)
    rank = np.zeros(3, np.int32)
    rss0, base, lod, coef = np.zeros(R), np.zeros(R), np.zeros(R), np.zeros((R, 1 if additive else 2))
    rc = L.cnf2h_qtlcof_marker(_p(g), R, _p(b), _p(y2), n_c, n_cov, n_cof, int(skip), int(additive), _p(rank), _p(rss0), _p(base),
                               _p(lod), _p(coef))
    if rc != 0:
        raise RuntimeError("cnf2h_qtlcof_marker failed (%d)" % rc)
    return dict(usable=bool(rank[0]), rank_cof=int(rank[1]), rank=int(rank[2]), rss0=rss0, lod_base=base, lod=lod, coef=coef)


def kinship_sums(origin, chromstarts, chrom_begin=0, chrom_end=None):
    """cnf2h_kinship_sums: (sum[n][n], markers) of the chromosomes chrom_begin .. chrom_end-1 (None: to the last) on origin rows
    origin[n][M][4] -- what Context.kinship_sums computes on the GPU.  K = (1 + sum / markers) / 2.  CPU only."""
    L = load()
    o = np.ascontiguousarray(origin, np.float64)
    cs = np.ascontiguousarray(chromstarts, np.int32)
    if o.ndim != 3 or o.shape[2] != 4 or cs[-1] != o.shape[1]:
        raise ValueError("origin must be [n][M][4] with M the map's markers")
    n, C = o.shape[0], len(cs) - 1
    chrom_end = C if chrom_end is None else chrom_end
    out, cnt = np.zeros((n, n)), np.zeros(1, np.int32)
    rc = L.cnf2h_kinship_sums(n, o.shape[1], _p(o), _p(cs), C, chrom_begin, chrom_end, _p(out), _p(cnt))
    if rc != 0:
        raise ValueError("cnf2h_kinship_sums refused its arguments (%d)" % rc)
    return out, int(cnt[0])


def qtl_cols_marker(reg, x0, y, scale=None):
    """cnf2h_qtl_cols_marker: one marker of the column scan (cnf2_qtl_scan_cols) on reg[n][ne], x0[n][nx] and the columns
    y[n][R].  A dict: lod[R], coef[R][2], rank, rss0[R].  CPU only."""
    L = load()
    r = np.ascontiguousarray(reg, np.float64)
    r = r[:, None] if r.ndim == 1 else r
    x = np.ascontiguousarray(x0, np.float64)
    v = np.ascontiguousarray(y, np.float64)
    v = v[:, None] if v.ndim == 1 else v
    n = r.shape[0]
    if x.ndim != 2 or x.shape[0] != n or v.shape[0] != n:
        raise ValueError("reg, x0 and y must have n rows")
    s = None if scale is None else np.ascontiguousarray(scale, np.float64)
    R = v.shape[1]
    lod, coef, rank, rss0 = np.zeros(R), np.zeros((R, 2)), np.zeros(1, np.int32), np.zeros(R)
    rc = L.cnf2h_qtl_cols_marker(n, r.shape[1], _p(r), None if s is None else _p(s), x.shape[1], _p(x), R, _p(v), _p(lod), _p(coef),
                                 _p(rank), _p(rss0))
    if rc != 0:
        raise ValueError("cnf2h_qtl_cols_marker refused its arguments (%d)" % rc)
    return dict(lod=lod, coef=coef, rank=int(rank[0]), rss0=rss0)


def qtl_bootstrap_counts(n, B, seed, use=None, strata=None):
    """cnf2h_qtl_bootstrap_counts: count[B][n] by the rule of cnf2freq_amd.qtl.bootstrap_counts, as `cnF2freq --qtlboot` makes
    them.  CPU only."""
    L = load()
    u = None if use is None else np.ascontiguousarray(np.asarray(use) != 0, np.uint8)
    st = None if strata is None else np.ascontiguousarray(strata, np.int32)
    out = np.zeros((B, n), np.int32)
    rc = L.cnf2h_qtl_bootstrap_counts(n, B, seed, None if u is None else _p(u), None if st is None else _p(st), _p(out))
    if rc != 0:
        raise RuntimeError("cnf2h_qtl_bootstrap_counts failed (%d)" % rc)
    return out


def qtl_boot_marker(origin, y, count, cov=None, c=None, additive=False):
    """cnf2h_qtl_boot_marker: one (replicate, marker) cell of the bootstrap scan (cnf2_qtl_scan_boot) on the marker's rows
    origin[n][4], the columns y[n][T] and cov[n][K] as they enter the sums, the chromosome's mask c[n] (None: all) and the
    replicate count[n].  A dict: lod[T], coef[T][2], rank, rss0[T], n_bc.  CPU only."""
    L = load()
    o = np.ascontiguousarray(origin, np.float64)
    n = o.shape[0]
    v = np.ascontiguousarray(y, np.float64).reshape(n, -1)
    z = None if cov is None else np.ascontiguousarray(cov, np.float64).reshape(n, -1)
    K = 0 if z is None else z.shape[1]
    m = np.ones(n, np.uint8) if c is None else np.ascontiguousarray(np.asarray(c) != 0, np.uint8)
    w = np.ascontiguousarray(count, np.int32)
    if o.shape != (n, 4) or m.shape != (n,) or w.shape != (n,):
        raise ValueError("origin must be [n][4], c and count [n]")
    T = v.shape[1]
    lod, coef, rss0 = np.zeros(T), np.zeros((T, 2)), np.zeros(T)
    rank, n_bc = np.zeros(1, np.int32), np.zeros(1, np.int32)
    rc = L.cnf2h_qtl_boot_marker(n, _p(o), T, _p(v), K, None if K == 0 else _p(z), _p(m), _p(w), int(additive), _p(lod), _p(coef),
                                 _p(rank), _p(rss0), _p(n_bc))
    if rc != 0:
        raise ValueError("cnf2h_qtl_boot_marker refused its arguments (%d)" % rc)
    return dict(lod=lod, coef=coef, rank=int(rank[0]), rss0=rss0, n_bc=int(n_bc[0]))


def qtlimp_marker(state, y, cov=None, c=None, additive=False):
    """cnf2h_qtlimp_marker: one marker of the multiple-imputation scan (cnf2_qtl_scan_imp) on the marker's sampled states
    state[n][D] (uint8), the columns y[n][T] and cov[n][K] as they enter the sums and the chromosome's mask c[n] (None: all).
    A dict: lod[T] the combined LOD, coef[T][2], rank (the smallest over the draws), rss0[T], n_used, draw_lod[D][T].
    CPU only."""
    L = load()
    st = np.ascontiguousarray(state, np.uint8)
    st = st[:, None] if st.ndim == 1 else st
    n, D = st.shape
    v = np.ascontiguousarray(y, np.float64).reshape(n, -1)
    z = None if cov is None else np.ascontiguousarray(cov, np.float64).reshape(n, -1)
    K = 0 if z is None else z.shape[1]
    m = np.ones(n, np.uint8) if c is None else np.ascontiguousarray(np.asarray(c) != 0, np.uint8)
    if m.shape != (n,):
        raise ValueError("state must be [n][D] and c [n]")
    T = v.shape[1]
    lod, coef, rss0, draw = np.zeros(T), np.zeros((T, 2)), np.zeros(T), np.zeros((D, T))
    rank, n_used = np.zeros(1, np.int32), np.zeros(1, np.int32)
    rc = L.cnf2h_qtlimp_marker(n, D, _p(st), T, _p(v), K, None if K == 0 else _p(z), _p(m), int(additive), _p(lod), _p(coef),
                               _p(rank), _p(rss0), _p(n_used), _p(draw))
    if rc != 0:
        raise ValueError("cnf2h_qtlimp_marker refused its arguments (%d)" % rc)
    return dict(lod=lod, coef=coef, rank=int(rank[0]), rss0=rss0, n_used=int(n_used[0]), draw_lod=draw)


def qtlfam_marker(origin, side, grp, n_fam, y, cell=None, cov=None, c=None, slopes=True):
    """cnf2h_qtlfam_marker: one marker of the within-family scan (cnf2_qtl_scan_fam) on the marker's rows origin[n][4], the
    slope groups grp[n] (< 0: not nested), the mean cells cell[n] (None: grp), y[n][T] and cov[n][K] as they enter the sums and
    the chromosome's mask c[n].  A dict: lod[T], df, slope[T][F] (None without slopes), rss0[T], n_used, n_cells.  CPU only."""
    L = load()
    o = np.ascontiguousarray(origin, np.float64).reshape(-1, 4)
    n = o.shape[0]
    g = np.ascontiguousarray(grp, np.int32)
    q = None if cell is None else np.ascontiguousarray(cell, np.int32)
    v = np.ascontiguousarray(y, np.float64).reshape(n, -1)
    T = v.shape[1]
    z = None if cov is None else np.ascontiguousarray(cov, np.float64).reshape(n, -1)
    K = 0 if z is None else z.shape[1]
    m = np.ones(n, np.uint8) if c is None else np.ascontiguousarray(np.asarray(c) != 0, np.uint8)
    lod, rss0, slope = np.zeros(T), np.zeros(T), np.zeros((T, n_fam)) if slopes else None
    df, n_used, n_cells = np.zeros(1, np.int32), np.zeros(1, np.int32), np.zeros(1, np.int32)
    rc = L.cnf2h_qtlfam_marker(n, _p(o), int(side), _p(g), None if q is None else _p(q), int(n_fam), T, _p(v), K,
                               None if K == 0 else _p(z), _p(m), _p(lod), _p(df), None if slope is None else _p(slope), _p(rss0),
                               _p(n_used), _p(n_cells))
    if rc != 0:
        raise ValueError("cnf2h_qtlfam_marker refused its arguments (%d)" % rc)
    return dict(lod=lod, df=int(df[0]), slope=slope, rss0=rss0, n_used=int(n_used[0]), n_cells=int(n_cells[0]))


def qtl_families(par, dous, side):
    """cnf2h_qtl_families: (grp[n], cell[n], F) of the analysed records dous[n] from the pedigree's par[n_rec][2] -- the parent
    on the side (0: the first, 1: the second) and the pair of parents, numbered from 0; -1 where that parent is missing or has
    no recorded parents.  CPU only."""
    L = load()
    par = np.ascontiguousarray(par, np.int32).reshape(-1, 2)
    dous = np.ascontiguousarray(dous, np.int32)
    grp, cell, F = np.zeros(len(dous), np.int32), np.zeros(len(dous), np.int32), np.zeros(1, np.int32)
    rc = L.cnf2h_qtl_families(len(par), _p(par), len(dous), _p(dous), int(side), _p(grp), _p(cell), _p(F))
    if rc != 0:
        raise ValueError("cnf2h_qtl_families refused its arguments (%d)" % rc)
    return grp, cell, int(F[0])


def qtlhap_marker(descent, col, n_columns, y, cov=None, c=None, coef=True):
    """cnf2h_qtlhap_marker: one marker of the founder-haplotype scan (cnf2_qtl_scan_hap) on the marker's rows descent[n][8],
    the columns col[n][8], y[n][T] and cov[n][K] as they enter the sums and the chromosome's mask c[n].  A dict: lod[T], df,
    coef[T][H] (None without coef), rss0[T], n_used.  CPU only."""
    L = load()
    d = np.ascontiguousarray(descent, np.float64).reshape(-1, 8)
    n = d.shape[0]
    q = np.ascontiguousarray(col, np.int32).reshape(n, 8)
    v = np.ascontiguousarray(y, np.float64).reshape(n, -1)
    T, H = v.shape[1], int(n_columns)
    z = None if cov is None else np.ascontiguousarray(cov, np.float64).reshape(n, -1)
    K = 0 if z is None else z.shape[1]
    m = np.ones(n, np.uint8) if c is None else np.ascontiguousarray(np.asarray(c) != 0, np.uint8)
    lod, rss0, co = np.zeros(T), np.zeros(T), np.zeros((T, max(H, 0))) if coef else None
    df, n_used = np.zeros(1, np.int32), np.zeros(1, np.int32)
    rc = L.cnf2h_qtlhap_marker(n, _p(d), _p(q), H, T, _p(v), K, None if K == 0 else _p(z), _p(m), _p(lod), _p(df),
                               None if co is None else _p(co), _p(rss0), _p(n_used))
    if rc != 0:
        raise ValueError("cnf2h_qtlhap_marker refused its arguments (%d)" % rc)
    return dict(lod=lod, df=int(df[0]), coef=co, rss0=rss0, n_used=int(n_used[0]))


def qtlvc_marker(descent, col, n_columns, y, cov=None, c=None, blup=True):
    """cnf2h_qtlvc_marker: one marker of the variance-component scan (cnf2_qtl_scan_vc), the arguments of qtlhap_marker with up to
    64 columns.  A dict: lod[T], h[T], sigma2[T], blup[T][H] (None without blup), eval[H], rank (-1: the Jacobi iteration did not
    converge), rss0[T], n_used.  CPU only."""
    L = load()
    d = np.ascontiguousarray(descent, np.float64).reshape(-1, 8)
    n = d.shape[0]
    q = np.ascontiguousarray(col, np.int32).reshape(n, 8)
    v = np.ascontiguousarray(y, np.float64).reshape(n, -1)
    T, H = v.shape[1], int(n_columns)
    z = None if cov is None else np.ascontiguousarray(cov, np.float64).reshape(n, -1)
    K = 0 if z is None else z.shape[1]
    m = np.ones(n, np.uint8) if c is None else np.ascontiguousarray(np.asarray(c) != 0, np.uint8)
    lod, h, s2, rss0 = np.zeros(T), np.zeros(T), np.zeros(T), np.zeros(T)
    bl, ev = np.zeros((T, max(H, 0))) if blup else None, np.zeros(max(H, 0))
    rank, n_used = np.zeros(1, np.int32), np.zeros(1, np.int32)
    rc = L.cnf2h_qtlvc_marker(n, _p(d), _p(q), H, T, _p(v), K, None if K == 0 else _p(z), _p(m), _p(lod), _p(h), _p(s2),
                              None if bl is None else _p(bl), _p(ev), _p(rank), _p(rss0), _p(n_used))
    if rc != 0:
        raise ValueError("cnf2h_qtlvc_marker refused its arguments (%d)" % rc)
    return dict(lod=lod, h=h, sigma2=s2, blup=bl, eval=ev, rank=int(rank[0]), rss0=rss0, n_used=int(n_used[0]))


def descent_columns(par, dous, by="haplotype"):
    """cnf2h_descent_columns: (col[n][8], G), the model column of every cell of the analysed records' descent rows by
    "haplotype", "founder" or "line" (origins.descent_columns' rule, which `cnF2freq --qtlhap` uses) and the number of distinct
    grandparents.  CPU only."""
    L = load()
    par = np.ascontiguousarray(par, np.int32).reshape(-1, 2)
    dous = np.ascontiguousarray(dous, np.int32)
    col, G = np.zeros((len(dous), 8), np.int32), np.zeros(1, np.int32)
    rc = L.cnf2h_descent_columns(len(par), _p(par), len(dous), _p(dous), ("haplotype", "founder", "line").index(by), _p(col), _p(G))
    if rc != 0:
        raise ValueError("cnf2h_descent_columns refused its arguments (%d)" % rc)
    return col, int(G[0])


def qtl_marker_map(chromstarts, tile, chrom_begin=0, chrom_end=None, with_mchrom=False, whole_map_header=True):
    """cnf2h_qtl_marker_map: the marker map a QTL scan uploads (cnf2_qtlplan.h) as dict(image, o_mchrom, o_tiles, o_tstart,
    n_tiles) -- the int32 words and the offsets of their blocks.  CPU only."""
    L = load()
    cs = np.ascontiguousarray(chromstarts, np.int32)
    nc = len(cs) - 1
    args = (_p(cs), nc, chrom_begin, nc if chrom_end is None else chrom_end, tile, int(with_mchrom), int(whole_map_header))
    off = np.zeros(4, np.int64)
    words = L.cnf2h_qtl_marker_map(*args, None, 0, _p(off))
    if words < 0:
        raise ValueError("cnf2h_qtl_marker_map refused its arguments (%d)" % words)
    image = np.zeros(words, np.int32)
    L.cnf2h_qtl_marker_map(*args, _p(image), words, _p(off))
    return dict(image=image, o_mchrom=int(off[0]), o_tiles=int(off[1]), o_tstart=int(off[2]), n_tiles=int(off[3]))


def qtl_column_tile(n, R, P, maxima_doubles_per_column=0, cap=0):
    """cnf2h_qtl_column_tile: the columns a QTL scan takes per pass (cnf2_qtlplan.h).  CPU only."""
    rt = load().cnf2h_qtl_column_tile(n, R, P, maxima_doubles_per_column, cap)
    if rt < 0:
        raise ValueError("cnf2h_qtl_column_tile refused its arguments (%d)" % rt)
    return rt


def qtlmv_marker(origin, y, cov=None, c=None, additive=False):
    """cnf2h_qtlmv_marker: one (marker, group) cell of the multi-trait scan (cnf2_qtl_scan_mv) on the marker's rows
    origin[n][4], the columns y[n][T] and cov[n][K] as they enter the sums and the chromosome's mask c[n] (None: all).  A
    dict: lod, rank, trait_rank, n_used.  CPU only."""
    L = load()
    o = np.ascontiguousarray(origin, np.float64)
    n = o.shape[0]
    v = np.ascontiguousarray(y, np.float64).reshape(n, -1)
    z = None if cov is None else np.ascontiguousarray(cov, np.float64).reshape(n, -1)
    K = 0 if z is None else z.shape[1]
    m = np.ones(n, np.uint8) if c is None else np.ascontiguousarray(np.asarray(c) != 0, np.uint8)
    if o.shape != (n, 4) or m.shape != (n,):
        raise ValueError("origin must be [n][4] and c [n]")
    lod, rank, trank, n_c = np.zeros(1), np.zeros(1, np.int32), np.zeros(1, np.int32), np.zeros(1, np.int32)
    rc = L.cnf2h_qtlmv_marker(n, _p(o), v.shape[1], _p(v), K, None if K == 0 else _p(z), _p(m), int(additive), _p(lod), _p(rank),
                              _p(trank), _p(n_c))
    if rc != 0:
        raise ValueError("cnf2h_qtlmv_marker refused its arguments (%d)" % rc)
    return dict(lod=float(lod[0]), rank=int(rank[0]), trait_rank=int(trank[0]), n_used=int(n_c[0]))


def qtl_group_tile(n, T, G, P, n_tiles, cap=0):
    """cnf2h_qtl_group_tile: the groups the multi-trait scan takes per pass (cnf2_qtlplan.h).  CPU only."""
    gt = load().cnf2h_qtl_group_tile(n, T, G, P, n_tiles, cap)
    if gt < 0:
        raise ValueError("cnf2h_qtl_group_tile refused its arguments (%d)" % gt)
    return gt


def qtlx_columns(n_cov, n_int=0, additive=False, imprint=False):
    """cnf2h_qtlx_column for every column of the design: a list of (effect, modifier) codes as cnf2_qtlx.h defines them --
    effect 0 = 1, 1 = a, 2 = d, 3 = i; modifier 0 = 1, k = covariate k - 1.  CPU only."""
    L = load()
    e, z = np.zeros(1, np.int32), np.zeros(1, np.int32)
    W = L.cnf2h_qtlx_column(n_cov, n_int, int(additive), int(imprint), 0, _p(e), _p(z))
    if W < 0:
        raise RuntimeError("cnf2h_qtlx_column failed (%d)" % W)
    out = []
    for j in range(W):
        L.cnf2h_qtlx_column(n_cov, n_int, int(additive), int(imprint), j, _p(e), _p(z))
        out.append((int(e[0]), int(z[0])))
    return out


def qtlem_fit(origin, y, cov=None, c=None, additive=False, imprint=False, max_iter=1000, tol=1e-6):
    """cnf2h_qtlem_fit: one (marker, column) fit of the maximum-likelihood scan (cnf2_qtlem.h) on the marker's rows
    origin[n][4], the phenotype y[n], covariates cov[n][K] and the chromosome's mask c[n] (None: everybody).  A dict: lod,
    coef[ne], sigma2, iters, status, rank, rss0, n_used.  CPU only."""
    L = load()
    o = np.ascontiguousarray(origin, np.float64)
    y = np.ascontiguousarray(y, np.float64).reshape(-1)
    n = len(y)
    if o.shape != (n, 4):
        raise ValueError("origin must be [n][4] and y [n]")
    z = None if cov is None else np.ascontiguousarray(cov, np.float64).reshape(n, -1)
    K = 0 if z is None else z.shape[1]
    m = np.ones(n, np.uint8) if c is None else np.ascontiguousarray(np.asarray(c) != 0, np.uint8)
    ne = 1 + (0 if additive else 1) + (1 if imprint else 0)
    d, coef, i3 = np.zeros(3), np.zeros(ne), np.zeros(4, np.int32)
    rc = L.cnf2h_qtlem_fit(n, _p(o), _p(y), K, None if K == 0 else _p(z), _p(m), int(additive), int(imprint), int(max_iter),
                           float(tol), _p(d[0:1]), _p(coef), _p(d[1:2]), _p(i3[0:1]), _p(i3[1:2]), _p(i3[2:3]), _p(d[2:3]),
                           _p(i3[3:4]))
    if rc != 0:
        raise RuntimeError("cnf2h_qtlem_fit failed (%d)" % rc)
    return dict(lod=float(d[0]), coef=coef, sigma2=float(d[1]), iters=int(i3[0]), status=int(i3[1]), rank=int(i3[2]),
                rss0=float(d[2]), n_used=int(i3[3]))


def qtlbin_fit(origin, y, cov=None, c=None, additive=False, imprint=False, max_iter=50, tol=1e-7):
    """cnf2h_qtlbin_fit: one (marker, column) fit of the binary-trait scan (cnf2_qtlbin.h) on the marker's rows origin[n][4],
    the 0/1 phenotype y[n], covariates cov[n][K] and the chromosome's mask c[n] (None: everybody).  A dict: lod, coef[ne],
    iters, status, rank, ll0, n_ones, n_used.  CPU only."""
    L = load()
    o = np.ascontiguousarray(origin, np.float64)
    y = np.ascontiguousarray(y, np.float64).reshape(-1)
    n = len(y)
    if o.shape != (n, 4):
        raise ValueError("origin must be [n][4] and y [n]")
    z = None if cov is None else np.ascontiguousarray(cov, np.float64).reshape(n, -1)
    K = 0 if z is None else z.shape[1]
    m = np.ones(n, np.uint8) if c is None else np.ascontiguousarray(np.asarray(c) != 0, np.uint8)
    ne = 1 + (0 if additive else 1) + (1 if imprint else 0)
    d, coef, i5 = np.zeros(2), np.zeros(ne), np.zeros(5, np.int32)
    rc = L.cnf2h_qtlbin_fit(n, _p(o), _p(y), K, None if K == 0 else _p(z), _p(m), int(additive), int(imprint), int(max_iter),
                            float(tol), _p(d[0:1]), _p(coef), _p(i5[0:1]), _p(i5[1:2]), _p(i5[2:3]), _p(d[1:2]), _p(i5[3:4]),
                            _p(i5[4:5]))
    if rc != 0:
        raise RuntimeError("cnf2h_qtlbin_fit failed (%d)" % rc)
    return dict(lod=float(d[0]), coef=coef, iters=int(i5[0]), status=int(i5[1]), rank=int(i5[2]), ll0=float(d[1]),
                n_ones=int(i5[3]), n_used=int(i5[4]))


def qtlsurv_fit(origin, time, status, cov=None, c=None, additive=False, imprint=False, max_iter=50, tol=1e-7):
    """cnf2h_qtlsurv_fit: one (marker, column) fit of the survival-trait scan (cnf2_qtlsurv.h) on the marker's rows
    origin[n][4], time[n] and status[n] (1 = event, 0 = censored), covariates cov[n][K] and the chromosome's mask c[n] (None:
    everybody).  A dict: lod, coef[ne], iters, status, rank, ll0, n_events, n_used.  CPU only."""
    L = load()
    o = np.ascontiguousarray(origin, np.float64)
    t = np.ascontiguousarray(time, np.float64).reshape(-1)
    s = np.ascontiguousarray(status, np.float64).reshape(-1)
    n = len(t)
    if o.shape != (n, 4) or s.shape != (n,):
        raise ValueError("origin must be [n][4], time and status [n]")
    z = None if cov is None else np.ascontiguousarray(cov, np.float64).reshape(n, -1)
    K = 0 if z is None else z.shape[1]
    m = np.ones(n, np.uint8) if c is None else np.ascontiguousarray(np.asarray(c) != 0, np.uint8)
    ne = 1 + (0 if additive else 1) + (1 if imprint else 0)
    d, coef, i5 = np.zeros(2), np.zeros(ne), np.zeros(5, np.int32)
    rc = L.cnf2h_qtlsurv_fit(n, _p(o), _p(t), _p(s), K, None if K == 0 else _p(z), _p(m), int(additive), int(imprint),
                             int(max_iter), float(tol), _p(d[0:1]), _p(coef), _p(i5[0:1]), _p(i5[1:2]), _p(i5[2:3]), _p(d[1:2]),
                             _p(i5[3:4]), _p(i5[4:5]))
    if rc != 0:
        raise RuntimeError("cnf2h_qtlsurv_fit failed (%d)" % rc)
    return dict(lod=float(d[0]), coef=coef, iters=int(i5[0]), status=int(i5[1]), rank=int(i5[2]), ll0=float(d[1]),
                n_events=int(i5[3]), n_used=int(i5[4]))


def qtlvar_fit(origin, y, cov=None, n_var=0, c=None, additive=False, imprint=False, max_iter=50, tol=1e-7):
    """cnf2h_qtlvar_fit: one (marker, column) cell of the variance-QTL scan (cnf2_qtlvar.h) on the marker's rows origin[n][4],
    the trait y[n], covariates cov[n][K] of which the first n_var enter the variance design, and the chromosome's mask c[n]
    (None: everybody).  A dict: lod[3] (joint, mean, variance), coef_mean[ne] and coef_var[ne] of the full fit, iters[3] and
    status[3] by fit (mean-only, variance-only, full), rank, ll0, n_used.  CPU only."""
    L = load()
    o = np.ascontiguousarray(origin, np.float64)
    y = np.ascontiguousarray(y, np.float64).reshape(-1)
    n = len(y)
    if o.shape != (n, 4):
        raise ValueError("origin must be [n][4] and y [n]")
    z = None if cov is None else np.ascontiguousarray(cov, np.float64).reshape(n, -1)
    K = 0 if z is None else z.shape[1]
    m = np.ones(n, np.uint8) if c is None else np.ascontiguousarray(np.asarray(c) != 0, np.uint8)
    ne = 1 + (0 if additive else 1) + (1 if imprint else 0)
    lod, cm, cv, d = np.zeros(3), np.zeros(ne), np.zeros(ne), np.zeros(1)
    iters, status, i2 = np.zeros(3, np.int32), np.zeros(3, np.int32), np.zeros(2, np.int32)
    rc = L.cnf2h_qtlvar_fit(n, _p(o), _p(y), K, None if K == 0 else _p(z), int(n_var), _p(m), int(additive), int(imprint),
                            int(max_iter), float(tol), _p(lod), _p(cm), _p(cv), _p(iters), _p(status), _p(i2[0:1]), _p(d),
                            _p(i2[1:2]))
    if rc != 0:
        raise RuntimeError("cnf2h_qtlvar_fit failed (%d)" % rc)
    return dict(lod=lod, coef_mean=cm, coef_var=cv, iters=iters, status=status, rank=int(i2[0]), ll0=float(d[0]),
                n_used=int(i2[1]))


def qtl_null_residuals(pheno, cov=None, use=None):
    """cnf2h_qtl_null_residuals: cnf2freq_amd.qtl.null_residuals as `cnF2freq --qtl` computes them (normal equations).  CPU only."""
    L = load()
    y = np.ascontiguousarray(pheno, np.float64)
    y = np.ascontiguousarray(y[:, None]) if y.ndim == 1 else y
    n, T = y.shape
    z = None if cov is None else np.ascontiguousarray(np.asarray(cov, np.float64).reshape(n, -1))
    u = np.ones(n, np.uint8) if use is None else np.ascontiguousarray(np.asarray(use) != 0, np.uint8)
    out = np.zeros((n, T))
    rc = L.cnf2h_qtl_null_residuals(n, T, _p(y), 0 if z is None else z.shape[1], None if z is None else _p(z), _p(u), _p(out))
    if rc != 0:
        raise RuntimeError("cnf2h_qtl_null_residuals failed (%d): %s" % (rc, (L.cnf2h_last_error() or b"").decode()))
    return out


def write_map(path, pos, chromstarts):
    """cnf2h_write_map: the map as a .map file, read back and checked (RuntimeError if it does not round-trip)."""
    L = load()
    pos = np.ascontiguousarray(pos, np.float64)
    cs = np.ascontiguousarray(chromstarts, np.int32)
    rc = L.cnf2h_write_map(os.fsencode(path), _p(pos), len(pos), _p(cs), len(cs) - 1)
    if rc != 0:
        raise RuntimeError("cnf2h_write_map failed (%d): %s" % (rc, (L.cnf2h_last_error() or b"").decode()))


class Run:
    """One run over a cnf2freq_amd.synth.Pedigree (records that are not `empty` count as genotyped, i.e. they have
    priors, unless has_prior is given)."""

    def __init__(self, ped, has_prior=None, quiet=True, device=0):
        self.L = load()
        if np.array_equal(ped.row_of, np.arange(1, ped.n_rec + 1)):
            a, s, h = ped.allele[1:], ped.sure[1:], ped.hw[1:]       # one row per record already: no copies (bench-scale inputs)
        else:
            a, s, h = ped.dense()
        hp = (1 - np.asarray(ped.empty)).astype(np.uint8) if has_prior is None else np.ascontiguousarray(has_prior, np.uint8)
        args = [np.ascontiguousarray(ped.par, np.int32), np.ascontiguousarray(ped.empty, np.uint8),
                np.ascontiguousarray(ped.gen, np.int32), hp, np.ascontiguousarray(a, np.uint8),
                np.ascontiguousarray(s, np.float64), np.ascontiguousarray(h, np.float64),
                np.ascontiguousarray(ped.pos, np.float64)]
        cs = np.ascontiguousarray(ped.chromstarts, np.int32)
        dous = np.ascontiguousarray(ped.dous, np.int32)
        self._adopt(self.L.cnf2h_create_on(device, ped.n_rec, *[_p(x) for x in args[:8]], ped.n_markers, _p(cs), len(cs) - 1,
                                           _p(dous), len(dous), 1 if quiet else 0), "cnf2h_create")

    @classmethod
    def from_files(cls, mapfile, pedfile, genfile, quiet=True, device=0):
        """cnf2h_create_from_files: a run over PlantImpute-format files, read by the executable's own readers; n_dous is
        the number of analysed individuals"""
        self = cls.__new__(cls)
        self.L = load()
        self._adopt(self.L.cnf2h_create_from_files(device, os.fsencode(mapfile), os.fsencode(pedfile), os.fsencode(genfile),
                                                   1 if quiet else 0), "cnf2h_create_from_files")
        return self

    def _adopt(self, handle, what):
        """the one place where a run's attributes are set, for every constructor: the handle and, from cnf2h_get_dims,
        n_rec, M, n_chrom, n_dous"""
        self.h = handle
        if not self.h:
            raise RuntimeError("%s: %s" % (what, self.L.cnf2h_last_error().decode()))
        dims = np.zeros(4, np.int32)
        self._chk(self.L.cnf2h_get_dims(self.h, _p(dims)), "cnf2h_get_dims")
        self.n_rec, self.M, self.n_chrom, self.n_dous = (int(v) for v in dims)

    def close(self):
        if getattr(self, "h", None):
            self.L.cnf2h_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _chk(self, rc, what):
        if rc != 0:
            raise RuntimeError("%s: %s" % (what, self.L.cnf2h_last_error().decode()))

    def postmarkerdata(self, indcount=None):
        self._chk(self.L.cnf2h_postmarkerdata(self.h, self.n_rec + 1 if indcount is None else indcount), "cnf2h_postmarkerdata")

    def iteration(self, rows_path=None, update=True):
        self._chk(self.L.cnf2h_iteration(self.h, None if rows_path is None else str(rows_path).encode(), 1 if update else 0),
                  "cnf2h_iteration")

    def set_block(self, begin, end):
        self._chk(self.L.cnf2h_set_block(self.h, begin, end), "cnf2h_set_block")

    def balanced_block(self, rank, world):
        b, e = C.c_int32(0), C.c_int32(0)
        self._chk(self.L.cnf2h_balanced_block(self.h, rank, world, C.byref(b), C.byref(e)), "cnf2h_balanced_block")
        return b.value, e.value

    def set_partition(self, rank, world, fn=None):
        """Plans the multi-process run and sets this rank's block (cnf2host.h: cnf2h_set_partition).
        fn(op, buf, count, seg) -> 0 is the transport: op one of X_SUM_SEGMENTS (buf = device address, count doubles),
        X_SUM_HITS (buf = host address of int32[count]), X_GATHER_SEGMENTS (buf = device address, count bytes)."""
        def tramp(_user, op, buf, count, seg):
            try:
                return int(fn(op, buf, count, seg) or 0)
            except Exception:                 # an exception must not unwind through the C frames
                import traceback
                traceback.print_exc()
                return -1
        self._exchange = EXCHANGE_FN(tramp if fn is not None else 0)   # keep the trampoline alive
        self._chk(self.L.cnf2h_set_partition(self.h, rank, world, self._exchange, None), "cnf2h_set_partition")
        return self.partition()

    def partition(self):
        info = np.zeros(10, np.int64)
        self._chk(self.L.cnf2h_get_partition(self.h, _p(info), None), "cnf2h_get_partition")
        owned = np.zeros(int(info[2]), np.int32)
        self._chk(self.L.cnf2h_get_partition(self.h, _p(info), _p(owned) if len(owned) else None), "cnf2h_get_partition")
        return dict(block=(int(info[0]), int(info[1])), owned=owned, n_shared=int(info[3]), segment_records=int(info[4]),
                    bytes_accumulators=int(info[5]), bytes_rows=int(info[6]), bytes_hits=int(info[7]), bytes_payload=int(info[8]),
                    n_private=int(info[9]))

    def reserve(self):
        """The device buffers of the iterations now, not inside the first one (optional)."""
        self._chk(self.L.cnf2h_reserve(self.h), "cnf2h_reserve")

    def timing(self):
        """Wall time of the last iteration by where it went (seconds)."""
        t = np.zeros(5)
        self._chk(self.L.cnf2h_get_timing(self.h, _p(t)), "cnf2h_get_timing")
        return dict(sweep_accumulate_s=float(t[0]), exchange_s=float(t[1]), update_s=float(t[2]), host_s=float(t[3]), total_s=float(t[4]))

    def set_update_flags(self, flags):
        """capi.UPDATE_BOTH_FLOWS (bit-exact fast form), capi.UPDATE_PLAIN (literal kernels), capi.UPDATE_ONE_SCOUT; 0 = default."""
        self._chk(self.L.cnf2h_set_update_flags(self.h, flags), "cnf2h_set_update_flags")

    def set_deterministic(self, on=True):
        self._chk(self.L.cnf2h_set_deterministic(self.h, 1 if on else 0), "cnf2h_set_deterministic")

    def context(self):
        return self.L.cnf2h_context(self.h)

    def passes(self, accumulators=True):
        """hits[C] of the last iteration's update passes and (optionally) haplobase / haplocount [R][M] as left behind."""
        hits = np.zeros(self.n_chrom, np.int32)
        hb = np.zeros((self.n_rec, self.M)) if accumulators else None
        hc = np.zeros((self.n_rec, self.M)) if accumulators else None
        self._chk(self.L.cnf2h_get_passes(self.h, _p(hits), None if hb is None else _p(hb), None if hc is None else _p(hc)),
                  "cnf2h_get_passes")
        return dict(hits=hits, haplobase=hb, haplocount=hc)

    def dump(self, path, limit=1000000):
        assert self.L.cnf2h_dump(self.h, str(path).encode(), limit) == 0

    def deserialize(self, path):
        assert self.L.cnf2h_deserialize(self.h, str(path).encode()) == 0

    def state(self):
        R, M = self.n_rec, self.M
        allele = np.zeros((R, M, 2), np.uint8)
        sure = np.zeros((R, M, 2))
        hw = np.zeros((R, M))
        desc = np.zeros(R, np.int32)
        ch = np.zeros(R, np.int32)
        var = np.zeros((R, M))
        sf = C.c_double(0)
        hits = C.c_int(0)
        rc = self.L.cnf2h_get_state(self.h, _p(allele), _p(sure), _p(hw), _p(desc), _p(ch), _p(var), C.byref(sf),
                                    C.byref(hits))
        assert rc == 0
        return dict(allele=allele, sure=sure, hw=hw, descendants=desc, children=ch, variances=var,
                    scalefactor=sf.value, hits=hits.value)
