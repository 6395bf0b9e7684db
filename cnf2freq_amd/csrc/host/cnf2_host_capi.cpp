// cnf2_host_capi.cpp -- implementation of include/cnf2host.h: the engine of the `cnF2freq` command line
// (cnf2_engine.cpp) driven from arrays.
#include "../../../include/cnf2host.h"

#include <stdio.h>

#include <string>

#include "cnf2_engine.h"
#include "cnf2_qtl_host.h"
#include "../cnf2_qtl2.h"
#include "../cnf2_qtlx.h"
#include "../cnf2_qtlcof.h"
#include "../cnf2_qtlem.h"
#include "../cnf2_qtlbin.h"
#include "../cnf2_qtlsurv.h"
#include "../cnf2_qtlvar.h"
#include "../cnf2_qtlboot.h"
#include "../cnf2_qtlimp.h"
#include "../cnf2_qtlmv.h"
#include "../cnf2_qtlfam.h"
#include "../cnf2_qtlhap.h"
#include "../cnf2_qtlvc.h"
#include "../cnf2_qtlplan.h"
#include "cnf2_remap.h"

using namespace cnf2host;

struct cnf2h_run {
    Pedigree  P;
    cnf2_ctx* ctx = nullptr;
    Engine*   E = nullptr;
};

static std::string g_err;

// runs f(); an EngineError becomes its code and g_err
template <class F>
static int guarded(F&& f)
{
    try {
        f();
        return 0;
    } catch (const EngineError& e) {
        g_err = e.what();
        return e.code;
    } catch (const std::exception& e) {
        g_err = e.what();
        return CNF2_ERR_STATE;
    }
}

// context, engine and upload of a run whose pedigree is filled; deletes the run where that fails
static cnf2h_run* start(cnf2h_run* run, int device, int quiet)
{
    if (cnf2_ctx_create(device, &run->ctx) != CNF2_OK) {
        g_err = cnf2_last_error(nullptr);
        delete run;
        return nullptr;
    }
    EngineOptions eo;
    eo.quiet = quiet != 0;
    run->E = new Engine(run->P, run->ctx, eo);
    if (guarded([&] { run->E->upload(); }) != 0) {
        cnf2h_destroy(run);
        return nullptr;
    }
    return run;
}

extern "C" {

const char* cnf2h_last_error(void) { return g_err.c_str(); }

cnf2h_run* cnf2h_create(int n_rec, const int32_t* par, const uint8_t* empty, const int32_t* gen, const uint8_t* has_prior,
                        const uint8_t* allele, const double* sure, const double* hw, const double* pos, int n_markers,
                        const int32_t* chromstarts, int n_chrom, const int32_t* dous, int n_dous, int quiet)
{
    return cnf2h_create_on(0, n_rec, par, empty, gen, has_prior, allele, sure, hw, pos, n_markers, chromstarts, n_chrom, dous,
                           n_dous, quiet);
}

cnf2h_run* cnf2h_create_on(int device, int n_rec, const int32_t* par, const uint8_t* empty, const int32_t* gen,
                           const uint8_t* has_prior, const uint8_t* allele, const double* sure, const double* hw, const double* pos,
                           int n_markers, const int32_t* chromstarts, int n_chrom, const int32_t* dous, int n_dous, int quiet)
{
    if (n_rec <= 0 || !par || !empty || !gen || !has_prior || !allele || !sure || !hw || !pos || n_markers <= 0 || !chromstarts ||
        n_chrom <= 0 || !dous || n_dous < 0) {
        g_err = "bad arguments";
        return nullptr;
    }
    cnf2h_run* run = new cnf2h_run();
    Pedigree&  P = run->P;
    P.pos.assign(pos, pos + n_markers);
    P.chromstarts.assign(chromstarts, chromstarts + n_chrom + 1);
    P.index["0"] = -1;
    const size_t M = (size_t)n_markers;
    P.inds.resize(n_rec);
#pragma omp parallel for schedule(static) num_threads(host_threads())
    for (int r = 0; r < n_rec; r++) {
        Individual& I = P.inds[r];
        I.n = r + 1;
        I.name = "r" + std::to_string(r);
        I.gen = gen[r];
        I.empty = empty[r] != 0;
        I.pars[0] = par[r * 2];
        I.pars[1] = par[r * 2 + 1];
        I.allele.assign(allele + (size_t)r * M * 2, allele + (size_t)(r + 1) * M * 2);
        I.sure.assign(sure + (size_t)r * M * 2, sure + (size_t)(r + 1) * M * 2);
        I.hw.assign(hw + (size_t)r * M, hw + (size_t)(r + 1) * M);
        I.has_prior = has_prior[r] != 0;
        if (I.has_prior) {
            I.prior_allele = I.allele;
            I.prior_sure = I.sure;
        }
    }
    for (int r = 0; r < n_rec; r++) P.index[P.inds[r].name] = r;
    P.dous.assign(dous, dous + n_dous);
    return start(run, device, quiet);
}

cnf2h_run* cnf2h_create_from_files(int device, const char* mapfile, const char* pedfile, const char* genfile, int quiet)
{
    if (!mapfile || !pedfile || !genfile) {
        g_err = "bad arguments";
        return nullptr;
    }
    cnf2h_run* run = new cnf2h_run();
    bool (*const readers[3])(FILE*, Pedigree&) = {read_alpha_map, read_alpha_ped, read_alpha_gen};
    const char* const paths[3] = {mapfile, pedfile, genfile};
    for (int k = 0; k < 3; k++) {
        FILE* f = fopen(paths[k], "rt");
        const bool ok = f && readers[k](f, run->P);
        if (f) fclose(f);
        if (!ok) {
            g_err = std::string("cannot read ") + paths[k];
            delete run;
            return nullptr;
        }
    }
    return start(run, device, quiet);
}

int cnf2h_get_dims(cnf2h_run* run, int32_t* out4)
{
    if (!run || !out4) return -2;
    out4[0] = (int32_t)run->P.inds.size();
    out4[1] = run->P.n_markers();
    out4[2] = (int32_t)run->P.chromstarts.size() - 1;
    out4[3] = (int32_t)run->P.dous.size();
    return 0;
}

void cnf2h_destroy(cnf2h_run* run)
{
    if (!run) return;
    delete run->E;
    cnf2_ctx_destroy(run->ctx);
    delete run;
}

int cnf2h_postmarkerdata(cnf2h_run* run, int indcount)
{
    if (!run) return -2;
    return guarded([&] { run->E->postmarkerdata(indcount); });
}

int cnf2h_iteration(cnf2h_run* run, const char* rows_path, int update)
{
    if (!run) return -2;
    FILE* f = fopen(rows_path ? rows_path : "/dev/null", "a");
    if (!f) {
        g_err = "cannot open rows file";
        return -2;
    }
    run->E->set_update(update != 0);
    run->E->set_print_rows(rows_path != nullptr);
    const int rc = guarded([&] { run->E->iteration(f); });
    fclose(f);
    return rc;
}

int cnf2h_dump(cnf2h_run* run, const char* path, int limit)
{
    if (!run || !path) return -2;
    FILE* f = fopen(path, "a");
    if (!f) return -2;
    const int rc = guarded([&] { run->E->dump(f, limit); });
    fclose(f);
    return rc;
}

int cnf2h_deserialize(cnf2h_run* run, const char* path)
{
    if (!run || !path) return -2;
    bool ok = false;
    const int rc = guarded([&] { ok = run->E->deserialize(path); });
    return rc ? rc : (ok ? 0 : -2);
}

int cnf2h_get_state(cnf2h_run* run, uint8_t* allele, double* sure, double* hw, int32_t* descendants, int32_t* children,
                    double* variances, double* scalefactor, int32_t* last_hits)
{
    if (!run) return -2;
    const int rc = guarded([&] { run->E->sync_rows(); });
    if (rc) return rc;
    const Pedigree& P = run->P;
    const size_t    M = P.pos.size();
    for (size_t r = 0; r < P.inds.size(); r++) {
        const Individual& I = P.inds[r];
        if (allele) std::copy(I.allele.begin(), I.allele.end(), allele + r * M * 2);
        if (sure) std::copy(I.sure.begin(), I.sure.end(), sure + r * M * 2);
        if (hw) std::copy(I.hw.begin(), I.hw.end(), hw + r * M);
        if (descendants) descendants[r] = run->E->descendants()[r];
        if (children) children[r] = run->E->children()[r];
    }
    if (variances) std::copy(run->E->variances().begin(), run->E->variances().end(), variances);
    if (scalefactor) *scalefactor = run->E->scalefactor();
    if (last_hits) *last_hits = run->E->last_hits();
    return 0;
}

int cnf2h_set_block(cnf2h_run* run, int begin, int end)
{
    if (!run) return -2;
    return guarded([&] { run->E->set_block(begin, end); });
}

int cnf2h_balanced_block(cnf2h_run* run, int rank, int world, int32_t* begin, int32_t* end)
{
    if (!run || !begin || !end) return -2;
    int b = 0, e = 0;
    const int rc = guarded([&] { run->E->balanced_block(rank, world, &b, &e); });
    *begin = b;
    *end = e;
    return rc;
}

int cnf2h_set_partition(cnf2h_run* run, int rank, int world, cnf2h_exchange_fn fn, void* user)
{
    if (!run) return -2;
    return guarded([&] { run->E->set_partition(rank, world, fn, user); });
}

int cnf2h_get_partition(cnf2h_run* run, int64_t* info10, int32_t* owned)
{
    if (!run || !info10) return -2;
    const Partition& Q = run->E->partition();
    size_t bytes[4];
    run->E->exchange_bytes(bytes);
    const bool set = !Q.bounds.empty();
    info10[0] = set ? Q.bounds[Q.rank] : 0;
    info10[1] = set ? Q.bounds[Q.rank + 1] : (int64_t)run->P.dous.size();
    info10[2] = (int64_t)Q.owned.size();
    info10[3] = (int64_t)Q.n_shared;
    info10[4] = (int64_t)Q.seg_shared;
    for (int i = 0; i < 4; i++) info10[5 + i] = (int64_t)bytes[i];
    info10[9] = set ? (int64_t)Q.private_of[Q.rank].size() : 0;
    if (owned) std::copy(Q.owned.begin(), Q.owned.end(), owned);
    return 0;
}

int cnf2h_reserve(cnf2h_run* run)
{
    if (!run) return -2;
    return guarded([&] { run->E->reserve(); });
}

int cnf2h_get_timing(cnf2h_run* run, double* out5)
{
    if (!run || !out5) return -2;
    std::copy(run->E->last_timing(), run->E->last_timing() + 5, out5);
    return 0;
}

int cnf2h_set_update_flags(cnf2h_run* run, uint32_t flags)
{
    if (!run) return -2;
    run->E->set_update_flags(flags);
    return 0;
}

int cnf2h_set_deterministic(cnf2h_run* run, int on)
{
    if (!run) return -2;
    run->E->set_deterministic(on != 0);
    return 0;
}

void* cnf2h_context(cnf2h_run* run) { return run ? run->ctx : nullptr; }

int cnf2h_get_passes(cnf2h_run* run, int32_t* hits, double* haplobase, double* haplocount)
{
    if (!run) return -2;
    if (hits) std::copy(run->E->pass_hits().begin(), run->E->pass_hits().end(), hits);
    if (haplobase || haplocount) return guarded([&] { run->E->accumulators(haplobase, haplocount); });
    return 0;
}

int cnf2h_map_mstep(const double* pos, int n_markers, const int32_t* chromstarts, int n_chrom, const double* genrec,
                    const double* xo_sum, const int32_t* n_contrib, double* new_pos)
{
    if (!pos || !chromstarts || !xo_sum || !n_contrib || !new_pos || n_markers <= 0 || n_chrom <= 0) return -2;
    if (chromstarts[0] != 0 || chromstarts[n_chrom] != n_markers) return -2;
    cnf2host::map_mstep(pos, n_markers, chromstarts, n_chrom, genrec, xo_sum, n_contrib, new_pos);
    return 0;
}

int cnf2h_write_map(const char* path, const double* pos, int n_markers, const int32_t* chromstarts, int n_chrom)
{
    if (!path || !pos || !chromstarts || n_markers <= 0 || n_chrom <= 0) return -2;
    std::string err;
    if (!cnf2host::write_map_checked(path, pos, n_markers, chromstarts, n_chrom, &err)) {
        g_err = err;
        return -3;
    }
    return 0;
}

int cnf2h_qtl_permutations(int n, int n_perm, uint64_t seed, const uint8_t* use, const int32_t* strata, int32_t* perm_out)
{
    if (n < 1 || n_perm < 0 || !perm_out) return -2;
    cnf2host::qtl_permutations(n, n_perm, seed, use, strata, perm_out);
    return 0;
}

int cnf2h_qtl2_pair(const double* gram, int n_col, const double* xty, const double* yy, int n_c, int n_cov, int additive,
                    int same_chrom, int32_t* out_rank, double* rss0_out, double* lod_add_out, double* lod_full_out)
{
    using namespace cnf2;
    if (!gram || n_col < 0 || (n_col > 0 && (!xty || !yy || !rss0_out || !lod_add_out || !lod_full_out)) || n_cov < 0 ||
        n_cov > QTL2_MAXK || !out_rank)
        return -2;
    double G[QTL2_W * QTL2_W];
    std::copy(gram, gram + QTL2_W * QTL2_W, G);
    const Qtl2Design ds = qtl2_design(n_cov, additive != 0, same_chrom != 0);
    const Qtl2Factor f  = qtl2_factor(G, QTL2_W, ds, n_c, n_cov, same_chrom != 0);
    out_rank[0] = f.usable, out_rank[1] = f.rank_add, out_rank[2] = f.rank_full;
    for (int r = 0; r < n_col; r++) {
        const Qtl2Cell c = qtl2_cell(G, QTL2_W, ds, f, xty + (size_t)r * QTL2_W, 1, yy[r], n_c, same_chrom != 0);
        rss0_out[r] = c.rss0, lod_add_out[r] = c.lod_add, lod_full_out[r] = c.lod_full;
    }
    return 0;
}

int cnf2h_qtl2_pair_linked(int n, const double* o1, const double* o2, const double* joint, const uint8_t* mask, int n_cov,
                           const double* cov, int n_col, const double* y, int additive, int32_t* out_rank, double* rss0_out,
                           double* lod_add_out, double* lod_full_out)
{
    using namespace cnf2;
    if (n < 0 || !o1 || !o2 || !joint || n_col < 0 || (n_col > 0 && (!y || !rss0_out || !lod_add_out || !lod_full_out)) || n_cov < 0 ||
        n_cov > QTL2_MAXK || (n_cov > 0 && !cov) || !out_rank)
        return -2;
    const Qtl2Design ds = qtl2_design(n_cov, additive != 0, false);
    const int        W  = ds.nx + ds.nadd + ds.nint;
    double G[QTL2_W * QTL2_W] = {};
    std::vector<double> B((size_t)n_col * QTL2_W, 0.0), yy((size_t)n_col, 0.0);
    int n_c = 0;
    for (int i = 0; i < n; i++) {
        if (mask && !mask[i]) continue;
        n_c++;
        const double *p = o1 + (size_t)i * 4, *r = o2 + (size_t)i * 4, *J = joint + (size_t)i * 16;
        const double a1 = p[3] - p[0], d1 = p[1] + p[2], a2 = r[3] - r[0], d2 = r[1] + r[2];
        double x[QTL2_W] = {};
        for (int j = 0; j < W; j++) {
            int su, sv;
            qtl2_column(ds, additive != 0, j, &su, &sv);
            if (su >= 2 && su != 4 && sv >= 1) {
                int cell[4], neg;
                qtl2_joint_cells(su == 3, sv == 2, cell, &neg);
                x[j] = qtl2_joint_value(J[cell[0]], J[cell[1]], J[cell[2]], J[cell[3]], neg);
            } else {
                const double uu = su == 0 ? 1.0 : (su == 1 ? cov[(size_t)i * n_cov + (j - 1)] : (su == 2 ? a1 : d1));
                x[j] = uu * (sv == 0 ? 1.0 : (sv == 1 ? a2 : d2));
            }
        }
        for (int j = 0; j < W; j++)
            for (int k = 0; k <= j; k++) G[j * QTL2_W + k] += x[j] * x[k];
        for (int c = 0; c < n_col; c++) {
            const double v = y[(size_t)i * n_col + c];
            for (int j = 0; j < W; j++) B[(size_t)c * QTL2_W + j] += x[j] * v;
            yy[c] += v * v;
        }
    }
    const Qtl2Factor f = qtl2_factor(G, QTL2_W, ds, n_c, n_cov, false);
    out_rank[0] = f.usable, out_rank[1] = f.rank_add, out_rank[2] = f.rank_full;
    for (int c = 0; c < n_col; c++) {
        const Qtl2Cell cl = qtl2_cell(G, QTL2_W, ds, f, B.data() + (size_t)c * QTL2_W, 1, yy[c], n_c, false);
        rss0_out[c] = cl.rss0, lod_add_out[c] = cl.lod_add, lod_full_out[c] = cl.lod_full;
    }
    return 0;
}

int cnf2h_qtlx_marker(const double* gram, int n_col, const double* xty, const double* yy, int n_c, int n_cov, int n_int,
                      int additive, int imprint, int32_t* out_rank, double* rss0_out, double* lod_out, double* coef_out)
{
    using namespace cnf2;
    if (!gram || n_col < 0 || (n_col > 0 && (!xty || !yy || !rss0_out || !lod_out || !coef_out)) || n_cov < 0 || n_int < 0 ||
        n_int > n_cov || !out_rank)
        return -2;
    const QtlxDesign ds = qtlx_design(n_cov, n_int, additive != 0, imprint != 0);
    if (ds.w > QTLX_MAXW) return -2;
    double G[QTL2_W * QTL2_W];
    std::copy(gram, gram + QTL2_W * QTL2_W, G);
    const QtlxFactor f = qtlx_factor(G, QTL2_W, ds, n_c, ds.w);
    out_rank[0] = f.usable, out_rank[1] = f.rank[0], out_rank[2] = f.rank[1], out_rank[3] = f.rank[2];
    const int ncoef = ds.w - ds.nx;
    for (int r = 0; r < n_col; r++) {
        double beta[QTL2_W];
        std::copy(xty + (size_t)r * QTL2_W, xty + (size_t)(r + 1) * QTL2_W, beta);
        const QtlxCell c = qtlx_cell(G, QTL2_W, ds, f, beta, 1, yy[r], n_c, true);
        rss0_out[r] = c.rss0;
        for (int s = 0; s < 3; s++) lod_out[(size_t)r * 3 + s] = c.lod[s];
        for (int e = 0; e < ncoef; e++) coef_out[(size_t)r * ncoef + e] = beta[ds.nx + e];
    }
    return 0;
}

// what column j of the extended scan's design is: the two codes of qtlx_column (cnf2_qtlx.h); the design's width is returned
int cnf2h_qtlx_column(int n_cov, int n_int, int additive, int imprint, int j, int32_t* effect_out, int32_t* modifier_out)
{
    using namespace cnf2;
    if (n_cov < 0 || n_int < 0 || n_int > n_cov || !effect_out || !modifier_out) return -2;
    const QtlxDesign ds = qtlx_design(n_cov, n_int, additive != 0, imprint != 0);
    int e, z;
    qtlx_column(ds, j, &e, &z);
    *effect_out = e, *modifier_out = z;
    return ds.w;
}

// one marker of the cofactor scan from its normal matrix: qtlcof_factor and qtlcof_cell (cnf2_qtlcof.h).  The columns of the
// cofactors in `skip` are made the zero columns that the kernel feeds for a cofactor left out at the marker
int cnf2h_qtlcof_marker(const double* gram, int n_col, const double* xty, const double* yy, int n_c, int n_cov, int n_cof,
                        uint32_t skip, int additive, int32_t* out_rank, double* rss0_out, double* lod_base_out, double* lod_out,
                        double* coef_out)
{
    using namespace cnf2;
    if (!gram || n_col < 0 || (n_col > 0 && (!xty || !yy || !rss0_out || !lod_base_out || !lod_out || !coef_out)) || n_cov < 0 ||
        n_cof < 0 || n_cof > QTLCOF_MAXQ || !out_rank)
        return -2;
    const QtlcofDesign ds = qtlcof_design(n_cov, n_cof, additive != 0);
    if (ds.w > QTLCOF_MAXW) return -2;
    bool zero[QTL2_W];
    for (int j = 0; j < QTL2_W; j++) {
        int e, z;
        qtlcof_column(ds, j, &e, &z);
        zero[j] = e == QTLX_NONE || (e == QTLCOF_COF && ((skip >> (z / ds.ne)) & 1u));
    }
    double G[QTL2_W * QTL2_W];
    for (int j = 0; j < QTL2_W; j++)
        for (int k = 0; k < QTL2_W; k++) G[j * QTL2_W + k] = (zero[j] || zero[k]) ? 0.0 : gram[j * QTL2_W + k];
    const QtlcofFactor f = qtlcof_factor(G, QTL2_W, ds, n_c, ds.w);
    out_rank[0] = f.usable, out_rank[1] = f.rank_cof, out_rank[2] = f.rank;
    for (int r = 0; r < n_col; r++) {
        double beta[QTL2_W];
        for (int j = 0; j < QTL2_W; j++) beta[j] = zero[j] ? 0.0 : xty[(size_t)r * QTL2_W + j];
        const QtlcofCell c = qtlcof_cell(G, QTL2_W, ds, f, beta, 1, yy[r], n_c, true);
        rss0_out[r] = c.rss0, lod_base_out[r] = c.lod_base, lod_out[r] = c.lod;
        for (int e = 0; e < ds.ne; e++) coef_out[(size_t)r * ds.ne + e] = beta[ds.nx + ds.nc + e];
    }
    return 0;
}

// one (marker, column) fit of the maximum-likelihood scan: qtlem_fit_serial (cnf2_qtlem.h)
int cnf2h_qtlem_fit(int n, const double* origin, const double* y, int n_cov, const double* cov, const uint8_t* c, int additive,
                    int imprint, int max_iter, double tol, double* lod_out, double* coef_out, double* sigma2_out,
                    int32_t* iters_out, int32_t* status_out, int32_t* rank_out, double* rss0_out, int32_t* n_used_out)
{
    if (!lod_out || !coef_out || !sigma2_out || !iters_out || !status_out || !rank_out || !rss0_out || !n_used_out) return -2;
    return cnf2::qtlem_fit_serial(n, origin, y, n_cov, cov, c, additive != 0, imprint != 0, max_iter, tol, lod_out, coef_out,
                                  sigma2_out, iters_out, status_out, rank_out, rss0_out, n_used_out)
               ? 0
               : -2;
}

// one (marker, column) fit of the binary-trait scan: qtlbin_fit_serial (cnf2_qtlbin.h)
int cnf2h_qtlbin_fit(int n, const double* origin, const double* y, int n_cov, const double* cov, const uint8_t* c, int additive,
                     int imprint, int max_iter, double tol, double* lod_out, double* coef_out, int32_t* iters_out,
                     int32_t* status_out, int32_t* rank_out, double* ll0_out, int32_t* n_ones_out, int32_t* n_used_out)
{
    if (!lod_out || !coef_out || !iters_out || !status_out || !rank_out || !ll0_out || !n_ones_out || !n_used_out) return -2;
    return cnf2::qtlbin_fit_serial(n, origin, y, n_cov, cov, c, additive != 0, imprint != 0, max_iter, tol, lod_out, coef_out,
                                   iters_out, status_out, rank_out, ll0_out, n_ones_out, n_used_out)
               ? 0
               : -2;
}

// one (marker, column) fit of the survival-trait scan: qtlsurv_fit_serial (cnf2_qtlsurv.h)
int cnf2h_qtlsurv_fit(int n, const double* origin, const double* time, const double* status, int n_cov, const double* cov,
                      const uint8_t* c, int additive, int imprint, int max_iter, double tol, double* lod_out, double* coef_out,
                      int32_t* iters_out, int32_t* status_out, int32_t* rank_out, double* ll0_out, int32_t* n_events_out,
                      int32_t* n_used_out)
{
    if (!lod_out || !coef_out || !iters_out || !status_out || !rank_out || !ll0_out || !n_events_out || !n_used_out) return -2;
    return cnf2::qtlsurv_fit_serial(n, origin, time, status, n_cov, cov, c, additive != 0, imprint != 0, max_iter, tol, lod_out,
                                    coef_out, iters_out, status_out, rank_out, ll0_out, n_events_out, n_used_out)
               ? 0
               : -2;
}

// one (marker, column) cell of the variance-QTL scan: qtlvar_fit_serial (cnf2_qtlvar.h)
int cnf2h_qtlvar_fit(int n, const double* origin, const double* y, int n_cov, const double* cov, int n_var, const uint8_t* c,
                     int additive, int imprint, int max_iter, double tol, double* lod_out, double* coef_mean_out,
                     double* coef_var_out, int32_t* iters_out, int32_t* status_out, int32_t* rank_out, double* ll0_out,
                     int32_t* n_used_out)
{
    if (!lod_out || !coef_mean_out || !coef_var_out || !iters_out || !status_out || !rank_out || !ll0_out || !n_used_out) return -2;
    return cnf2::qtlvar_fit_serial(n, origin, y, n_cov, cov, n_var, c, additive != 0, imprint != 0, max_iter, tol, lod_out,
                                   coef_mean_out, coef_var_out, iters_out, status_out, rank_out, ll0_out, n_used_out)
               ? 0
               : -2;
}

int cnf2h_qtl_null_residuals(int n, int n_traits, const double* pheno, int n_cov, const double* cov, const uint8_t* use,
                             double* res_out)
{
    if (n < 1 || n_traits < 1 || !pheno || n_cov < 0 || n_cov > 8 || (n_cov > 0 && !cov) || !use || !res_out) return -2;
    if (!cnf2host::qtl_null_residuals(n, n_traits, pheno, n_cov, cov, use, res_out)) {
        g_err = "the null design [1, cov] of the used individuals has no full rank";
        return -2;
    }
    return 0;
}

// cnf2_kinship_sums on the CPU: the same sums, the markers in ascending order, the lower triangle mirrored
int cnf2h_kinship_sums(int n, int n_markers, const double* origin, const int32_t* chromstarts, int n_chrom, int chrom_begin,
                       int chrom_end, double* sum_out, int32_t* n_markers_out)
{
    if (n < 1 || n_markers < 1 || !origin || !chromstarts || n_chrom < 1 || chrom_begin < 0 || chrom_end > n_chrom ||
        chrom_begin >= chrom_end || !sum_out || !n_markers_out || chromstarts[0] != 0 || chromstarts[n_chrom] != n_markers)
        return -2;
    const int m_lo = chromstarts[chrom_begin], m_hi = chromstarts[chrom_end];
    if (m_lo < 0 || m_hi > n_markers || m_lo >= m_hi) return -2;
    auto a = [&](int i, int m) { return origin[((size_t)i * n_markers + m) * 4 + 3] - origin[((size_t)i * n_markers + m) * 4]; };
#pragma omp parallel for schedule(dynamic)
    for (int i = 0; i < n; i++)
        for (int j = 0; j <= i; j++) {
            double s = 0.0;
            for (int m = m_lo; m < m_hi; m++) s += a(i, m) * a(j, m);
            sum_out[(size_t)i * n + j] = sum_out[(size_t)j * n + i] = s;
        }
    *n_markers_out = m_hi - m_lo;
    return 0;
}

// one marker of cnf2_qtl_scan_cols: the sums in the kernels' order, then qtl_marker_record and qtl_cell (cnf2_qtl.h)
int cnf2h_qtl_cols_marker(int n, int ne, const double* reg, const double* scale, int nx, const double* x0, int n_col,
                          const double* y, double* lod_out, double* coef_out, int32_t* rank_out, double* rss0_out)
{
    using namespace cnf2;
    if (n < 1 || ne < 1 || ne > 2 || !reg || nx < 1 || nx > QTL_NX || !x0 || n_col < 0 || (n_col > 0 && (!y || !lod_out || !coef_out || !rss0_out)) ||
        !rank_out)
        return -2;
    double S[QTL_NX * QTL_NX] = {0.0};
    for (int j = 0; j < nx; j++)
        for (int k = 0; k <= j; k++) {
            double s = 0.0;
            for (int i = 0; i < n; i++) s += x0[(size_t)i * nx + j] * x0[(size_t)i * nx + k];
            S[j * QTL_NX + k] = s;
        }
    const bool usable = qtl_cholesky(S, nx) && n >= nx + 3;
    double     sa[QTL_NX] = {0.0}, sd[QTL_NX] = {0.0}, saa = 0.0, sad = 0.0, sdd = 0.0;
    auto       ra = [&](int i) { return (scale ? scale[i] : 1.0) * reg[(size_t)i * ne]; };
    auto       rd = [&](int i) { return ne == 2 ? (scale ? scale[i] : 1.0) * reg[(size_t)i * ne + 1] : 0.0; };
    for (int i = 0; i < n; i++) {
        const double a = ra(i), d = rd(i);
        for (int k = 0; k < nx; k++) {
            sa[k] += a * x0[(size_t)i * nx + k];
            sd[k] += d * x0[(size_t)i * nx + k];
        }
        saa += a * a, sad += a * d, sdd += d * d;
    }
    double rec[QTL_MK];
    *rank_out = qtl_marker_record(S, nx, usable, sa, sd, saa, sad, sdd, ne == 1, rec);
    for (int r = 0; r < n_col; r++) {
        double b[QTL_NX] = {0.0}, z[QTL_NX], yy = 0.0, va = 0.0, vd = 0.0;
        for (int i = 0; i < n; i++) {
            const double v = y[(size_t)i * n_col + r];
            for (int k = 0; k < nx; k++) b[k] += x0[(size_t)i * nx + k] * v;
            yy += v * v;
            va += ra(i) * v;
            vd += rd(i) * v;
        }
        double rss0 = 0.0;
        if (usable) {
            for (int k = 0; k < QTL_NX; k++) z[k] = b[k];
            qtl_chol_solve(S, nx, z);
            double e = 0.0;
            for (int k = 0; k < nx; k++) e += b[k] * z[k];
            rss0 = yy - e;
        }
        for (int k = 0; k < nx; k++) {
            va -= rec[k] * b[k];
            vd -= rec[QTL_NX + k] * b[k];
        }
        const QtlCell c = qtl_cell(va, vd, rec[QTL_PA], rec[QTL_L], rec[QTL_PD], rss0, n, usable);
        rss0_out[r] = rss0, lod_out[r] = c.lod, coef_out[2 * r] = c.ca, coef_out[2 * r + 1] = c.cd;
    }
    return 0;
}

int cnf2h_qtl_bootstrap_counts(int n, int n_boot, uint64_t seed, const uint8_t* use, const int32_t* strata, int32_t* count_out)
{
    if (n < 1 || n_boot < 0 || !count_out) return -2;
    cnf2host::qtl_bootstrap_counts(n, n_boot, seed, use, strata, count_out);
    return 0;
}

// one (replicate, marker) cell of cnf2_qtl_scan_boot: qtlboot_marker_serial (cnf2_qtlboot.h)
int cnf2h_qtl_boot_marker(int n, const double* origin, int n_traits, const double* y, int n_cov, const double* cov, const uint8_t* c,
                          const int32_t* count, int additive, double* lod_out, double* coef_out, int32_t* rank_out,
                          double* rss0_out, int32_t* n_bc_out)
{
    if (n < 1 || !origin || n_traits < 1 || !y || n_cov < 0 || n_cov > cnf2::QTL_MAXK || (n_cov > 0 && !cov) || !c || !count ||
        !lod_out || !coef_out || !rank_out || !rss0_out || !n_bc_out)
        return -2;
    return cnf2::qtlboot_marker_serial(n, origin, n_traits, y, n_cov, cov, c, count, additive != 0, lod_out, coef_out, rank_out,
                                       rss0_out, n_bc_out)
               ? 0
               : -2;
}

// one marker's combined cells of cnf2_qtl_scan_imp: qtlimp_marker_serial (cnf2_qtlimp.h)
int cnf2h_qtlimp_marker(int n, int n_draws, const uint8_t* state, int n_traits, const double* y, int n_cov, const double* cov,
                        const uint8_t* c, int additive, double* lod_out, double* coef_out, int32_t* rank_out, double* rss0_out,
                        int32_t* n_used_out, double* draw_lod_out)
{
    if (n < 1 || !state || n_traits < 1 || !y || n_cov < 0 || n_cov > cnf2::QTL_MAXK || (n_cov > 0 && !cov) || !c || !lod_out ||
        !coef_out || !rank_out || !rss0_out || !n_used_out)
        return -2;
    return cnf2::qtlimp_marker_serial(n, n_draws, state, n_traits, y, n_cov, cov, c, additive != 0, lod_out, coef_out, rank_out,
                                      rss0_out, n_used_out, draw_lod_out)
               ? 0
               : -2;
}

// the scans' marker map and column tile: qtl_marker_map and qtl_column_tile (cnf2_qtlplan.h)
int64_t cnf2h_qtl_marker_map(const int32_t* chromstarts, int n_chrom, int chrom_begin, int chrom_end, int tile, int with_mchrom,
                             int whole_map_header, int32_t* image_out, int64_t cap, int64_t* offsets_out)
{
    if (!chromstarts || n_chrom < 1 || chrom_begin < 0 || chrom_end > n_chrom || chrom_begin > chrom_end || tile < 1 || !offsets_out)
        return -2;
    for (int c = 0; c < n_chrom; c++)
        if (chromstarts[c] > chromstarts[c + 1]) return -2;
    const cnf2::QtlMarkerMap m = cnf2::qtl_marker_map(chromstarts, n_chrom, chrom_begin, chrom_end, tile, with_mchrom != 0, whole_map_header != 0);
    offsets_out[0] = (int64_t)m.o_mchrom, offsets_out[1] = (int64_t)m.o_tiles, offsets_out[2] = (int64_t)m.o_tstart;
    offsets_out[3] = (int64_t)m.n_tiles;
    if (image_out && cap >= (int64_t)m.image.size()) std::copy(m.image.begin(), m.image.end(), image_out);
    return (int64_t)m.image.size();
}

int64_t cnf2h_qtl_column_tile(int64_t n, int64_t R, int64_t P, int64_t maxima_doubles_per_column, int cap)
{
    if (n < 0 || R < 0 || P < 0 || maxima_doubles_per_column < 0 || cap < 0) return -2;
    return (int64_t)cnf2::qtl_column_tile((size_t)n, (size_t)R, (size_t)P, (size_t)maxima_doubles_per_column, cap);
}

// one (marker, group) cell of cnf2_qtl_scan_mv: qtlmv_marker_serial (cnf2_qtlmv.h)
int cnf2h_qtlmv_marker(int n, const double* origin, int n_traits, const double* y, int n_cov, const double* cov, const uint8_t* c,
                       int additive, double* lod_out, int32_t* rank_out, int32_t* trait_rank_out, int32_t* n_used_out)
{
    if (n < 1 || !origin || !y || (n_cov > 0 && !cov) || !c || !lod_out || !rank_out || !trait_rank_out || !n_used_out) return -2;
    return cnf2::qtlmv_marker_serial(n, origin, n_traits, y, n_cov, cov, c, additive != 0, lod_out, rank_out, trait_rank_out, n_used_out)
               ? 0
               : -2;
}

// the multi-trait scan's group tile: qtl_group_tile (cnf2_qtlplan.h)
int64_t cnf2h_qtl_group_tile(int64_t n, int64_t T, int64_t G, int64_t P, int64_t n_tiles, int cap)
{
    if (n < 0 || T < 1 || T > cnf2::QTLMV_MAXT || G < 1 || P < 0 || n_tiles < 0 || cap < 0) return -2;
    return (int64_t)cnf2::qtl_group_tile((size_t)n, (size_t)T, (size_t)G, (size_t)P, (size_t)n_tiles, cap);
}

// one marker of cnf2_qtl_scan_fam: qtlfam_marker_serial (cnf2_qtlfam.h)
int cnf2h_qtlfam_marker(int n, const double* origin, int side, const int32_t* grp, const int32_t* cell, int n_fam, int n_traits,
                        const double* y, int n_cov, const double* cov, const uint8_t* c, double* lod_out, int32_t* df_out,
                        double* slope_out, double* rss0_out, int32_t* n_used_out, int32_t* n_cells_out)
{
    if (n < 1 || !origin || !grp || n_traits < 1 || !y || n_cov < 0 || n_cov > cnf2::QTL_MAXK || (n_cov > 0 && !cov) || !c || !lod_out ||
        !df_out || !rss0_out || !n_used_out || !n_cells_out)
        return -2;
    return cnf2::qtlfam_marker_serial(n, origin, side, grp, cell, n_fam, n_traits, y, n_cov, cov, c, lod_out, df_out, slope_out,
                                      rss0_out, n_used_out, n_cells_out)
               ? 0
               : -2;
}

// grp / cell of the analysed individuals from the pedigree's parents: the parent on the side and the pair of parents, both
// numbered in ascending order of the records; -1 where the parent on the side is missing or has no recorded parents
int cnf2h_qtl_families(int n_rec, const int32_t* par, int n, const int32_t* dous, int side, int32_t* grp_out, int32_t* cell_out,
                       int32_t* n_fam_out)
{
    if (n_rec < 1 || !par || n < 1 || !dous || side < 0 || side > 1 || !grp_out || !cell_out || !n_fam_out) return -2;
    for (int r = 0; r < n_rec; r++)
        for (int s = 0; s < 2; s++)
            if (par[2 * r + s] >= n_rec) return -2;
    for (int i = 0; i < n; i++)
        if (dous[i] < 0 || dous[i] >= n_rec) return -2;
    *n_fam_out = cnf2host::qtl_families(par, n, dous, side, grp_out, cell_out);
    return 0;
}

// one marker of cnf2_qtl_scan_hap: qtlhap_marker_serial (cnf2_qtlhap.h)
int cnf2h_qtlhap_marker(int n, const double* descent, const int32_t* col, int n_columns, int n_traits, const double* y, int n_cov,
                        const double* cov, const uint8_t* c, double* lod_out, int32_t* df_out, double* coef_out, double* rss0_out,
                        int32_t* n_used_out)
{
    if (n < 1 || !descent || !col || n_traits < 1 || !y || n_cov < 0 || n_cov > cnf2::QTL_MAXK || (n_cov > 0 && !cov) || !c || !lod_out ||
        !df_out || !rss0_out || !n_used_out)
        return -2;
    return cnf2::qtlhap_marker_serial(n, descent, col, n_columns, n_traits, y, n_cov, cov, c, lod_out, df_out, coef_out, rss0_out,
                                      n_used_out)
               ? 0
               : -2;
}

// one marker of cnf2_qtl_scan_vc: qtlvc_marker_serial (cnf2_qtlvc.h)
int cnf2h_qtlvc_marker(int n, const double* descent, const int32_t* col, int n_columns, int n_traits, const double* y, int n_cov,
                       const double* cov, const uint8_t* c, double* lod_out, double* h_out, double* sigma2_out, double* blup_out,
                       double* eval_out, int32_t* rank_out, double* rss0_out, int32_t* n_used_out)
{
    if (n < 1 || !descent || !col || n_traits < 1 || !y || n_cov < 0 || n_cov > cnf2::QTL_MAXK || (n_cov > 0 && !cov) || !c || !lod_out ||
        !h_out || !sigma2_out || !rank_out || !rss0_out || !n_used_out)
        return -2;
    return cnf2::qtlvc_marker_serial(n, descent, col, n_columns, n_traits, y, n_cov, cov, c, lod_out, h_out, sigma2_out, blup_out,
                                     eval_out, rank_out, rss0_out, n_used_out)
               ? 0
               : -2;
}

// col[n][8] of the descent rows from the pedigree's parents: descent_columns (cnf2_qtl_host.h)
int cnf2h_descent_columns(int n_rec, const int32_t* par, int n, const int32_t* dous, int by, int32_t* col_out, int32_t* n_grand_out)
{
    if (n_rec < 1 || !par || n < 1 || !dous || by < 0 || by > 2 || !col_out || !n_grand_out) return -2;
    for (int r = 0; r < n_rec; r++)
        for (int s = 0; s < 2; s++)
            if (par[2 * r + s] >= n_rec) return -2;
    for (int i = 0; i < n; i++)
        if (dous[i] < 0 || dous[i] >= n_rec) return -2;
    *n_grand_out = cnf2host::descent_columns(par, n, dous, by, col_out);
    return 0;
}

}  // extern "C"
