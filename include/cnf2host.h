/*
 * cnf2host.h -- C ABI of libcnf2host.so: the host side of a cnF2freq run above libcnf2hip.so (readers' data model,
 * postmarkerdata, the haplotyping iteration with its device-side updates, dump / deserialize), i.e. what main() and
 * doit<> do around the sweep (cnF2freq.cpp:8083-8192, 5189-6410, 3190-3412), driven from arrays instead of files.
 * The `cnF2freq` executable links the same code; this entry exists for callers that already hold the pedigree in
 * memory, for multi-process drivers (one run per GPU, cnf2h_set_block / cnf2h_set_exchange) and for the parity tests.
 * One run owns one cnf2_ctx.  int status: 0 ok, < 0 error (the codes of cnf2hip.h; text in cnf2h_last_error()): a failure
 * below the ABI (out of memory, a launch error) comes back as a status, it does not end the process.
 */
#ifndef CNF2HOST_H
#define CNF2HOST_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct cnf2h_run cnf2h_run;

/* Individuals are records 0..n_rec-1 (the reference's number n = record + 1, order of first mention,
 * cnF2freq.cpp:6480-6491).  par[n_rec][2] record or -1; allele[n_rec][M][2], sure[n_rec][M][2], hw[n_rec][M] as
 * readalphadata leaves them (they are also the priors of the records with has_prior set, cnF2freq.cpp:6664-6665);
 * dous[n_dous] the analysed records in output order. */
cnf2h_run *cnf2h_create(int n_rec, const int32_t *par, const uint8_t *empty, const int32_t *gen, const uint8_t *has_prior,
                        const uint8_t *allele, const double *sure, const double *hw, const double *pos, int n_markers,
                        const int32_t *chromstarts, int n_chrom, const int32_t *dous, int n_dous, int quiet);
/* the same on HIP device `device` (one process per GPU: its local rank) */
cnf2h_run *cnf2h_create_on(int device, int n_rec, const int32_t *par, const uint8_t *empty, const int32_t *gen,
                           const uint8_t *has_prior, const uint8_t *allele, const double *sure, const double *hw, const double *pos,
                           int n_markers, const int32_t *chromstarts, int n_chrom, const int32_t *dous, int n_dous, int quiet);
/* the same from PlantImpute-format files, through the readers of the `cnF2freq` executable (map, pedigree, genotypes with
 * read-count tokens): the run's state is the executable's after reading, before postmarkerdata.  NULL (text in
 * cnf2h_last_error) where a file cannot be read.  cnf2h_get_dims: out4 = records, markers, chromosomes, analysed individuals */
cnf2h_run *cnf2h_create_from_files(int device, const char *mapfile, const char *pedfile, const char *genfile, int quiet);
int        cnf2h_get_dims(cnf2h_run *run, int32_t *out4);
void       cnf2h_destroy(cnf2h_run *run);
const char *cnf2h_last_error(void);

/* postmarkerdata(indcount) as main() calls it (cnF2freq.cpp:8083-8085) */
int cnf2h_postmarkerdata(cnf2h_run *run, int indcount);
/* one doit<false, genotypereporter> (cnF2freq.cpp:8132): rows and pass lines appended to rows_path (NULL: not formatted at all);
 * update = 0 sweeps without the parameter updates */
int cnf2h_iteration(cnf2h_run *run, const char *rows_path, int update);
/* allocates the device buffers of the iterations now (the batch buffer of the accumulate sweep is up to half of the free
 * memory: a first hipMalloc of that size takes seconds) instead of inside the first iteration; optional */
int cnf2h_reserve(cnf2h_run *run);
/* wall time of the last cnf2h_iteration by where it went, seconds: out5[0] sweep + accumulators, [1] exchanges (multi-process),
 * [2] update passes, [3] the rest on the host (bookkeeping, likelihood lines, rows), [4] total */
int cnf2h_get_timing(cnf2h_run *run, double *out5);
/* Multi-process runs (the reference's dead MPI code: partition cnF2freq.cpp:5297-5299, reduce
 * 6245-6254, updates on the reduced values 6344-6392).  Every rank holds the whole pedigree (ancestors' rows replicated)
 * and runs the same postmarkerdata.  cnf2h_set_partition(rank, world, transport) plans the run -- the same plan on every
 * rank, a pure function of the pedigree:
 *   blocks    contiguous blocks of the analysed individuals (positions in dous) balanced by what the sweep kernels spend
 *             on an individual (markers x (1 + tie combinations)), their boundaries moved by up to a quarter of a block to
 *             where the fewest records are touched from both sides: families that fit in a block stay whole;
 *   records   a record only one rank's windows touch is PRIVATE to that rank; a record several ranks touch is SHARED and
 *             owned by one of them (the one with the fewest so far);
 * and sets this rank's block.  An iteration then is: sweep + accumulators of the block; the accumulators of the SHARED
 * records, packed by owner, summed by one reduce-scatter (nothing at all when no family straddles a boundary); per
 * chromosome the update pass of the records the rank owns and one sum of the hit counters (the step-size control,
 * cnF2freq.cpp:6373-6392, stays identical on all ranks); the new rows of the shared records from their owners to
 * everybody by one all-gather.  The rows of private records stay on their rank until the whole state is asked for
 * (cnf2h_get_state, cnf2h_dump, cnf2h_postmarkerdata, cnf2h_deserialize: collectives then -- call them on every rank).
 * Rows are printed for the rank's block.
 *
 * The transport carries the collectives; the engine does all packing on the device.  op:
 *   CNF2H_X_SUM_SEGMENTS     buf = DEVICE pointer, `count` doubles in `world` segments of `seg`: on return segment `rank`
 *                            holds the sum over all ranks of that segment (a reduce-scatter; other segments undefined)
 *   CNF2H_X_SUM_HITS         buf = HOST int32[count]: in-place sum over all ranks
 *   CNF2H_X_GATHER_SEGMENTS  buf = DEVICE pointer, `count` BYTES in `world` segments of `seg`: every rank has filled its
 *                            own segment; on return all segments are filled on every rank (an all-gather)
 *   CNF2H_X_BARRIER          nothing to move: returns when every rank has called it (used by the `cnF2freq --gpus N`
 *                            executable, whose ranks spool their rows to files for rank 0; runs through this C ABI never
 *                            receive it)
 *   CNF2H_X_BCAST_HOST       buf = HOST pointer, `count` bytes: on return every rank holds rank 0's bytes (cnf2h_postmarkerdata
 *                            of a run whose partition is set: rank 0 does the genotype inference for all and broadcasts
 *                            the rows, descendant counts and lock positions it leaves)
 * 0 = ok.  cnf2freq_amd/dist.py holds the torch.distributed transport (RCCL on the device buffer in place; gloo staged
 * through the host); csrc/host/cnf2_shm_transport.h the one of the executable (forked ranks, staged through shared memory). */
enum { CNF2H_X_SUM_SEGMENTS = 0, CNF2H_X_SUM_HITS = 1, CNF2H_X_GATHER_SEGMENTS = 2, CNF2H_X_BARRIER = 3, CNF2H_X_BCAST_HOST = 4 };
typedef int (*cnf2h_exchange_fn)(void *user, int op, void *buf, size_t count, size_t seg);
int cnf2h_set_partition(cnf2h_run *run, int rank, int world, cnf2h_exchange_fn fn, void *user);
/* the plan in numbers: info[0..1] this rank's block [begin, end); [2] records the rank owns; [3] shared records in all;
 * [4] shared records per segment (the largest owner's); bytes per iteration of [5] the reduce-scatter buffer, [6] the
 * all-gather buffer, [7] the hit counters; [8] the payload (what the shared records occupy in them); [9] private records of
 * the rank.  owned (optional) receives the records the rank owns, ascending (info[2] entries). */
int cnf2h_get_partition(cnf2h_run *run, int64_t *info10, int32_t *owned);
/* a sub-range [begin, end) of the analysed individuals for this process's sweeps and rows (single-process use) */
int cnf2h_set_block(cnf2h_run *run, int begin, int end);
/* block `rank` of `world` as cnf2h_set_partition would cut it; does not set it */
int cnf2h_balanced_block(cnf2h_run *run, int rank, int world, int32_t *begin, int32_t *end);
/* form of the update passes: 0 = fast kernels, one certainty flow per side and its mirror image (within rounding of the
 * reference's form), or CNF2_UPDATE_BOTH_FLOWS (fast kernels, bit-exact form), CNF2_UPDATE_PLAIN (literal kernels),
 * CNF2_UPDATE_ONE_SCOUT of cnf2hip.h.  Until this is called a run uses 0, or CNF2_UPDATE_BOTH_FLOWS once
 * cnf2h_set_deterministic is on.  Nothing in the libraries reads the environment for this. */
int cnf2h_set_update_flags(cnf2h_run *run, uint32_t flags);
/* accumulators added in a fixed order (CNF2_DETERMINISTIC of cnf2hip.h) and the update passes in their bit-exact form
 * (CNF2_UPDATE_BOTH_FLOWS): iterations reproduce to the bit */
int cnf2h_set_deterministic(cnf2h_run *run, int on);
/* the cnf2_ctx of the run (for callers that move the accumulators themselves: cnf2_download_accumulators, ...) */
void *cnf2h_context(cnf2h_run *run);
/* after an iteration: hitnnn of every chromosome's update pass (hits[n_chrom]) and haplobase / haplocount [n_rec][M] as
 * the last pass left them; any pointer may be NULL */
int cnf2h_get_passes(cnf2h_run *run, int32_t *hits, double *haplobase, double *haplocount);
/* the dump of cnF2freq.cpp:8157-8192 to a file (append), and deserialize (cnF2freq.cpp:7757-7832) from one */
int cnf2h_dump(cnf2h_run *run, const char *path, int limit);
int cnf2h_deserialize(cnf2h_run *run, const char *path);
/* current state: allele[n_rec][M][2], sure[n_rec][M][2], hw[n_rec][M], descendants / children[n_rec],
 * variances[n_rec][M]; any pointer may be NULL */
int cnf2h_get_state(cnf2h_run *run, uint8_t *allele, double *sure, double *hw, int32_t *descendants, int32_t *children,
                    double *variances, double *scalefactor, int32_t *last_hits);

/* Map M-step from summed crossover posteriors (cnf2_sweep_crossovers of cnf2hip.h: xo_sum[n_markers][6],
 * n_contrib[n_chrom]).  For every interval m -> m+1 with pos[m+1] - pos[m] > 0 and a contributing individual, the length d
 * that maximises sum_t S_t log r_t(d) + (C - S_t) log(1 - r_t(d)), r_t(d) = 0.5 (1 - exp(genrec[TYPEGENS[t]] d)),
 * TYPEGENS = {1,0,0,1,0,0}: closed form r = sum S / 6C when genrec[0] == genrec[1], a safeguarded Newton iteration
 * otherwise.  r is clamped to [1e-9, 0.499] (an interval neither closes -- a zero-length gap is frozen -- nor opens to
 * infinity).  Other intervals keep their length; new_pos[n_markers] starts every chromosome at its old first position.
 * genrec NULL = {-0.02, -0.02, -0.02}.  With the summed window log-likelihood of the sweep this is an exact EM step. */
int cnf2h_map_mstep(const double *pos, int n_markers, const int32_t *chromstarts, int n_chrom, const double *genrec,
                    const double *xo_sum, const int32_t *n_contrib, double *new_pos);
/* the map in the .map format the readers parse (one position per line), read back and compared: -3 (text in
 * cnf2h_last_error) when it does not give the same positions and chromstarts, e.g. a chromosome grown past the next one's
 * first position (a new chromosome starts where a value decreases) */
int cnf2h_write_map(const char *path, const double *pos, int n_markers, const int32_t *chromstarts, int n_chrom);

/* The host side of a QTL permutation test (cnf2_qtl_scan of cnf2hip.h scans; `cnF2freq --qtl` uses these):
 *  cnf2h_qtl_permutations    perm_out[n_perm][n] (int32): permutation p gives individual i the phenotype of perm[p][i].  Within
 *                            every stratum (strata[n], NULL = one) the used individuals (use[n], NULL = all), in ascending
 *                            order idx[0..k), are ordered by the key splitmix64(seed, p n + i) with a stable sort:
 *                            perm[p][idx[j]] = idx[order[j]]; unused individuals map to themselves.  No sequential generator
 *                            enters: cnf2freq_amd/qtl.py's permutations() gives the same arrays
 *  cnf2h_qtl_null_residuals  res_out[n][n_traits]: the residuals of every phenotype column on [1, cov] over the used
 *                            individuals, 0 for the others: with covariates a permutation test permutes these
 *                            (Freedman-Lane), not the raw values */
int cnf2h_qtl_permutations(int n, int n_perm, uint64_t seed, const uint8_t *use, const int32_t *strata, int32_t *perm_out);
int cnf2h_qtl_null_residuals(int n, int n_traits, const double *pheno, int n_cov, const double *cov, const uint8_t *use,
                             double *res_out);

/* The small algebra of the pair scan (cnf2_qtl_scan2 of cnf2hip.h; cnf2freq_amd/csrc/cnf2_qtl2.h) on the host, as its tests
 * use it: gram[16][16] is the normal matrix of one pair's design in the model's column order (zero past its width; only the
 * lower triangle is read), xty[n_col][16] and yy[n_col] the columns' X'y and sum c y^2.  Factors once with the rank rule,
 * then per column the cell: out_rank[3] = usable, rank_add, rank_full; rss0_out, lod_add_out, lod_full_out [n_col]. */
int cnf2h_qtl2_pair(const double *gram, int n_col, const double *xty, const double *yy, int n_c, int n_cov, int additive,
                    int same_chrom, int32_t *out_rank, double *rss0_out, double *lod_add_out, double *lod_full_out);
/* One pair of loci on one chromosome as cnf2_qtl_scan2_linked fits it, on the host: o1, o2 [n][4] the origin rows at the two
 * loci, joint [n][16] the pair's rows of cnf2_sweep_pairs, mask [n] (uint8; NULL = everyone) the individuals of the
 * chromosome's mask, cov [n][n_cov], y [n][n_col] the phenotype columns.  Forms the full design -- the interaction columns
 * from the joint (cnf2_qtl2.h) --, its normal matrix, X'y and sum y^2 over the masked individuals in ascending order, factors
 * once with the rank rule, then per column the cell: outputs as cnf2h_qtl2_pair's. */
int cnf2h_qtl2_pair_linked(int n, const double *o1, const double *o2, const double *joint, const uint8_t *mask, int n_cov,
                           const double *cov, int n_col, const double *y, int additive, int32_t *out_rank, double *rss0_out,
                           double *lod_add_out, double *lod_full_out);

/* The small algebra of the extended single-locus scan (cnf2_qtl_scanx of cnf2hip.h; cnf2freq_amd/csrc/cnf2_qtlx.h) on the
 * host, as its tests use it: gram[16][16] is the normal matrix of one marker's design in the model's column order (zero past
 * its width; only the lower triangle is read), xty[n_col][16] and yy[n_col] the columns' X'y and sum c y^2.  Factors once
 * with the rank rule, then per column the cell: out_rank[4] = usable, rank[0 .. 2]; rss0_out [n_col], lod_out [n_col][3],
 * coef_out [n_col][ne (1 + n_int)].  -2: a bad argument or a design wider than 15 columns.
 * cnf2h_qtlx_column: the effect code (0 = 1, 1 = a, 2 = d, 3 = i, 4 = none) and the modifier (0 = 1, k = covariate k - 1) of
 * design column j; returns the design's width W (or -2). */
int cnf2h_qtlx_marker(const double *gram, int n_col, const double *xty, const double *yy, int n_c, int n_cov, int n_int,
                      int additive, int imprint, int32_t *out_rank, double *rss0_out, double *lod_out, double *coef_out);
int cnf2h_qtlx_column(int n_cov, int n_int, int additive, int imprint, int j, int32_t *effect_out, int32_t *modifier_out);

/* The small algebra of the cofactor scan (cnf2_qtl_scan_cof of cnf2hip.h; cnf2freq_amd/csrc/cnf2_qtlcof.h) on the host, as
 * its tests use it: gram[16][16] is the normal matrix of one marker's design with ALL n_cof cofactors in the model's column
 * order -- X0, the cofactors' a, d in the order of cof, the marker's a, d (zero past its width; only the lower triangle is
 * read) --, xty[n_col][16] and yy[n_col] the columns' X'y and sum c y^2.  Bit q of `skip` leaves cofactor q out: its columns
 * become the zero columns the kernel feeds there.  Factors once with the rank rule, then per column the cell: out_rank[3] =
 * usable, rank_cof, rank; rss0_out, lod_base_out, lod_out [n_col], coef_out [n_col][ne].  -2: a bad argument or a design
 * wider than 15 columns. */
int cnf2h_qtlcof_marker(const double *gram, int n_col, const double *xty, const double *yy, int n_c, int n_cov, int n_cof,
                        uint32_t skip, int additive, int32_t *out_rank, double *rss0_out, double *lod_base_out,
                        double *lod_out, double *coef_out);

/* One (marker, phenotype column) fit of the maximum-likelihood scan (cnf2_qtl_scan_em of cnf2hip.h) on the host, by the
 * functions of cnf2freq_amd/csrc/cnf2_qtlem.h that the kernels use, the individuals in ascending order: origin[n][4] the
 * marker's rows, y[n], cov[n][n_cov], c[n] the chromosome's mask.  lod_out, coef_out [ne], sigma2_out, iters_out, status_out,
 * rank_out, rss0_out and n_used_out receive one cell.  -2: a bad argument (n_cov above 8, max_iter outside 1 .. 10 000, a
 * tol that is not finite). */
int cnf2h_qtlem_fit(int n, const double *origin, const double *y, int n_cov, const double *cov, const uint8_t *c,
                    int additive, int imprint, int max_iter, double tol, double *lod_out, double *coef_out,
                    double *sigma2_out, int32_t *iters_out, int32_t *status_out, int32_t *rank_out, double *rss0_out,
                    int32_t *n_used_out);

/* One (marker, phenotype column) fit of the binary-trait scan (cnf2_qtl_scan_binary of cnf2hip.h) on the host, by the
 * functions of cnf2freq_amd/csrc/cnf2_qtlbin.h that the kernels use, the individuals in ascending order: origin[n][4] the
 * marker's rows, y[n] (0 or 1 where c is set), cov[n][n_cov], c[n] the chromosome's mask.  lod_out, coef_out [ne], iters_out,
 * status_out, rank_out, ll0_out, n_ones_out and n_used_out receive one cell.  -2: a bad argument (n_cov above 8, max_iter
 * outside 1 .. 1000, a tol that is not finite, a y under the mask that is neither 0 nor 1). */
int cnf2h_qtlbin_fit(int n, const double *origin, const double *y, int n_cov, const double *cov, const uint8_t *c,
                     int additive, int imprint, int max_iter, double tol, double *lod_out, double *coef_out,
                     int32_t *iters_out, int32_t *status_out, int32_t *rank_out, double *ll0_out, int32_t *n_ones_out,
                     int32_t *n_used_out);

/* One (marker, column) fit of the survival-trait scan (cnf2_qtl_scan_surv of cnf2hip.h) on the host, by the functions of
 * cnf2freq_amd/csrc/cnf2_qtlsurv.h that the kernels use, the running sums in the plain order of the risk order: origin[n][4]
 * the marker's rows, time[n] (finite) and status[n] (0 or 1) where c is set, cov[n][n_cov], c[n] the chromosome's mask.
 * lod_out, coef_out [ne], iters_out, status_out, rank_out, ll0_out, n_events_out and n_used_out receive one cell.  -2: a bad
 * argument (n_cov above 8, max_iter outside 1 .. 1000, a tol that is not finite, under the mask a status that is neither 0
 * nor 1 or a time that is not finite). */
int cnf2h_qtlsurv_fit(int n, const double *origin, const double *time, const double *status, int n_cov, const double *cov,
                      const uint8_t *c, int additive, int imprint, int max_iter, double tol, double *lod_out,
                      double *coef_out, int32_t *iters_out, int32_t *status_out, int32_t *rank_out, double *ll0_out,
                      int32_t *n_events_out, int32_t *n_used_out);

/* One (marker, phenotype column) cell of the variance-QTL scan (cnf2_qtl_scan_var of cnf2hip.h) on the host, by the functions
 * of cnf2freq_amd/csrc/cnf2_qtlvar.h that the kernels use, the individuals in ascending order and one pass per step:
 * origin[n][4] the marker's rows, y[n], cov[n][n_cov] of which the first n_var enter the variance design, c[n] the
 * chromosome's mask.  lod_out [3], coef_mean_out and coef_var_out [ne], iters_out and status_out [3], rank_out, ll0_out and
 * n_used_out receive one cell.  -2: a bad argument (n_cov above 8, n_var outside 0 .. min(n_cov, 3), max_iter outside
 * 1 .. 1000, a tol that is not finite). */
int cnf2h_qtlvar_fit(int n, const double *origin, const double *y, int n_cov, const double *cov, int n_var, const uint8_t *c,
                     int additive, int imprint, int max_iter, double tol, double *lod_out, double *coef_mean_out,
                     double *coef_var_out, int32_t *iters_out, int32_t *status_out, int32_t *rank_out, double *ll0_out,
                     int32_t *n_used_out);

/* cnf2_kinship_sums (cnf2hip.h) on the CPU, for tests and for callers without a GPU: sum_out[n][n] = sum over the markers of
 * the chromosomes chrom_begin .. chrom_end-1 of a_i(m) a_j(m), a = origin[3] - origin[0], on origin[n][n_markers][4] and the
 * map's chromstarts[n_chrom + 1]; *n_markers_out the number of those markers.  The markers are added in ascending order
 * and the lower triangle is mirrored.  -2: a bad argument. */
int cnf2h_kinship_sums(int n, int n_markers, const double *origin, const int32_t *chromstarts, int n_chrom, int chrom_begin,
                       int chrom_end, double *sum_out, int32_t *n_markers_out);

/* One marker of cnf2_qtl_scan_cols (cnf2hip.h) through the shared algebra of cnf2_qtl.h: least squares of the columns
 * y[n][n_col] on [x0, scale_i reg(i, 0 .. ne-1)] with reg[n][ne], scale[n] or NULL, x0[n][nx].  lod_out[n_col],
 * coef_out[n_col][2], *rank_out, rss0_out[n_col].  -2: a bad argument. */
int cnf2h_qtl_cols_marker(int n, int ne, const double *reg, const double *scale, int nx, const double *x0, int n_col,
                          const double *y, double *lod_out, double *coef_out, int32_t *rank_out, double *rss0_out);

/* The host side of the bootstrap scan (cnf2_qtl_scan_boot of cnf2hip.h; `cnF2freq --qtlboot` uses the first):
 *  cnf2h_qtl_bootstrap_counts  count_out[n_boot][n] (int32): how often replicate b draws individual i.  Within every stratum
 *                              (strata[n], NULL = one) the k used individuals (use[n], NULL = all), in ascending order, are
 *                              idx[0..k); draw j of replicate b, one per used individual j, picks idx[floor(u k)] of j's
 *                              stratum with u = (splitmix64(seed, b n + j) >> 11) 2^-53, the keys cnf2h_qtl_permutations
 *                              sorts by.  A row sums to the used individuals of every stratum; unused individuals get 0.  No
 *                              sequential generator enters: cnf2freq_amd/qtl.py's bootstrap_counts() gives the same arrays
 *  cnf2h_qtl_boot_marker       one (replicate, marker) cell through cnf2freq_amd/csrc/cnf2_qtl.h, the individuals in ascending
 *                              order: origin[n][4] the marker's rows, y[n][n_traits] and cov[n][n_cov] as they enter the sums
 *                              (the scan centres them first), c[n] the chromosome's mask, count[n] the replicate.
 *                              lod_out[n_traits], coef_out[n_traits][2], *rank_out, rss0_out[n_traits], *n_bc_out.
 * -2: a bad argument (a negative count among them). */
int cnf2h_qtl_bootstrap_counts(int n, int n_boot, uint64_t seed, const uint8_t *use, const int32_t *strata, int32_t *count_out);
int cnf2h_qtl_boot_marker(int n, const double *origin, int n_traits, const double *y, int n_cov, const double *cov,
                          const uint8_t *c, const int32_t *count, int additive, double *lod_out, double *coef_out,
                          int32_t *rank_out, double *rss0_out, int32_t *n_bc_out);

/* One marker of the multiple-imputation scan (cnf2_qtl_scan_imp of cnf2hip.h) through cnf2freq_amd/csrc/cnf2_qtlimp.h, the
 * individuals and the draws in ascending order: state[n][n_draws] (uint8) the marker's sampled states, below 64 wherever c is
 * set; y[n][n_traits] and cov[n][n_cov] as they enter the sums (the scan centres them first); c[n] the chromosome's mask.
 * lod_out[n_traits] the combined LOD, coef_out[n_traits][2] the weighted mean effects (NaN once a draw drops the column),
 * *rank_out the smallest rank over the draws, rss0_out[n_traits], *n_used_out n_c, draw_lod_out[n_draws][n_traits] or NULL
 * the draws' own LODs.  -2: a bad argument (n_draws outside 1 .. 1024 and a state of 64 or more under the mask among them). */
int cnf2h_qtlimp_marker(int n, int n_draws, const uint8_t *state, int n_traits, const double *y, int n_cov, const double *cov,
                        const uint8_t *c, int additive, double *lod_out, double *coef_out, int32_t *rank_out, double *rss0_out,
                        int32_t *n_used_out, double *draw_lod_out);

/* What the QTL scans of cnf2hip.h plan on the host before they allocate (cnf2freq_amd/csrc/cnf2_qtlplan.h), for tests:
 *  cnf2h_qtl_marker_map   the marker map a scan uploads, in int32 words: the header -- chromstarts[n_chrom + 1] of the whole
 *                         map (whole_map_header) or the first marker of every chromosome of chrom_begin .. chrom_end-1;
 *                         with_mchrom (whole_map_header only) the chromosome of every marker; a record {c, m, len, 0} per
 *                         tile of at most `tile` markers m .. m+len-1 of the range's chromosomes in order, none across a
 *                         chromosome start, c counted from 0 (whole_map_header) or from chrom_begin; per chromosome of
 *                         the range and one past the last the index of its first tile.  offsets_out[4] = the word offsets
 *                         of the marker chromosomes, the tiles and the tile starts, and the number of tiles.  Returns the
 *                         words of the image and writes them to image_out where it is not NULL and cap holds them.
 *  cnf2h_qtl_column_tile  the columns a scan of n individuals takes per pass out of R, with P permutations: the column image
 *                         under 1 GB, 16 .. 4096; with P > 0 the maxima, maxima_doubles_per_column doubles per column (0 =
 *                         the scan has no such bound), under 256 MB, at least 16; at most R; at most cap (0 = none).
 * -2: a bad argument. */
int64_t cnf2h_qtl_marker_map(const int32_t *chromstarts, int n_chrom, int chrom_begin, int chrom_end, int tile, int with_mchrom,
                             int whole_map_header, int32_t *image_out, int64_t cap, int64_t *offsets_out);
int64_t cnf2h_qtl_column_tile(int64_t n, int64_t R, int64_t P, int64_t maxima_doubles_per_column, int cap);

/* The host side of the multi-trait scan (cnf2_qtl_scan_mv of cnf2hip.h):
 *  cnf2h_qtlmv_marker     one (marker, group) cell through cnf2freq_amd/csrc/cnf2_qtlmv.h, the individuals in ascending order:
 *                         origin[n][4] the marker's rows, y[n][n_traits] (1 .. 16 traits) and cov[n][n_cov] as they enter the
 *                         sums (the scan centres them first), c[n] the chromosome's mask.  *lod_out the joint LOD, *rank_out
 *                         the marker's rank, *trait_rank_out the traits kept, *n_used_out n_c.
 *  cnf2h_qtl_group_tile   the groups of T traits a scan of n individuals takes per pass out of G, with P permutations and
 *                         n_tiles marker tiles: a group is T columns padded to 4, 8 or 16; the padded image under 1 GB (16
 *                         .. 4096 columns), at least one group; with P > 0 the maxima, n_tiles doubles per group, under
 *                         256 MB, at least one group; at most G; at most cap (0 = none).
 * -2: a bad argument. */
int cnf2h_qtlmv_marker(int n, const double *origin, int n_traits, const double *y, int n_cov, const double *cov,
                       const uint8_t *c, int additive, double *lod_out, int32_t *rank_out, int32_t *trait_rank_out,
                       int32_t *n_used_out);
int64_t cnf2h_qtl_group_tile(int64_t n, int64_t T, int64_t G, int64_t P, int64_t n_tiles, int cap);

/* The host side of the within-family scan (cnf2_qtl_scan_fam of cnf2hip.h):
 *  cnf2h_qtlfam_marker    one marker through cnf2freq_amd/csrc/cnf2_qtlfam.h, by the steps and in the order of the kernels:
 *                         origin[n][4] the marker's rows, side 0 or 1, grp[n] and cell[n] (NULL: grp) as the scan takes
 *                         them, y[n][n_traits] and cov[n][n_cov] as they enter the sums (the scan centres them over the
 *                         used individuals first; the centring within cells is done here), c[n] the chromosome's mask
 *                         (an individual with grp < 0 is taken out here).  lod_out[n_traits], *df_out,
 *                         slope_out[n_traits][n_fam] (NULL: not asked for), rss0_out[n_traits], *n_used_out n_c,
 *                         *n_cells_out the cells with a used member.
 *  cnf2h_qtl_families     grp_out[n] / cell_out[n] of the analysed individuals dous[n] (records) from the pedigree's
 *                         par[n_rec][2]: grp the parent on the side (par[.][side]) and cell the pair (par0, par1), both
 *                         numbered from 0 in ascending order of the records; -1 where the parent on the side is missing or
 *                         has no recorded parents -- its bit of the origin rows has no meaning there.  *n_fam_out the
 *                         parents counted.
 * -2: a bad argument. */
int cnf2h_qtlfam_marker(int n, const double *origin, int side, const int32_t *grp, const int32_t *cell, int n_fam, int n_traits,
                        const double *y, int n_cov, const double *cov, const uint8_t *c, double *lod_out, int32_t *df_out,
                        double *slope_out, double *rss0_out, int32_t *n_used_out, int32_t *n_cells_out);
int cnf2h_qtl_families(int n_rec, const int32_t *par, int n, const int32_t *dous, int side, int32_t *grp_out, int32_t *cell_out,
                       int32_t *n_fam_out);

/* The host side of the descent rows and the founder-haplotype scan (cnf2_sweep_descent of cnf2hip.h):
 *  cnf2h_descent_columns  col_out[n][8] of the analysed individuals dous[n] (records) from the pedigree's par[n_rec][2]: the
 *                         model column of every cell of a descent row.  Cell 4 s + 2 w + b belongs to grandparent
 *                         par[par[dous[i]][s]][w], strand b; the distinct grandparents are numbered g from 0 in ascending
 *                         order of the records.  by 0 (haplotype): column 2 g + b; 1 (founder): column g; 2 (line): column w.
 *                         -1 in the four cells of a side whose parent is missing or has no two recorded parents.
 *                         *n_grand_out the grandparents counted.
 *  cnf2h_qtlhap_marker    one marker of the founder-haplotype scan (cnf2_qtl_scan_hap of cnf2hip.h) through
 *                         cnf2freq_amd/csrc/cnf2_qtlhap.h, by the steps and in the order of the kernels: descent[n][8] the
 *                         marker's rows, col[n][8] and n_columns as the scan takes them, y[n][n_traits] and cov[n][n_cov] as
 *                         they enter the sums (the scan centres them over the used individuals first), c[n] the chromosome's
 *                         mask (an individual with a column outside 0 .. n_columns-1 is taken out here).  lod_out[n_traits],
 *                         *df_out, coef_out[n_traits][n_columns] (NULL: not asked for), rss0_out[n_traits], *n_used_out n_c.
 * -2: a bad argument. */
int cnf2h_qtlhap_marker(int n, const double *descent, const int32_t *col, int n_columns, int n_traits, const double *y, int n_cov,
                        const double *cov, const uint8_t *c, double *lod_out, int32_t *df_out, double *coef_out, double *rss0_out,
                        int32_t *n_used_out);
int cnf2h_descent_columns(int n_rec, const int32_t *par, int n, const int32_t *dous, int by, int32_t *col_out,
                          int32_t *n_grand_out);

/* The host side of the variance-component scan (cnf2_qtl_scan_vc of cnf2hip.h):
 *  cnf2h_qtlvc_marker     one marker through cnf2freq_amd/csrc/cnf2_qtlvc.h, by the steps and in the order of the kernels (the
 *                         Jacobi schedule, the grid tables, the bisection): the inputs of cnf2h_qtlhap_marker with n_columns
 *                         1 .. 64.  lod_out[n_traits], h_out[n_traits], sigma2_out[n_traits], blup_out[n_traits][n_columns]
 *                         (NULL: not asked for), eval_out[n_columns] (NULL: not asked for), *rank_out (-1: the iteration did
 *                         not converge), rss0_out[n_traits], *n_used_out n_c.
 * -2: a bad argument. */
int cnf2h_qtlvc_marker(int n, const double *descent, const int32_t *col, int n_columns, int n_traits, const double *y, int n_cov,
                       const double *cov, const uint8_t *c, double *lod_out, double *h_out, double *sigma2_out, double *blup_out,
                       double *eval_out, int32_t *rank_out, double *rss0_out, int32_t *n_used_out);

#ifdef __cplusplus
}
#endif
#endif /* CNF2HOST_H */
