/*
 * cnf2hip.h -- C ABI of libcnf2hip.so, the MI355X (gfx950) implementation of
 * cnF2freq's per-individual HMM forward-backward sweep.
 *
 * The reference has no FFI; its seam for this path is the in-process call
 *   double individ::doanalyze<Turner,Stop>(tb, turner, startmark, endmark, stopdata,
 *                                          flag2, ruleout, realprobs, minfactor)
 * (cnF2freq.cpp:2122-2131) driven per individual by doit<> (cnF2freq.cpp:5294-5583),
 * reading the global individ graph (cnF2freq.cpp:853-914, 2448-2514), markerposes /
 * chromstarts / genrec (cnF2freq.cpp:233-239) and thread-private alpha/beta stores
 * (cnF2freq.cpp:392-394).  This header is the batch form of that seam: the globals
 * become explicit uploads, the OpenMP loop over `dous` becomes one call.
 *
 * Conventions: plain C types, caller-owned buffers, int status (0 = ok, <0 = error,
 * message via cnf2_last_error).  Impossible data is reported in-band exactly like the
 * reference: a log-likelihood <= CNF2_MINFACTOR (or NaN) means "skip this individual"
 * (cnF2freq.cpp:1659, 5403); no exceptions, no abort.
 * One context per GPU; a context is not thread-safe, distinct contexts are independent.
 * The library fails loudly (CNF2_ERR_NO_DEVICE) when no HIP device is usable; there is
 * no CPU fallback.
 */
#ifndef CNF2HIP_H
#define CNF2HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define CNF2_NUMTYPES   64      /* settings.h:27  inheritance states          */
#define CNF2_NUMSHIFTS  8       /* settings.h:35  phase-shift modes           */
#define CNF2_NUMPATHS   128     /* settings.h:32  allele-assignment paths     */
#define CNF2_MINFACTOR  (-1e15f)/* settings.h:29                              */
#define CNF2_IGNORED    (-1e30) /* factors[] value of a masked shift mode, cnF2freq.cpp:5378 */

enum {
    CNF2_OK            = 0,
    CNF2_ERR_NO_DEVICE = -1,
    CNF2_ERR_ARG       = -2,
    CNF2_ERR_STATE     = -3,   /* call order violated (e.g. sweep before uploads) */
    CNF2_ERR_HIP       = -4,
    CNF2_ERR_NOMEM     = -5
};

/* cnf2_sweep flags */
enum {
    CNF2_OUT_DEVICE   = 1u << 0, /* output pointers are device pointers (no D2H copy, no sync) */
    CNF2_NO_DOSAGE    = 1u << 1, /* HOT LOOP 1 only: factors/loglik, skip the per-locus rows    */
    CNF2_RAW_DOSAGE   = 1u << 2, /* rows un-normalised (sum of val by class, cnF2freq.cpp:3523) */
    CNF2_NO_TIES      = 1u << 3, /* drop ignoreflag2's all-or-none rule (cnF2freq.cpp:3484-3486) */
    CNF2_FULL_SPILL   = 1u << 4, /* store alpha-minus at every marker instead of every second one and
                                    recomputing the others in the backward pass (same results) */
    CNF2_MERGE_MODES  = 1u << 5, /* sweep bit-identical shift modes once: for a window whose two parents are
                                    homozygous with equal sure at every marker (e.g. the private empty F1
                                    parents of an F2, cnF2freq.cpp:6515-6527) the modes that differ in the
                                    parents' shift bits carry the same alpha/beta; four such individuals
                                    share a wavefront.  Same outputs for all 8 modes (rows to rounding).
                                    Ignored together with CNF2_FULL_SPILL. */
    CNF2_ACC_DEVICE   = 1u << 6, /* cnf2_sweep_accumulate: the four accumulator pointers are device pointers owned by the
                                    caller (a multi-GPU driver all-reduces them in place).  They must be ordinary
                                    (coarse-grained) device memory -- hipMalloc or a torch CUDA tensor: the kernels add with
                                    hardware f64 atomics (-munsafe-fp-atomics), which fine-grained or host-mapped memory
                                    silently drops.  The order of the additions is not fixed: accumulators are
                                    reproducible to rounding, not to the bit, unless CNF2_DETERMINISTIC is set */
    CNF2_ACC_KEEP     = 1u << 7, /* cnf2_sweep_accumulate: add to the per-record accumulators instead of zeroing them */
    CNF2_ACC_TABLE    = 1u << 10, /* cnf2_sweep_accumulate: evaluate every window in the table form (one lane per emission-table
                                    entry) instead of the path form (one lane per allele path of a line); same sums, the
                                    slower kernel -- kept as the cross-check of the fast one and for windows whose root
                                    is the top of its own lines, which always take it */
    CNF2_ACC_LANES    = 1u << 11, /* cnf2_sweep_accumulate: path form with one lane per path for every window (the kernel that
                                    windows with tie groups always take) instead of the tile form; A/B and cross-check */
    CNF2_TIES_GENERAL = 1u << 12, /* cnf2_sweep, cnf2_sweep_accumulate, cnf2_sweep_turn_scan: windows with tie groups through the general kernel (one lane per table entry, producer
                                    per marker) instead of the tile-producer kernel's pass per tie combination; cross-check */
    CNF2_UPDATE_PLAIN = 1u << 13, /* cnf2_update_pass: the literal form -- one thread per (record, marker), every bisection step with its
                                    quadrature as the reference's cappedgd runs it -- instead of the scout / finish kernels, which
                                    make the same decisions with a fraction of the gradient evaluations (cnf2_update.h).  The
                                    yardstick of the fast form and an A/B switch: the fast form gives the same results TO THE
                                    BIT only together with CNF2_UPDATE_BOTH_FLOWS; its default (one certainty flow per side, the
                                    other its mirror image) is within rounding of this form, not bit-identical */
    CNF2_UPDATE_BOTH_FLOWS = 1u << 16, /* cnf2_update_pass, fast form: run the certainty flow of BOTH allele values of a side, as
                                    processinfprobs does (cnF2freq.cpp:4222-4290), instead of one flow and its mirror image
                                    (DESIGN.md section 3.11).  The bit-exact form: equal to CNF2_UPDATE_PLAIN to the bit */
    CNF2_UPDATE_ONE_SCOUT = 1u << 17, /* cnf2_update_pass, fast form: the scouts (certainties and, since round 5, weights) in one pass
                                    instead of two (same results to the bit; A/B switch, tools/ab_scout.py) */
    CNF2_UPDATE_LITERAL_FINISH = 1u << 19, /* cnf2_update_pass, fast form: the flows the scouts set aside take one literal bisection
                                    step (midpoint, bound, quadrature) per round, as in rounds 3 / 4, instead of the guided
                                    bisection (cnf2_update.h: the same decisions from 3 - 4 quadratures per flow).  Same
                                    results to the bit; A/B switch and cross-check */
    CNF2_FLUSH_TINY   = 1u << 20, /* cnf2_sweep: every window through the general kernel (one lane per table entry, vectors
                                    normalised at every marker as the reference normalises them) WITH adjustprobs' rule that a
                                    state under 1e-300 of its vector is set to exactly 0 before the emission is applied
                                    (cnF2freq.cpp:1607-1611).  The fast kernels carry such states (no
                                    effect on valid data above 1e-6 -- except where every OTHER state then becomes exactly
                                    impossible, a locked phase contradicting certain genotypes: the reference declares the
                                    shift mode impossible, the fast kernels return the likelihood of the 1e-303 state).
                                    This flag is the reference's behaviour to the letter, at the general kernel's speed */
    CNF2_DETERMINISTIC = 1u << 14, /* cnf2_sweep_accumulate: every analysed individual writes what its window members receive at a
                                    locus into a row of its own (336 B per individual x marker, allocated for the whole
                                    range) and one more kernel adds the rows of every record in ascending order of the
                                    individual, instead of f64 atomics in order of arrival: accumulators -- and with them
                                    whole iterations -- reproduce to the bit from run to run */
    CNF2_TURN_VALU    = 1u << 15, /* cnf2_sweep_turn_scan: the 1 024 dot products per (individual, marker) on the vector ALU (one lane
                                    per pair of shift modes, flips as register renaming) instead of the matrix cores
                                    (v_mfma_f64_16x16x4: a 32 x 32 x 64 product per unit); same sums in another order: cross-check, A/B */
    CNF2_STATIC_JOBS  = 1u << 18, /* cnf2_sweep, cnf2_sweep_accumulate, cnf2_sweep_turn_scan: wavefront w of a launch sweeps jobs w, w + waves, ...
                                     instead of taking its jobs one at a time from the launch's counter (the default: whichever
                                     blocks are resident share the job list evenly, whatever the chromosomes' lengths and
                                     however the kernels of the tied and the untied windows share the machine).  Same results
                                     to the bit: a job's arithmetic does not depend on the wave that runs it. */
    CNF2_ALL_STATES   = 1u << 21, /* cnf2_sweep and its modes: the windows of crosses of inbred lines (both parents and all four
                                     grandparents homozygous with equal sure everywhere) through the fast kernel's ordinary
                                     instantiation, which carries all 64 states of a chain, instead of the instantiation that
                                     keeps the states their tables make equal only once.  Same results to the bit; A/B switch
                                     and cross-check.  Ignored where that instantiation is not used */
    CNF2_QTL_ADDITIVE = 1u << 22, /* cnf2_qtl_scan, cnf2_sweep_qtl: the additive model -- the dominance column is always dropped */
    CNF2_QTL_ORIGIN_DEVICE = 1u << 23, /* cnf2_qtl_scan: `origin` is a device pointer (aligned to 16 bytes), e.g. the rows a
                                     cnf2_sweep_origins call with CNF2_OUT_DEVICE filled; they are read in place */
    CNF2_NO_LINE_RECORDS = 1u << 24, /* cnf2_sweep and its modes: the instantiation for crosses of inbred lines forms every window's
                                     emission terms from the window's own seven rows, as the ordinary one does, instead of reading
                                     what a window's ancestors contribute from the launch's line records (cnf2_last_line_records).
                                     Same results to the bit; A/B switch and cross-check.  Ignored where no records are used */
    CNF2_NO_UNIFORM_PACK = 1u << 26, /* cnf2_sweep and its Viterbi mode: every window of a cross of inbred lines is swept by a wave of
                                     its own, instead of four windows of one chromosome to a wave where four of them have their
                                     lines among the launch's records (cnf2_last_uniform_pack).  Same results to the bit; A/B
                                     switch and cross-check.  Ignored where no windows are packed */
    CNF2_NO_UNIFORM_PACK8 = 1u << 27, /* cnf2_sweep and its Viterbi mode: the packed windows go four to a wave only, instead of eight
                                     where two groups of four of a chromosome have all eight shift modes of every window analysed
                                     (cnf2_last_uniform_pack8).  Same results to the bit; A/B switch and cross-check.  Ignored
                                     where no windows are packed */
    CNF2_QTL_REG_DEVICE = 1u << 28, /* cnf2_qtl_scan_cols: `reg` is a device pointer (aligned to 16 bytes); it is read in place */
    CNF2_QTL_IMPRINT  = 1u << 25, /* cnf2_qtl_scanx: the design gets the parent-of-origin (imprinting) effect i = o[1] - o[2] */
    CNF2_QTL_STATE_DEVICE = 1u << 29, /* cnf2_qtl_scan_imp: `state` is a device pointer, e.g. the states a cnf2_sweep_sample call with
                                     CNF2_OUT_DEVICE filled; they are read in place */
    CNF2_QTL_JOINT_DEVICE = 1u << 30, /* cnf2_qtl_scan2_linked: `joint` is a device pointer (aligned to 16 bytes), e.g. the rows a
                                     cnf2_sweep_pairs call with CNF2_OUT_DEVICE filled; they are read in place */
    CNF2_LOG_PATHS    = 1u << 9, /* cnf2_sweep records which kernel / producer specialisation swept every job (cnf2_last_paths) */
    CNF2_XPOSE        = 1u << 8  /* sweep kernel variant: the three lane-held state bits of the transition are brought into
                                    registers by a transpose through LDS instead of being exchanged by DPP moves (same
                                    results to rounding; A/B switch while the variant is evaluated) */
};

typedef struct cnf2_ctx cnf2_ctx;

/* Library / device ------------------------------------------------------------ */
int         cnf2_device_count(void);
int         cnf2_ctx_create(int device, cnf2_ctx **out);
void        cnf2_ctx_destroy(cnf2_ctx *ctx);
const char *cnf2_last_error(const cnf2_ctx *ctx);           /* ctx may be NULL: last create error */
const char *cnf2_version(void);

/* Marker map: replaces markerposes / chromstarts / genrec
 * (readalphamap cnF2freq.cpp:6669-6685; main cnF2freq.cpp:7927-7943).
 * pos[n_markers] in cM; chromstarts[n_chrom+1] with chromstarts[n_chrom] == n_markers;
 * genrec[3] (NULL = {-0.02,-0.02,-0.02}). */
int cnf2_upload_map(cnf2_ctx *ctx, const double *pos, int n_markers, const int32_t *chromstarts,
                    int n_chrom, const double *genrec);

/* Genotype rows: replaces individ::markerdata / markersure / haploweight
 * (cnF2freq.cpp:876-887; filled by readalphadata cnF2freq.cpp:6542-6667).
 * Rows are de-duplicated storage; several individuals may share one row (all
 * `empty` individuals normally share a blank row: alleles 0, sure 0, hw 0.5).
 *   allele [n_rows][n_markers][2]  MarkerVal values 0 (unknown), 1, 2, 9
 *   sure   [n_rows][n_markers][2]
 *   hw     [n_rows][n_markers]
 * cnf2_update_rows overwrites rows [row0,row0+n) between sweeps (the per-iteration
 * parameter updates of cnF2freq.cpp:6344-6368 stay on the host). */
int cnf2_upload_rows(cnf2_ctx *ctx, int n_rows, const uint8_t *allele, const double *sure,
                     const double *hw);
int cnf2_update_rows(cnf2_ctx *ctx, int row0, int n, const uint8_t *allele, const double *sure,
                     const double *hw);
/* cnf2_upload_rows with all three pointers NULL allocates n_rows blank rows (alleles 0,
 * sure 0, hw 0.5: an individual without data, getind cnF2freq.cpp:2486-2493).
 * cnf2_update_rows_device takes DEVICE pointers and the packed allele form the kernels use:
 * d_allele8[n][n_markers] = first | second << 4; d_sure[n][n_markers][2]; d_hw[n][n_markers]. */
int cnf2_update_rows_device(cnf2_ctx *ctx, int row0, int n, const uint8_t *d_allele8,
                            const double *d_sure, const double *d_hw);

/* Pedigree graph: replaces individer[] / individ::{pars,empty,gen} and `dous`
 * (readalphaped cnF2freq.cpp:6495-6540).  par[n_rec][2] record index or -1;
 * row_of[n_rec] row index; dous[n_dous] the analysed records in output order.
 * The library derives, per analysed individual, what fixtrees (cnF2freq.cpp:3099-3187)
 * produces: the 7-slot window, shiftignore, flag2ignore, founder flags (for every
 * record, as postmarkerdata does, cnF2freq.cpp:3373-3389) and the groups of slots
 * occupied by one ancestor (relmap). */
int cnf2_upload_pedigree(cnf2_ctx *ctx, int n_rec, const int32_t *par, const uint8_t *empty,
                         const int32_t *gen, const int32_t *row_of, const int32_t *dous,
                         int n_dous);

/* Window topology as derived by the library (parity hook for fixtrees):
 * out[0]=shiftignore out[1]=flag2ignore out[2]=founder out[3..9]=slot records (-1 none)
 * out[10..16]=tie group per slot (-1 = ancestor occupies a single slot). */
int cnf2_window_info(cnf2_ctx *ctx, int ind, int32_t *out17);
/* the same for every analysed individual in one call: out17_all[n_dous][17] */
int cnf2_window_table(cnf2_ctx *ctx, int32_t *out17_all);

/* The sweep: per-individual body of doit<> (cnF2freq.cpp:5294-5403) plus the per-locus
 * allele-2 dosage posterior row that genotypereporter accumulates (cnF2freq.cpp:5406-5553,
 * 3532-3538) for analysed individuals [ind_begin, ind_end), every chromosome.
 *   factors_out [n][n_chrom][8]  log-likelihood per shift mode (CNF2_IGNORED if masked)
 *   loglik_out  [n][n_chrom]     logsumexp over modes; <= CNF2_MINFACTOR or NaN => skipped
 *   dosage_out  [n][n_markers][3] posterior of 0/1/2 copies of allele 2, rows normalised
 *                                (all-zero row for a skipped individual); may be NULL with
 *                                CNF2_NO_DOSAGE
 * With CNF2_OUT_DEVICE the three pointers are device pointers and the call only enqueues
 * work on the context's stream (use cnf2_sync). */
int cnf2_sweep(cnf2_ctx *ctx, int ind_begin, int ind_end, double *factors_out, double *loglik_out,
               double *dosage_out, uint32_t flags);
int cnf2_sync(cnf2_ctx *ctx);

/* Parity/debug view of the alpha/beta store of one individual and chromosome in the
 * reference's layout (cnF2freq.cpp:392-393): fwbw_out[8][mc][3][64] with slot 0 = alpha
 * before emission, 1 = beta, 2 = alpha after emission; fwbwfactors_out[8][mc][3] the
 * cumulative log scales; mc = markers on the chromosome.  Masked modes are left zero. */
int cnf2_fwbw_store(cnf2_ctx *ctx, int ind, int chrom, double *fwbw_out, double *fwbwfactors_out);

/* Stage-2 consumers of the alpha/beta store (parity level, one individual x chromosome per call;
 * not tuned).  They answer in bulk the queries that doit<> issues one by one:
 *  cnf2_locked_query    val_out[8][64][128]: exp(doanalyze(classicstop(q, g), flag2) - factor) for
 *                       every shift mode, state g and path flag2 at `marker` (cnF2freq.cpp:5499-5508;
 *                       0 where the reference would not count the term).  No ignoreflag2 pruning
 *                       is applied (cnF2freq.cpp:5464): the caller masks.
 *  cnf2_turn_scan       rawervals_out[128][8]: doanalyze<aroundturner>(turn, classicstop(q, -1)) - factor
 *                       (cnF2freq.cpp:5686-5724) for every turn and shift mode, unmasked.
 *  cnf2_state_posterior rows_out[mc][64]: what statereporter::addval accumulates (cnF2freq.cpp:3540-3546),
 *                       i.e. sum of val over shift modes and admissible paths by state, per marker. */
int cnf2_locked_query(cnf2_ctx *ctx, int ind, int chrom, int marker, double *val_out);
int cnf2_turn_scan(cnf2_ctx *ctx, int ind, int chrom, int marker, double *rawervals_out);
/*  cnf2_turn_scan_rows  the same for every marker of the chromosome in one launch: rows_out[mc][128][8] */
int cnf2_turn_scan_rows(cnf2_ctx *ctx, int ind, int chrom, double *rows_out);
int cnf2_state_posterior(cnf2_ctx *ctx, int ind, int chrom, double *rows_out, uint32_t flags);
/*  cnf2_haplos          rows_out[mc][7][2]: the HAPLOS accumulators HOT LOOP 2 leaves per window slot
 *                       (slot order of cnf2_window_info) before movehaplos: sum of val by the phase with
 *                       which the slot's individual is used (cnF2freq.cpp:1347-1350, 1561-1575, 5556).
 *                       An individual occupying several slots gets the sum of its slots in the reference. */
int cnf2_haplos(cnf2_ctx *ctx, int ind, int chrom, double *rows_out, uint32_t flags);
/*  cnf2_infprobs        the other accumulators of HOT LOOP 2 at `marker` (DOINFPROBS, cnF2freq.cpp:5513-5577):
 *                       inf_out[7][2][2] = thread-private infprobs[slot][allele index][markerval - 1] before
 *                       moveinfprobs (cnF2freq.cpp:3577-3597; trackpossible<GENOSPROBE> weights, <GENOS>
 *                       updates, cnF2freq.cpp:1351-1354), hz_out[2] = what is added to the individual's
 *                       homozyg[marker] (trackpossible<HOMOZYGOUS>, cnF2freq.cpp:1304-1320).  Brute force over
 *                       (shift mode, state, path) like the reference; sums are accumulated atomically. */
int cnf2_infprobs(cnf2_ctx *ctx, int ind, int chrom, int marker, double *inf_out, double *hz_out, uint32_t flags);
/*  cnf2_infprobs_rows   the same accumulators for every marker of the chromosome, rows_out[mc][30] = infprobs
 *                       [7][2][2] followed by homozyg[2], through their closed form (cnf2_accum.h: the weight of
 *                       a path depends on one line of descent only, the other line enters as its restricted
 *                       total) instead of the 128-path fan-out. */
int cnf2_infprobs_rows(cnf2_ctx *ctx, int ind, int chrom, double *rows_out, uint32_t flags);
/*  cnf2_crossover_rows  rows_out[mc][6]: the crossover posteriors of cnf2_sweep_crossovers for one individual and
 *                       chromosome, from the store by brute force (explicit 64 x 64 transition, one thread per state):
 *                       the cross-check of the sweep's fused form. */
int cnf2_crossover_rows(cnf2_ctx *ctx, int ind, int chrom, double *rows_out);

/* Crossover posteriors (Baum-Welch pairwise posterior of the transition; not a port of the reference's disabled
 * DOREMAPDISTANCES path).  For analysed individual i, marker m and state bit t, xi_t(m) = posterior probability that
 * bit t differs between markers m and m+1, given the individual's window data, summed over the shift modes with the
 * weights and the 40-log-unit rule of the dosage rows (cnF2freq.cpp:5421).  Column t is one meiosis:
 *   0  the first parent's meiosis that made the individual    (genrec[1], TYPEGENS = 1)
 *   1  the first parent's first parent's meiosis that made the first parent   (genrec[0])
 *   2  the first parent's second parent's meiosis that made the first parent  (genrec[0])
 *   3  the second parent's meiosis that made the individual   (genrec[1])
 *   4  the second parent's first parent's meiosis that made the second parent (genrec[0])
 *   5  the second parent's second parent's meiosis that made the second parent (genrec[0])
 * ("first" / "second" parent in the order of the pedigree's par columns; bits 1-2 and 4-5 trace the grandparents.)
 * xi = 0 where pos[m+1] - pos[m] <= 0, at the last marker of every chromosome and for a skipped individual
 * (loglik <= CNF2_MINFACTOR or NaN).  xi depends on alpha / beta only: ties, CNF2_NO_TIES and ignoreflag2 do not enter.
 *   factors_out / loglik_out  as cnf2_sweep: bit-equal (the same forward passes)
 *   xo_out        [n][n_markers][6] per individual, or NULL
 *   xo_sum_out    [n_markers][6] the same summed over the individuals of the range (reduced on the device, f64 atomics:
 *                 equal to the host sum of xo_out to rounding, not to the bit)
 *   n_contrib_out [n_chrom] (int32) individuals of the range with a likelihood on that chromosome (not skipped)
 * Outputs are overwritten, not accumulated; a range split [a,b) + [b,c) adds up to [a,c).
 * One pass: untied windows through the fast kernel's crossover instantiation (likelihoods and posteriors together), tied
 * windows through the tied kernel without rows (likelihoods) and the general kernel's crossover instantiation.
 * Flags: CNF2_OUT_DEVICE (all five pointers are device pointers; xo_sum_out / n_contrib_out must be ordinary device
 * memory as for CNF2_ACC_DEVICE), CNF2_STATIC_JOBS, CNF2_FULL_SPILL (fast kernel with the full spill) and
 * CNF2_TIES_GENERAL (tied likelihoods from the general kernel) as in cnf2_sweep: same values to rounding.
 * CNF2_MERGE_MODES, CNF2_XPOSE and the dosage flags are ignored.  The call synchronises the context's stream once (the
 * job list), also with CNF2_OUT_DEVICE.  To re-estimate the map, call cnf2_upload_map again with new positions
 * (same marker count and chromstarts: the rows stay) and sweep again; cnf2h_map_mstep of cnf2host.h is the M-step. */
int cnf2_sweep_crossovers(cnf2_ctx *ctx, int ind_begin, int ind_end, double *factors_out, double *loglik_out,
                          double *xo_out, double *xo_sum_out, int32_t *n_contrib_out, uint32_t flags);

/* Viterbi decoding: the maximum a-posteriori (MAP) inheritance path of every analysed individual on every chromosome.
 * For shift mode s, logmax[s] = log max over state paths g_1..g_n of pi(g_1) prod_m e_s,m(g_m) prod_m T_m(g_m, g_m+1),
 * the max-product twin of factors[s] (pi = 1/64, e the sweep's path-free emission, T the 64 x 64 Kronecker transition;
 * it includes the same dropped per-gap constants as factors).  The MAP mode s* is the argmax of logmax over the active
 * modes; the MAP path is the argmax state sequence in mode s*, and exp(logmax[s*] - loglik) is the posterior probability
 * of the decoded (mode, path).  Ties, of which the model has many exactly symmetric ones, are broken as follows: at every
 * butterfly stage a state keeps its own value unless the flipped partner is strictly larger; at the last marker the
 * lowest state index among the maxima; across modes the lowest mode index.
 * A state is g = j*8 + lo as in cnf2_state_posterior; bit t of g is the meiosis of column t of cnf2_sweep_crossovers.
 * The path is in the frame of mode s*; its bit flips between markers m and m+1 (the crossover calls) do not depend on it.
 *   factors_out / loglik_out  as cnf2_sweep: bit-equal (the same forward passes)
 *   logmax_out  [n][n_chrom][8]  CNF2_IGNORED for masked modes, CNF2_MINFACTOR for a mode without likelihood
 *   state_out   [n][n_markers]   (uint8) MAP state of every marker
 *   shift_out   [n][n_chrom]     (int32) s*
 * An individual is skipped on a chromosome where the sweep skips it (no shift mode with a likelihood): its states there
 * are 0xFF, its shift -1 and its logmax CNF2_IGNORED.  A range split [a,b) + [b,c) gives [a,c) bit for bit.
 * One pass: untied windows through the fast kernel's Viterbi instantiation (likelihoods, max-product recursion, decision
 * bits in the wave's spill slot, backtrace in the same wave), tied windows through the tied kernel without rows
 * (likelihoods) and then the same Viterbi instantiation.
 * Flags: CNF2_OUT_DEVICE (all five pointers are device pointers), CNF2_STATIC_JOBS, CNF2_FULL_SPILL (the fast kernel
 * without the half spill) and CNF2_TIES_GENERAL (tied likelihoods from the general kernel) as in cnf2_sweep.
 * CNF2_MERGE_MODES, CNF2_XPOSE, CNF2_FLUSH_TINY and the dosage flags are ignored.  The call synchronises the context's
 * stream once (the job list), also with CNF2_OUT_DEVICE. */
int cnf2_sweep_viterbi(cnf2_ctx *ctx, int ind_begin, int ind_end, double *factors_out, double *loglik_out,
                       double *logmax_out, uint8_t *state_out, int32_t *shift_out, uint32_t flags);

/* Posterior sampling: n_draws whole (mode, path) draws from P(mode, path | data) for every analysed individual on every
 * chromosome, by forward filtering and backward sampling in the model of the Viterbi and crossover calls (the sweep's
 * path-free emission; no tie rule).  Draw k of individual i on a chromosome:
 *   1. the mode s with weights exp(factors[s] - loglik) over the modes the dosage rows count (active, with a likelihood,
 *      not 40 log-units below the total), renormalised over them;
 *   2. the state at the last marker with weights alpha_last(g), alpha the forward vector after the marker's emission in
 *      mode s;
 *   3. for m = last-1 down to first the state g_m with weights alpha_m(g) T_m(g, g_m+1) (T the 64 x 64 Kronecker
 *      transition of the gap; where the marker distance is <= 0 it is the identity and g_m = g_m+1).
 * logp = log P(mode, path | data) = factors[s] - loglik + the log of w(chosen) / sum w of every state pick; it is comparable
 * with the Viterbi path's log posterior (logmax[s*] - loglik) and never above it.
 * Random numbers (all arithmetic mod 2^64): mix(z) = SplitMix64's output function of z (z += 0x9E3779B97F4A7C15, then the
 * two xor-shift-multiply steps and a final xor-shift), key = mix(mix(mix(seed) ^ i) ^ k), u = (mix(key ^ j) >> 11) 2^-53,
 * with i the absolute index of the analysed individual, k the draw, j = m for the state at marker m and j = n_markers + c
 * for the mode on chromosome c.  A pick is an inverse CDF: weights laid on [0, W) in a fixed order, the first state whose
 * running sum exceeds u W, or else (rounding) the last one with a positive weight; a weight of 0 is never chosen.  Modes
 * are laid in ascending order, and so are the 64 states (STATE_ORDER of cnf2freq_amd/sampling.py is the identity).
 * A draw depends on (seed, i, k) only: range splits, job order, CNF2_STATIC_JOBS and n_draws do not change it.
 * A state is g = j*8 + lo as in cnf2_state_posterior; bit t of g is the meiosis of column t of cnf2_sweep_crossovers; the
 * path is in the frame of the drawn mode.
 *   n_draws      K, 1 .. 1024 (else CNF2_ERR_ARG, nothing written)
 *   factors_out / loglik_out  as cnf2_sweep: bit-equal
 *   state_out    [n][K][n_markers] (uint8), not NULL
 *   shift_out    [n][K][n_chrom]   (int32) the drawn mode, not NULL
 *   logp_out     [n][K][n_chrom]   (double) or NULL
 * An individual is skipped on a chromosome where the sweep skips it: every draw there has states 0xFF, shift -1 and logp
 * CNF2_IGNORED.  Host outputs are staged whole on the device (CNF2_ERR_NOMEM if that fails: split the individual range).
 * One pass: untied windows through the fast kernel's sampling instantiation (likelihoods, then backward walks of up to 64
 * draws in the same wave), tied windows through the tied kernel without rows (likelihoods) and then the same sampling
 * instantiation.  Flags: CNF2_OUT_DEVICE (all five pointers are device pointers), CNF2_STATIC_JOBS, CNF2_FULL_SPILL and
 * CNF2_TIES_GENERAL as in cnf2_sweep_viterbi; CNF2_MERGE_MODES, CNF2_XPOSE, CNF2_FLUSH_TINY and the dosage flags are
 * ignored.  The call synchronises the context's stream once (the job list), also with CNF2_OUT_DEVICE. */
int cnf2_sweep_sample(cnf2_ctx *ctx, int ind_begin, int ind_end, int n_draws, uint64_t seed, double *factors_out,
                      double *loglik_out, uint8_t *state_out, int32_t *shift_out, double *logp_out, uint32_t flags);

/* Marker placement: where on the map does an unmapped marker go?  For n_cand candidate markers, given by rows of their own
 * in the row index space of cnf2_upload_rows, and every mapped marker m,
 *   place[i][q][m] = log( sum_s w_s sum_g gamma_s,m(g) e'_s,q(g) )
 * is the growth of individual i's window log-likelihood when candidate q is laid on the map at the position of m (zero
 * distance: the identity transition).  gamma_s,m(g) is the posterior of state g at marker m in shift mode s (alpha after
 * the emission x beta, normalised within the mode), w_s = exp(factors[s] - loglik) over the modes the dosage rows count
 * (active, with a likelihood, not 40 log-units below the total), e'_s,q(g) the candidate's path-free emission for the
 * window, what cnf2_emission returns for a mapped marker.  Ties, CNF2_NO_TIES and ignoreflag2 do not enter.
 *   n_cand        Q >= 1 (else CNF2_ERR_ARG, nothing written)
 *   cand_allele   [n_rows][Q][2] (uint8), cand_sure [n_rows][Q][2], cand_hw [n_rows][Q] or NULL (= 0.5 everywhere):
 *                 host pointers, also with CNF2_OUT_DEVICE; a NULL allele / sure pointer is CNF2_ERR_ARG
 *   factors_out / loglik_out  as cnf2_sweep: bit-equal (the placement sweep's forward pass is cnf2_sweep's; a range that
 *                 holds tied windows takes them from cnf2_sweep's own launches without rows)
 *   place_out     [n][Q][n_markers] or NULL (the normal case of a large run).  CNF2_MINFACTOR where the sum is exactly 0
 *                 (the candidate's data is impossible at that position for that individual), CNF2_IGNORED where the
 *                 individual is skipped on that chromosome.  A host buffer is staged whole on the device (CNF2_ERR_NOMEM if
 *                 that fails: split the individual range)
 *   place_sum_out [Q][n_markers] the sum of place over the individuals of the range that are neither skipped nor impossible
 *                 there (reduced on the device, f64 atomics: equal to the host sum to rounding, not to the bit)
 *   n_zero_out    [Q][n_markers] (int32) the impossible individuals
 *   null_out      [Q] the unlinked baseline: the sum over the range's individuals of log( mean over the individual's
 *                 active shift modes of (1/64) sum_g e'_s,q(g) ); an individual whose mean is 0 is left out
 *   n_contrib_out [n_chrom] (int32) individuals of the range with a likelihood on that chromosome (not skipped)
 * (place_sum - null) / ln 10 is the LOD of the position against "unlinked"; cnf2freq_amd/placement.py reads the profile.
 * Outputs are overwritten, not accumulated; a range split [a,b) + [b,c) adds up to [a,c) (sums to rounding, counts exactly).
 * The result does not depend on cnf2_set_batch_jobs.  Launches: per batch
 * the fast kernel's placement instantiation for every window (the state posteriors, 4 KB per individual x marker) and, per
 * tile of up to 256 candidates, the contraction on the matrix cores; the sweep runs once per batch, not once per tile.
 * Flags: CNF2_OUT_DEVICE (the seven output pointers are device pointers; the sums and counts must be ordinary device
 * memory as for CNF2_ACC_DEVICE), CNF2_STATIC_JOBS, CNF2_FULL_SPILL and CNF2_TIES_GENERAL as in cnf2_sweep_crossovers;
 * CNF2_MERGE_MODES, CNF2_XPOSE, CNF2_FLUSH_TINY and the dosage flags are ignored.  The call synchronises the context's
 * stream, also with CNF2_OUT_DEVICE (its outputs are then complete when the stream is). */
int cnf2_sweep_place(cnf2_ctx *ctx, int ind_begin, int ind_end, int n_cand, const uint8_t *cand_allele,
                     const double *cand_sure, const double *cand_hw, double *factors_out, double *loglik_out,
                     double *place_out, double *place_sum_out, int32_t *n_zero_out, double *null_out,
                     int32_t *n_contrib_out, uint32_t flags);

/* Leave-one-marker-out: what does the data at one marker cost an individual's likelihood?  The multipoint analogue of an
 * error LOD: it finds genotypes that imply a double crossover and markers that do not belong where the map has them.  For
 * analysed individual i, chromosome c and marker m on c, with L_s the likelihood of shift mode s and L = sum_s L_s (loglik):
 *   loo[i][m]      = log( sum_s L_s,-m ) - log L,  L_s,-m = mode s's likelihood with marker m's emission replaced by 1:
 *                    the surprisal, in nats, of the window's data at m given its data at every other marker of c
 *   unlinked[i][m] = -log( mean over the individual's analysed modes of (1/64) sum_g e_s,m(g) ): the surprisal of the same
 *                    data with the marker off the map, the per-individual term of cnf2_sweep_place's null
 * unlinked - loo is the log-likelihood the marker gains by sitting where the map has it; summed over individuals and divided
 * by ln 10 it is the LOD of the marker's own position.  The sum over s runs over EVERY mode with a likelihood, not only
 * those within the 40 log-units of the dosage rows (a marker that alone pushes a mode out of that band is what the call
 * looks for); a mode without a likelihood on the full map contributes nothing.  The map is Haldane, so two adjacent gaps
 * compose exactly: loo[i][m] equals loglik of cnf2_sweep with column m taken off the map (the others' positions kept) minus
 * loglik on the full map; on a chromosome of one marker, where nothing is left, log(the modes with a likelihood) - loglik.
 * Ties, CNF2_NO_TIES and ignoreflag2 do not enter.
 *   factors_out / loglik_out  as cnf2_sweep: bit-equal (the same forward passes; tied windows from the tied kernel)
 *   loo_out          [n][n_markers] or NULL
 *   unlinked_out     [n][n_markers] or NULL; both CNF2_IGNORED where the individual is skipped on the chromosome (no mode
 *                    with a likelihood).  Rows that are not asked for, and host rows, live whole in a buffer of the
 *                    context (CNF2_ERR_NOMEM if it cannot be had: split the individual range)
 *   loo_sum_out      [n_markers] the sum of loo over the individuals of the range that are not skipped
 *   unlinked_sum_out [n_markers] likewise.  Both are reduced on the device in ascending order of the individuals, without
 *                    atomics: the same bits on every call, and the sums of loo_out / unlinked_out added in that order
 *   n_contrib_out    [n_chrom] (int32) individuals of the range with a likelihood on that chromosome (not skipped)
 * Outputs are overwritten, not accumulated; a range split [a,b) + [b,c) adds up to [a,c) (sums to rounding, counts and rows
 * exactly).  Bad arguments (a NULL pointer other than the two rows, a range out of bounds) write nothing.
 * One pass: untied windows through the fast kernel's leave-one-out instantiation (likelihoods, then a backward pass without
 * rows that leaves the two ratios per marker), tied windows through the tied kernel without rows (likelihoods) and then the
 * same instantiation; a finish kernel takes the logarithms in place and reduces the columns.
 * Flags: CNF2_OUT_DEVICE (all seven output pointers are device pointers), CNF2_STATIC_JOBS, CNF2_FULL_SPILL and
 * CNF2_TIES_GENERAL as in cnf2_sweep_crossovers; CNF2_MERGE_MODES, CNF2_XPOSE, CNF2_FLUSH_TINY and the dosage flags are
 * ignored.  The call synchronises the context's stream once (the job list), also with CNF2_OUT_DEVICE. */
int cnf2_sweep_loo(cnf2_ctx *ctx, int ind_begin, int ind_end, double *factors_out, double *loglik_out,
                   double *loo_out, double *unlinked_out, double *loo_sum_out, double *unlinked_sum_out,
                   int32_t *n_contrib_out, uint32_t flags);
/*  cnf2_loo_rows        rows_out[mc][2] = (loo, unlinked) of cnf2_sweep_loo for one individual and chromosome, from the
 *                       store by brute force (one thread per state on slots 0, 1 and 2 with their cumulative scales): the
 *                       cross-check of the sweep's fused form. */
int cnf2_loo_rows(cnf2_ctx *ctx, int ind, int chrom, double *rows_out);

/* Origin sweep: from which grandparent does each of the individual's two alleles descend at every marker, and with what
 * probability?  In an F2 that is P(AA), P(AB), P(BA), P(BB), the quantity a QTL scan regresses on and the segregation check
 * of a cross.  For analysed individual i and marker m, with g = j*8 + lo as in cnf2_state_posterior and bit t of g the
 * meiosis of column t of cnf2_sweep_crossovers:
 *   gamma_i,m(g)    = sum_s w_s gamma_s,m(g) / sum_s w_s
 *   origin[i][m][k] = sum_g gamma(g) [ bit0(g) + 2 bit3(g) == k ]      k = 0..3
 *   bits[i][m][t]   = sum_g gamma(g) bit_t(g)                          t = 0..5
 * gamma_s,m and w_s are those of cnf2_sweep_place: gamma_s,m is alpha after the emission x beta, normalised within the mode,
 * w_s = exp(factors[s] - loglik) over the modes the dosage rows count (active, with a likelihood, not 40 log-units below the
 * total).  Ties, CNF2_NO_TIES and ignoreflag2 do not enter.  Each origin row sums to 1; bits[0] = origin[1] + origin[3],
 * bits[3] = origin[2] + origin[3].
 * THE FRAME IS ABSOLUTE, not relative to a phase the sweep chose: bit 0 = 1 means that the allele the individual has from
 * its first parent (pedigree column par[.][0]) descends from that parent's par[.][1], bit 0 = 0 from that parent's
 * par[.][0]; bit 3 says the same of the allele from the second parent (par[.][1]).  So k = 0 is "both alleles from the
 * parents' first parent", k = 3 "both from the parents' second parent" -- in an F2 whose F1 parents list line A first, AA
 * and BB -- and k = 1, 2 the two heterozygotes by the side that carries the second grandparent's allele.  Swapping the two
 * grandparents in a parent's pedigree entry swaps bit = 0 and bit = 1 of that side.  Bits 1, 2 (first parent's side) and 4,
 * 5 (second parent's side) are the grandparents' own meioses, labelled relative to each grandparent's phase: they carry
 * information only where the grandparents are heterozygous, and sit at 0.5 in a cross of inbred lines.
 *   factors_out / loglik_out  as cnf2_sweep: bit-equal (the same forward passes; tied windows from the tied kernel)
 *   origin_out      [n][n_markers][4] or NULL
 *   bits_out        [n][n_markers][6] or NULL; both all zero where the individual is skipped on the chromosome (no mode
 *                   with a likelihood), as the dosage rows are.  Rows that are not asked for, and host rows, live whole in
 *                   a buffer of the context (CNF2_ERR_NOMEM if it cannot be had: split the individual range)
 *   origin_sum_out  [n_markers][4] the sum of origin over the individuals of the range that are not skipped: the expected
 *                   class counts.  Reduced on the device in ascending order of the individuals, without atomics: the same
 *                   bits on every call, and the sum of origin_out added in that order
 *   n_contrib_out   [n_chrom] (int32) individuals of the range with a likelihood on that chromosome (not skipped)
 * Outputs are overwritten, not accumulated; a range split [a,b) + [b,c) adds up to [a,c) (sums to rounding, counts and rows
 * exactly).  Bad arguments (a NULL pointer other than the two rows, a range out of bounds) write nothing.
 * Posteriors at positions between markers: add a column without data there (alleles 0, sure 0, hw 0.5 in every row) -- the
 * map is Haldane, so the gaps compose exactly and the rows of the real markers do not change (origins.with_positions).
 * One pass: untied windows through the fast kernel's origin instantiation (likelihoods, then a backward pass without rows
 * that reduces eight masked sums of the state posterior per marker in the wave), tied windows through the tied kernel
 * without rows (likelihoods) and then the same instantiation; a finish kernel reduces the columns.  Uniform windows
 * (crosses of inbred lines) take the same instantiation.
 * Flags: CNF2_OUT_DEVICE (all six output pointers are device pointers), CNF2_STATIC_JOBS, CNF2_FULL_SPILL and
 * CNF2_TIES_GENERAL as in cnf2_sweep_loo; CNF2_MERGE_MODES, CNF2_XPOSE, CNF2_FLUSH_TINY, CNF2_ALL_STATES and the dosage
 * flags are ignored.  The call synchronises the context's stream once (the job list), also with CNF2_OUT_DEVICE. */
int cnf2_sweep_origins(cnf2_ctx *ctx, int ind_begin, int ind_end, double *factors_out, double *loglik_out,
                       double *origin_out, double *bits_out, double *origin_sum_out, int32_t *n_contrib_out,
                       uint32_t flags);
/*  cnf2_origin_rows     rows_out[mc][10] = origin[4], bits[6] of cnf2_sweep_origins for one individual and chromosome, from
 *                       the store by brute force (one thread per state on slots 1 and 2, every mode normalised on its own
 *                       and weighted with exp(factors[s] - loglik)): the cross-check of the sweep's fused form. */
int cnf2_origin_rows(cnf2_ctx *ctx, int ind, int chrom, double *rows_out);

/* Descent rows: from which grandparent AND which of that grandparent's two strands does each of an individual's alleles
 * descend, per marker.  The origin rows answer the first half; the joint of a parent's meiosis with the meiosis of the
 * grandparent it selected cannot be had from the marginals bits[], so it is summed here.  gamma_i,m(g), the modes, the
 * weights w_s, the 40-log-unit rule and the renormalisation are exactly those of cnf2_sweep_origins.  Per side a class
 * k = 0..3:
 *   first parent's side    k = 2 bit0(g) + (bit0(g) ? bit2(g) : bit1(g))
 *   second parent's side   k = 2 bit3(g) + (bit3(g) ? bit5(g) : bit4(g))
 *   descent[i][m][0..3] = sum_g gamma(g) [ first side's class == k ],  descent[i][m][4..7] the same of the second side
 * A row is 64 bytes; each side sums to 1; a skipped individual's rows are all zero.
 * Class 2 w + b reads "the allele from this parent descends from that parent's par[.][w], strand b of that grandparent".
 * THE STRAND IS LABELLED BY THE GRANDPARENT'S OWN RECORD, that is by its stored allele order and hw: with hw near 1 where a
 * heterozygous grandparent's strand 0 carries the first stored allele and near 0 where it carries the second, b is that
 * strand; with the two values exchanged along the chromosome b names the other strand, and the two strand cells of that
 * grandparent change places.  Where a grandparent is homozygous (hw 0.5 in a cross of inbred lines) its two strand cells
 * are equal.  Identities with cnf2_sweep_origins: d0 + d1 = 1 - bits[0], d2 + d3 = bits[0], d4 + d5 = 1 - bits[3],
 * d6 + d7 = bits[3].
 *   factors_out / loglik_out  as cnf2_sweep: bit-equal
 *   descent_out     [n][n_markers][8] or NULL.  Rows that are not asked for, and host rows, live whole in a buffer of the
 *                   context of their own (CNF2_ERR_NOMEM if it cannot be had: split the individual range)
 *   n_contrib_out   [n_chrom] (int32) individuals of the range with a likelihood on that chromosome (not skipped)
 * Outputs are overwritten; a range split gives the same rows and counts.  Bad arguments (a NULL pointer other than
 * descent_out, a range out of bounds) write nothing.  Positions between markers: as for cnf2_sweep_origins.
 * Routing, tied windows and flags (CNF2_OUT_DEVICE: all four output pointers are device pointers; CNF2_STATIC_JOBS,
 * CNF2_FULL_SPILL, CNF2_TIES_GENERAL) are cnf2_sweep_origins'; the fast kernel's descent instantiation reduces the eight
 * values of a marker together by halving and eight lanes store the row.  Uniform windows take the same instantiation. */
int cnf2_sweep_descent(cnf2_ctx *ctx, int ind_begin, int ind_end, double *factors_out, double *loglik_out,
                       double *descent_out, int32_t *n_contrib_out, uint32_t flags);
/*  cnf2_descent_rows    rows_out[mc][8] = the descent row of cnf2_sweep_descent for one individual and chromosome, from the
 *                       store by brute force as cnf2_origin_rows: the cross-check of the sweep's fused form. */
int cnf2_descent_rows(cnf2_ctx *ctx, int ind, int chrom, double *rows_out);

/* Pair posteriors: the joint origin classes of two markers of one chromosome.  The product of two origin rows is the joint
 * distribution only across chromosomes; on one chain the two loci are linked.  For an analysed individual i, a chromosome
 * and two selected markers j < k of it, with the classes, the frame, the modes and the weights w_s of cnf2_sweep_origins:
 *   J_s(u, v)  = sum_(g, g') [cls g = u] [cls g' = v] A_s,j(g) Phi_s(j -> k)(g, g') B_s,k(g'),     cls g = bit0(g) + 2 bit3(g)
 *   Phi_s(j -> k) = prod_(m = j+1 .. k) T_(m-1 -> m) diag(e_s,m)
 *   joint[i][p][4 u + v] = sum_s w_s J_s(u, v) / Z_s / sum_s w_s,     Z_s = sum_(u, v) J_s(u, v)
 * A = alpha after the emission, B = beta, T the transition of the gap (rate rho.y on bits 0 and 3, rho.x on the others; a
 * gap of rate 0 is the identity), e the path-free emission of cnf2_emission.  A mode with Z_s not above 0 is left out of the
 * pair and the weights renormalised.  Every row sums to 1; its margins are the origin rows of the two markers; for adjacent
 * markers the mass with u & 1 != v & 1 is xi[j][0] of cnf2_sweep_crossovers and that with u >> 1 != v >> 1 is xi[j][3].
 * Ties, CNF2_NO_TIES and ignoreflag2 do not enter.
 *   sel [n_sel]     cnf2_qtl_scan2's selection: 2 .. 4096 strictly ascending marker indices.  The pairs are those on one
 *                   chromosome, in ascending first, then ascending second locus: cnf2_linked_pairs lists them as indices into
 *                   sel (pairs_out [n_pairs][2] int32 or NULL; n_pairs_out their number, 0 where no two loci are linked)
 *   factors_out / loglik_out  as cnf2_sweep: bit-equal
 *   joint_out       [n][n_pairs][16] or NULL; all zero where the individual is skipped on the chromosome.  Rows that are not
 *                   asked for, and host rows, live whole in a buffer of the context (CNF2_ERR_NOMEM: split the range)
 *   joint_sum_out   [n_pairs][16] the rows added over the individuals in ascending order, without atomics
 *   n_contrib_out   [n_chrom] (int32) individuals of the range with a likelihood on that chromosome
 * Outputs are overwritten; a range split adds up (rows and counts exactly, sums to rounding).  A NULL pointer other than
 * joint_out, a range out of bounds, everything cnf2_qtl_scan2 refuses in sel and a selection without a linked pair return
 * CNF2_ERR_ARG and write nothing.
 * In batches sized to the free memory (cnf2_set_batch_jobs caps them; the result does not depend on it, to the bit): the
 * turn-scan instantiation of the sweep leaves alpha and beta of every marker in the batch buffer, then a wave per
 * (individual x chromosome, first locus) walks four class-restricted copies of alpha to the chromosome's last selected
 * marker and forms a row at every selected one.  A call gives the same bits every time.
 * Flags: CNF2_OUT_DEVICE (the five outputs are device pointers), CNF2_STATIC_JOBS and CNF2_TIES_GENERAL as in
 * cnf2_sweep_origins.  The call synchronises the context's stream (the job list and the selection). */
int cnf2_linked_pairs(cnf2_ctx *ctx, int n_sel, const int32_t *sel, int32_t *pairs_out, int32_t *n_pairs_out);
int cnf2_sweep_pairs(cnf2_ctx *ctx, int ind_begin, int ind_end, int n_sel, const int32_t *sel, double *factors_out,
                     double *loglik_out, double *joint_out, double *joint_sum_out, int32_t *n_contrib_out, uint32_t flags);
/*  cnf2_pair_rows       rows_out[S (S - 1) / 2][16] = the rows of cnf2_sweep_pairs for one individual and the S markers of sel
 *                       on one chromosome (nothing is written where S < 2), from the store by brute force: one block per
 *                       first locus, one thread per state, the explicit 64 x 64 transition. */
int cnf2_pair_rows(cnf2_ctx *ctx, int ind, int chrom, int n_sel, const int32_t *sel, double *rows_out);

/* QTL scan: where on the map does a trait sit?  Haley-Knott regression of phenotypes on the origin rows of
 * cnf2_sweep_origins, at every marker, for the observed phenotypes and for permuted ones (the genome-wide threshold of a
 * peak is a quantile of the permutations' maxima).  One definition for this header, cnf2freq_amd/csrc/cnf2_qtl.h (the small
 * algebra, shared by host and device code), the kernels and tests/qtl_reference.py:
 *   origin [n][M][4]   the origin rows; an individual whose row at a chromosome's first marker is all zero is skipped there
 *   pheno  [n][T]      phenotypes;  use [n] (uint8, NULL = all ones) the individuals to use;  cov [n][K], 0 <= K <= 8, fixed
 *                      effects.  pheno and cov must be finite where use is set
 *   perm   [P][n]      (int32) permutations of 0 .. n-1 that give used individuals used ones
 * Per chromosome c: c_i = use[i] and not skipped, n_c = sum c_i, null design X0 = [c, c z_1 .. c z_K], full design X0 plus
 * (c a, c d) with a_i = origin[i][m][3] - origin[i][m][0], d_i = origin[i][m][1] + origin[i][m][2] at marker m.
 * Phenotype columns: R = T (1 + P); column (0, t) is pheno[.][t], column (1 + p, t) is pheno[perm[p][i]][t] at individual
 * i -- covariates, use and the origin rows stay with i.  Whether raw values or residuals of the null model are permuted is
 * the caller's choice (cnf2freq_amd/qtl.py permutes residuals: Freedman-Lane).
 *   S11 = X0'X0, b0 = X0'y, RSS0 = sum c y^2 - b0' S11^-1 b0                                   per chromosome (and column)
 *   S21 = A'X0, S22 = A'A, G = S21 S11^-1, W = S22 - G S21' (2 x 2)                            per marker
 *   v = A'y - G b0, dRSS = v' W^-1 v, lod = (n_c / 2) log10(RSS0 / (RSS0 - dRSS)), coef = W^-1 v   per marker and column
 * Rank rule: W is factored in the order a, d; a column is dropped when its raw diagonal (S22) is 0 or its pivot is below
 * 1e-8 times that diagonal; CNF2_QTL_ADDITIVE always drops d.  rank[m] (0, 1, 2) depends on the design only.  A dropped
 * column's coefficient is NaN; rank 0 gives lod = 0 exactly.  A chromosome with n_c < K + 4, or whose X0 has no Cholesky
 * factor, is not scanned: rank 0, lod 0 and coef NaN at its markers.  A column with RSS0 <= 0 gives lod 0 and coef NaN.  dRSS
 * is clamped to [0, RSS0 (1 - 2^-52)]: a LOD is finite and not negative.
 * Units and offsets: with the intercept in X0 the model does not depend on them -- under y -> alpha y + beta and
 * z_k -> gamma_k z_k + delta_k LOD, rank, n_c and perm_max stay, coef scales with alpha and RSS0 with alpha^2 -- and neither do
 * the results, here and in the three scans below: every call subtracts from each trait and each covariate column of X0 its
 * mean over the used individuals before any sum is formed (a constant column becomes exactly 0), so no sum cancels a large
 * mean against a small spread.  An interaction column of cnf2_qtl_scanx is the product with the covariate as given.
 *   lod_out      [T][M]       coef_out [T][M][2] (additive, dominance effect)       rank_out [M] (int32)
 *   rss0_out     [T][C]       n_used_out [C] (int32) n_c
 *   perm_max_out [P][T][C]    per permutation, trait and chromosome the largest LOD; NULL exactly when P = 0.  The maximum
 *                             over C is the genome-wide statistic
 * cnf2_qtl_scan is the scan alone on rows the caller has: a host array, staged whole (CNF2_ERR_NOMEM if that fails), or with
 * CNF2_QTL_ORIGIN_DEVICE device memory read in place -- repeated scans (other traits, the permutations, grid positions from
 * origins.with_positions) then cost the scan only.  n is the number of rows; M and the chromosomes are the uploaded map's.
 * With CNF2_QTL_ORIGIN_DEVICE and origin NULL the rows are those the context's last cnf2_sweep_qtl left in its buffer (n must
 * be that call's; CNF2_ERR_STATE when a map, rows or a pedigree have been uploaded or another call has used the buffer
 * since): further traits and the permutations of a cross without a second sweep and without a device allocation of the
 * caller's.
 * cnf2_sweep_qtl sweeps the range as cnf2_sweep_origins does, with the rows in the context's buffer, and scans them:
 * factors_out / loglik_out are bit-equal to cnf2_sweep, CNF2_STATIC_JOBS, CNF2_FULL_SPILL and CNF2_TIES_GENERAL act as there,
 * n = ind_end - ind_begin >= 1.  A regression is NOT additive over range splits: scan the individuals of a cross in one call.
 * pheno, use, cov and perm are host pointers in both calls, also with CNF2_OUT_DEVICE, which makes the outputs (and factors_out
 * / loglik_out) device pointers.  Outputs are overwritten.  Bad arguments -- a NULL pointer, K or P out of range, a value that
 * is used and not finite, a row of perm that is no permutation or moves an unused individual -- return CNF2_ERR_ARG and write
 * nothing.  Both calls synchronise the context's stream, also with CNF2_OUT_DEVICE.
 * Launches: per call the design (c_i, S11 and its factor per chromosome; S21, S22, G and the pivots per marker, sums over
 * the individuals in ascending order); per tile of columns the column image Y[n][tile], b0 / RSS0, and the product
 * C[(m, a|d)][r] = sum_i A(m, i) Y(i, r) on the f64 matrix cores with the epilogue in registers; a finish kernel reduces the
 * permutations' maxima.  No atomics: a call gives the same bits every time.  The tile holds as many columns as keep the image
 * under 1 GB (4096 at most); cnf2_set_qtl_columns caps it (0 = no cap) so that several tiles can be exercised at test sizes.
 * The result does not depend on that cap or on cnf2_set_batch_jobs, to the bit. */
int cnf2_qtl_scan(cnf2_ctx *ctx, int n, const double *origin, int n_traits, const double *pheno, const uint8_t *use,
                  int n_cov, const double *cov, int n_perm, const int32_t *perm, double *lod_out, double *coef_out,
                  int32_t *rank_out, double *rss0_out, int32_t *n_used_out, double *perm_max_out, uint32_t flags);
int cnf2_sweep_qtl(cnf2_ctx *ctx, int ind_begin, int ind_end, double *factors_out, double *loglik_out, int n_traits,
                   const double *pheno, const uint8_t *use, int n_cov, const double *cov, int n_perm, const int32_t *perm,
                   double *lod_out, double *coef_out, int32_t *rank_out, double *rss0_out, int32_t *n_used_out,
                   double *perm_max_out, uint32_t flags);
int cnf2_set_qtl_columns(cnf2_ctx *ctx, int cap);

/* Two-QTL pair scan: is there a second locus, and do two loci interact?  For every pair (j, k), j < k, of the selected
 * markers sel[L] (strictly ascending, 2 <= L <= 4096; locus 1 = sel[j] on chromosome c1, locus 2 = sel[k] on c2) three nested
 * Haley-Knott designs are fitted to every phenotype column, observed and permuted.  One definition for this header,
 * cnf2freq_amd/csrc/cnf2_qtl2.h (host and device), the kernels and tests/qtl2_reference.py.  origin, pheno, use, cov (K <= 6
 * here: the widest design has 1 + K + 8 <= 15 columns) and perm are cnf2_qtl_scan's.
 *   mask      c_i = use[i], and the row at c1's first marker is not all zero, and the same at c2's;  n_c = sum c_i.  It
 *             depends on (c1, c2) only
 *   null      X0 = [c, c z_1 .. c z_K]
 *   additive  X0, a1, d1, a2, d2                              with CNF2_QTL_ADDITIVE: X0, a1, a2
 *   full      additive, then a1 a2, a1 d2, d1 a2, d1 d2       with CNF2_QTL_ADDITIVE: additive, then a1 a2
 * with a = o[3] - o[0], d = o[1] + o[2] at each locus.  The additive design is linear in each locus's indicators, so the
 * marginal rows give its exact Haley-Knott regressors and it is fitted for every pair.  The interaction regressors are
 * E[a1 a2 | data] and the other products: the jobs are individual x chromosome and the posterior factorises across
 * chromosomes, so for c1 != c2 a product's expectation is the product of the marginal expectations, exactly.  For c1 = c2 it
 * needs the joint posterior of two loci on one chain, which the origin rows do not hold: this call fits the full model only
 * for pairs on different chromosomes, and a pair on one chromosome reports lod_full = NaN and rank_full = -1.
 * cnf2_qtl_scan2_linked (below) takes that joint posterior from cnf2_sweep_pairs and fits every pair.
 * One factorisation gives all three: the normal matrix of [full design | y] under the mask, one sequential Cholesky in the
 * column order above; an added column is dropped (pivot 0) when its raw diagonal is 0 or its pivot is below 1e-8 times its
 * raw diagonal.  With w = L^-1 X'y over the kept columns
 *   RSS0 = sum c y^2 - sum_{X0} w^2,  RSS_add = RSS0 - sum_{kept additive} w^2,  RSS_full = RSS_add - sum_{kept interaction} w^2
 *   lod_x = (n_c / 2) log10(RSS0 / RSS_x), the cumulative reduction clamped to [0, RSS0 (1 - 2^-52)]: every LOD is finite and
 *   not negative, and lod_full >= lod_add.
 * rank_add (0 .. 4; 0 .. 2 additive) counts the kept additive columns, rank_full (0 .. 8; 0 .. 3) all kept added columns;
 * they depend on the design only, and rank 0 gives LOD 0 exactly.  A chromosome pair with n_c < K + 10, or whose X0 has no
 * Cholesky factor, is not scanned: ranks 0, LODs 0, rss0 0 (lod_full stays NaN and rank_full -1 on one chromosome).  A
 * column with RSS0 <= 0 gives LOD 0.
 *   lod_add_out, lod_full_out [T][L][L]    rank_add_out, rank_full_out [L][L] (int32)
 *       only cells j < k carry results; every other cell is NaN / -1
 *   rss0_out [T][C][C], n_used_out [C][C] (int32)    symmetric, filled for every chromosome pair, the diagonal included
 *   perm_max_out [P][T][3]    per permutation and trait the maxima over all pairs of lod_add, and over the pairs with
 *       c1 != c2 of lod_full and of lod_full - lod_add; 0 where no pair qualifies; NULL exactly when P = 0
 * CNF2_QTL_ADDITIVE, CNF2_QTL_ORIGIN_DEVICE (also with origin NULL: the rows the last cnf2_sweep_qtl left in the context,
 * CNF2_ERR_STATE as for cnf2_qtl_scan) and CNF2_OUT_DEVICE act as for cnf2_qtl_scan.  Device rows are read in place and the
 * call does not invalidate the context's rows: cnf2_qtl_scan and cnf2_qtl_scan2 can follow one sweep in any order.  sel and
 * the phenotype side are host pointers.  Everything cnf2_qtl_scan refuses, K > 6, and a sel that is unsorted, repeats a
 * marker or leaves the map return CNF2_ERR_ARG and write nothing; an allocation that fails returns CNF2_ERR_NOMEM before
 * anything is written.
 * Launches: the masks; per tile of columns the column image (as cnf2_qtl_scan), per chromosome pair n_c, sum c y^2 and RSS0,
 * and the pair kernel, a batched small SYRK on the f64 matrix cores -- a wave owns a pair, forms the design entries in
 * registers from the two origin rows, accumulates X'X and X'Y over the individuals in ascending order, factors the 16 x 16
 * tile once and lets one lane per column do the substitution; a finish kernel reduces the permutations' maxima.  No atomics
 * and no split of the individuals: a call gives the same bits every time, for every column cap (cnf2_set_qtl2_columns,
 * 0 = no cap; the tile keeps the image under 1 GB and the maxima under 256 MB) and from host or device rows. */
int cnf2_qtl_scan2(cnf2_ctx *ctx, int n, const double *origin, int n_sel, const int32_t *sel, int n_traits,
                   const double *pheno, const uint8_t *use, int n_cov, const double *cov, int n_perm, const int32_t *perm,
                   double *lod_add_out, double *lod_full_out, int32_t *rank_add_out, int32_t *rank_full_out,
                   double *rss0_out, int32_t *n_used_out, double *perm_max_out, uint32_t flags);
int cnf2_set_qtl2_columns(cnf2_ctx *ctx, int cap);
/* cnf2_qtl_scan2_linked: cnf2_qtl_scan2 with the full (epistatic) model on the pairs of one chromosome too.  joint
 * [n][n_pairs][16] holds the rows of cnf2_sweep_pairs for the same sel and the same individuals (a host array, staged whole,
 * or device memory with CNF2_QTL_JOINT_DEVICE; it is not read where sel has no two loci on one chromosome, and must not be
 * NULL).  For a pair on one chromosome the full design's interaction columns are the expectations of the products under the
 * pair's row J[4 u + v]:
 *   E[a1 a2] = J33 - J30 - J03 + J00      E[a1 d2] = (J31 + J32) - (J01 + J02)
 *   E[d1 a2] = (J13 + J23) - (J10 + J20)  E[d1 d2] = J11 + J12 + J21 + J22          (CNF2_QTL_ADDITIVE: E[a1 a2] alone)
 * the additive columns come from the origin rows as ever, and the mask, the rank rule, the factorisation, the clamps and the
 * cell are cnf2_qtl_scan2's: such a pair reports lod_full and rank_full like any other.  Every other output -- lod_add,
 * rank_add, rss0, n_used, and lod_full / rank_full of the pairs on two chromosomes -- is cnf2_qtl_scan2's to the bit, and
 * perm_max[..][1] and [..][2] run over all pairs.  Arguments, flags, refusals and launches are cnf2_qtl_scan2's; the lane that
 * there forms a product from two origin rows reads four cells of the pair's 128-byte row here. */
int cnf2_qtl_scan2_linked(cnf2_ctx *ctx, int n, const double *origin, const double *joint, int n_sel, const int32_t *sel,
                          int n_traits, const double *pheno, const uint8_t *use, int n_cov, const double *cov, int n_perm,
                          const int32_t *perm, double *lod_add_out, double *lod_full_out, int32_t *rank_add_out,
                          int32_t *rank_full_out, double *rss0_out, int32_t *n_used_out, double *perm_max_out, uint32_t flags);

/* Extended single-locus scan: does a locus act differently by the parent it came from, and does its effect depend on a
 * covariate?  Per marker three nested Haley-Knott designs are fitted to every phenotype column, observed and permuted.  One
 * definition for this header, cnf2freq_amd/csrc/cnf2_qtlx.h (host and device), the kernels and tests/qtlx_reference.py.
 * origin, pheno, use, cov, perm, the mask c of a chromosome, n_c and the columns R = T (1 + P) are cnf2_qtl_scan's.  The
 * interactive covariates are the first n_int (= Ki, 0 <= Ki <= K) columns of cov.
 *   effects   a = o[3] - o[0];  d = o[1] + o[2] (not with CNF2_QTL_ADDITIVE);  i = o[1] - o[2] (only with CNF2_QTL_IMPRINT):
 *             o[1] is the heterozygote whose allele from the first parent descends from that parent's second grandparent,
 *             o[2] the same of the second parent, so i is the classical imprinting regressor of line-cross analysis.
 *             ne = 1, 2 or 3 of them
 *   null      X0 = [c, c z_1 .. c z_K]
 *   stage 0   "Mendelian"    a, d
 *   stage 1   "imprinting"   i
 *   stage 2   "interaction"  for k = 1 .. Ki: a z_k, d z_k, i z_k (those effects that are present)
 * The width W = 1 + K + ne (1 + Ki) must be at most 15 (the 16 rows of one matrix instruction less a padding row).
 * One factorisation gives every stage: the normal matrix of [design | y] under the mask, one sequential Cholesky in the
 * column order above; a column of X0 needs a positive pivot, an added column is dropped (pivot 0) when its raw diagonal is 0
 * or its pivot is below 1e-8 times its raw diagonal.  With w = L^-1 X'y over the kept columns
 *   RSS0 = sum c y^2 - sum_{X0} w^2,  lod[s] = (n_c / 2) log10(RSS0 / (RSS0 - sum of w^2 over the kept columns of stages 0 .. s))
 * with the cumulative reduction clamped to [0, RSS0 (1 - 2^-52)]: lod[0] <= lod[1] <= lod[2], all finite and not negative; a
 * stage without columns repeats the previous value exactly.  lod[1] - lod[0] is the imprinting test (the (a, d, i) against
 * the Mendelian model), lod[2] - lod[1] the interaction test.  rank[s] is the cumulative count of kept added columns; it
 * depends on the design only and rank 0 gives LOD 0 exactly.  coef holds the effects of the FULL model -- back-substitution
 * on the kept added columns -- in the column order above, NaN for a dropped column; the effects of a smaller model are had
 * by a call with n_int = 0 and / or without CNF2_QTL_IMPRINT.  A chromosome with n_c < W + 1, or whose X0 has no Cholesky
 * factor, is not scanned: ranks 0, LODs 0, coef NaN, rss0 0.  A column with RSS0 <= 0 gives LODs 0 and coef NaN.
 * The rank rule is relative to a column's own length.  In a cross whose two heterozygotes cannot be told apart (an F2 of
 * inbred lines: both F1 parents carry the same two lines) o[1] - o[2] is exactly 0 or the sweep's rounding noise; a noise
 * column that is not exactly 0 is kept, with an effect of the order of 1e16 and the LOD of a random regressor.  The imprinting
 * effect is for crosses whose founders are outbred; do not set CNF2_QTL_IMPRINT elsewhere.
 *   lod_out      [T][M][3]    coef_out [T][M][ne (1 + Ki)]    rank_out [M][3] (int32)
 *   rss0_out     [T][C]       n_used_out [C] (int32) n_c
 *   perm_max_out [P][T][C][5] per permutation, trait and chromosome the maxima over the chromosome's markers of lod[0],
 *                             lod[1], lod[2], lod[1] - lod[0] and lod[2] - lod[1] (each difference taken per cell); NULL
 *                             exactly when P = 0
 * CNF2_QTL_ADDITIVE, CNF2_QTL_ORIGIN_DEVICE (also with origin NULL: the rows the last cnf2_sweep_qtl left in the context,
 * CNF2_ERR_STATE as for cnf2_qtl_scan) and CNF2_OUT_DEVICE act as for cnf2_qtl_scan2: device rows are read in place and the
 * call leaves the context's rows valid.  Everything cnf2_qtl_scan refuses, n_int outside 0 .. K and W > 15 return
 * CNF2_ERR_ARG and write nothing; an allocation that fails returns CNF2_ERR_NOMEM before anything is written.
 * Launches: the masks; per tile of columns the column image (as cnf2_qtl_scan), per chromosome n_c, sum c y^2 and RSS0, and
 * the marker kernel, a batched small SYRK on the f64 matrix cores -- a wave owns a marker, forms the design entries in
 * registers from the origin row and the covariates, accumulates X'X and X'Y over the individuals in ascending order, factors
 * the 16 x 16 tile once and lets one lane per column do the substitutions; the waves of a block take adjacent markers of
 * one chromosome; a finish kernel reduces the permutations' maxima per chromosome.  No atomics and no split of the
 * individuals: a call gives the same bits every time, for every column cap (cnf2_set_qtlx_columns, 0 = no cap; the tile
 * keeps the image under 1 GB and the maxima under 256 MB) and from host or device rows. */
int cnf2_qtl_scanx(cnf2_ctx *ctx, int n, const double *origin, int n_traits, const double *pheno, const uint8_t *use,
                   int n_cov, const double *cov, int n_int, int n_perm, const int32_t *perm, double *lod_out,
                   double *coef_out, int32_t *rank_out, double *rss0_out, int32_t *n_used_out, double *perm_max_out,
                   uint32_t flags);
int cnf2_set_qtlx_columns(cnf2_ctx *ctx, int cap);

/* Cofactor scan: composite interval mapping.  Is there a further QTL given the ones already found, and what does the
 * multiple-QTL model say about each of them?  Every marker is fitted together with the cofactors -- loci found before --
 * and each cofactor is left out of the design while the scan passes through its own window.  One definition for this
 * header, cnf2freq_amd/csrc/cnf2_qtlcof.h (host and device), the kernels and tests/qtlcof_reference.py.
 * origin, pheno, use, cov, perm and the columns R = T (1 + P) are cnf2_qtl_scan's.  n_cof = Q >= 0 and cof[Q], excl_lo[Q],
 * excl_hi[Q] (int32, host; NULL only with Q = 0): cof holds marker indices, strictly ascending; cofactor q is left out of the
 * design at the markers excl_lo[q] <= m <= excl_hi[q].  The range must lie on the cofactor's chromosome and contain cof[q];
 * ranges of different cofactors may overlap.
 *   effects   per locus a = o[3] - o[0] and d = o[1] + o[2] (a only with CNF2_QTL_ADDITIVE): ne = 1 or 2, for the cofactors
 *             and the tested marker alike.  The additive model is linear in each locus's indicators, so the marginal origin
 *             rows are its exact Haley-Knott regressors: a cofactor on the tested marker's own chromosome is exact
 *   width     W = 1 + K + ne Q + ne must be at most 15 (cnf2_qtl_scanx's bound, for its reason): six loci with dominance,
 *             thirteen in the additive model
 *   mask      c_i = use[i], and i is not skipped on the tested chromosome, and i is not skipped on the chromosome of any
 *             cofactor, left out here or not: n_c and the mask depend on the chromosome only
 *   design    X0 = [c, c z_1 .. c z_K], then the cofactors' columns in the order of cof with the left-out ones skipped, then
 *             the marker's a, d
 * One factorisation: the normal matrix of [design | y] under the mask, one sequential Cholesky in that column order; a column
 * of X0 needs a positive pivot, every later column is dropped (pivot 0) when its raw diagonal is 0 or its pivot is below 1e-8
 * times its raw diagonal.  With w = L^-1 X'y over the kept columns and LOD(s) = (n_c / 2) log10(RSS0 / (RSS0 - s)), s clamped
 * to [0, RSS0 (1 - 2^-52)]:
 *   RSS0 = sum c y^2 - sum_{X0} w^2
 *   lod_base[m] = LOD(sum of w^2 over the kept cofactor columns): the cofactors against X0
 *   lod[m]      = LOD(sum of w^2 over the kept cofactor and marker columns) - lod_base[m]: the CONDITIONAL LOD of the marker's
 *                 kept effects against X0 + cofactors; finite, not negative, exactly 0 where rank[m] = 0
 *   rank[m] = the kept effects of the marker, rank_cof[m] = the kept cofactor columns; both depend on the design only
 *   coef[t][m][ne] = the marker's effects in the full model, NaN for a dropped one
 * A chromosome with n_c < W + 1 (W the full width, whatever is left out), or whose X0 has no Cholesky factor, is not scanned:
 * ranks 0, LODs 0, coef NaN, rss0 0.  A column with RSS0 <= 0 gives LODs 0 and coef NaN.
 * Reading a multiple-QTL fit off the scan: at m = cof[q] the marker stands in for cofactor q.  With ranges that leave out
 * only the cofactor itself at its own marker (excl_lo[q] = excl_hi[q] = cof[q]), lod[cof[q]] is the drop-one LOD of locus q in
 * the Q-locus model, lod_base + lod there is the full model's LOD (the same at every cofactor) and coef there holds locus
 * q's effects in it.
 *   lod_out [T][M]   lod_base_out [T][M]   coef_out [T][M][ne]   rank_out [M] (int32)   rank_cof_out [M] (int32)
 *   rss0_out [T][C]  n_used_out [C] (int32) n_c
 *   perm_max_out [P][T][C]  per permutation, trait and chromosome the largest conditional LOD over the chromosome's markers
 *                           that lie in NO exclusion range (inside a range the value is a drop-one statistic of a known
 *                           locus, not a candidate); 0 where a chromosome has no such marker; NULL exactly when P = 0
 * CNF2_QTL_ADDITIVE, CNF2_QTL_ORIGIN_DEVICE (also with origin NULL: the rows the last cnf2_sweep_qtl left in the context,
 * CNF2_ERR_STATE as for cnf2_qtl_scan) and CNF2_OUT_DEVICE act as for cnf2_qtl_scanx: device rows are read in place and the
 * call leaves the context's rows valid.  Everything cnf2_qtl_scan refuses, W > 15, CNF2_QTL_IMPRINT, a cof that is unsorted,
 * repeated or off the map, and a range that leaves its chromosome or misses its cofactor return CNF2_ERR_ARG and write
 * nothing; an allocation that fails returns CNF2_ERR_NOMEM before anything is written.
 * Launches: the masks; the cofactor columns [n][ne Q], once; per tile of columns the column image (as cnf2_qtl_scan), per
 * chromosome n_c, sum c y^2 and RSS0, and the marker kernel, cnf2_qtl_scanx's batched small SYRK on the f64 matrix cores with
 * this design -- a left-out cofactor's columns are fed as exact zeros, so the column order is the same at every marker; a
 * finish kernel reduces the permutations' maxima per chromosome.  No atomics and no split of the individuals: a call gives
 * the same bits every time, for every column cap (cnf2_set_qtlcof_columns, 0 = no cap; the tile keeps the image under 1 GB
 * and the maxima under 256 MB), from host or device rows and into host or device outputs. */
int cnf2_qtl_scan_cof(cnf2_ctx *ctx, int n, const double *origin, int n_traits, const double *pheno, const uint8_t *use,
                      int n_cov, const double *cov, int n_cof, const int32_t *cof, const int32_t *excl_lo,
                      const int32_t *excl_hi, int n_perm, const int32_t *perm, double *lod_out, double *lod_base_out,
                      double *coef_out, int32_t *rank_out, int32_t *rank_cof_out, double *rss0_out, int32_t *n_used_out,
                      double *perm_max_out, uint32_t flags);
int cnf2_set_qtlcof_columns(cnf2_ctx *ctx, int cap);
/* rows_out[n_sel][n][4] (host) = the origin rows that the last cnf2_sweep_qtl left in the context, at the markers sel[n_sel]:
 * what a caller needs of them on the host, e.g. the cofactors' columns for the null model whose residuals a permutation test
 * of the cofactor scan permutes.  CNF2_ERR_STATE where the context holds no such rows of n individuals; the rows stay valid. */
int cnf2_qtl_kept_rows(cnf2_ctx *ctx, int n, int n_sel, const int32_t *sel, double *rows_out);

/* Kinship from the origin rows, as raw sums: the first half of a polygenic (mixed-model) scan, whose second half is the column
 * scan below.  origin[n][M][4] are cnf2_qtl_scan's rows -- a host array, staged whole, or with CNF2_QTL_ORIGIN_DEVICE a
 * device pointer read in place, NULL for the rows the last cnf2_sweep_qtl left in the context (CNF2_ERR_STATE as there; the
 * call leaves them valid).  With a_i(m) = o[i][m][3] - o[i][m][0], the additive line-origin score in -1 .. 1,
 *   sum_out[i][j] = sum over the markers m of the chromosomes chrom_begin .. chrom_end-1 of a_i(m) a_j(m)
 * and *n_markers_out is the number M' of those markers.  An all-zero row (an individual the sweep skipped on the chromosome)
 * contributes 0.  The kinship itself is the caller's: K = (1 + S / M') / 2, which is R/qtl2's allele-probability kinship for
 * two founder lines; leaving a chromosome out is then a subtraction of two calls' sums and counts.  With CNF2_OUT_DEVICE
 * sum_out and n_markers_out are device pointers.  n outside 1 .. 46340, an empty or misplaced chromosome range and a NULL
 * pointer return CNF2_ERR_ARG and write nothing; an allocation that fails returns CNF2_ERR_NOMEM before anything is written.
 * Launches: a pack kernel writes the image a[markers][n] (8 bytes per entry, zero-padded to whole tiles); the product is a
 * SYRK over the markers on the f64 matrix cores, 128 x 128 output tiles on or below the diagonal fed through LDS panels,
 * the mirror written from the same accumulator: sum_out[i][j] and sum_out[j][i] are the same bits.  No atomics; the markers
 * are summed in ascending order.  Where the lower triangle has fewer than 128 tiles (n <= 1920) and the range more than 256
 * markers, every chunk of 256 markers is summed from zero and a finish kernel adds the chunks in ascending order: which of
 * the two forms runs depends on n and M' alone, so a call gives the same bits every time, on every machine, from host or
 * device rows and into host or device outputs. */
int cnf2_kinship_sums(cnf2_ctx *ctx, int n, const double *origin, int chrom_begin, int chrom_end,
                      double *sum_out /* [n][n] */, int32_t *n_markers_out, uint32_t flags);

/* The Haley-Knott product on prepared columns: ordinary least squares of every phenotype column on
 * [x0, scale_i reg(i, m, 0 .. ne-1)] at each marker m of one block of n_mark markers.  It is cnf2_qtl_scan with four
 * differences: there is no implicit intercept and no centring -- x0[n][nx], 1 <= nx <= 9, is the whole null design as
 * given; the regressors reg[n][n_mark][ne], ne = 1 or 2, are doubles, not origin rows; scale[n] (NULL: ones) multiplies
 * the regressor rows on the fly; and a call is one block of markers -- no map, no masks, all n rows used, one rss0 per
 * trait and one maximum per permutation and trait.  After rotation by a kinship's eigenvectors the big operand U'[a, d] is
 * the same for every trait while the whitening weights depend on the trait's heritability: with scale the big array is read
 * in place once per trait and never rewritten.
 * Phenotype columns are cnf2_qtl_scan's: column (0, t) is pheno[i][t], column (1 + p, t) is pheno[perm[p][i]][t]; every row
 * of perm[n_perm][n] is a permutation of 0 .. n-1.  Every decision about a cell is cnf2freq_amd/csrc/cnf2_qtl.h's, with
 * n_c = n: the rank rule and its pivot threshold 1e-8 (the second regressor is tested after the first; with ne = 1 it is
 * the additive model's dropped column), NaN in coef_out for a dropped column, dRSS clamped to [0, RSS0 (1 - 2^-52)],
 * lod = (n / 2) log10(RSS0 / (RSS0 - dRSS)), lod 0 and coef NaN for a column with RSS0 = 0, and "not scanned" (lod 0, coef
 * NaN, rank 0, rss0 0) when n < nx + 3 or x0'x0 has no Cholesky factor.
 * Outputs: lod_out[T][n_mark], coef_out[T][n_mark][2], rank_out[n_mark], rss0_out[T], perm_max_out[P][T] (NULL exactly when
 * n_perm is 0) -- host pointers, or device pointers with CNF2_OUT_DEVICE.  reg is a host pointer, staged whole, or with
 * CNF2_QTL_REG_DEVICE a device pointer aligned to 16 bytes, read in place; scale, x0, pheno and perm are host pointers.
 * Arguments out of range, a value of scale, x0 or pheno that is not finite and a row of perm that is no permutation return
 * CNF2_ERR_ARG and write nothing.  The call needs no map and does not touch the context's rows.
 * Launches, in cnf2_qtl_scan's form: the null design's factor; a record per marker; per tile of columns (the cap of
 * cnf2_set_qtl_columns applies; results do not depend on it, to the bit) the column image, the null fit, the product on the
 * f64 matrix cores -- marker tiles of 16, the epilogue in registers -- and the maxima's finish.  No atomics, every sum over
 * the individuals in ascending order: a call gives the same bits every time. */
int cnf2_qtl_scan_cols(cnf2_ctx *ctx, int n, int n_mark, int ne, const double *reg /* [n][n_mark][ne] */,
                       const double *scale /* [n] or NULL */, int nx, const double *x0 /* [n][nx] */, int n_traits,
                       const double *pheno /* [n][T] */, int n_perm, const int32_t *perm, double *lod_out /* [T][n_mark] */,
                       double *coef_out /* [T][n_mark][2] */, int32_t *rank_out /* [n_mark] */, double *rss0_out /* [T] */,
                       double *perm_max_out /* [P][T] */, uint32_t flags);

/* Bootstrap scan: cnf2_qtl_scan on resampled individuals, for the confidence interval of a QTL's position (Visscher, Thompson
 * and Haley 1996; scanoneboot of other packages).  A replicate draws the individuals with replacement, the chromosome is
 * scanned again, and the replicates' best positions form the interval (qtl.boot_interval of the Python package).  One
 * definition for this header, cnf2freq_amd/csrc/cnf2_qtlboot.h, the kernels and tests/qtlboot_reference.py.
 * origin, pheno, use, cov (0 <= K <= 8), the mask c of a chromosome (an individual whose row at the chromosome's first marker
 * is all zero is skipped there), X0, a, d and CNF2_QTL_ADDITIVE are cnf2_qtl_scan's.  The chromosomes chrom_begin ..
 * chrom_end-1 are scanned, C' = chrom_end - chrom_begin >= 1, M' their markers.  count[B][n] (int32, B >= 1): individual i
 * occurs count[b][i] times in replicate b; it is >= 0, and 0 where use is 0.
 * Per replicate b and chromosome c, with the weights w_i = count[b][i] c_i: n_bc = sum w_i, S11 = X0'WX0 with its Cholesky
 * factor, b0 = X0'Wy, RSS0 = y'Wy - b0' S11^-1 b0.  The replicate is usable there when the factor exists, n_bc >= K + 4, and
 * no covariate takes one single value on all its individuals with w_i > 0 (compared as values: such a column is a multiple
 * of the intercept, which rounding alone would leave to the factor's last pivot).  Per replicate and marker S21 = A'WX0,
 * S22 = A'WA and v = A'Wy - G b0 go through the rank rule (pivot threshold 1e-8), the clamps and the logarithm of
 * cnf2freq_amd/csrc/cnf2_qtl.h with n_bc for n_c: ordinary least squares on the resampled data set.  Traits and covariates
 * are centred by their unweighted means over the used individuals, as in every scan; the intercept takes up the rest.
 * Outputs: boot_max_out[B][T][C'] the largest LOD of the chromosome, 0 when the replicate is unusable there;
 * boot_arg_out[B][T][C'] (int32) the global index of the marker that has it, the lowest among equal maxima (so the
 * chromosome's first marker when every LOD is 0), -1 when unusable; n_boot_out[B][C'] (int32) n_bc; boot_lod_out[B][T][M']
 * or NULL the whole profiles (all 0 where unusable).  Host pointers, or device pointers with CNF2_OUT_DEVICE.  origin is a
 * host pointer, or with CNF2_QTL_ORIGIN_DEVICE a device pointer read in place -- NULL: the rows the context's last
 * cnf2_sweep_qtl left, by cnf2_qtl_scan's rules (CNF2_ERR_STATE when there are none for n); the call leaves them valid.
 * pheno, use, cov and count are host pointers.  A NULL pointer, K, B or the chromosome range out of range, a used value that
 * is not finite, a negative count and a count on an unused individual return CNF2_ERR_ARG and write nothing.
 * Launches: the masks; per tile of replicates (a multiple of 16; results do not depend on it) the weight image W[n][B]
 * (doubles), a record per (replicate, chromosome) and trait, the product, the finish.  The product has cnf2_qtl_scan's
 * shape with the weight image for the column image: a wave owns 16 markers x 16 replicates, walks the individuals in
 * ascending order four per v_mfma_f64_16x16x4_f64, and forms the marker operand of every weighted sum (a a, a d, d d, a x_k,
 * d x_k, a y_t, d y_t) in registers from the origin rows read in place; cell, profile and the tile's (maximum, marker) follow
 * in registers.  More than four traits are taken in chunks that repeat the design sums.  No atomics, every sum over the
 * individuals in ascending order: a call gives the same bits every time, with and without boot_lod_out, from host or
 * device rows, whatever the chunking. */
int cnf2_qtl_scan_boot(cnf2_ctx *ctx, int n, const double *origin, int n_traits, const double *pheno, const uint8_t *use,
                       int n_cov, const double *cov, int chrom_begin, int chrom_end, int n_boot,
                       const int32_t *count /* [B][n] */, double *boot_max_out /* [B][T][C'] */,
                       int32_t *boot_arg_out /* [B][T][C'] */, int32_t *n_boot_out /* [B][C'] */,
                       double *boot_lod_out /* [B][T][M'] or NULL */, uint32_t flags);

/* Multi-trait scan: is there a locus that moves T correlated traits jointly?  Multivariate Haley-Knott regression (Knott and
 * Haley 2000; Jiang and Zeng 1995): Wilks' lambda of the T traits on (a, d) at every marker, which finds a pleiotropic locus
 * whose single-trait effects each stay below their threshold.  One definition for this header,
 * cnf2freq_amd/csrc/cnf2_qtlmv.h (host and device), the kernels and tests/qtlmv_reference.py.
 * origin, pheno[n][T], use, cov (0 <= K <= 8), perm[P][n], the mask c of a chromosome, n_c, X0 = [c, c z_1 .. c z_K], a, d, G,
 * W = (pa, l, pd) with the marker rank rule, CNF2_QTL_ADDITIVE and the centring of traits and covariates are cnf2_qtl_scan's.
 * 1 <= T <= 16.  A group g is the T columns of the observed data (g = 0) or of permutation p (g = 1 + p): a permutation moves
 * all T traits of an individual together.
 * Per chromosome and group B0 = X0'Y (nx x T) and E0 = Y'CY - B0' S11^-1 B0 (T x T), factored E0 = L L' in trait order; trait t is
 * dropped when E0[t][t] <= 0 or its pivot is below 1e-8 times E0[t][t]: its row of L is absent and it contributes nothing.
 * Per marker and group, with V = A'Y - G B0 (2 x T): Vw = V L^-T, u_t = vwd_t - l vwa_t, and over the kept traits
 *   qaa = sum vwa_t^2 / pa,  qdd = sum u_t^2 / pd,  qad = sum vwa_t u_t / sqrt(pa pd),
 *   Lambda = (1 - qaa)(1 - qdd) - qad^2,  lod = -(n_c / 2) log10 Lambda.
 * A dropped marker column (pivot 0) gives no terms: rank 1 is Lambda = 1 - qaa (or 1 - qdd), rank 0 a LOD of exactly 0.  Lambda
 * is clamped to [2^-52, 1], and lod is exactly 0 where it is 1.  This is Wilks' det(E1) / det(E0), by
 * det(I_T - E0^-1 V'W^-1 V) = det(I_2 - W^-1 V E0^-1 V'); for T = 1 it is 1 - dRSS / RSS0, cnf2_qtl_scan's lod.  It does not change
 * under Y -> Y B + offsets for an invertible B.  A chromosome is not scanned (lod 0, rank 0) when n_c < K + 3 + T, S11 has no
 * factor, or every trait is dropped.
 * Outputs: lod_out[M] the joint LOD of the observed group; rank_out[M] the marker's rank, 0 where the chromosome is not
 * scanned; trait_rank_out[C] the traits kept for the observed group; n_used_out[C] n_c; perm_max_out[P][C] the largest LOD of
 * permutation p on chromosome c (NULL exactly when P = 0).  Host pointers, or device pointers with CNF2_OUT_DEVICE.  origin
 * is a host pointer, or with CNF2_QTL_ORIGIN_DEVICE a device pointer read in place -- NULL: the rows the context's last
 * cnf2_sweep_qtl left, by cnf2_qtl_scan's rules (CNF2_ERR_STATE when there are none for n); the call leaves them valid.
 * T > 16, K > 8 and everything cnf2_qtl_scan refuses return CNF2_ERR_ARG and write nothing.
 * Launches: the masks and marker records (cnf2_qtl_scan's kernels); per tile of groups (cnf2_set_qtlmv_groups caps it, 0 =
 * what memory allows; results do not depend on it) the column image in operand order with the traits padded by zero
 * columns to 4, 8 or 16, one wave per (chromosome, group) for B0, E0 and its factor, the product, the maxima's finish.  The
 * product is cnf2_qtl_scan's -- 16 markers x 64 padded columns per wave on v_mfma_f64_16x16x4_f64, operands from global
 * memory, no LDS -- with the columns assigned to MFMA rows so that a lane's 16 accumulators are whole groups of one marker;
 * whitening, the three sums, clamp and logarithm follow in the lane's registers.  No atomics, every sum over the
 * individuals in ascending order: a call gives the same bits every time, for every cap, from host or device rows, into
 * host or device outputs. */
int cnf2_qtl_scan_mv(cnf2_ctx *ctx, int n, const double *origin, int n_traits, const double *pheno, const uint8_t *use,
                     int n_cov, const double *cov, int n_perm, const int32_t *perm, double *lod_out /* [M] */,
                     int32_t *rank_out /* [M] */, int32_t *trait_rank_out /* [C] */, int32_t *n_used_out /* [C] */,
                     double *perm_max_out /* [P][C] */, uint32_t flags);
int cnf2_set_qtlmv_groups(cnf2_ctx *ctx, int cap);

/* Within-family scan: the nested (half-sib) model of Knott, Elsen and Haley (1996).  Every scan above regresses on
 * a = P(BB) - P(AA), which assumes that the two founder lines are fixed for different QTL alleles.  In an outbred cross an F1
 * parent may be heterozygous or homozygous at the QTL, and the sign of "allele from its first parent" against "allele from its
 * second" differs from parent to parent: a line-cross scan averages the signs away.  Here every F1 parent on one side gets
 * its own mean and its own substitution effect, fitted on its offspring.  The regressor is bit 0 (side 0) or bit 3 (side 1)
 * of the origin sweep's absolute frame -- the allele from par[.][side] descends from that parent's par[.][1] -- which is the
 * same labelling for every offspring of the parent and a linear function of the origin row: P(bit0 = 1) = o[1] + o[3],
 * P(bit3 = 1) = o[2] + o[3].  One definition for this header, cnf2freq_amd/csrc/cnf2_qtlfam.h (host and device), the kernels and
 * tests/qtlfam_reference.py.
 * Inputs: origin[n][M][4], pheno[n][T], use, cov[n][K] (0 <= K <= 8) and perm[P][n] are cnf2_qtl_scan's, as are
 * CNF2_QTL_ORIGIN_DEVICE and the centring of traits and covariates over the used individuals.  side is 0 or 1.  grp[n] is the
 * slope group of individual i: 0 .. n_fam-1 the F1 parent on the side, < 0 not nested, not used.  cell[n] (NULL: grp) is the
 * mean cell -- typically sire slopes and full-sib family means; all members of a cell must share one grp.  perm must keep
 * every used individual inside its cell.
 * Per chromosome c: c_i = use[i] and grp[i] >= 0 and the row at c's first marker is not all zero; n_c = sum c_i.  Every column
 * v -- a trait, a permuted trait, a covariate -- is centred within cells: v~_i = c_i (v_i - mean of v over the used members of
 * cell(i)).  S11 = Z~'Z~ (K x K), b0 = Z~'y~, yy = y~'y~, RSS0 = yy - b0' S11^-1 b0.  A chromosome is not scanned when S11 has no
 * Cholesky factor or n_c - n_cells_used - K < 2: its markers get df 0, lod 0 and slopes NaN.
 * Per marker m: x_i = c_i (o1 + o3 - o0 - o2) for side 0 and c_i (o2 + o3 - o0 - o1) for side 1.  For every family p, the sums
 * over its used members:
 *   d_p = sum over the cells q of p (sum x^2 - (sum x)^2 / n_q),  raw_p = sum x^2,  u_p = sum x_i z~_i,  r_p = sum x_i y~_i.
 * A family is fitted when raw_p > 0 and d_p >= 1e-8 raw_p; df[m] is the number of fitted families.  The diagonal slope block
 * is eliminated:
 *   H = S11 - sum_fitted u_p u_p' / d_p,  g = b0 - sum_fitted u_p r_p / d_p,  gamma = H^-1 g,
 *   RSS1 = yy - sum_fitted r_p^2 / d_p - g' gamma,  slope_p = (r_p - u_p' gamma) / d_p
 * (K = 0: no H).  dRSS = RSS0 - RSS1 is clamped to [0, RSS0 (1 - 2^-52)] and lod = (n_c / 2) log10(RSS0 / (RSS0 - dRSS)).  If H has
 * no factor under cnf2_qtl.h's relative-pivot rule against S11's diagonal (a pivot below 1e-8 times it), or if
 * n_c - n_cells_used - K - df[m] < 1: df 0, lod 0, slopes NaN.  df varies along the map, so a bare LOD is not comparable
 * between markers without it (cnf2freq_amd.qtl.fam_fstat).
 * Outputs: lod_out[T][M]; df_out[M], which depends on the design only; slope_out[T][M][n_fam] of the observed columns (NULL:
 * not asked for), NaN for a family that is not fitted; rss0_out[T][C]; n_used_out[C] n_c; n_cells_out[C] the cells with a used
 * member; perm_max_out[P][T][C] (NULL exactly when P = 0).  Host pointers, or device pointers with CNF2_OUT_DEVICE.
 * Everything cnf2_qtl_scan refuses, a side other than 0 or 1, n_fam < 1, a grp of n_fam or more, a negative cell of a used
 * individual, a cell with members of two groups and a permutation that takes a used individual out of its cell return
 * CNF2_ERR_ARG and write nothing.
 * Launches: on the host the gather list -- the used individuals ordered by (grp, cell, index), every cell padded to a
 * multiple of 4 slots; per chromosome the mask, the centred covariates in gather order, S11 and its factor; per (marker,
 * family) the record (1 / d_p or 0, u_p); per marker H's factor and df; per column tile (cnf2_set_qtl_columns caps it; results
 * do not depend on it) the centred column image in gather order, the null fits, the product and the maxima's finish; the
 * slopes.  The product is cnf2_qtl_scan's -- 16 markers x 64 columns per wave (32 with more than 2 covariates) on
 * v_mfma_f64_16x16x4_f64, the marker operand formed in registers from the 32-byte rows read in place through the gather
 * list, no LDS -- segmented by family: at every family end the accumulators r_p are folded into sum r_p^2 / d_p and into g in
 * registers and cleared; the solve, clamp and logarithm follow in the lane's registers.  No atomics, every sum in ascending
 * order of the individuals within a family and of the families within a marker: a call gives the same bits every time,
 * for every cap, from host or device rows, into host or device outputs. */
int cnf2_qtl_scan_fam(cnf2_ctx *ctx, int n, const double *origin, int side, const int32_t *grp, const int32_t *cell, int n_fam,
                      int n_traits, const double *pheno, const uint8_t *use, int n_cov, const double *cov, int n_perm,
                      const int32_t *perm, double *lod_out /* [T][M] */, int32_t *df_out /* [M] */,
                      double *slope_out /* [T][M][n_fam] or NULL */, double *rss0_out /* [T][C] */, int32_t *n_used_out /* [C] */,
                      int32_t *n_cells_out /* [C] */, double *perm_max_out /* [P][T][C] */, uint32_t flags);

/* Founder-haplotype scan for outbred crosses: the founder-allele regression of multi-parent and outbred-F2 analyses.  The
 * line-cross scans regress on the line origin of an allele and assume the lines fixed for the QTL alleles; the within-family
 * scan above gives every F1 parent a slope of its own.  This model sits between the two: the trait is regressed on the
 * expected dosage of every founder haplotype, QTL alleles being shared by all families that descend from the same founder
 * chromosome -- far fewer parameters than a slope per F1 parent, and no assumption about the lines.  One definition for this
 * header, cnf2freq_amd/csrc/cnf2_qtlhap.h (host and device), the kernels and tests/qtlhap_reference.py.
 * Inputs: descent[n][M][8] are cnf2_sweep_descent's rows -- a host array, staged whole, or with CNF2_QTL_ORIGIN_DEVICE a device
 * pointer (aligned to 16 bytes) read in place.  col[n][8] (int32) assigns every cell of an individual's row to a model column
 * 0 .. n_columns-1, or to -1 (cnf2h_descent_columns of cnf2host.h, origins.descent_columns).  n_columns H is 1 .. 32: the cap
 * is 16 phased grandparents; for more founders than that the within-family scan is the tool.  pheno[n][T], use, cov[n][K]
 * (0 <= K <= 8), perm[P][n], the columns R = T (1 + P), X0, the centring of traits and covariates over the used individuals,
 * S11, b0 and RSS0 per chromosome and column, the clamp of dRSS and the LOD formula are cnf2_qtl_scan's.
 * Per chromosome c: c_i = use[i] and all eight col[i][k] in [0, H) and the descent row at c's first marker is not all zero;
 * n_c = sum c_i.  Per marker m
 *   Z[i][h] = c_i sum_k [col[i][k] == h] descent[i][m][k]                the expected dosage of column h, 0 .. 2
 *   S22 = Z'Z,  S21 = Z'X0,  W = S22 - S21 S11^-1 S21',  v = Z'y - S21 S11^-1 X0'y.
 * W is factored in ascending column order; column h is dropped when S22[h][h] == 0 or its pivot is below 1e-8 times
 * S22[h][h]; df[m] is the number of columns kept.  The rows of Z add up to 2 c_i (with one column per strand each side adds
 * up to c_i), so the rule acts at every marker: it is the normal path, and which of the dependent columns is dropped -- the
 * last of them in column order -- is part of the definition.  dRSS = |L^-1 v|^2 over the kept columns, lod = (n_c / 2)
 * log10(RSS0 / (RSS0 - dRSS)), coef = W_kept^-1 v, NaN where dropped: effects relative to the dropped columns.  A chromosome is
 * not scanned under cnf2_qtl_scan's conditions (S11 without a Cholesky factor, n_c < K + 4); a marker with
 * n_c - 1 - K - df < 1 reports df 0, lod 0 and coef NaN.  df varies along the map (cnf2freq_amd.qtl.hap_fstat).
 * Outputs: lod_out[T][M]; df_out[M] (int32), which depends on the design only; coef_out[T][M][H] of the observed columns (NULL:
 * not asked for); rss0_out[T][C]; n_used_out[C] n_c; perm_max_out[P][T][C] (NULL exactly when P = 0).  Host pointers, or device
 * pointers with CNF2_OUT_DEVICE.  Everything cnf2_qtl_scan refuses, a NULL descent or col, n_columns outside 1 .. 32 and a col
 * value >= n_columns or < -1 return CNF2_ERR_ARG and write nothing.
 * Launches: on the host the gather list -- the used individuals ordered by their col row (a pattern: in a cross from few
 * founders one per pair of F1 parents), every pattern padded to 4 slots; per chromosome the mask, S11 and its factor; per
 * marker, a wave: S22 and S21 over the individuals in ascending order, W's packed factor in LDS (528 doubles at H = 32), the kept
 * mask and df; per column tile (cnf2_set_qtl_columns caps it; results do not depend on it) cnf2_qtl_scan's column image and
 * null fits, the product and the maxima's finish.  The product takes two markers x 32 columns per wave on
 * v_mfma_f64_16x16x4_f64: the eight cells of a row at two markers are sixteen consecutive doubles, the operand as they lie in
 * memory; at a pattern's end the 8 x 32 block per marker is added into the wave's G[H][32] in LDS at the rows the pattern's
 * columns name.  The epilogue forms v, substitutes through the marker's factor, and forms the cell, the coefficients and the
 * tile's maximum.  No atomics, every sum in a fixed order: a call gives the same bits every time, for every cap, from host or
 * device rows, into host or device outputs. */
int cnf2_qtl_scan_hap(cnf2_ctx *ctx, int n, const double *descent, const int32_t *col, int n_columns, int n_traits,
                      const double *pheno, const uint8_t *use, int n_cov, const double *cov, int n_perm, const int32_t *perm,
                      double *lod_out /* [T][M] */, int32_t *df_out /* [M] */, double *coef_out /* [T][M][H] or NULL */,
                      double *rss0_out /* [T][C] */, int32_t *n_used_out /* [C] */, double *perm_max_out /* [P][T][C] */,
                      uint32_t flags);

/* Variance-component scan for outbred crosses: random founder-haplotype effects, the flexible intercross analysis of
 * Ronnegard, Besnier and Carlborg (2008).  The founder-haplotype scan above fits the founder alleles as fixed effects: it pays
 * a degree of freedom per column, needs a drop rule at every marker and stops at 32 columns.  Here y = X0 b + Z u + e with
 * u ~ N(0, s_u^2 I_H) and e ~ N(0, s_e^2 I): one variance component per locus, whatever the number of founders, no drop rule,
 * and BLUPs of the founder-allele effects that show which alleles differ.  (Not the polygenic scan, which has one kinship
 * matrix for the whole genome and fixed locus effects: here the variance component is the locus.)  One definition for this
 * header, cnf2freq_amd/csrc/cnf2_qtlvc.h (host and device), the kernels and tests/qtlvc_reference.py.
 * Inputs: cnf2_qtl_scan_hap's, with n_columns H in 1 .. 64; the mask c_i, n_c, Z[i][h], X0 = [1, centred cov], the centring,
 * S11, b0, RSS0 and the conditions under which a chromosome is not scanned are that scan's.  Per marker m
 *   W = Z'Z - S21 S11^-1 S21',  v = Z'y - S21 S11^-1 X0'y,  nu = n_c - 1 - K,
 *   W = Q diag(d) Q' (eigenvalues below 0 count as 0),  rank[m] = the number of d_k > 1e-10 d_max,  t = Q'v,
 * and only the terms of the rank enter the sums below.  The rows of Z add up to 2 c_i, so W always has null directions: they
 * are the normal path and need no rule beyond this one.  The restricted likelihood is the likelihood of A'y with
 * A A' = I - X0 (X0'X0)^-1 X0', so log|I + g A'ZZ'A| = log|I_H + g W| and by Woodbury the quadratic form is
 * RSS0 - g v'(I + g W)^-1 v.  With g = h / (1 - h) and h in [0, 0.999]:
 *   q(h) = RSS0 - sum_k g t_k^2 / (1 + g d_k)          clamped below at RSS0 2^-52
 *   f(h) = ( nu log10(RSS0 / q(h)) - sum_k log10(1 + g d_k) ) / 2,     f(0) = 0.
 * The search is deterministic: 41 grid points h_j = 0.999 j / 40, j* the first arg-max, h^ the maximiser of f on
 * [h_max(j*-1,0), h_min(j*+1,40)] located within 1e-7 (21 bisections on the sign of f'(h), which needs no logarithm; where f
 * does not rise into the bracket from an end, between h_j* and the other end, or h_j* itself: never below the grid's maximum), lod = max(f(h^), 0), and h^ = 0 wherever the LOD is 0.
 * The eigenvalues come from a cyclic Jacobi iteration with a fixed round-robin order of disjoint pairs; it stops when every
 * |W_pq| <= 2^-52 sqrt(|W_pp W_qq|), or after 30 sweeps: a marker that has not converged reports rank -1 and lod 0.
 * Outputs: lod_out[T][M]; h_out[T][M]; sigma2_out[T][M] the residual variance q(h^) / nu (s_u^2 = g s_e^2);
 * blup_out[T][M][H] (NULL: not asked for) u^ = Q diag(g / (1 + g d_k)) t, all zero at h^ = 0; eval_out[M][H] (NULL: not asked
 * for) the clamped eigenvalues in descending order and rank_out[M] (int32), which depend on the design only; rss0_out[T][C];
 * n_used_out[C]; perm_max_out[P][T][C] (NULL exactly when P = 0).  Host pointers, or device pointers with CNF2_OUT_DEVICE.  A
 * marker with nu < 2 or rank 0 reports lod 0, h 0 and blup 0.  Everything cnf2_qtl_scan_hap refuses, and n_columns outside
 * 1 .. 64, return CNF2_ERR_ARG and write nothing; CNF2_ERR_NOMEM when the marker records (about 60 KB each at H = 64) do not fit.
 * Launches: the gather list, the chromosome kernel, the column image, the null fits and the finish are the founder-haplotype
 * scan's.  Per marker, a wave: S22, S21 and W as that scan forms them, then the Jacobi iteration in the same wave with W and
 * Q in LDS, and the marker's record: d, Q, G = S11^-1 S21', and for the 41 grid points the column-independent tables
 * 10^(-sum_k log10(1 + g_j d_k) / nu) and g_j / (1 + g_j d_k), so that the grid pass of a cell has no logarithm and no division.
 * The product is that scan's (two markers x 32 columns per wave on v_mfma_f64_16x16x4_f64, the wave's G[2][H][32] in LDS); the
 * epilogue, a lane per (marker, column), forms v, rotates it, walks the grid, bisects and forms the cell, the BLUP of an
 * observed column and the tile's maximum of a permuted one.  No atomics, every sum in a fixed order, every loop bounded: a
 * call gives the same bits every time, for every cnf2_set_qtl_columns cap, from host or device rows, into host or device
 * outputs. */
int cnf2_qtl_scan_vc(cnf2_ctx *ctx, int n, const double *descent, const int32_t *col, int n_columns, int n_traits,
                     const double *pheno, const uint8_t *use, int n_cov, const double *cov, int n_perm, const int32_t *perm,
                     double *lod_out /* [T][M] */, double *h_out /* [T][M] */, double *sigma2_out /* [T][M] */,
                     double *blup_out /* [T][M][H] or NULL */, double *eval_out /* [M][H] or NULL */, int32_t *rank_out /* [M] */,
                     double *rss0_out /* [T][C] */, int32_t *n_used_out /* [C] */, double *perm_max_out /* [P][T][C] */,
                     uint32_t flags);

/* Maximum-likelihood single-locus scan: Lander and Botstein's interval mapping, the normal mixture over the four origin
 * classes fitted by EM.  Haley-Knott regression (the three scans above) is exact only where the origin rows are certain;
 * where a row is soft it leaves the within-individual genotype variance in the residual.  One definition for this header,
 * cnf2freq_amd/csrc/cnf2_qtlem.h (host and device), the kernels and tests/qtlem_reference.py.
 * origin, pheno, use, cov (0 <= K <= 8), perm, the mask c of a chromosome, n_c, X0 = [c, c z_1 .. c z_K] and the columns
 * R = T (1 + P) are cnf2_qtl_scan's.
 *   classes   g = 0 .. 3 = AA, BA, AB, BB in the order of the origin row, priors pi_ig = o_ig / sum_g o_ig at the marker; a class
 *             with pi = 0 has weight 0 and never enters a logarithm
 *   effects   a = (-1, 0, 0, 1);  d = (0, 1, 1, 0) (not with CNF2_QTL_ADDITIVE);  i = (0, 1, -1, 0) (only with
 *             CNF2_QTL_IMPRINT);  ne of them, design width W = 1 + K + ne
 *   model     y_i | g ~ N(x0_i' gamma + e(g)' beta, sigma^2);  l(theta) = sum_i c_i log sum_g pi_ig phi(y_i; mu_ig, sigma^2), with
 *             the individual's largest exponent taken out;  l0 = -(n_c / 2)(log(2 pi RSS0 / n_c) + 1), RSS0 as in cnf2_qtl_scan
 *   rank      from the design only: the prior means sum_g pi_ig e(g) are factored against X0 in the order a, d, i, as
 *             cnf2_qtl_scanx treats its Mendelian and imprinting columns; an effect is dropped (beta = 0, coefficient NaN) when its
 *             raw diagonal is 0 or its pivot is below 1e-8 times the diagonal.  rank[m] = the kept effects; rank 0: lod 0, iters
 *             0, status 0.  A marker whose rows carry no linkage information is not fitted.
 *   start     the null fit: gamma = S11^-1 b0, beta = 0, sigma^2 = RSS0 / n_c.  Fixed, so a fit is deterministic; EM may stop
 *             at a local maximum.
 *   iterate   t = 1, 2, ..: E-step w_ig ~ pi_ig exp(-(y_i - mu_ig)^2 / (2 sigma^2)) at theta_{t-1}; M-step = weighted least
 *             squares over the expanded data, solved by the Schur complement on the factor of S11; sigma^2_t = the weighted
 *             residual sum of squares / n_c; l_t = l(theta_t)
 *   stop      after iteration t when (l_t - l_{t-1}) / ln 10 < tol or t = max_iter (a negative tol: exactly max_iter)
 *   report    theta_t, lod = max(0, (l_t - l0) / ln 10), iters = t, status 0 (tol), 1 (max_iter) or 2 (breakdown: a kept pivot
 *             of the M-step's Schur block not positive, or sigma^2_t not positive and finite; the last complete iterate is
 *             reported)
 *   not scanned   a chromosome with n_c < max(W + 1, K + 4) or without a factor of X0 (K + 4: RSS0 is cnf2_qtl_scan's):
 *             rank 0, lod 0, coef and sigma2 NaN, rss0 0; a column with RSS0 <= 0: lod 0, coef and sigma2 NaN, iters 0
 * max_iter is 1 .. 10 000 and tol finite.  Outputs (host memory, or device memory with CNF2_OUT_DEVICE): lod_out [T][M],
 * coef_out [T][M][ne], sigma2_out [T][M], iters_out and status_out [T][M] int32, rank_out [M], rss0_out [T][C], n_used_out
 * [C], perm_max_out [P][T][C] (the permuted columns contribute only there).  CNF2_QTL_ORIGIN_DEVICE: origin is device memory,
 * or NULL for the rows the last cnf2_sweep_qtl left in the context (CNF2_ERR_STATE where it holds none of n individuals); the
 * call leaves those rows valid.  Everything cnf2_qtl_scan refuses is refused, and so are max_iter and tol out of range:
 * CNF2_ERR_ARG, and nothing is written.
 * One wavefront owns one (marker, column) fit from start to stop: its lanes stride the individuals in ascending order, the
 * sums of a pass are added across the wave in a fixed order and every lane takes the same step.  The waves of a block take
 * adjacent markers of one chromosome; a finish kernel reduces the permutations' maxima per chromosome.  No atomics and no
 * split of the individuals: a call gives the same bits every time, for every column cap (cnf2_set_qtlem_columns, 0 = no cap)
 * and from host or device rows. */
int cnf2_qtl_scan_em(cnf2_ctx *ctx, int n, const double *origin, int n_traits, const double *pheno, const uint8_t *use,
                     int n_cov, const double *cov, int n_perm, const int32_t *perm, int max_iter, double tol,
                     double *lod_out, double *coef_out, double *sigma2_out, int32_t *iters_out, int32_t *status_out,
                     int32_t *rank_out, double *rss0_out, int32_t *n_used_out, double *perm_max_out, uint32_t flags);
int cnf2_set_qtlem_columns(cnf2_ctx *ctx, int cap);

/* Binary-trait single-locus scan: logistic regression of a 0/1 trait on the origin rows, fitted per marker and phenotype
 * column, observed and permuted, by iteratively reweighted least squares (Newton's method).  The four scans above assume a
 * normally distributed trait.  One definition for this header, cnf2freq_amd/csrc/cnf2_qtlbin.h (host and device), the kernels
 * and tests/qtlbin_reference.py.
 * origin, use, cov (0 <= K <= 8, taken minus their means), perm, the mask c of a chromosome, n_c and the columns R = T (1 + P)
 * are cnf2_qtl_scan's; pheno[n][T] is 0.0 or 1.0 for every used individual (its values are not centred).
 *   design    per marker that of cnf2_qtl_scanx's models 0 and 1: X0 = [1, z_1 .. z_K], then a = o[3] - o[0], d = o[1] + o[2]
 *             (not with CNF2_QTL_ADDITIVE), i = o[1] - o[2] (only with CNF2_QTL_IMPRINT); ne effects, width W = 1 + K + ne
 *   model     eta_i = x_i' theta;  l(theta) = sum_i c_i [ y_i eta_i - softplus(eta_i) ], softplus(eta) = max(eta, 0) +
 *             log1p(exp(-|eta|)); p and w = p (1 - p) from that one exponential: nothing overflows for a finite eta
 *   rank      from the design only, cnf2_qtl_scanx's rule: the unweighted columns are factored in the order X0, a, d, i; an
 *             effect is dropped (beta = 0, coefficient NaN) when its raw diagonal is 0 or its pivot is below 1e-8 times the
 *             diagonal.  rank[m] = the kept effects = cnf2_qtl_scanx's rank[m][1] with imprinting, rank[m][0] without.
 *             rank 0: lod 0, iters 0, status 0.
 *   null fit  per chromosome and column on X0, from gamma = (logit(n_1 / n_c), 0, ..), n_1 the ones among the n_c: at most 50
 *             iterations, stopped by a gain below 1e-13 LOD.  It gives l0 (ll0_out, always < 0) and gamma0.
 *   fit       from theta_0 = (gamma0, 0), l_0 = l0.  A pass at theta_t gives l_t, G = X'WX and s = X'(y - p) over the kept
 *             columns.  After the pass at theta_t, t >= 1: (l_t - l_{t-1}) / ln 10 < tol stops with status 0 (a negative tol:
 *             never), else t = max_iter stops with status 1.  Otherwise theta_{t+1} = theta_t + G^-1 s by a Cholesky factor; a
 *             pivot that is not positive or a theta_{t+1} that is not finite is a breakdown, status 2 (where separation ends).
 *             There is no step-halving: a loss of likelihood stops the fit by the first rule.
 *   report    theta_t, lod = max(0, (l_t - l0) / ln 10), iters = t, status
 *   not scanned   a chromosome with n_c < W + 1 or without a factor of X0: rank 0; on a chromosome a column with n_1 = 0 or
 *             n_1 = n_c, or whose null fit does not stop by its tolerance or breaks down.  Then lod 0, coef NaN, iters 0,
 *             status 0, ll0 0.
 * max_iter is 1 .. 1000 and tol finite.  Outputs (host memory, or device memory with CNF2_OUT_DEVICE): lod_out [T][M],
 * coef_out [T][M][ne], iters_out and status_out [T][M] int32, rank_out [M], ll0_out [T][C], n_ones_out [T][C] int32,
 * n_used_out [C], perm_max_out [P][T][C] (the permuted columns contribute only there; perm permutes the phenotype only).
 * CNF2_QTL_ORIGIN_DEVICE: origin is device memory, or NULL for the rows the last cnf2_sweep_qtl left in the context
 * (CNF2_ERR_STATE where it holds none of n individuals); the call leaves those rows valid.  Everything cnf2_qtl_scan refuses
 * is refused, and so are max_iter and tol out of range and a used phenotype that is not exactly 0 or 1: CNF2_ERR_ARG, and
 * nothing is written.
 * One wavefront owns one (marker, column) fit from start to stop: its lanes stride the individuals in ascending order, the
 * sums of a pass are added across the wave in a fixed order and every lane takes the same step.  No atomics and no split of
 * the individuals: a call gives the same bits every time, for every column cap (the setter below, 0 = no cap) and from host
 * or device rows. */
int cnf2_qtl_scan_binary(cnf2_ctx *ctx, int n, const double *origin, int n_traits, const double *pheno, const uint8_t *use,
                         int n_cov, const double *cov, int n_perm, const int32_t *perm, int max_iter, double tol,
                         double *lod_out, double *coef_out, int32_t *iters_out, int32_t *status_out, int32_t *rank_out,
                         double *ll0_out, int32_t *n_ones_out, int32_t *n_used_out, double *perm_max_out, uint32_t flags);
int cnf2_set_qtlbin_columns(cnf2_ctx *ctx, int cap);

/* Survival-trait single-locus scan: Cox's proportional hazards regression of a time-to-event trait with right censoring on
 * the origin rows, fitted per marker and column, observed and permuted, by Newton's method on Breslow's partial likelihood.
 * One definition for this header, cnf2freq_amd/csrc/cnf2_qtlsurv.h (host and device), the kernels and
 * tests/qtlsurv_reference.py.
 * origin, use, cov (0 <= K <= 8, taken minus their means), perm, the mask c of a chromosome, n_c and the columns R = T (1 + P)
 * are cnf2_qtl_scan's.  time[n][T] is finite and status[n][T] is 1.0 (the event was observed at `time`) or 0.0 (censored at
 * `time`) for every used individual; a permutation moves the pair (time, status) of an individual together.  Only the order
 * of the times enters: a strictly increasing function of them gives the same bits.
 *   design    no intercept (it is not identifiable): x_i = [z_1 .. z_K, a, d, i], a = o[3] - o[0], d = o[1] + o[2] (not with
 *             CNF2_QTL_ADDITIVE), i = o[1] - o[2] (only with CNF2_QTL_IMPRINT); the effects are on the log hazard
 *   model     w_j = exp(x_j' theta), S0(t) = sum_{j: c_j, t_j >= t} w_j;
 *             l(theta) = sum_{k: c_k, status_k = 1} [ x_k' theta - log S0(t_k) ]  (Breslow's form for tied times)
 *   rank      cnf2_qtl_scanx's rule on the unweighted columns [1, z, a, d, i] in that order; the intercept takes part in this
 *             rule only, so that a column that is constant over the individuals of c is dropped.  rank[m] = the kept effects
 *             = cnf2_qtl_scanx's rank[m][1] with imprinting, rank[m][0] without.  rank 0: lod 0, iters 0, status 0.
 *   null fit  per chromosome and column on the covariates alone, from theta = 0: at most 50 iterations, stopped by a gain
 *             below 1e-13 LOD; without covariates the single pass at theta = 0, l0 = -sum_groups ev_g log(n at risk).  It
 *             gives l0 (ll0_out, never positive) and gamma0.
 *   fit       from theta_0 = (gamma0, 0), l_0 = l0.  A pass at theta_t gives l_t, the score s and the information G over the
 *             kept columns.  After the pass at theta_t, t >= 1: (l_t - l_{t-1}) / ln 10 < tol stops with status 0 (a negative
 *             tol: never), else t = max_iter stops with status 1.  Otherwise theta_{t+1} = theta_t + G^-1 s by a Cholesky
 *             factor; a pivot that is not positive or a theta_{t+1} that is not finite is a breakdown, status 2, and theta_t,
 *             l_t are reported.  A pass at theta_t, t >= 1, whose l is not finite (an S0 that overflowed) is a breakdown too:
 *             theta_{t-1}, l_{t-1} and iters = t - 1 are reported with status 2.  This is where a monotone likelihood ends if
 *             max_iter does not end it first.  There is no step-halving.
 *   report    theta_t, lod = max(0, (l_t - l0) / ln 10), iters = t, status
 *   not scanned   a chromosome with n_c < W + 1, W = 1 + K + ne, or without a factor of [1, z]: rank 0; on a chromosome a
 *             column without an event among the n_c, or whose null fit does not stop by its tolerance or breaks down.  Then
 *             lod 0, coef NaN, iters 0, status 0, ll0 0.
 * max_iter is 1 .. 1000 and tol finite.  Outputs (host memory, or device memory with CNF2_OUT_DEVICE): lod_out [T][M],
 * coef_out [T][M][ne], iters_out and status_out [T][M] int32, rank_out [M], ll0_out [T][C], n_events_out [T][C] int32 (the
 * events among the n_c), n_used_out [C], perm_max_out [P][T][C] (the permuted columns contribute only there).
 * CNF2_QTL_ORIGIN_DEVICE is cnf2_qtl_scan_binary's.  Everything cnf2_qtl_scan refuses is refused, and so are max_iter and tol
 * out of range, a used status that is not exactly 0 or 1 and a used time that is not finite: CNF2_ERR_ARG, and nothing is
 * written.
 * One wavefront owns one (marker, column) fit from start to stop.  The individuals of a column stand in risk order
 * (descending time, ties by ascending index); the sums over risk sets are running sums along that order, formed in rounds
 * of 64 positions by wave scans of a fixed order.  No atomics: a call gives the same bits every time, for every column cap
 * and every block cap (the setters below, 0 = no cap) and from host or device rows. */
int cnf2_qtl_scan_surv(cnf2_ctx *ctx, int n, const double *origin, int n_traits, const double *time, const double *status,
                       const uint8_t *use, int n_cov, const double *cov, int n_perm, const int32_t *perm, int max_iter,
                       double tol, double *lod_out, double *coef_out, int32_t *iters_out, int32_t *status_out,
                       int32_t *rank_out, double *ll0_out, int32_t *n_events_out, int32_t *n_used_out, double *perm_max_out,
                       uint32_t flags);
int cnf2_set_qtlsurv_columns(cnf2_ctx *ctx, int cap);
/* cap on the blocks of the scan's null and fit launches (0 = the default, 1024; at most 65536): each block strides over its
 * cells, and the context owns two work rows of n doubles per wave of the launch */
int cnf2_set_qtlsurv_blocks(cnf2_ctx *ctx, int cap);

/* Variance-QTL single-locus scan: the double generalised linear model of a quantitative trait on the origin rows -- a mean
 * part and a log-variance part -- fitted per marker and phenotype column, observed and permuted, by maximum likelihood.  It
 * asks whether a locus moves the trait's level, its variability, or either.  One definition for this header,
 * cnf2freq_amd/csrc/cnf2_qtlvar.h (host and device), the kernels and tests/qtlvar_reference.py.
 * origin, use, pheno, cov (0 <= K <= 8), perm, the mask c of a chromosome, n_c and the columns R = T (1 + P) are
 * cnf2_qtl_scan's; traits and covariates are taken minus their means over the used individuals.  The variance covariates are
 * the first n_var columns of cov, 0 <= n_var <= min(K, 3).
 *   designs   mean x_i = [1, z_1 .. z_K, E], variance v_i = [1, z_1 .. z_nvar, E]; E is cnf2_qtl_scan_binary's: a = o[3] - o[0],
 *             d = o[1] + o[2] (not with CNF2_QTL_ADDITIVE), i = o[1] - o[2] (only with CNF2_QTL_IMPRINT); ne effects
 *   model     mu_i = x_i' beta, eta_i = v_i' gamma = log sigma_i^2;
 *             l(beta, gamma) = -1/2 sum_i c_i [ log 2pi + eta_i + (y_i - mu_i)^2 exp(-eta_i) ]
 *   fits      null (X0, V0) per chromosome and column; per marker fit 0 mean-only (X0 + E, V0), fit 1 variance-only
 *             (X0, V0 + E), fit 2 full (X0 + E, V0 + E)
 *   LODs      lod[0] joint = (l_full - l_null) / ln 10, lod[1] mean = (l_full - l_variance-only) / ln 10, lod[2] variance =
 *             (l_full - l_mean-only) / ln 10; each max(0, .)
 *   iteration from (beta_t, gamma_t, l_t): w_i = exp(-v_i' gamma_t), beta_{t+1} = (X'WX)^-1 X'Wy by a Cholesky factor;
 *             r = y - X beta_{t+1}, q_i = w_i r_i^2, delta = (V' diag(q) V)^-1 V'(q - 1); gamma' = gamma_t + 2^-h delta for
 *             h = 0 .. 8, the first h with (l_t - l(beta_{t+1}, gamma')) / ln 10 <= 1e-9 is taken and gives gamma_{t+1}, l_{t+1}.
 *             (l_{t+1} - l_t) / ln 10 < tol stops with status 0 (a negative tol: never), else t + 1 = max_iter with status 1.
 *   breakdown status 2, and (beta_t, gamma_t, l_t) are reported: a pivot of either factor that is not positive; a beta, gamma or
 *             l that is not finite; an |eta_i| above 700; no h accepted.
 *   rank      cnf2_qtl_scan_binary's rule on the mean design; an effect dropped there is dropped from the variance design too.
 *             rank 0: lod 0, iters 0, status 0, coef NaN.
 *   null fit  the same iteration on (X0, V0) from beta = 0, gamma = (log(sum c y^2 / n_c), 0, ..): at most 50 iterations,
 *             stopped by a gain below 1e-13 LOD.  The three fits start from (beta0, 0; gamma0, 0) with l_0 = l0.
 *   not scanned   a chromosome with n_c < (1 + K + ne) + (1 + n_var + ne) + 1 or without a factor of X0: rank 0; on a
 *             chromosome a column that is constant there, or whose null fit does not stop by its tolerance or breaks down.
 *             Then lod 0, coef NaN, iters 0, status 0, ll0 0.
 * max_iter is 1 .. 1000 and tol finite.  Outputs (host memory, or device memory with CNF2_OUT_DEVICE): lod_out [T][M][3],
 * coef_mean_out and coef_var_out [T][M][ne] of the full fit (coef_var on the log-variance scale; NaN where dropped or not
 * fitted), iters_out and status_out [T][M][3] int32 by fit, rank_out [M], ll0_out [T][C], n_used_out [C], perm_max_out
 * [P][T][C][3] (the permuted columns contribute only there; perm permutes the phenotype only).
 * CNF2_QTL_ORIGIN_DEVICE is cnf2_qtl_scan_binary's.  Everything cnf2_qtl_scan refuses is refused, and so are n_var, max_iter
 * and tol out of range: CNF2_ERR_ARG, and nothing is written.
 * One wavefront owns a cell: its three fits in sequence, each from start to stop; its lanes stride the individuals in
 * ascending order, the sums of a pass are added across the wave in a fixed order and every lane takes the same step.  No
 * atomics and no split of the individuals: a call gives the same bits every time, for every column cap (the setter below,
 * 0 = no cap) and from host or device rows. */
int cnf2_qtl_scan_var(cnf2_ctx *ctx, int n, const double *origin, int n_traits, const double *pheno, const uint8_t *use,
                      int n_cov, const double *cov, int n_var, int n_perm, const int32_t *perm, int max_iter, double tol,
                      double *lod_out, double *coef_mean_out, double *coef_var_out, int32_t *iters_out, int32_t *status_out,
                      int32_t *rank_out, double *ll0_out, int32_t *n_used_out, double *perm_max_out, uint32_t flags);
int cnf2_set_qtlvar_columns(cnf2_ctx *ctx, int cap);

/* Multiple-imputation scan: cnf2_qtl_scan on hard genotypes drawn from the posterior instead of on the soft origin rows (Sen
 * and Churchill 2001; sim.geno with scanone(method = "imp") of other packages).  Where the rows are soft Haley-Knott regression
 * misjudges the residual variance; every draw of cnf2_sweep_sample has hard classes, every fit is ordinary least squares, and
 * the draws are combined on the likelihood scale.  One definition for this header, cnf2freq_amd/csrc/cnf2_qtlimp.h (host and
 * device), the kernels and tests/qtlimp_reference.py.
 *   state [n][D][M]   (uint8) the layout cnf2_sweep_sample writes, 1 <= D <= 1024.  A state g < 64 has the origin class
 *                     k = bit0(g) + 2 bit3(g) -- the absolute frame of cnf2_sweep_origins, which takes these two bits the same
 *                     way in every shift mode; bits 1, 2, 4 and 5 are ignored.  0xFF: skipped
 * pheno, use, cov (0 <= K <= 8), perm, the columns R = T (1 + P), X0, the centring and CNF2_QTL_ADDITIVE are cnf2_qtl_scan's.
 * Per chromosome c_i = use[i] and state[i][0][first marker of c] != 0xFF; n_c, S11, its factor, b0 and RSS0 follow as there and
 * do not depend on the draw.  Per draw d the one-hot row of the class gives a = [k = 3] - [k = 0], d = [k = 1] + [k = 2]
 * (a d = 0: S22 is diagonal), and S21, G, W, the rank rule (1e-8), v, the clamps and lod_d, coef_d are cnf2_qtl_scan's on
 * that row.  Per (marker, column), the draws in ascending order through one recurrence:
 *   m = max_d lod_d,  s = sum_d 10^(lod_d - m),  lod = m + log10(s / D)   the log of the mean likelihood ratio: the draws
 *                                                                          share the null fit, so the ratios share a denominator
 *   coef = sum_d 10^(lod_d - m) coef_d / s   kept as a running weighted mean; NaN as soon as one draw drops the column (NaN
 *                                            propagating through the sum is the definition)
 * Equal draws give lod = m and the draw's coefficients to the bit.  rank_out[m] is the smallest rank over the draws.
 *   lod_out [T][M]   coef_out [T][M][2]   rank_out [M]   rss0_out [T][C]   n_used_out [C]      as cnf2_qtl_scan
 *   perm_max_out [P][T][C]   the largest COMBINED lod of the chromosome (NULL exactly when P = 0): D separate scans cannot
 *                            give it
 *   draw_lod_out [D][T][M]   or NULL: lod_d of the observed columns
 * state is a host pointer, staged whole (CNF2_ERR_NOMEM if that fails), or with CNF2_QTL_STATE_DEVICE device memory read in
 * place.  Outputs are host pointers, or device pointers with CNF2_OUT_DEVICE; pheno, use, cov and perm are host pointers.
 * CNF2_ERR_ARG, nothing written: a state in 64 .. 254; an (individual, chromosome) that is 0xFF in some of its D x len cells
 * and not in all; D out of range; state NULL; whatever cnf2_qtl_scan refuses.  Device states are checked by a kernel before
 * any output is written.  The call synchronises the context's stream, also with CNF2_OUT_DEVICE.
 * Launches: the check (device states); the masks and the factor; a record per (draw, marker), 192 bytes each, held for the
 * call; per tile of columns cnf2_qtl_scan's image and null fit, then the product: a wave owns 16 markers x 16 columns, loops
 * over the draws in ascending order and per draw over the individuals in ascending order, four per v_mfma_f64_16x16x4_f64,
 * with the (a, d) operand built in registers from the state bytes read in place; the cell, the recurrence, and the tile's
 * maximum of the combined lod stay in registers; cnf2_qtl_scan's finish kernel reduces the maxima.  No atomics: a call gives
 * the same bits every time, from host or device states, whatever the column cap (cnf2_set_qtlimp_columns, 0 = no cap) and
 * cnf2_set_batch_jobs. */
int cnf2_qtl_scan_imp(cnf2_ctx *ctx, int n, int n_draws, const uint8_t *state, int n_traits, const double *pheno,
                      const uint8_t *use, int n_cov, const double *cov, int n_perm, const int32_t *perm, double *lod_out,
                      double *coef_out, int32_t *rank_out, double *rss0_out, int32_t *n_used_out, double *perm_max_out,
                      double *draw_lod_out /* [D][T][M] or NULL */, uint32_t flags);
int cnf2_set_qtlimp_columns(cnf2_ctx *ctx, int cap);

/* HOT LOOP 2 with its reductions: for the analysed individuals
 * [ind_begin, ind_end), in that order, the per-locus accumulators of cnF2freq.cpp:5416-5577 are formed on the GPU
 * (closed forms: cnf2_haplos, cnf2_infprobs_rows) and reduced per individual as the reference does after every
 * locus (cnF2freq.cpp:5876-5902): homozyg scaled by 1 / sum of the individual's own allele-index-0 infprobs;
 * moveinfprobs (cnF2freq.cpp:3577-3597) and movehaplos (cnF2freq.cpp:3599-3616) for every window member, with the
 * individual's `descendants` count as weight.  Outputs are zeroed first: infprobs_out[n_rec][M][2][2] (side,
 * markerval 1/2), haplobase_out / haplocount_out[n_rec][M], homozyg_out[ind_end - ind_begin][M][2].
 * cnf2_descendants fills descendants[n_rec] as postmarkerdata computes them (cnF2freq.cpp:3224-3255). */
int cnf2_descendants(cnf2_ctx *ctx, int32_t *desc_out);
int cnf2_accumulate(cnf2_ctx *ctx, int ind_begin, int ind_end, const int32_t *descendants, double *infprobs_out,
                    double *haplobase_out, double *haplocount_out, double *homozyg_out, uint32_t flags);
/* The product form: one call = one haplotyping sweep of doit<> over the individuals (cnF2freq.cpp:5294-5583, 5876-5902):
 * the outputs of cnf2_sweep (may be NULL unless CNF2_OUT_DEVICE) AND the per-record accumulators, all individuals and
 * chromosomes batched on the device.  The sweep kernels run in their accumulate instantiation (posterior weights of
 * every (individual, marker, shift mode, state) into a batch buffer); one more kernel forms every accumulator of a
 * locus through per-line tables (cnf2_acctab.h) and applies homozyg's scale, moveinfprobs and movehaplos with f64
 * atomics.  CNF2_ACC_DEVICE: infprobs / haplobase / haplocount / homozyg are caller-owned device buffers
 * ([n_rec][M][2][2], [n_rec][M], [n_rec][M], [ind_end - ind_begin][M][2]); several GPUs that share ancestors sum
 * the first three with one all-reduce (the reference's reduce calls, cnF2freq.cpp:6245-6254).
 * dosage_out == NULL: the per-locus rows are not formed at all (an iteration that prints none, cnF2freq.cpp:6183: all but
 * the last of a run): the sweep runs in an instantiation without class sums, restricted tables and row epilogue;
 * likelihoods and accumulators are those of a call with rows (to the bit for windows without tie groups, to rounding
 * for the others, whose posterior weights then come from another instantiation of the kernel). */
int cnf2_sweep_accumulate(cnf2_ctx *ctx, int ind_begin, int ind_end, const int32_t *descendants, double *factors_out,
                          double *loglik_out, double *dosage_out, double *infprobs, double *haplobase,
                          double *haplocount, double *homozyg, uint32_t flags);
/* The allocations a later cnf2_sweep_accumulate(ind_begin, ind_end, ..., flags) makes -- accumulators, outputs, spill rows and
 * the batch buffer of posterior weights (sized to half of the free device memory; a first hipMalloc of that size takes
 * seconds) -- without the sweep, so that a run's first iteration (doit, cnF2freq.cpp:5294) costs what the others cost. */
int cnf2_reserve_accumulate(cnf2_ctx *ctx, int ind_begin, int ind_end, uint32_t flags);

/* Batched turn scan (HOT LOOP 3; cnF2freq.cpp:5686-5752 with aroundturner 498-554): for every
 * analysed individual in [ind_begin, ind_end) and every marker,
 *   rawervals_out [n][M][128][8]  doanalyze<aroundturner>(turn, classicstop(q, -1)) - factor for every turn and shift mode,
 *                                 unmasked like cnf2_turn_scan (the caller applies flag2ignore / shiftignore), and / or
 *   turn_lse_out  [n][M][128]     per turn the log-sum-exp of those values over the admissible shift modes: the quantity
 *                                 the clause weights are made of (computew, cnF2freq.cpp:5800-5817: weight(turn) =
 *                                 (lse[turn] - lse[0] * descendants) * descendants).
 * Either pointer may be NULL.  Host buffers are staged through one device buffer of the full size (9 KB per
 * individual x marker); with CNF2_OUT_DEVICE they are device pointers and only the batch buffer is allocated.
 * The sweep kernels run in their turn-scan instantiation; all individuals and chromosomes in batched launches. */
int cnf2_sweep_turn_scan(cnf2_ctx *ctx, int ind_begin, int ind_end, double *rawervals_out, double *turn_lse_out,
                         uint32_t flags);

/* Pre-processing user of the emission (parity level): individ::addvariance
 * (cnF2freq.cpp:1489-1558, called by postmarkerdata for every marker, cnF2freq.cpp:3373-3389) for one analysed
 * individual and chromosome: var_out[mc] = variances[marker], NaN where the reference leaves the entry alone
 * (every term zero).  Brute force over (shift mode 0-1, flag, path) with trackpossible<false, NO_EQUIVALENCE>. */
int cnf2_addvariance(cnf2_ctx *ctx, int ind, int chrom, double *var_out);

/* The same two pre-processing users for ARBITRARY records, batched (postmarkerdata runs them on every individual,
 * cnF2freq.cpp:3257-3279, 3373-3389):
 *  cnf2_fixparents_scan  ok_out[n][M][2]: fixparents' admissibility test (cnF2freq.cpp:1411-1431): is any (state, path of
 *                        parity b) possible at the marker under shift mode 0 with CORRECTIONINFERENCE set, no founder flag
 *                        assigned yet (main() calls postmarkerdata before any fixtrees, cnF2freq.cpp:8083-8085)
 *  cnf2_variances        var_out[n][M] as cnf2_addvariance, through the closed form of cnf2_variance.h (the sums over states and
 *                        paths factorise per line; one thread per record x marker).  ordered bit 0: founder flags as fixtrees
 *                        has assigned them when the records are visited in ascending order (an ancestor's flag counts if its
 *                        record index is not above the record's own), else every flag; bit 1: brute force like
 *                        cnf2_addvariance (cross-check).
 *  cnf2_variances_exact  var_out[n]: the entry of record recs[q] at marker markers[q] with the reference's OWN rounding -- the
 *                        reference's additions in the reference's order (cnF2freq.cpp:1514-1541), bit-equal to its variances[]
 *                        on goldens G10 / G12.  lockhaplos (cnF2freq.cpp:3056) takes the first marker of STRICTLY largest
 *                        variance, and mirror-image configurations tie in exact arithmetic: which of them the reference locks
 *                        is decided by the last bits of its sums, so the host evaluates the markers that can win through this
 *                        entry (a handful per record and chromosome) and compares those. */
int cnf2_fixparents_scan(cnf2_ctx *ctx, const int32_t *recs, int n, uint8_t *ok_out);
int cnf2_variances(cnf2_ctx *ctx, const int32_t *recs, int n, int ordered, double *var_out);
int cnf2_variances_exact(cnf2_ctx *ctx, const int32_t *recs, const int32_t *markers, int n, int ordered, double *var_out);

/* Per-iteration parameter updates on the device (processinfprobs cnF2freq.cpp:4179-4323,
 * updatehaploweights 4533-4734, cappedgd 4040-4177 with an own 15-point Gauss-Legendre rule; toulbar2 and the phase
 * inversions it decides stay out: negshift is never set, no haplotype is inverted between iterations).
 *  cnf2_snapshot_priors  remembers the rows as they are now as priormarkerdata / priormarkersure (what readalphadata
 *                        copies at cnF2freq.cpp:6664-6665); has_prior[n_rec] = the record was genotyped.  Call after
 *                        cnf2_upload_rows / cnf2_upload_pedigree, before any correction is written to the rows.
 *  cnf2_update_pass      what doit does after the sweep of chromosome `chrom` (cnF2freq.cpp:6232-6392): new markerdata /
 *                        markersure from the infprobs of that chromosome's markers (then cleared), new haplotype weights
 *                        for every marker of chromosomes 0..chrom (haplobase / haplocount are rewritten as the reference
 *                        leaves them), written straight into the rows; *hits_out = hitnnn of this pass.  Accumulators:
 *                        NULL = the ones cnf2_sweep_accumulate left in the context; device pointers with CNF2_ACC_DEVICE;
 *                        else host arrays (uploaded, updated, copied back).  children[n_rec]: analysed children per record
 *                        (cnF2freq.cpp:5248-5260), descendants[n_rec].  Non-empty records must not share a row.
 *  cnf2_download_rows    rows [row0, row0 + n) back to the host in the layout of cnf2_upload_rows. */
int cnf2_snapshot_priors(cnf2_ctx *ctx, const uint8_t *has_prior);
int cnf2_update_pass(cnf2_ctx *ctx, int chrom, const int32_t *children, const int32_t *descendants, double *infprobs,
                     double *haplobase, double *haplocount, double scalefactor, double entropyfactor, int *hits_out,
                     uint32_t flags);
int cnf2_download_rows(cnf2_ctx *ctx, int row0, int n, uint8_t *allele, double *sure, double *hw);
/* cnf2_update_pass restricted to the listed records (ascending; n_recs may be 0), on the accumulators the context holds:
 * the form a rank of a multi-process run uses -- every record's update reads only its own accumulators and rows
 * (cnF2freq.cpp:6344-6368 loops over individuals), so ranks update the records they own and *hits_out counts those. */
int cnf2_update_pass_records(cnf2_ctx *ctx, int chrom, const int32_t *recs, int n_recs, const int32_t *children,
                             const int32_t *descendants, double scalefactor, double entropyfactor, int *hits_out, uint32_t flags);

/* Exchange support of multi-process haplotyping runs (the reference's reduce calls,
 * cnF2freq.cpp:6245-6254): what ranks exchange is the records their windows SHARE, packed -- not the [n_rec][M] slabs.
 *  cnf2_exchange_buffer            a device staging buffer of at least `bytes` owned by the context (grows; the pointer is
 *                                  valid until the next call with a larger size)
 *  cnf2_pack_accumulators          d_packed[n][M][6] <- the context's accumulators of the listed records: per record
 *                                  infprobs [M][2][2], then haplobase [M], then haplocount [M]
 *  cnf2_unpack_accumulators        the reverse (overwrites the listed records' accumulators)
 *  cnf2_pack_rows / _unpack_rows   the genotype rows of the listed records, cnf2_packed_row_bytes() per record:
 *                                  sure [M][2] f64, haploweight [M] f64, alleles [M] u8 (a0 | a1 << 4), padded to 8 bytes
 * d_packed are device pointers; the calls return when the copy is done. */
int    cnf2_exchange_buffer(cnf2_ctx *ctx, size_t bytes, void **d_buf);
/* the first `bytes` of the exchange buffer to / from host memory: for transports that move host memory (gloo, MPI without
 * GPU support); a device-aware transport (RCCL) works on the buffer in place */
int    cnf2_exchange_download(cnf2_ctx *ctx, void *host_dst, size_t bytes);
int    cnf2_exchange_upload(cnf2_ctx *ctx, const void *host_src, size_t bytes);
/* ... and any byte range of it (transports that stage the buffer in chunks: the shared-memory transport of `cnF2freq --gpus N`) */
int    cnf2_exchange_read(cnf2_ctx *ctx, size_t offset, void *host_dst, size_t bytes);
int    cnf2_exchange_write(cnf2_ctx *ctx, size_t offset, const void *host_src, size_t bytes);
size_t cnf2_packed_accumulator_doubles(const cnf2_ctx *ctx);
size_t cnf2_packed_row_bytes(const cnf2_ctx *ctx);
int    cnf2_pack_accumulators(cnf2_ctx *ctx, const int32_t *recs, int n, double *d_packed);
int    cnf2_unpack_accumulators(cnf2_ctx *ctx, const int32_t *recs, int n, const double *d_packed);
int    cnf2_pack_rows(cnf2_ctx *ctx, const int32_t *recs, int n, void *d_packed);
int    cnf2_unpack_rows(cnf2_ctx *ctx, const int32_t *recs, int n, const void *d_packed);
/* Diagnostics of the update passes since the last pass of chromosome 0, i.e. of an iteration so far (flow kernels; see cnf2_update_kernels.hip).  out16[0..3] for the genotype
 * certainties, out16[4..7] for the haplotype weights: flows; gradient evaluations the scout spent on them; flows that ended
 * in the scout; flows pinned to their clamp (no evaluation beyond the first).  out16[8..11] / out16[12..15] for the flows the
 * scout set aside: steps taken in the finish kernel; lane slots offered (steps / slots = lane utilisation); quadratures;
 * flows that ended because the tolerance was met.  Collected only when the environment holds CNF2_UPDATE_STATS. */
int cnf2_update_stats(cnf2_ctx *ctx, uint64_t *out16);
/* The same for the lock-step kernels of the guided bisection (cnf2_update.h; the flows the scouts set aside go through
 * them first, out16[8..15] of cnf2_update_stats then describe the persistent kernel that takes what they leave):
 * out8[0..3] certainties, out8[4..7] haplotype weights: literal points evaluated; lane slots offered; gradient evaluations;
 * flows that ended because the tolerance was met. */
int cnf2_update_stats_guided(cnf2_ctx *ctx, uint64_t *out8);
/* The accumulators the context holds (what cnf2_sweep_accumulate left and cnf2_update_pass rewrote when they were called
 * with NULL accumulator pointers): host copies infprobs[n_rec][M][2][2], haplobase / haplocount[n_rec][M]; any pointer may
 * be NULL.  cnf2_upload_accumulators is the reverse (a multi-process driver whose transport moves host memory sums the
 * slabs of its ranks between the two calls). */
int cnf2_download_accumulators(cnf2_ctx *ctx, double *infprobs, double *haplobase, double *haplocount);
/* Device addresses of the same three slabs (valid until the pedigree or the map is replaced): what a multi-GPU driver
 * hands to its all-reduce (RCCL) between cnf2_sweep_accumulate and cnf2_update_pass.  Call cnf2_sync first. */
int cnf2_accumulator_ptrs(cnf2_ctx *ctx, double **infprobs, double **haplobase, double **haplocount);
int cnf2_upload_accumulators(cnf2_ctx *ctx, const double *infprobs, const double *haplobase, const double *haplocount);

/* Emission lookup of one analysed individual and marker, all 8 shift modes (parity hook
 * for trackpossible, cnF2freq.cpp:1075-1359): e_out[8][64] path-free emission e(g). */
int cnf2_emission(cnf2_ctx *ctx, int ind, int marker, double *e_out);
/* The same resolved by allele path: e_out[8][64][128] = trackpossible(..., 2g, flag2, s) for every shift mode,
 * state and path flag2 (calltrackpossible with flag2 >= 0, cnF2freq.cpp:1380-1385, 1141-1146). */
int cnf2_emission_paths(cnf2_ctx *ctx, int ind, int marker, double *e_out);

/* Diagnostic: out384[k*64 + lane] = value 1000+src received by `lane` from the lane-exchange
 * primitive of distance 1<<k (k = 0..5) that the transition butterflies are built on. */
int cnf2_selftest_lane_xor(cnf2_ctx *ctx, double *out384);

/* Measurement support for bench.py: duration in ms of the kernels of the last cnf2_sweep
 * measured with hipEvents on the context's stream (kernel_ms[0] = forward-backward kernel),
 * and workspace bytes currently allocated on the device. */
int    cnf2_last_kernel_ms(cnf2_ctx *ctx, float *kernel_ms, int n);
/* After a cnf2_sweep with CNF2_LOG_PATHS: paths_out[n] (n = individuals of that sweep x chromosomes, [ind][chrom]) = which
 * code swept the job: 0-3 the fast kernel with producer class 0 general / 1 both parents homozygous everywhere / 2 and the
 * grandparents too / 3 complete window (restricted table = unrestricted); 16 the fast kernel's instantiation for windows with
 * tie groups (a backward pass per tie combination); 32 | homleaf the merged-modes kernel; 64 the general kernel (tied windows
 * with CNF2_TIES_GENERAL or CNF2_FULL_SPILL).  Test support: the specialisations are exact shortcuts and must all be exercised. */
int    cnf2_last_paths(cnf2_ctx *ctx, int32_t *paths_out, int n);
size_t cnf2_workspace_bytes(cnf2_ctx *ctx);
/* Shader clock the device runs at under a double-precision vector load, MHz (a loop of independent FMAs on every SIMD:
 * one wave-wide FMA issues per 4 cycles).  Boxes of the same model differ by several per cent; an issue-bound kernel
 * tracks this clock, so bench.py reports it next to the roofline fraction. */
int    cnf2_clock_probe(cnf2_ctx *ctx, double *mhz_out);
/* Shader clock of the last cnf2_sweep's untied fast-kernel launch itself, MHz: its first wave reads the shader-clock
 * counter and the constant-rate wall clock when it starts and when it ends (s_memtime / s_memrealtime); 0 when no such
 * launch has run.  Synchronises the context's stream. */
int    cnf2_sweep_clock(cnf2_ctx *ctx, double *mhz_out);
void  *cnf2_stream(cnf2_ctx *ctx); /* hipStream_t of the context */
/* The sweep kernels are persistent (one resident wave per job in flight) and normally fill every
 * workgroup slot of the GPU.  Leaving `blocks` slots free lets another kernel -- the RCCL gather of
 * the previous sweep's posteriors -- run beside the sweep instead of behind it. */
int    cnf2_set_grid_reserve(cnf2_ctx *ctx, int blocks);
/* The batched consumers (cnf2_sweep_accumulate, cnf2_sweep_turn_scan) run their jobs (individual x chromosome) in batches
 * sized to the memory that is free; `jobs` > 0 caps a batch at that many jobs (0 = no cap).  Results do not depend on the
 * batch size; the knob exists so that the multi-batch path can be exercised at test sizes and memory use bounded by a caller
 * that shares the GPU. */
int    cnf2_set_batch_jobs(cnf2_ctx *ctx, int jobs);
/* Line records.  In a window of a cross of inbred lines (class 2 of cnf2_last_paths) whose root and parents are not founders,
 * what a parent and its two grandparents contribute to the emission tables depends on their three rows and slot flags (a
 * "line"), the marker and the allele the root hands down, not on the individual.  A sweep gives every distinct line of its
 * call a number, a small kernel in front of the sweep kernel evaluates the lines' records (64 bytes per line, marker,
 * allele value 0..15 and grandparent traced: 2 KB per line and marker), and the sweep kernel reads a root's own row and
 * two records where it read seven rows.  The records live for one launch and are rebuilt by every call; the numbering of the
 * lines is kept while the windows, the call's range and the cap stay the same.  A call holds at most 64 lines and at most
 * `lines` of cnf2_set_line_records (negative = no cap of its own, the default; 0 = no records).  The record buffer is
 * allocated after the spill slots and the call's outputs; when it has to grow it may take half of the memory free at that
 * moment, and the lines that did not fit then stay without records until the rows or the pedigree change.  The windows
 * of further lines, windows whose root or a parent is a founder, and every window under CNF2_NO_LINE_RECORDS are swept as
 * before, to the same bits.
 * cnf2_last_line_records: out[4] = lines of the last sweep's call, its jobs swept on records, its class-2 jobs swept
 * without, bytes of records (0 0 0 0 after a call whose mode or flags use no such instantiation). */
int    cnf2_set_line_records(cnf2_ctx *ctx, int lines);
int    cnf2_last_line_records(cnf2_ctx *ctx, int32_t *out);
/* Four windows to a wave.  The jobs of a call that are swept on line records are taken four at a time, chromosome by
 * chromosome in the order of the job list, and each group of four is swept by one wavefront: in such a window the recursion does
 * not depend on four of the six state bits, and the lanes that would repeat it carry the other three jobs instead.  What does
 * not fill a group of four, and every job under CNF2_NO_UNIFORM_PACK, CNF2_NO_LINE_RECORDS, CNF2_ALL_STATES, CNF2_FULL_SPILL or
 * CNF2_XPOSE, is swept one job to a wave, to the same bits.  Packed jobs count as swept on records in cnf2_last_line_records.
 * cnf2_last_uniform_pack: out[2] = the packed jobs of the last sweep's call and their groups (0 0 where nothing was packed). */
int    cnf2_last_uniform_pack(cnf2_ctx *ctx, int32_t *out);
/* Eight windows to a wave.  Two groups of four of one chromosome whose eight windows have all eight shift modes analysed are
 * swept by one wavefront: on line records the recursion of such a window does not depend on the first parent's shift bit
 * either, and the lanes that would repeat it carry the second group.  With at least as many eights as waves are resident, a
 * whole number of rounds of eights is formed and the last pairs stay groups of four, swept behind them.  An eight counts as two
 * groups in cnf2_last_uniform_pack.  Under CNF2_NO_UNIFORM_PACK8, and wherever nothing is packed, there are none.
 * cnf2_last_uniform_pack8: out[2] = the eights of the last sweep's call and their jobs (0 0 where there were none). */
int    cnf2_last_uniform_pack8(cnf2_ctx *ctx, int32_t *out);

/* The plan kept across sweeps.  The job list of cnf2_sweep and its modes, the groups of four and eight and their device copies
 * depend on the windows (the rows and the pedigree), the map's chromosomes, the range, the flags that route windows, the
 * call's lines and the packed grid (cnf2_set_grid_reserve): the context keeps them from the last sweep, and a call for which
 * all of that is unchanged builds and uploads no list and does not synchronise the stream in front of its kernels.  The grids
 * and the spill are formed per call all the same.  Same results to the bit.
 * cnf2_last_plan_reused: 1 if the last sweep's call took the kept plan as it stood, else 0.
 * cnf2_last_plan_ms: host milliseconds the last sweep's call spent before its first launch (planning, uploads, allocations). */
int    cnf2_last_plan_reused(cnf2_ctx *ctx);
float  cnf2_last_plan_ms(cnf2_ctx *ctx);

#ifdef __cplusplus
}
#endif
#endif /* CNF2HIP_H */
