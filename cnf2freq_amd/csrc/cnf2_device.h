// cnf2_device.h -- structures shared by the HIP kernels (cnf2_kernels.hip) and the C-ABI
// implementation (cnf2_capi.hip).  Device memory layout is described in DESIGN.md.
#ifndef CNF2_DEVICE_H
#define CNF2_DEVICE_H

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "cnf2_job.h"
#include "cnf2_window.h"

namespace cnf2 {

struct LineRec;     // cnf2_emtab.h
struct LineKey;

#define CNF2_MINFACTOR_F (-1e15f)  /* settings.h:29 */
#define CNF2_IGNORED_D (-1e30)     /* cnF2freq.cpp:5378 */

enum { KP_NO_DOSAGE = 1, KP_RAW_DOSAGE = 2, KP_NO_TIES = 4,
       KP_ACC_TABLE = 8,      // accumulate: the table-form kernel does every window
       KP_ACC_ATTOP = 16,     // accumulate: the batch holds windows whose root is the top of its lines (table form)
       KP_ACC_LANES = 32,     // accumulate: path form with one lane per path (acc_paths_kernel) instead of the tile form
       KP_FLUSH_TINY = 64,    // general sweep kernel: a state under 1e-300 of its vector is set to 0 before the emission (cnF2freq.cpp:1607-1611)
       KP_SKIP_UNIFORM = 128 }; // fast kernel, plain half-spill sweep: the jobs of uniform windows (slots_uniform) belong to the UNI instantiation's launch

// What a sweep kernel leaves behind besides the likelihoods: the STOREW template argument of fb_kernel / fb_fast_kernel
// (an int there, so that the kernels' names stay what the tools and logs in profiles/ match on)
enum SweepVariant : int {
    SW_PLAIN        = 0,   // the per-locus rows (p.dosage) unless KP_NO_DOSAGE
    SW_WEIGHTS_ROWS = 1,   // accumulate mode: also the posterior weights wg of every marker into p.wbuf
    SW_ALPHA_BETA   = 2,   // turn-scan mode: alpha e, beta and their scales into p.wbuf (CNF2_TURN_ROW doubles per marker); no rows
    SW_WEIGHTS      = 3,   // accumulate mode of a call that did not ask for the per-locus rows (wg only)
    SW_CROSSOVERS   = 4,   // posterior probability of a flip of every state bit across every gap (p.xo / p.xo_sum / p.xo_cnt); no rows
    SW_VITERBI      = 5,   // max-product recursion and backtrace in place of the backward pass (p.vit_*); no rows
    SW_SAMPLING     = 6,   // whole paths drawn from the posterior, one draw per lane (p.smp_*); no beta, no rows
    SW_POSTERIOR    = 7,   // placement mode: the state posteriors gamma = wg e of every marker into p.wbuf (SW_WEIGHTS' row and
                           // layout), the jobs with a likelihood counted in p.xo_cnt; no rows
    SW_LOO          = 8,   // leave-one-marker-out mode: per marker the likelihood ratio without the marker's emission (p.loo) and
                           // the marker's unlinked emission mean (p.unl), over every mode with a likelihood; the jobs with a
                           // likelihood counted in p.xo_cnt; no rows
    SW_ORIGINS      = 9,   // origin mode: per marker the four grandparental-origin probabilities (p.org) and P(bit t = 1) of the
                           // six meiosis bits (p.obits), masked sums of the state posterior over the modes the rows count; the
                           // jobs with a likelihood counted in p.xo_cnt; no rows
    SW_PLAIN_UNIFORM_ROWS = 10, // fb_fast_kernel's UNI instantiation only: SW_PLAIN for the uniform windows without line records
    SW_DESCENT      = 11   // descent mode: per marker the eight descent classes, four per side -- which grandparent and which of
                           // its strands an allele descends from -- as masked sums of the same posterior (p.org, eight to a
                           // row); the jobs with a likelihood counted in p.xo_cnt; no rows
};

struct KernelParams {
    // inputs, resident in HBM
    const Window*  windows;    // [n_ind]
    const Job*     jobs;       // [n_jobs]
    const uint8_t* allele8;    // [n_rows][n_markers]  a0 | a1 << 4
    const double2* sure;       // [n_rows][n_markers]
    const double*  hw;         // [n_rows][n_markers]
    const double2* rho;        // [n_markers] recombination fraction of gap m -> m+1 for
                               //             genrec[0] (.x) and genrec[1] (.y); 0 when dist <= 0
    const double2* tq;         // [n_markers] r / (1 - r) of the same gaps (fast kernel's scaled butterflies)
    const double*  chrom_logk; // [n_chrom] sum over the chromosome's gaps of 4 log(1-r0) + 2 log(1-r1)
    const PackedJob* pjobs;    // [n_pjobs] (fb_packed_kernel)
    int            n_pjobs;
    int            n_jobs;
    int            n_markers;
    int            n_chrom;
    uint32_t       flags;
    // workspace: alpha-minus spill, one slot per resident wave, [len][8][64] doubles
    double*        spill;
    size_t         spill_stride;   // doubles per wave slot
    // outputs
    double*        factors;    // [n_ind][n_chrom][8]
    double*        loglik;     // [n_ind][n_chrom]
    double*        dosage;     // [n_ind][n_markers][3]
    // debug store (fwbw_store): reference layout for ONE job
    double*        dbg_fwbw;     // [8][len][3][64]
    double*        dbg_factors;  // [8][len][3]
    // accumulate mode (STOREW instantiations): posterior weights wg(s, g) = exp(scales - factor) alphaminus beta of
    // every marker of every job of the launch, [job][wstride markers][4][64 lanes][2] in the sweep's own
    // lane / register layout (lane = chain << 3 | l, registers 2k, 2k+1)
    double*        wbuf;
    size_t         wstride;      // markers per job slot
    // which kernel / producer specialisation swept a job (tests): [n_ind][n_chrom], 0-3 = fast kernel with that `hom`
    // class, 32 | homleaf = packed kernel, 64 = general kernel; NULL = not recorded
    int32_t*       path_log;
    // fast kernel: the likelihoods leave the sweep as mantissa (in factors / loglik) and binary exponent (here); the
    // logarithms are taken by likelihood_logs_kernel right after it, so that no transcendental sits in the sweep kernel.
    // [n_ind][n_chrom][8] and [n_ind][n_chrom]; CNF2_LEXP_* mark chains / jobs without a likelihood
    int32_t*       fexp;
    int32_t*       lexp;
    // [4] or NULL: shader-clock and wall-clock ticks of block 0's first wave (launch_fb_fast: the bench's effective clock)
    unsigned long long* clock_out;
    // fast kernel: the launch's job counter (zeroed before the launch), from which its waves take their jobs one at a
    // time -- whichever waves are resident share the list evenly, whatever the jobs' lengths and whenever their blocks
    // got onto the machine; NULL = wave w sweeps jobs w, w + waves, ...
    int*           job_next;
    double*        xo;         // crossover mode: [n_ind][n_markers][6] per-individual crossover posteriors, or null
    double*        xo_sum;     // crossover mode: [n_markers][6] summed over the jobs' individuals (f64 atomics)
    int32_t*       xo_cnt;     // crossover / placement mode: [n_chrom] individuals that contribute (not skipped)
    double*        vit_logmax; // Viterbi mode: [n_ind][n_chrom][8] log max-product per shift mode
    uint8_t*       vit_state;  // Viterbi mode: [n_ind][n_markers] MAP state g = j*8 + lo of every marker
    int32_t*       vit_shift;  // Viterbi mode: [n_ind][n_chrom] MAP shift mode, -1 where skipped
    uint8_t*       smp_state;  // sampling mode: [n_ind][smp_draws][n_markers] drawn state g = j*8 + lo of every marker
    int32_t*       smp_shift;  // sampling mode: [n_ind][smp_draws][n_chrom] drawn shift mode, -1 where skipped
    double*        smp_logp;   // sampling mode: [n_ind][smp_draws][n_chrom] log P(mode, path | data), or null
    unsigned long long smp_seed;   // sampling mode: the generator's seed
    int            smp_draws;  // sampling mode: draws per individual and chromosome (1..1024)
    int            smp_ind0;   // sampling mode: absolute index of the individual at windows[0] (the generator's i)
    double*        loo;        // leave-one-out mode: [n_ind][n_markers] sum_s L_s,-m / L as the sweep leaves it (-1: skipped);
                               // loo_finish_kernel takes the logarithm in place
    double*        unl;        // leave-one-out mode: [n_ind][n_markers] mean over the analysed modes of (1/64) sum_g e_s,m(g),
                               // likewise (-1: skipped); minus its logarithm after loo_finish_kernel
    double*        org;        // origin mode: [n_ind][n_markers][4] P(bit 0 + 2 bit 3 = k), each row summing to 1 (0: skipped)
                               // descent mode: [n_ind][n_markers][8], the first side's four classes, then the second side's
    double*        obits;      // origin mode: [n_ind][n_markers][6] P(bit t = 1) (0: skipped)
    // fast kernel's UNI instantiation: the launch's line records (cnf2_emtab.h; [lines][n_markers][LINE_VALUES][2], built by
    // line_records_kernel in front of the launch) and the two lines of every window [n_ind][2] (offset like windows), -1 -1 for a
    // window that keeps the ordinary tile producer; NULL = every window does
    const LineRec* line_rec;
    const int32_t* line_keys;
};
#define CNF2_LEXP_IGNORED (-2147483647 - 1)   /* shift mode not analysed: CNF2_IGNORED_D */
#define CNF2_LEXP_DEAD    (-2147483647)       /* no likelihood left: CNF2_MINFACTOR_F */
enum { PATH_TIED = 16, PATH_PACKED = 32, PATH_GENERAL = 64 };

// Inputs of the batched HOT LOOP 2 kernel (acc_rows_kernel): the weights a STOREW sweep left for `n_jobs` jobs and
// where the per-record accumulators live.  After every locus the reference scales homozyg, then moveinfprobs /
// movehaplos add the thread-private sums to the window members (cnF2freq.cpp:5876-5902, 3577-3616): done here with
// f64 atomics, one wave per (job, marker).
struct AccParams {
    KernelParams   kp;           // windows (offset to ind_begin), jobs (offset to the batch), rows, wbuf, loglik, factors
    int            n_jobs;       // jobs in this batch
    int            max_len;      // longest chromosome of the batch (grid.y)
    uint32_t       flags;        // KP_NO_TIES, KP_ACC_TABLE, KP_ACC_ATTOP
    const int32_t* slot_rec;     // [n_ind][7] record per window slot, -1 none (offset like windows)
    const int32_t* desc;         // [n_rec] individ::descendants
    const uint8_t* rec_empty;    // [n_rec]
    double*        acc_inf;      // [n_rec][n_markers][2][2]
    double*        acc_hb;       // [n_rec][n_markers] haplobase
    double*        acc_hc;       // [n_rec][n_markers] haplocount
    double*        acc_hz;       // [n_ind][n_markers][2] homozyg of the analysed individual (offset like windows)
    double*        part;         // CNF2_DETERMINISTIC: [n_ind][n_markers][7][6] per-job rows (offset like windows), else null
};
void launch_acc_rows(const AccParams& q, hipStream_t stream);
void launch_acc_gather(const AccParams& q, const int32_t* rec_start, const int32_t* list, int n_rec, hipStream_t stream);

// Inputs of the per-iteration update kernels (cnf2_update.h): what doit does after the sweep of chromosome `chrom`
// (cnF2freq.cpp:6232-6392): processinfprobs for the markers of that chromosome, updatehaploweights for every marker
// of the chromosomes swept so far in this iteration.
struct UpdateParams {
    int            n_rec, n_markers, n_chrom, chrom, first, last;   // first / last marker of `chrom`; n_rec = records this pass updates
    const int32_t* rec_list;      // device [n_rec] the records this pass updates (ascending), or null = records 0 .. n_rec - 1
    int            chromstarts_host_upto;                           // chromstarts[chrom + 1]
    const int32_t* chromstarts;   // device [n_chrom + 1]
    const int32_t* row_of;        // [n_rec]
    const uint8_t* rec_empty;     // [n_rec]
    const uint8_t* has_prior;     // [n_rec] priormarkerdata exists (the individual was genotyped)
    const int32_t* children;      // [n_rec] analysed children (cnF2freq.cpp:5248-5260)
    const int32_t* descendants;   // [n_rec]
    uint8_t*       allele8;       // rows, updated in place
    double2*       sure;
    double*        hw;
    const uint8_t* prior_allele8; // rows as they were read (cnF2freq.cpp:6664-6665)
    const double2* prior_sure;
    double*        acc_inf;       // [n_rec][n_markers][2][2] cleared as it is consumed
    double*        acc_hb;        // [n_rec][n_markers] rewritten as the reference leaves it
    double*        acc_hc;
    uint8_t*       anyinfo;       // [n_rec][n_chrom] scratch
    double*        fw;            // [n_rec][n_markers][2] scratch
    double*        ratio;         // [n_rec][n_markers] scratch
    double         relhaplo;      // 0.5 on this path (cnF2freq.cpp:2496)
    double         scalefactor, entropyfactor;
    int*           hits;          // device counter
    unsigned long long* flow_next;   // [32]: [0..1] item counters of the persistent flow kernels; null = one thread per element
    unsigned long long* stats;       // [24] diagnostics of the flow kernels (cnf2_update_stats), may be null
    void*          todo;          // flows the scouts set aside for the finish kernels (24 bytes each)
    void*          todo2, *todo3; // two more lists of the same size (the packed lists of the guided kernels)
    unsigned long long* todo_counts;  // [todo_cap / 256 + 2] scratch of the packing
    size_t         todo_cap;      // flows per chunk of a scout = entries of todo
    int            mirror;        // certainties: run one flow per side where both values have evidence, the other is its mirror image
    int            scout_passes;  // 2 = a short first scout pass and a second for the flows still going; 1 = one pass (A/B)
    int            literal_finish; // the flows set aside take one literal bisection step per round (rounds 3 / 4) instead of the guided bisection (A/B, cross-check)
    double*        flow_out;      // [n_rec][markers of chrom][2][2] new probabilities from the certainty flows
};
void launch_update_pass(const UpdateParams& u, hipStream_t stream);
void launch_clock_probe(int n_cu, int iters, double* sink, hipStream_t stream);
void launch_copy_rows_f64(const double* src, size_t src_stride, const int32_t* src_idx, double* dst, size_t dst_stride,
                          const int32_t* dst_idx, int n, size_t elems, hipStream_t stream);
void launch_copy_rows_u8(const uint8_t* src, size_t src_stride, const int32_t* src_idx, uint8_t* dst, size_t dst_stride,
                         const int32_t* dst_idx, int n, size_t elems, hipStream_t stream);
void launch_okvals(const KernelParams& p, int n_windows, uint8_t* out, hipStream_t stream);
void launch_addvariance_batch(const KernelParams& p, int n_windows, double* out, hipStream_t stream);
void launch_variance_exact(const KernelParams& p, const int32_t* markers, int n, double* out, hipStream_t stream);
void launch_variance_closed(const KernelParams& p, int n_windows, double* out, hipStream_t stream);
// Inputs of the batched turn scan (turn_rows_kernel): what a turn-scan sweep (STOREW == 2) left in kp.wbuf
// Row of the turn-scan mode's batch buffer (doubles per job and marker): A = alphaminus e [4][64 lanes][2], B = beta
// likewise, then per shift mode s the scales that make them absolute as mantissa and binary exponent
// [8][4] = (mA, eA, mB, eB): absolute A_s = A * mA * 2^eA, absolute B_s = B * mB * 2^eB.
#define CNF2_TURN_ROW 1056
struct TurnParams {
    KernelParams kp;
    int          n_jobs, max_len;
    int          scaled_transitions;   // the batch came from the fast kernel (log-likelihoods include chrom_logk)
    int          valu_form;            // the dot products on the vector ALU instead of the matrix cores (cross-check, A/B)
    double*      rawervals;   // [n_ind][n_markers][128][8] or NULL
    double*      turn_lse;    // [n_ind][n_markers][128] or NULL
};
void launch_turn_rows(const TurnParams& q, hipStream_t stream);

// Inputs of the pair sweep (pair_sweep_kernel): what a turn-scan sweep left in kp.wbuf for the `n_jobs` jobs at kp.jobs (with
// kp.factors / kp.loglik finished), and the selection.  Pair (j, k) of sel indices j < k on one chromosome is row
// pair_off[j] + k - j - 1 of an individual's n_pairs rows.
struct PairParams {
    KernelParams   kp;
    int            n_jobs;
    int            max_anchors;   // the most selected markers of a chromosome, less one (grid.y covers them)
    int            n_pairs;
    const int32_t* sel;           // [L] marker indices, strictly ascending
    const int32_t* chrom_sel;     // [n_chrom + 1] the chromosomes' ranges in sel
    const int32_t* pair_off;      // [L]
    double*        joint;         // [n_ind][n_pairs][16]
};
void launch_pair_sweep(const PairParams& q, hipStream_t stream);
// cnt[c] = how many of the n_ind individuals have a shift mode with a likelihood on chromosome c
void launch_pair_count(const double* factors, const double* loglik, int n_ind, int n_chrom, int32_t* cnt, hipStream_t stream);

// Inputs of the placement kernels: what a placement sweep (SW_POSTERIOR) left in kp.wbuf for the `n_jobs` jobs at kp.jobs,
// and the candidates' emission tables.  place_emission_kernel fills `emis` for candidates [q0, q0 + qn) of every
// individual of the call from the candidate rows (a KernelParams whose row pointers are the candidates', n_markers = Q);
// place_rows_kernel contracts the two: place[i][q][m] = log sum_(s, g) gamma_(s, m)(g) e'_(s, q)(g).
struct PlaceParams {
    KernelParams kp;           // windows (offset to ind_begin), jobs (offset to the batch), wbuf / wstride, lexp
    int          n_jobs;       // jobs in this batch
    int          max_len;      // longest chromosome of the batch (grid.y)
    int          group;        // consecutive jobs a block walks, carrying its tile's sums while the chromosome stays the same
    int          n_cand;       // Q
    int          q0, qn;       // the candidates `emis` holds: [q0, q0 + qn)
    int          qcap;         // candidates per individual `emis` has room for (a multiple of 16)
    const double* emis;        // [n_ind][qcap][512] in a weight row's (k, lane, register) order
    double*      place;        // [n_ind][Q][n_markers] or null
    double*      place_sum;    // [Q][n_markers], added to (f64 atomics)
    int32_t*     n_zero;       // [Q][n_markers], added to
};
// cand: the candidate rows (allele8 / sure / hw with n_markers = Q; windows offset to ind_begin); null_sum [Q] is added to, or null
void launch_place_emission(const KernelParams& cand, int n_ind, int q0, int qn, int qcap, double* emis, double* null_sum,
                           hipStream_t stream);
void launch_place_rows(const PlaceParams& q, hipStream_t stream);

// Inputs of the stage-2 parity kernels: the reference-layout store of ONE individual x chromosome.
struct Stage2Params {
    KernelParams  kp;          // windows (already offset to the individual), rows, n_markers
    const double* fwbw;        // [8][len][3][64]
    const double* fwbwfactors; // [8][len][3]
    const double* factors;     // [8]
    const double* loglik;      // [1]
    int           first, len;
};
void launch_locked_query(const Stage2Params& q, int marker, double* out, hipStream_t stream);
void launch_turn_scan(const Stage2Params& q, int marker, double* out, hipStream_t stream);
void launch_turn_scan_rows(const Stage2Params& q, double* out, hipStream_t stream);
void launch_state_rows(const Stage2Params& q, uint32_t flags, double* out, hipStream_t stream);
void launch_haplos_rows(const Stage2Params& q, uint32_t flags, double* out, hipStream_t stream);
void launch_infprobs(const Stage2Params& q, int marker, uint32_t flags, double* out, hipStream_t stream);
void launch_infprobs_rows(const Stage2Params& q, uint32_t flags, double* out, hipStream_t stream);
void launch_addvariance(const KernelParams& p, int first, int len, double* out, hipStream_t stream);
// The general kernel's instantiation for `variant` (SW_PLAIN, SW_WEIGHTS_ROWS, SW_ALPHA_BETA, SW_CROSSOVERS); debug_store: the
// reference-layout store of ONE job (SW_PLAIN only).  Returns the launch's error; a combination that is not instantiated is
// hipErrorInvalidValue, never another kernel.
hipError_t launch_fb(const KernelParams& p, int grid, SweepVariant variant, hipStream_t stream, bool debug_store = false);
int  fb_xo_blocks_per_cu();
void launch_crossover_rows(const Stage2Params& q, double* out, hipStream_t stream);
// out[len][2] = (loo, unlinked) of cnf2_sweep_loo from the store, brute force
void launch_loo_rows(const Stage2Params& q, double* out, hipStream_t stream);
// What a leave-one-out sweep (SW_LOO) left in loo / unl [n_ind][n_markers] becomes loo = log(ratio) and unlinked = -log(mean)
// in place (CNF2_IGNORED where skipped); loo_sum / unl_sum [n_markers] = their sums over the n_ind individuals in ascending
// order, one thread per marker (no atomics: the same bits on every call)
void launch_loo_finish(double* loo, double* unl, int n_ind, int n_markers, double* loo_sum, double* unl_sum, hipStream_t stream);
// out[len][10] = origin[4], bits[6] of cnf2_sweep_origins from the store, brute force
void launch_origin_rows(const Stage2Params& q, double* out, hipStream_t stream);
// out[len][8] = the descent row of cnf2_sweep_descent from the store, brute force
void launch_descent_rows(const Stage2Params& q, double* out, hipStream_t stream);
// out[S (S - 1) / 2][16] = the pair rows of cnf2_sweep_pairs for the S selected markers of the chromosome (sel: local indices,
// ascending, device memory) from the store, brute force
void launch_pair_rows(const Stage2Params& q, const int32_t* sel, int S, double* out, hipStream_t stream);
// org_sum [n_markers][4] = the origin rows an origin sweep (SW_ORIGINS) left in org [n_ind][n_markers][4], added over the n_ind
// individuals in ascending order, one thread per column (no atomics: the same bits on every call; a skipped individual's
// rows are zeros)
void launch_origin_finish(const double* org, int n_ind, int n_markers, double* org_sum, hipStream_t stream);
// Which instantiation of fb_fast_kernel a launch takes.  half: alpha-minus spilled at every second marker (not
// CNF2_FULL_SPILL); xpose: the transposing variant of the plain sweep; tied: the tile producer with a pass per tie
// combination (windows with tie groups).  SW_WEIGHTS forms no per-locus rows: windows with tie groups can take it untied
// (the posterior weights do not see the tie rule).
// n_uniform ({SW_PLAIN, half} only): how many of the launch's jobs belong to windows with slots_uniform (cnf2_emission.h);
// they are swept by the UNI instantiation (grid_uniform blocks, job counter job_next_uniform), the rest -- if any -- by the
// ordinary one behind it on the stream.  0 (CNF2_ALL_STATES): every job through the ordinary instantiation.
struct FastVariant {
    SweepVariant storew;
    bool         half = true, xpose = false, tied = false;
    int          n_uniform = 0, grid_uniform = 0;
    int*         job_next_uniform = nullptr;
    // the lines whose records the UNI launch reads (KernelParams::line_rec has room for n_lines of them; 0 = no records), and
    // how many of the n_uniform jobs belong to windows without their lines among them: those are swept by
    // the UNI instantiation with SW_PLAIN_UNIFORM_ROWS (job counter job_next_uniform + 1)
    const LineKey* lines = nullptr;
    int          n_lines = 0, n_uniform_rows = 0;
    // groups of four jobs swept by fb_unipack_kernel in front of the UNI launches (grid_pack blocks, job counter
    // job_next_uniform + 2).  Their 4 n_pack_groups jobs are the LAST of the launch's p.n_jobs jobs and are not among the n_uniform:
    // the other kernels sweep the jobs before them, the logarithms are taken of all
    const PackedJob* pack_groups = nullptr;
    int          n_pack_groups = 0, grid_pack = 0;
    // of which the first 2 n_pack_eights form pairs swept by fb_unipack8_kernel, eight jobs to a wave, in front of the others
    // (pair_uniform_groups; grid_pack8 blocks, job counter job_next_uniform + 3)
    int          n_pack_eights = 0, grid_pack8 = 0;
};
// Zeroes the launch's job counter, launches the instantiation (asking once for the tied instantiations' dynamic LDS) and
// the kernel that takes the logarithms of its likelihoods.  Returns the launches' error; a combination that is not
// instantiated is hipErrorInvalidValue, never another kernel.
hipError_t launch_fb_fast(const KernelParams& p, int grid, FastVariant v, hipStream_t stream);
void launch_fb_packed(const KernelParams& p, int grid, hipStream_t stream);
void launch_row_flags(const uint8_t* allele8, const double2* sure, int n_rows, int n_markers, uint8_t* flags,
                      hipStream_t stream);
int  fb_fast_blocks_per_cu();
int  fb_fast_uniform_blocks_per_cu();
void launch_emission(const KernelParams& p, int ind, int marker, double* out, hipStream_t stream);
void launch_emission_paths(const KernelParams& p, int marker, double* out, hipStream_t stream);
void launch_xor_selftest(double* out, hipStream_t stream);
int  fb_blocks_per_cu();

} // namespace cnf2
#endif
