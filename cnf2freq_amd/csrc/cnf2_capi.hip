// cnf2_capi.hip -- implementation of the C ABI declared in include/cnf2hip.h.
// Host side only: owns device memory, derives the window tables, builds the job list and
// launches the kernels of cnf2_kernels.hip on the context's stream.  There is no CPU
// compute path here: without a usable HIP device every entry point fails.
#include "../../include/cnf2hip.h"

#include <hip/hip_runtime.h>
#include <math.h>
#include <cmath>
#include <stdarg.h>
#include <chrono>
#include <stdio.h>
#include <string.h>

#include <string>
#include <algorithm>
#include <vector>

#include "cnf2_device.h"
#include "cnf2_emission.h"
#include "cnf2_emtab.h"
#include "cnf2_plan.h"
#include "cnf2_qtl.h"
#include "cnf2_qtlplan.h"
#include "cnf2_qtl2.h"
#include "cnf2_qtlx.h"
#include "cnf2_qtlcof.h"
#include "cnf2_qtlem.h"
#include "cnf2_qtlbin.h"
#include "cnf2_qtlsurv.h"
#include "cnf2_qtlvar.h"
#include "cnf2_kinship.h"
#include "cnf2_qtlcols.h"
#include "cnf2_qtlboot.h"
#include "cnf2_qtlmv.h"
#include "cnf2_qtlimp.h"
#include "cnf2_qtlfam.h"
#include "cnf2_qtlhap.h"
#include "cnf2_qtlvc.h"

using namespace cnf2;

struct cnf2_ctx;
static int fail(cnf2_ctx* ctx, int code, const char* fmt, ...);

#define HIP_TRY(ctx, call)                                                                     \
    do {                                                                                       \
        hipError_t e_ = (call);                                                                \
        if (e_ != hipSuccess)                                                                  \
            return fail(ctx, e_ == hipErrorOutOfMemory ? CNF2_ERR_NOMEM : CNF2_ERR_HIP,        \
                        "%s failed: %s", #call, hipGetErrorString(e_));                        \
    } while (0)
#define RC_TRY(call)                                                                           \
    do {                                                                                       \
        const int rc_ = (call);                                                                \
        if (rc_) return rc_;                                                                   \
    } while (0)

// A device buffer the context owns: freed with the context (cnf2_ctx_destroy), so a new one cannot be forgotten there.
template <class T>
struct DevBuf {
    T*     ptr = nullptr;
    size_t cap = 0;          // elements
    DevBuf() = default;
    DevBuf(const DevBuf&) = delete;
    DevBuf& operator=(const DevBuf&) = delete;
    ~DevBuf() { (void)hipFree(ptr); }
    operator T*() const { return ptr; }
    int release(cnf2_ctx* ctx)
    {
        if (ptr) HIP_TRY(ctx, hipFree(ptr));
        ptr = nullptr;
        cap = 0;
        return CNF2_OK;
    }
    // exactly `count` elements, whatever was held (freed first)
    int alloc(cnf2_ctx* ctx, size_t count)
    {
        RC_TRY(release(ctx));
        HIP_TRY(ctx, hipMalloc((void**)&ptr, count * sizeof(T)));
        cap = count;
        return CNF2_OK;
    }
    // at least `count` elements: what is held if it suffices, else exactly `count`
    int ensure(cnf2_ctx* ctx, size_t count) { return (cap >= count && ptr) ? CNF2_OK : alloc(ctx, count); }
};

// What each of the four iteratively fitted scans keeps (qtl_fit_scan): the marker map (chromstarts, marker -> chromosome, tiles
// of 4, tile starts), which effects a marker keeps, which chromosomes are scanned, the null fits, the tile maxima, and the
// staged outputs
struct QtlFitBufs {
    DevBuf<double>  null, tilemax, lod, coef, ll0, pmax;      // ll0: the EM scan's rss0
    DevBuf<int32_t> map, keep, scan, nc, rank, iters, status;
};

// the scans whose column tile the caller can cap (cnf2_set_*_columns); the column scan shares the single scan's, and the
// multi-trait scan's cap counts groups (cnf2_set_qtlmv_groups)
enum QtlCap { QTL_CAP_SCAN, QTL_CAP_SCAN2, QTL_CAP_SCANX, QTL_CAP_COF, QTL_CAP_EM, QTL_CAP_BIN, QTL_CAP_MV, QTL_CAP_SURV, QTL_CAP_VAR, QTL_CAP_IMP, QTL_CAP_COUNT };

struct cnf2_ctx {
    int         device = -1;
    hipStream_t stream = nullptr;
    hipStream_t stream2 = nullptr;   // tied windows (general kernel) run beside the fast kernel
    hipEvent_t  ev0 = nullptr, ev1 = nullptr, ev2 = nullptr;
    bool        timed = false;
    std::string err;
    int         n_cu = 0;
    int         blocks_per_cu = 1;

    // map
    int                  n_markers = 0, n_chrom = 0;
    std::vector<int32_t> chromstarts;
    double               genrec[3] = {-0.02, -0.02, -0.02};
    DevBuf<double2>      d_rho, d_tq;
    DevBuf<double>       d_logk;

    // rows
    int             n_rows = 0;
    DevBuf<uint8_t> d_allele8;
    DevBuf<double2> d_sure;
    DevBuf<double>  d_hw;

    // pedigree
    HostPedigree        ped;
    std::vector<Window> windows;     // one per analysed individual
    DevBuf<Window>      d_windows;
    bool                windows_dirty = true;   // rows or pedigree changed since the last derivation
    DevBuf<uint8_t>     d_rowflags;
    int                 fast_blocks_per_cu = 1;
    int                 uni_blocks_per_cu = 1;   // the fast kernel's instantiation for uniform windows
    int                 reserve_blocks = 0;     // workgroup slots left free for concurrent kernels (RCCL)
    int                 batch_jobs = 0;         // cap on the jobs per batch of the batched consumers (0 = what memory allows)

    // line records of the uniform windows (cnf2_emtab.h): the call's lines, the two lines of every window of the call, the
    // records; host images and the lookup table are kept so that a call allocates nothing in steady state
    int                  line_cap = -1;            // cnf2_set_line_records (negative: no cap of its own)
    int32_t              last_lines[4] = {0, 0, 0, 0};   // cnf2_last_line_records
    int32_t              last_pack[2] = {0, 0};          // cnf2_last_uniform_pack
    int32_t              last_pack8[2] = {0, 0};         // cnf2_last_uniform_pack8
    unsigned             windows_gen = 0;          // counts the derivations of `windows`
    // what h_lines / h_line_keys and their device copies describe: a call with the same windows, range and cap reuses them
    bool                 lines_valid = false;
    unsigned             lines_gen = 0;
    int                  lines_begin = 0, lines_n = 0, lines_cap = 0;
    int                  lines_fit = 1 << 30;      // lines the memory had room for when the record buffer last had to grow
    std::vector<LineKey> h_lines;
    std::vector<int32_t> h_line_keys, h_line_hash;
    DevBuf<LineKey>      d_lines;
    DevBuf<int32_t>      d_line_keys;
    DevBuf<LineRec>      d_line_rec;

    // the plan of the last sweep (cnf2_plan.h PlanKey): the job list as grouped, the groups of four, the groups as paired and
    // the counts formed from them; d_jobs, d_pjobs and d_upjobs hold their device copies.  A sweep with an equal key reuses it
    unsigned               map_gen = 0;            // counts the uploads of the map
    bool                   plan_valid = false;
    PlanKey                plan_key;
    JobPlan                plan_list;
    std::vector<PackedJob> plan_fours, plan_groups;
    size_t                 plan_n_uniform = 0, plan_n_on_records = 0, plan_n_eights = 0;
    int                    last_plan_reused = 0;   // cnf2_last_plan_reused
    float                  last_plan_ms = 0.f;     // cnf2_last_plan_ms

    // workspace
    DevBuf<Job>       d_jobs;
    DevBuf<PackedJob> d_pjobs;
    DevBuf<double>    d_spill;
    DevBuf<double>    d_factors, d_loglik, d_dosage;
    DevBuf<int32_t>   d_lexp;                  // binary exponents of the fast kernel's likelihoods: [n][C][8] then [n][C]
    DevBuf<unsigned long long> d_clock;        // [4] clock stamps of the last plain fast-kernel launch
    DevBuf<PackedJob> d_upjobs;                // the groups of four of fb_unipack_kernel (group_uniform_jobs)
    DevBuf<int>       d_jobnext;               // [7] job counters of the fast-kernel launches in flight (KernelParams::job_next)
    DevBuf<double>    d_scratch;               // small parity buffers

    // crossover posteriors (cnf2_sweep_crossovers)
    DevBuf<double>  d_xo_f;               // likelihoods of the second pass over tied windows (any mode; not reported)
    int             xo_blocks_per_cu = 1; // occupancy of the general kernel's crossover instantiation
    DevBuf<double>  d_xo;                 // [n][n_markers][6] per-individual rows (host-output calls that ask for them)
    DevBuf<double>  d_xo_sum;             // [n_markers][6]
    DevBuf<int32_t> d_xo_cnt;             // [n_chrom]

    // Viterbi decoding (cnf2_sweep_viterbi), host-output calls
    DevBuf<double>  d_vit_lm;             // [n][n_chrom][8]
    DevBuf<uint8_t> d_vit_st;             // [n][n_markers]
    DevBuf<int32_t> d_vit_sh;             // [n][n_chrom]

    // posterior sampling (cnf2_sweep_sample), host-output calls
    DevBuf<uint8_t> d_smp_st;             // [n][K][n_markers]
    DevBuf<int32_t> d_smp_sh;             // [n][K][n_chrom]
    DevBuf<double>  d_smp_lp;             // [n][K][n_chrom]

    // leave-one-marker-out rows (cnf2_sweep_loo): the rows a call did not hand device memory for, and its staged sums
    DevBuf<double>  d_loo, d_unl;         // [n][n_markers]
    DevBuf<double>  d_loo_sum, d_unl_sum; // [n_markers]

    // origin rows (cnf2_sweep_origins): the rows a call did not hand device memory for, and its staged sums
    DevBuf<double>  d_org;                // [n][n_markers][4]
    DevBuf<double>  d_obits;              // [n][n_markers][6]
    DevBuf<double>  d_descent;            // descent rows (cnf2_sweep_descent) a call did not hand device memory for: [n][n_markers][8]
    DevBuf<double>  d_org_sum;            // [n_markers][4]

    // pair rows (cnf2_sweep_pairs): the selection as the kernels read it (sel, the chromosomes' ranges in it, the pair
    // offsets), the rows a call did not hand device memory for, and its staged sums
    DevBuf<int32_t> d_pair_map;
    DevBuf<double>  d_pair;               // [n][n_pairs][16]
    DevBuf<double>  d_pair_sum;           // [n_pairs][16]

    // QTL scan (cnf2_qtl_scan, cnf2_sweep_qtl): staged inputs, design, the column image of a tile, staged outputs
    int             qtl_columns[QTL_CAP_COUNT] = {};   // caps on the columns per tile (cnf2_set_*_columns; 0 = what memory allows)
    int             qtl_rows_n = 0;       // individuals whose rows the last cnf2_sweep_qtl left in d_org: 0 (none to vouch for) after
                                          // every upload of a map, rows or a pedigree and every other use of d_org
    int             qtl_rows_m = 0;       // ... and the markers of those rows
    DevBuf<double>  d_q_pheno, d_q_cov, d_q_Y, d_q_null, d_q_mk, d_q_chol, d_q_tilemax;
    DevBuf<double>  d_q_lod, d_q_coef, d_q_rss0, d_q_pmax;
    DevBuf<uint8_t> d_q_use, d_q_cmask;
    DevBuf<int32_t> d_q_perm, d_q_map, d_q_nc, d_q_rank;   // d_q_map: chromstarts, marker -> chromosome, tiles, tile starts

    // two-QTL pair scan (cnf2_qtl_scan2): the per-pair sums of the null design, the chunk maxima, staged
    // outputs; the staged inputs, the mask and the column image are the single scan's buffers
    DevBuf<double>  d_q2_yy, d_q2_chunkmax, d_q2_lod_add, d_q2_lod_full, d_q2_rss0, d_q2_pmax;
    DevBuf<int32_t> d_q2_map, d_q2_nc, d_q2_rank_add, d_q2_rank_full;   // d_q2_map: chromstarts, sel, the chromosomes of sel

    // extended single-locus scan (cnf2_qtl_scanx): sum c y^2 per chromosome, the tile maxima, staged outputs;
    // the staged inputs, the mask and the column image are the single scan's buffers
    DevBuf<double>  d_qx_yy, d_qx_tilemax, d_qx_lod, d_qx_coef, d_qx_rss0, d_qx_pmax;
    DevBuf<int32_t> d_qx_map, d_qx_nc, d_qx_rank;   // d_qx_map: chromstarts, tiles, tile starts

    // cofactor scan (cnf2_qtl_scan_cof): the cofactor columns, sum c y^2 per chromosome, the tile maxima,
    // staged outputs; the staged inputs, the mask and the column image are the single scan's buffers
    DevBuf<double>  d_qc_img, d_qc_yy, d_qc_tilemax, d_qc_lod, d_qc_lod_base, d_qc_coef, d_qc_rss0, d_qc_pmax;
    DevBuf<int32_t> d_qc_map, d_qc_nc, d_qc_rank, d_qc_rank_cof;   // d_qc_map: chromstarts, tiles, tile starts, cof, their chromosomes' starts, skip words

    // The four scans that fit a model by iteration per (marker, column) -- cnf2_qtl_scan_em, _binary, _surv, _var -- run through
    // one driver (qtl_fit_scan) on one QtlFitBufs each; what only one of them has stands beside its instance.  The staged
    // inputs, the mask and the column image are the single scan's buffers, and for the EM scan the factor and the null fit
    // too (d_q_chol only receives what qtl_chrom_kernel writes beside the mask: the other three do not read it).
    QtlFitBufs       qe;                             // EM: no scan words, no null fits of its own
    DevBuf<double>   d_qe_sigma2, d_qe_rss0_null;    // _null: what qtl_null_kernel reports
    QtlFitBufs       qb;                             // binary
    DevBuf<int32_t>  d_qb_ones;
    QtlFitBufs       qs;                             // survival (the times are staged as the phenotypes and read by no kernel)
    DevBuf<int32_t>  d_qs_events;
    DevBuf<uint32_t> d_qs_ord;                       // the order words of a column tile
    DevBuf<double>   d_qs_work;                      // the waves' work rows
    int              qtlsurv_blocks = 0;             // cnf2_set_qtlsurv_blocks
    QtlFitBufs       qv;                             // variance: three fits per cell
    DevBuf<double>   d_qv_coefv;                     // the full fit's coefficients of the variance part

    // kinship sums (cnf2_kinship_sums): the image a[m_pad][n_pad], the chunks' partial sums of a split range, the staged sum
    DevBuf<double>  d_kin_image, d_kin_part, d_kin_sum;

    // column scan (cnf2_qtl_scan_cols): staged regressors and inputs, the factor, the marker records, the column image of a
    // tile, its null fit, the tile maxima, staged outputs; the column cap is the single scan's (cnf2_set_qtl_columns)
    DevBuf<double>  d_ql_reg, d_ql_scale, d_ql_x0, d_ql_pheno, d_ql_chol, d_ql_mk, d_ql_Y, d_ql_null, d_ql_tilemax;
    DevBuf<double>  d_ql_lod, d_ql_coef, d_ql_rss0, d_ql_pmax;
    DevBuf<int32_t> d_ql_perm, d_ql_rank;

    // bootstrap scan (cnf2_qtl_scan_boot): the counts, the weight image of a replicate tile, the (replicate, chromosome)
    // records, the tile maxima with their markers, staged outputs; the staged phenotypes, covariates and mask are the single
    // scan's buffers
    DevBuf<double>  d_qo_W, d_qo_rec, d_qo_tilemax, d_qo_max, d_qo_lod;
    DevBuf<int32_t> d_qo_count, d_qo_map, d_qo_tilearg, d_qo_arg, d_qo_nb;   // d_qo_map: first markers, tiles, tile starts
    DevBuf<uint8_t> d_qo_cmask;

    // multi-trait scan (cnf2_qtl_scan_mv): the (chromosome, group) records of a group tile, the tile maxima, staged outputs;
    // the staged inputs, the masks, the factors, the marker records and the image are the single scan's buffers
    DevBuf<double>  d_qm_rec, d_qm_tilemax, d_qm_lod, d_qm_pmax;
    DevBuf<int32_t> d_qm_map, d_qm_nc, d_qm_rank, d_qm_trank;   // d_qm_map: as d_q_map

    // multiple-imputation scan (cnf2_qtl_scan_imp): staged host states, the marker records of every draw, the two words of the
    // check, the tile maxima, staged outputs; the staged inputs, the masks, the factors, the image and the null fit are the
    // single scan's buffers
    DevBuf<uint8_t> d_qi_state;
    DevBuf<double>  d_qi_mkd, d_qi_tilemax, d_qi_lod, d_qi_coef, d_qi_rss0, d_qi_pmax, d_qi_draw;
    DevBuf<int32_t> d_qi_map, d_qi_bad, d_qi_nc, d_qi_rank;   // d_qi_map: as d_q_map

    // within-family scan (cnf2_qtl_scan_fam): the centred covariates and column image in gather order, the chromosome, family
    // and marker records, the null fits, the tile maxima, the observed columns' gamma, staged outputs; the staged inputs and
    // the masks are the single scan's buffers
    DevBuf<double>  d_qf_Z, d_qf_Y, d_qf_chrom, d_qf_rec, d_qf_hrec, d_qf_null, d_qf_tilemax, d_qf_gamma;
    DevBuf<double>  d_qf_lod, d_qf_slope, d_qf_rss0, d_qf_pmax;
    DevBuf<int32_t> d_qf_map, d_qf_nc, d_qf_ncells, d_qf_df;   // d_qf_map: as d_q_map, then the gather list (cnf2_qtlfam.h)

    // founder-haplotype scan (cnf2_qtl_scan_hap): the marker records (packed factor and G), the kept masks, the null fits, the
    // tile maxima, staged outputs; host descent rows are staged in d_descent; the staged inputs, the masks, the Cholesky
    // factors and the column image are the single scan's buffers
    DevBuf<double>   d_qh_rec, d_qh_null, d_qh_tilemax, d_qh_lod, d_qh_coef, d_qh_rss0, d_qh_pmax;
    DevBuf<uint32_t> d_qh_kept;
    DevBuf<int32_t>  d_qh_map, d_qh_nc, d_qh_df;   // d_qh_map: as d_q_map on tiles of two markers, then col and the gather list (cnf2_qtlhap.h)

    // variance-component scan (cnf2_qtl_scan_vc): the marker records (eigenvalues, Qt, G, grid tables), the null fits, the tile
    // maxima, staged outputs; the rest as in the founder-haplotype scan
    DevBuf<double>  d_qv_rec, d_qv_null, d_qv_tilemax, d_qv_lod, d_qv_h, d_qv_sigma2, d_qv_blup, d_qv_eval, d_qv_rss0, d_qv_pmax;
    DevBuf<int32_t> d_qv_map, d_qv_nc, d_qv_rank;   // d_qv_map: as d_qh_map

    // marker placement (cnf2_sweep_place)
    DevBuf<uint8_t> d_pl_allele8;         // [n_rows][Q] candidate rows
    DevBuf<double2> d_pl_sure;
    DevBuf<double>  d_pl_hw;
    DevBuf<double>  d_pl_emis;            // [n][qcap][512] candidate emission tables
    DevBuf<double>  d_pl_out;             // [n][Q][n_markers] (host-output calls that ask for it)
    DevBuf<double>  d_pl_sum, d_pl_null;  // [Q][n_markers], [Q]
    DevBuf<int32_t> d_pl_nz;              // [Q][n_markers]

    // batched HOT LOOP 2 (cnf2_sweep_accumulate)
    std::vector<int32_t> slot_rec;   // [n_dous][7] record per window slot (derive_window), -1 none
    DevBuf<int32_t> d_slot_rec;
    DevBuf<int32_t> d_desc;          // [n_rec]; allocated together with d_rec_empty (ensure_rec_tables)
    DevBuf<uint8_t> d_rec_empty;
    DevBuf<double>  d_wbuf;
    DevBuf<double>  d_acc_inf, d_acc_hb, d_acc_hc, d_acc_hz;

    // per-iteration updates (cnf2_update_pass) and pre-processing scans
    DevBuf<uint8_t> d_prior_allele8;
    DevBuf<double2> d_prior_sure;
    DevBuf<uint8_t> d_has_prior;         // [n_rec]
    bool            priors_set = false;
    DevBuf<int32_t> d_row_of, d_children;    // [n_rec], allocated together
    DevBuf<int32_t> d_chromstarts;       // [65536]
    DevBuf<uint8_t> d_anyinfo;
    DevBuf<double>  d_fw, d_ratio;
    DevBuf<int>     d_hits;              // [1]
    DevBuf<unsigned long long> d_flow_next;   // [32]
    DevBuf<double>  d_flow_out;
    DevBuf<double>  d_todo;              // flows set aside by the scouts (3 doubles each)
    DevBuf<double>  d_part;              // CNF2_DETERMINISTIC rows
    DevBuf<int32_t> d_gather;            // rec_start [n_rec + 1] followed by the list
    DevBuf<int32_t> d_pathlog;
    int             pathlog_n = 0;
    DevBuf<int32_t> d_updrecs;           // the records an update pass is restricted to
    DevBuf<int32_t> d_xidx;              // index lists of the exchange packers
    DevBuf<uint8_t> d_xbuf;              // staging buffer of the exchanges (cnf2_exchange_buffer)
    DevBuf<Window>  d_scanwin;
    DevBuf<uint8_t> d_okout;
};

static std::string g_create_error;

static int fail(cnf2_ctx* ctx, int code, const char* fmt, ...)
{
    char    buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof(buf), fmt, ap);
    va_end(ap);
    if (ctx) ctx->err = buf;
    else g_create_error = buf;
    return code;
}

// ------------------------------------------------------------------------------------------------
// Function templates of the entry points below (outside their extern "C" block), and what they use of it
// ------------------------------------------------------------------------------------------------
static int ready(cnf2_ctx* ctx);
static int run_store(cnf2_ctx* ctx, int ind, int chrom, Stage2Params* q, size_t extra, double** extra_ptr);

// The body the stage-2 queries share: the store of (ind, chrom), `launch(q, d_out)` fills n doubles behind it, and they are
// copied to `out`.  marker (the single-marker queries) must lie on the chromosome.
template <class Launch>
static int stage2_query(cnf2_ctx* ctx, int ind, int chrom, const int* marker, size_t n, double* out, Launch launch)
{
    Stage2Params q;
    double*      d_out = nullptr;
    RC_TRY(run_store(ctx, ind, chrom, &q, n, &d_out));
    if (marker && (*marker < q.first || *marker >= q.first + q.len))
        return fail(ctx, CNF2_ERR_ARG, "marker not on this chromosome");
    launch(q, d_out);
    HIP_TRY(ctx, hipGetLastError());
    HIP_TRY(ctx, hipMemcpyAsync(out, d_out, n * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    return CNF2_OK;
}

// ... with per_marker doubles for every marker of the chromosome
template <class Launch>
static int stage2_rows(cnf2_ctx* ctx, int ind, int chrom, size_t per_marker, double* rows_out, Launch launch)
{
    RC_TRY(ready(ctx));
    if (chrom < 0 || chrom >= ctx->n_chrom) return fail(ctx, CNF2_ERR_ARG, "chromosome out of range");
    const size_t n = (size_t)(ctx->chromstarts[chrom + 1] - ctx->chromstarts[chrom]) * per_marker;
    return stage2_query(ctx, ind, chrom, nullptr, n, rows_out, launch);
}

// An output of a sweep mode.  With CNF2_OUT_DEVICE (`dev`) the caller's pointer is device memory and the kernels write
// through it; else it is host memory (null: not asked for) and the output is staged whole in `buf`.  *field = where the
// kernels write, null for none.
template <class T>
static int stage_out(cnf2_ctx* ctx, bool dev, T* user, DevBuf<T>& buf, size_t count, T** field)
{
    *field = user;
    if (dev || !user) return CNF2_OK;
    *field = nullptr;
    if (count == 0) return CNF2_OK;
    RC_TRY(buf.ensure(ctx, count));
    *field = buf;
    return CNF2_OK;
}
// ... and a staged output back to the caller's host memory
template <class T>
static int fetch_out(cnf2_ctx* ctx, T* user, const T* staged, size_t count)
{
    if (staged) HIP_TRY(ctx, hipMemcpyAsync(user, staged, count * sizeof(T), hipMemcpyDeviceToHost, ctx->stream));
    return CNF2_OK;
}

// The outputs of a QTL scan are written down once, as a function `list(each)` that hands `each` the four things of every
// output -- the caller's pointer, the context's staging buffer, the element count, the kernels' field -- and returns the
// first status that is not CNF2_OK.  Both walks below go through that one list.  An output the caller did not ask for, or
// one without elements, has a null field after staging, and fetch_out skips it.
template <class List>
static int qtl_stage_outputs(cnf2_ctx* ctx, bool dev, List& list)
{
    return list([&](auto* user, auto& buf, size_t count, auto** field) { return stage_out(ctx, dev, user, buf, count, field); });
}
// ... back to the caller's host memory (nothing to do for device outputs), then the stream is drained
template <class List>
static int qtl_fetch_outputs(cnf2_ctx* ctx, bool dev, List& list)
{
    if (!dev) RC_TRY(list([&](auto* user, auto&, size_t count, auto** field) { return fetch_out(ctx, user, *field, count); }));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    return CNF2_OK;
}

// What the two batched consumers (cnf2_sweep_accumulate, cnf2_sweep_turn_scan) share before their launches: the job list on
// the device, the plan of grid and batches from the memory that is free (cnf2_plan.h), and the spill slots
struct Batched {
    JobPlan   list;        // untied windows (fast kernel) first, tied ones after
    BatchPlan plan;
    int       max_len = 0; // longest chromosome
};
// The launches of a batched consumer: the untied windows' jobs (pass 0), then the tied ones' (pass 1), in batches.  Sets
// p->jobs / p->n_jobs and hands `body` -- the sweep launch and the consumer's -- the pass, the sweep's grid and the length
// of the batch's longest job, which is its first (chrom_order)
template <class Body>
static int for_each_batch(cnf2_ctx* ctx, const Batched& b, KernelParams* p, Body body)
{
    const std::vector<Job>& jobs = b.list.jobs;
    for (int pass = 0; pass < 2; pass++) {
        const size_t lo = pass ? b.list.n_fast : 0, hi = pass ? jobs.size() : b.list.n_fast;
        for (size_t b0 = lo; b0 < hi; b0 += b.plan.batch) {
            const size_t nb = std::min(hi - b0, b.plan.batch);
            p->jobs   = ctx->d_jobs + b0;
            p->n_jobs = (int)nb;
            RC_TRY(body(pass, grid_for(nb, b.plan.grid_cap), jobs[b0].last - jobs[b0].first + 1));
        }
    }
    return CNF2_OK;
}

extern "C" {

const char* cnf2_version(void) { return "cnf2hip 0.1 (gfx950)"; }

int cnf2_device_count(void)
{
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

const char* cnf2_last_error(const cnf2_ctx* ctx) { return ctx ? ctx->err.c_str() : g_create_error.c_str(); }

int cnf2_ctx_create(int device, cnf2_ctx** out)
{
    if (!out) return fail(nullptr, CNF2_ERR_ARG, "out is NULL");
    *out = nullptr;
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n <= 0)
        return fail(nullptr, CNF2_ERR_NO_DEVICE, "no HIP device available (this library has no CPU fallback)");
    if (device < 0 || device >= n) return fail(nullptr, CNF2_ERR_ARG, "device %d out of range (%d devices)", device, n);
    cnf2_ctx* ctx = new cnf2_ctx();
    ctx->device   = device;
    hipError_t e  = hipSetDevice(device);
    if (e == hipSuccess) e = hipStreamCreate(&ctx->stream);
    if (e == hipSuccess) e = hipStreamCreate(&ctx->stream2);
    if (e == hipSuccess) e = hipEventCreate(&ctx->ev0);
    if (e == hipSuccess) e = hipEventCreate(&ctx->ev1);
    if (e == hipSuccess) e = hipEventCreateWithFlags(&ctx->ev2, hipEventDisableTiming);
    hipDeviceProp_t prop;
    if (e == hipSuccess) e = hipGetDeviceProperties(&prop, device);
    if (e != hipSuccess) {
        fail(nullptr, CNF2_ERR_HIP, "context creation failed: %s", hipGetErrorString(e));
        delete ctx;
        return CNF2_ERR_HIP;
    }
    ctx->n_cu          = prop.multiProcessorCount;
    ctx->blocks_per_cu = fb_blocks_per_cu();
    ctx->fast_blocks_per_cu = fb_fast_blocks_per_cu();
    ctx->uni_blocks_per_cu  = fb_fast_uniform_blocks_per_cu();
    ctx->xo_blocks_per_cu = fb_xo_blocks_per_cu();
    *out = ctx;
    return CNF2_OK;
}

void cnf2_ctx_destroy(cnf2_ctx* ctx)
{
    if (!ctx) return;
    (void)hipSetDevice(ctx->device);
    (void)hipStreamSynchronize(ctx->stream);
    const hipStream_t stream = ctx->stream, stream2 = ctx->stream2;
    const hipEvent_t  ev0 = ctx->ev0, ev1 = ctx->ev1, ev2 = ctx->ev2;
    delete ctx;                      // frees every device buffer (DevBuf) before the streams and events go
    (void)hipEventDestroy(ev0);
    (void)hipEventDestroy(ev1);
    (void)hipEventDestroy(ev2);
    (void)hipStreamDestroy(stream2);
    (void)hipStreamDestroy(stream);
}

void* cnf2_stream(cnf2_ctx* ctx) { return ctx ? (void*)ctx->stream : nullptr; }

int cnf2_set_grid_reserve(cnf2_ctx* ctx, int blocks)
{
    if (!ctx || blocks < 0) return CNF2_ERR_ARG;
    ctx->reserve_blocks = blocks;
    return CNF2_OK;
}

int cnf2_set_batch_jobs(cnf2_ctx* ctx, int jobs)
{
    if (!ctx || jobs < 0) return CNF2_ERR_ARG;
    ctx->batch_jobs = jobs;
    return CNF2_OK;
}

static int set_columns(cnf2_ctx* ctx, QtlCap which, int cap)
{
    if (!ctx) return CNF2_ERR_ARG;
    if (cap < 0) return fail(ctx, CNF2_ERR_ARG, "the column cap must not be negative");
    ctx->qtl_columns[which] = cap;
    return CNF2_OK;
}
int cnf2_set_qtl_columns(cnf2_ctx* ctx, int cap) { return set_columns(ctx, QTL_CAP_SCAN, cap); }
int cnf2_set_qtl2_columns(cnf2_ctx* ctx, int cap) { return set_columns(ctx, QTL_CAP_SCAN2, cap); }
int cnf2_set_qtlx_columns(cnf2_ctx* ctx, int cap) { return set_columns(ctx, QTL_CAP_SCANX, cap); }
int cnf2_set_qtlcof_columns(cnf2_ctx* ctx, int cap) { return set_columns(ctx, QTL_CAP_COF, cap); }
int cnf2_set_qtlem_columns(cnf2_ctx* ctx, int cap) { return set_columns(ctx, QTL_CAP_EM, cap); }
int cnf2_set_qtlbin_columns(cnf2_ctx* ctx, int cap) { return set_columns(ctx, QTL_CAP_BIN, cap); }
int cnf2_set_qtlmv_groups(cnf2_ctx* ctx, int cap) { return set_columns(ctx, QTL_CAP_MV, cap); }
int cnf2_set_qtlsurv_columns(cnf2_ctx* ctx, int cap) { return set_columns(ctx, QTL_CAP_SURV, cap); }
int cnf2_set_qtlvar_columns(cnf2_ctx* ctx, int cap) { return set_columns(ctx, QTL_CAP_VAR, cap); }
int cnf2_set_qtlimp_columns(cnf2_ctx* ctx, int cap) { return set_columns(ctx, QTL_CAP_IMP, cap); }
int cnf2_set_qtlsurv_blocks(cnf2_ctx* ctx, int cap)
{
    if (!ctx) return CNF2_ERR_ARG;
    if (cap < 0 || cap > 65536) return fail(ctx, CNF2_ERR_ARG, "the block cap must be 0 .. 65536");
    ctx->qtlsurv_blocks = cap;
    return CNF2_OK;
}

int cnf2_sync(cnf2_ctx* ctx)
{
    if (!ctx) return CNF2_ERR_ARG;
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    return CNF2_OK;
}

int cnf2_upload_map(cnf2_ctx* ctx, const double* pos, int n_markers, const int32_t* chromstarts, int n_chrom,
                    const double* genrec)
{
    if (!ctx || !pos || !chromstarts || n_markers <= 0 || n_chrom <= 0) return fail(ctx, CNF2_ERR_ARG, "bad map arguments");
    if (chromstarts[0] != 0 || chromstarts[n_chrom] != n_markers)
        return fail(ctx, CNF2_ERR_ARG, "chromstarts must run from 0 to n_markers");
    for (int c = 0; c < n_chrom; c++)
        if (chromstarts[c + 1] <= chromstarts[c]) return fail(ctx, CNF2_ERR_ARG, "empty chromosome %d", c);
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    if (ctx->n_markers != n_markers && (ctx->d_allele8 || ctx->d_sure || ctx->d_hw))
        return fail(ctx, CNF2_ERR_STATE, "marker count changed after rows were uploaded");
    ctx->qtl_rows_n = 0;               // (the rows a cnf2_sweep_qtl left have the old map's shape)
    ctx->n_markers = n_markers;
    ctx->n_chrom   = n_chrom;
    ctx->chromstarts.assign(chromstarts, chromstarts + n_chrom + 1);
    ctx->map_gen++;
    if (genrec) memcpy(ctx->genrec, genrec, sizeof(ctx->genrec));
    // recombination fraction per gap, exactly as realanalyze forms it (cnF2freq.cpp:2270-2286);
    // a gap with dist <= 0 performs no transition (cnF2freq.cpp:2273) == rho 0
    std::vector<double2> rho(n_markers);
    for (int m = 0; m < n_markers; m++) {
        double2 r = make_double2(0.0, 0.0);
        if (m + 1 < n_markers) {
            double dist = pos[m + 1] - pos[m];
            if (dist > 0) {
                r.x = 0.5 * (1.0 - exp(ctx->genrec[0] * dist));
                r.y = 0.5 * (1.0 - exp(ctx->genrec[1] * dist));
            }
        }
        rho[m] = r;
    }
    RC_TRY(ctx->d_rho.alloc(ctx, n_markers));
    HIP_TRY(ctx, hipMemcpy(ctx->d_rho, rho.data(), sizeof(double2) * n_markers, hipMemcpyHostToDevice));
    // fast kernel: butterflies x' = x + t * partner with t = r / (1 - r); the dropped scalar
    // (1-r0)^4 (1-r1)^2 per gap (bits with TYPEGENS 0: four, TYPEGENS 1: two, settings.h:23) is
    // accounted for in the log-likelihoods through its logarithm summed over each chromosome
    std::vector<double2> tq(n_markers);
    std::vector<double>  logk(n_chrom, 0.0);
    for (int c = 0; c < n_chrom; c++)
        for (int m = chromstarts[c]; m < chromstarts[c + 1]; m++) {
            tq[m] = make_double2(rho[m].x / (1.0 - rho[m].x), rho[m].y / (1.0 - rho[m].y));
            if (m + 1 < chromstarts[c + 1]) logk[c] += 4.0 * log1p(-rho[m].x) + 2.0 * log1p(-rho[m].y);
        }
    RC_TRY(ctx->d_tq.release(ctx));
    RC_TRY(ctx->d_logk.release(ctx));
    RC_TRY(ctx->d_tq.alloc(ctx, n_markers));
    RC_TRY(ctx->d_logk.alloc(ctx, n_chrom));
    HIP_TRY(ctx, hipMemcpy(ctx->d_tq, tq.data(), sizeof(double2) * n_markers, hipMemcpyHostToDevice));
    HIP_TRY(ctx, hipMemcpy(ctx->d_logk, logk.data(), sizeof(double) * n_chrom, hipMemcpyHostToDevice));
    return CNF2_OK;
}

static int copy_rows(cnf2_ctx* ctx, int row0, int n, const uint8_t* allele, const double* sure, const double* hw)
{
    const size_t M = ctx->n_markers;
    const size_t cnt = (size_t)n * M;
    // pack (a0, a1) into one byte on the host, in slabs to bound the staging buffer
    const size_t slab = 1u << 24;
    std::vector<uint8_t> packed(cnt < slab ? cnt : slab);
    for (size_t off = 0; off < cnt; off += slab) {
        size_t k = cnt - off < slab ? cnt - off : slab;
        for (size_t i = 0; i < k; i++) {
            uint8_t a0 = allele[(off + i) * 2], a1 = allele[(off + i) * 2 + 1];
            if (a0 > 15 || a1 > 15) return fail(ctx, CNF2_ERR_ARG, "allele value out of range");
            packed[i] = (uint8_t)(a0 | (a1 << 4));
        }
        HIP_TRY(ctx, hipMemcpy(ctx->d_allele8 + (size_t)row0 * M + off, packed.data(), k, hipMemcpyHostToDevice));
    }
    HIP_TRY(ctx, hipMemcpy(ctx->d_sure + (size_t)row0 * M, sure, cnt * sizeof(double2), hipMemcpyHostToDevice));
    HIP_TRY(ctx, hipMemcpy(ctx->d_hw + (size_t)row0 * M, hw, cnt * sizeof(double), hipMemcpyHostToDevice));
    return CNF2_OK;
}

static int blank_rows(cnf2_ctx* ctx)
{
    const size_t cnt = (size_t)ctx->n_rows * ctx->n_markers;
    HIP_TRY(ctx, hipMemset(ctx->d_allele8, 0, cnt));
    HIP_TRY(ctx, hipMemset(ctx->d_sure, 0, cnt * sizeof(double2)));
    // haploweight of an individual without data is 0.5 (getind, cnF2freq.cpp:2491)
    // (one row from the host, then the filled part copied onto the rest, doubling: ~log2(rows) copies instead of one per row)
    const size_t        M = (size_t)ctx->n_markers;
    std::vector<double> half(M, 0.5);
    HIP_TRY(ctx, hipMemcpy(ctx->d_hw, half.data(), sizeof(double) * M, hipMemcpyHostToDevice));
    for (size_t filled = 1; filled < (size_t)ctx->n_rows; filled *= 2) {
        const size_t k = std::min(filled, (size_t)ctx->n_rows - filled);
        HIP_TRY(ctx, hipMemcpy(ctx->d_hw + filled * M, ctx->d_hw, sizeof(double) * M * k, hipMemcpyDeviceToDevice));
    }
    return CNF2_OK;
}

int cnf2_upload_rows(cnf2_ctx* ctx, int n_rows, const uint8_t* allele, const double* sure, const double* hw)
{
    const bool blank = !allele && !sure && !hw;
    if (!ctx || n_rows <= 0 || (!blank && (!allele || !sure || !hw))) return fail(ctx, CNF2_ERR_ARG, "bad row arguments");
    if (ctx->n_markers <= 0) return fail(ctx, CNF2_ERR_STATE, "upload the map before the rows");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    RC_TRY(ctx->d_allele8.release(ctx));
    RC_TRY(ctx->d_sure.release(ctx));
    RC_TRY(ctx->d_hw.release(ctx));
    ctx->n_rows = 0;
    size_t cnt = (size_t)n_rows * ctx->n_markers;
    RC_TRY(ctx->d_allele8.alloc(ctx, cnt));
    RC_TRY(ctx->d_sure.alloc(ctx, cnt));
    RC_TRY(ctx->d_hw.alloc(ctx, cnt));
    ctx->n_rows = n_rows;
    ctx->qtl_rows_n = 0;               // (the rows a cnf2_sweep_qtl left are no longer this state's)
    ctx->windows_dirty = true;
    ctx->priors_set = false;
    // a pedigree uploaded against a larger table would index past the new one: drop it, it must be uploaded again
    for (int32_t r : ctx->ped.row_of)
        if (r >= n_rows) {
            ctx->ped = HostPedigree();
            ctx->windows.clear();
            break;
        }
    if (blank) return blank_rows(ctx);
    return copy_rows(ctx, 0, n_rows, allele, sure, hw);
}

int cnf2_update_rows_device(cnf2_ctx* ctx, int row0, int n, const uint8_t* d_allele8, const double* d_sure,
                            const double* d_hw)
{
    if (!ctx || !d_allele8 || !d_sure || !d_hw) return fail(ctx, CNF2_ERR_ARG, "bad row arguments");
    if (!ctx->d_allele8) return fail(ctx, CNF2_ERR_STATE, "no rows uploaded");
    if (row0 < 0 || n < 0 || row0 + n > ctx->n_rows) return fail(ctx, CNF2_ERR_ARG, "row range out of bounds");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    const size_t M = ctx->n_markers, cnt = (size_t)n * M;
    ctx->qtl_rows_n = 0;               // (the rows a cnf2_sweep_qtl left are no longer this state's)
    ctx->windows_dirty = true;
    HIP_TRY(ctx, hipMemcpyAsync(ctx->d_allele8 + (size_t)row0 * M, d_allele8, cnt, hipMemcpyDeviceToDevice, ctx->stream));
    HIP_TRY(ctx, hipMemcpyAsync(ctx->d_sure + (size_t)row0 * M, d_sure, cnt * sizeof(double2), hipMemcpyDeviceToDevice, ctx->stream));
    HIP_TRY(ctx, hipMemcpyAsync(ctx->d_hw + (size_t)row0 * M, d_hw, cnt * sizeof(double), hipMemcpyDeviceToDevice, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    return CNF2_OK;
}

int cnf2_update_rows(cnf2_ctx* ctx, int row0, int n, const uint8_t* allele, const double* sure, const double* hw)
{
    if (!ctx || !allele || !sure || !hw) return fail(ctx, CNF2_ERR_ARG, "bad row arguments");
    if (!ctx->d_allele8) return fail(ctx, CNF2_ERR_STATE, "no rows uploaded");
    if (row0 < 0 || n < 0 || row0 + n > ctx->n_rows) return fail(ctx, CNF2_ERR_ARG, "row range out of bounds");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    if (n == 0) return CNF2_OK;
    ctx->qtl_rows_n = 0;               // (the rows a cnf2_sweep_qtl left are no longer this state's)
    ctx->windows_dirty = true;
    return copy_rows(ctx, row0, n, allele, sure, hw);
}

int cnf2_upload_pedigree(cnf2_ctx* ctx, int n_rec, const int32_t* par, const uint8_t* empty, const int32_t* gen,
                         const int32_t* row_of, const int32_t* dous, int n_dous)
{
    if (!ctx || n_rec <= 0 || !par || !empty || !gen || !row_of || !dous || n_dous < 0)
        return fail(ctx, CNF2_ERR_ARG, "bad pedigree arguments");
    if (ctx->n_rows <= 0) return fail(ctx, CNF2_ERR_STATE, "upload the rows before the pedigree");
    for (int r = 0; r < n_rec; r++) {
        for (int k = 0; k < 2; k++)
            if (par[r * 2 + k] < -1 || par[r * 2 + k] >= n_rec) return fail(ctx, CNF2_ERR_ARG, "parent index out of range at record %d", r);
        if (row_of[r] < 0 || row_of[r] >= ctx->n_rows) return fail(ctx, CNF2_ERR_ARG, "row index out of range at record %d", r);
    }
    for (int j = 0; j < n_dous; j++)
        if (dous[j] < 0 || dous[j] >= n_rec) return fail(ctx, CNF2_ERR_ARG, "analysed record out of range at %d", j);
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    HostPedigree& P = ctx->ped;
    P.n_rec = n_rec;
    P.par.assign(par, par + 2 * (size_t)n_rec);
    P.empty.assign(empty, empty + n_rec);
    P.gen.assign(gen, gen + n_rec);
    P.row_of.assign(row_of, row_of + n_rec);
    P.dous.assign(dous, dous + n_dous);
    derive_founders(P);
    P.row_hom.clear();
    ctx->windows.assign(n_dous, Window());
    ctx->qtl_rows_n = 0;               // (the rows a cnf2_sweep_qtl left are no longer this state's)
    ctx->windows_dirty = true;
    ctx->priors_set = false;         // the per-record prior flags belong to the pedigree that was replaced
    return CNF2_OK;
}

// (Re)derive the window tables: per-row "always homozygous" flags from the device rows, then
// fixtrees per analysed individual.  Runs lazily before a sweep after rows or pedigree changed.
static int prepare_windows(cnf2_ctx* ctx)
{
    if (!ctx->windows_dirty) return CNF2_OK;
    HostPedigree& P = ctx->ped;
    const int n_dous = (int)P.dous.size();
    RC_TRY(ctx->d_rowflags.alloc(ctx, ctx->n_rows));
    launch_row_flags(ctx->d_allele8, ctx->d_sure, ctx->n_rows, ctx->n_markers, ctx->d_rowflags, ctx->stream);
    HIP_TRY(ctx, hipGetLastError());
    P.row_hom.assign(ctx->n_rows, 0);
    HIP_TRY(ctx, hipMemcpyAsync(P.row_hom.data(), ctx->d_rowflags, ctx->n_rows, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    ctx->windows.resize(n_dous);
    ctx->slot_rec.assign((size_t)n_dous * 7, -1);
    for (int j = 0; j < n_dous; j++) derive_window(P, P.dous[j], &ctx->windows[j], ctx->slot_rec.data() + (size_t)j * 7);
    RC_TRY(ctx->d_windows.release(ctx));
    RC_TRY(ctx->d_slot_rec.release(ctx));
    if (n_dous > 0) {
        RC_TRY(ctx->d_windows.alloc(ctx, n_dous));
        HIP_TRY(ctx, hipMemcpy(ctx->d_windows, ctx->windows.data(), sizeof(Window) * n_dous, hipMemcpyHostToDevice));
        RC_TRY(ctx->d_slot_rec.alloc(ctx, (size_t)7 * n_dous));
        HIP_TRY(ctx, hipMemcpy(ctx->d_slot_rec, ctx->slot_rec.data(), sizeof(int32_t) * 7 * n_dous, hipMemcpyHostToDevice));
    }
    ctx->windows_dirty = false;
    ctx->windows_gen++;
    ctx->lines_fit = 1 << 30;
    return CNF2_OK;
}

int cnf2_window_info(cnf2_ctx* ctx, int ind, int32_t* out17)
{
    if (!ctx || !out17) return CNF2_ERR_ARG;
    if (ind < 0 || ind >= (int)ctx->windows.size()) return fail(ctx, CNF2_ERR_ARG, "individual out of range");
    Window  w;
    int32_t slot_rec[7];
    {
        // topology exactly as fixtrees leaves it: tie groups are not pruned by row content here
        std::vector<uint8_t> keep;
        keep.swap(ctx->ped.row_hom);
        derive_window(ctx->ped, ctx->ped.dous[ind], &w, slot_rec);
        keep.swap(ctx->ped.row_hom);
    }
    out17[0] = w.shiftignore;
    out17[1] = w.flag2ignore;
    out17[2] = ctx->ped.founder[ctx->ped.dous[ind]];
    for (int i = 0; i < 7; i++) {
        out17[3 + i]  = slot_rec[i];
        out17[10 + i] = w.tie[i];
    }
    return CNF2_OK;
}

int cnf2_window_table(cnf2_ctx* ctx, int32_t* out17_all)
{
    if (!ctx || !out17_all) return CNF2_ERR_ARG;
    const int n = (int)ctx->windows.size();
    for (int j = 0; j < n; j++) {
        RC_TRY(cnf2_window_info(ctx, j, out17_all + (size_t)j * 17));
    }
    return CNF2_OK;
}

// the per-record tables of the accumulate and update kernels: one capacity, freed and allocated together
static int ensure_rec_tables(cnf2_ctx* ctx, size_t n_rec)
{
    if (ctx->d_desc.cap >= n_rec && ctx->d_rec_empty.cap >= n_rec) return CNF2_OK;
    RC_TRY(ctx->d_desc.release(ctx));
    RC_TRY(ctx->d_rec_empty.release(ctx));
    RC_TRY(ctx->d_desc.alloc(ctx, n_rec));
    return ctx->d_rec_empty.alloc(ctx, n_rec);
}

static int ready(cnf2_ctx* ctx)
{
    if (!ctx) return CNF2_ERR_ARG;
    if (!ctx->d_rho || !ctx->d_allele8 || ctx->ped.n_rec == 0)
        return fail(ctx, CNF2_ERR_STATE, "map, rows and pedigree must be uploaded first");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    RC_TRY(prepare_windows(ctx));
    const size_t ne = ctx->windows.size() * (size_t)ctx->n_chrom;
    RC_TRY(ctx->d_lexp.ensure(ctx, ne * 9 + 1));
    if (!ctx->d_clock) {
        RC_TRY(ctx->d_clock.ensure(ctx, (size_t)4));
        HIP_TRY(ctx, hipMemsetAsync(ctx->d_clock, 0, 4 * sizeof(unsigned long long), ctx->stream));
    }
    RC_TRY(ctx->d_jobnext.ensure(ctx, (size_t)7));
    return CNF2_OK;
}

static void base_params(cnf2_ctx* ctx, KernelParams* p)
{
    memset(p, 0, sizeof(*p));
    p->windows   = ctx->d_windows;
    p->allele8   = ctx->d_allele8;
    p->sure      = ctx->d_sure;
    p->hw        = ctx->d_hw;
    p->rho       = ctx->d_rho;
    p->tq        = ctx->d_tq;
    p->chrom_logk = ctx->d_logk;
    p->n_markers = ctx->n_markers;
    p->n_chrom   = ctx->n_chrom;
    p->fexp      = ctx->d_lexp;
    p->lexp      = ctx->d_lexp + ctx->windows.size() * (size_t)ctx->n_chrom * 8;
    p->job_next  = ctx->d_jobnext;
}

static int longest_chrom(const cnf2_ctx* ctx) { return max_chrom_len(ctx->chromstarts.data(), ctx->n_chrom); }

// the job list (cnf2_plan.h) of the analysed individuals [ind_begin, ind_begin + n)
static JobPlan job_plan(const cnf2_ctx* ctx, int ind_begin, int n, uint32_t flags)
{
    return plan_jobs(ctx->windows.data(), ctx->chromstarts.data(), ctx->n_chrom, ind_begin, n, flags, ctx->ped.row_hom.data());
}

// What a sweep leaves besides the likelihoods: its mode with that mode's device outputs
struct SweepMode {
    SweepVariant variant = SW_PLAIN;   // SW_PLAIN (cnf2_sweep: the rows), SW_CROSSOVERS, SW_VITERBI, SW_SAMPLING, SW_LOO, SW_ORIGINS or SW_DESCENT
    // SW_CROSSOVERS (cnf2_sweep_crossovers)
    double*  xo = nullptr;             // [n][n_markers][6] or null
    double*  xo_sum = nullptr;         // [n_markers][6], zeroed by the caller
    int32_t* xo_cnt = nullptr;         // [n_chrom], zeroed by the caller (SW_LOO, SW_ORIGINS and SW_DESCENT too)
    // SW_LOO (cnf2_sweep_loo): what the sweep leaves for loo_finish_kernel
    double*  loo = nullptr;            // [n][n_markers]
    double*  unl = nullptr;            // [n][n_markers]
    // SW_ORIGINS (cnf2_sweep_origins)
    double*  org = nullptr;            // [n][n_markers][4]; SW_DESCENT (cnf2_sweep_descent): [n][n_markers][8]
    double*  obits = nullptr;          // [n][n_markers][6]
    // SW_VITERBI (cnf2_sweep_viterbi) and, with a leading [K] of draws per individual, SW_SAMPLING (cnf2_sweep_sample)
    uint8_t* state = nullptr;          // [n][n_markers]
    int32_t* shift = nullptr;          // [n][n_chrom]
    double*  logmax = nullptr;         // Viterbi: [n][n_chrom][8]
    double*  logp = nullptr;           // sampling: [n][K][n_chrom] or null
    int      draws = 0;                // sampling: K
    unsigned long long seed = 0;       // sampling: the generator's seed
};

// The lines (cnf2_emtab.h LineKey) of the uniform windows among [ind_begin, ind_begin + n): every distinct one gets a number
// in order of appearance, up to `cap`; ctx->h_line_keys [n][2] = the numbers of a window's two lines, or -1 -1 where the window
// keeps the ordinary producer: not uniform, a line beyond the cap, or a founder as root or parent -- with all four
// grandparents present the parents are present too (derive_window), but a parent whose own parents are empty records is a
// founder, and so may the root be: those branches of the producer are not in the records.  Returns the number of lines.
// Linear in n; the lookup is an open-addressing table of 4 * CNF2_MAX_LINES entries the context keeps.
enum { CNF2_MAX_LINES = 64 };
static int assign_lines(cnf2_ctx* ctx, int ind_begin, int n, int cap)
{
    const int H = 4 * CNF2_MAX_LINES;
    ctx->h_line_keys.resize((size_t)2 * n);
    ctx->h_line_hash.assign(H, -1);
    ctx->h_lines.clear();
    ctx->h_lines.reserve(CNF2_MAX_LINES);
    cap = std::min(cap, (int)CNF2_MAX_LINES);
    LineKey prev[2];             // the last key looked up per side, and what it got: neighbours mostly repeat it
    int     prev_found[2] = {-1, -1};
    bool    prev_set[2] = {false, false};
    for (int i = 0; i < n; i++) {
        const Window& w = ctx->windows[ind_begin + i];
        int32_t k[2] = {-1, -1};
        const bool ok = slots_uniform(w.flags) && !((w.flags[0] | w.flags[1] | w.flags[4]) & SLOT_FOUNDER);
        for (int P = 0; ok && P < 2; P++) {
            const int s = 1 + 3 * P;
            if (w.row[s] < 0 || w.row[s + 1] < 0 || w.row[s + 2] < 0) break;
            LineKey key;
            key.row_par = w.row[s];
            key.row_a   = w.row[s + 1];
            key.row_b   = w.row[s + 2];
            key.fl_par  = w.flags[s];
            key.fl_a    = w.flags[s + 1];
            key.fl_b    = w.flags[s + 2];
            key.pad     = 0;
            if (prev_set[P] && memcmp(&prev[P], &key, sizeof(key)) == 0) {
                k[P] = prev_found[P];
                continue;
            }
            uint32_t h = (uint32_t)key.row_par * 0x9e3779b1u ^ (uint32_t)key.row_a * 0x85ebca6bu ^ (uint32_t)key.row_b * 0xc2b2ae35u ^
                         ((uint32_t)key.fl_par << 16 | (uint32_t)key.fl_a << 8 | key.fl_b);
            h ^= h >> 15;
            int slot = (int)(h % (uint32_t)H), found = -1;
            for (;; slot = (slot + 1) % H) {
                const int e = ctx->h_line_hash[slot];
                if (e < 0) break;
                if (memcmp(&ctx->h_lines[e], &key, sizeof(key)) == 0) {
                    found = e;
                    break;
                }
            }
            if (found < 0 && (int)ctx->h_lines.size() < cap) {
                found = (int)ctx->h_lines.size();
                ctx->h_lines.push_back(key);
                ctx->h_line_hash[slot] = found;
            }
            k[P] = found;
            prev[P] = key;
            prev_found[P] = found;
            prev_set[P] = true;
        }
        const bool both = k[0] >= 0 && k[1] >= 0;
        ctx->h_line_keys[2 * (size_t)i]     = both ? k[0] : -1;
        ctx->h_line_keys[2 * (size_t)i + 1] = both ? k[1] : -1;
    }
    return (int)ctx->h_lines.size();
}
// assign_lines and the upload of its two tables, unless the context holds them for these windows, this range and this cap
// already (the windows change with the rows or the pedigree, not from sweep to sweep).  *n_lines = the number of lines.
static int prepare_lines(cnf2_ctx* ctx, int ind_begin, int n, int cap, int* n_lines)
{
    cap = std::max(0, std::min(cap, (int)CNF2_MAX_LINES));
    if (!(ctx->lines_valid && ctx->lines_gen == ctx->windows_gen && ctx->lines_begin == ind_begin && ctx->lines_n == n &&
          ctx->lines_cap == cap)) {
        ctx->lines_valid = false;
        HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));      // (an earlier call's copies have read the host tables)
        const int nl = assign_lines(ctx, ind_begin, n, cap);
        if (nl > 0) {
            RC_TRY(ctx->d_lines.ensure(ctx, (size_t)CNF2_MAX_LINES));
            RC_TRY(ctx->d_line_keys.ensure(ctx, (size_t)2 * n));
            HIP_TRY(ctx, hipMemcpyAsync(ctx->d_lines, ctx->h_lines.data(), sizeof(LineKey) * nl, hipMemcpyHostToDevice, ctx->stream));
            HIP_TRY(ctx, hipMemcpyAsync(ctx->d_line_keys, ctx->h_line_keys.data(), sizeof(int32_t) * 2 * n, hipMemcpyHostToDevice, ctx->stream));
        }
        ctx->lines_gen   = ctx->windows_gen;
        ctx->lines_begin = ind_begin;
        ctx->lines_n     = n;
        ctx->lines_cap   = cap;
        ctx->lines_valid = true;
    }
    *n_lines = (int)ctx->h_lines.size();
    return CNF2_OK;
}

// cnf2_sweep, and its modes.  Crossover mode: the untied windows through the fast kernel's crossover instantiation (one
// pass: likelihoods and posteriors), the tied ones through the tied kernel without rows (their likelihoods, as cnf2_sweep
// forms them) and then the general kernel's crossover instantiation (their posteriors).  Viterbi mode: the same routing,
// with the fast kernel's Viterbi instantiation in place of both crossover instantiations.  Sampling mode: the untied windows
// through the fast kernel's sampling instantiation (one pass: likelihoods and draws), the tied ones through the tied kernel
// without rows (likelihoods) and then the same sampling instantiation (draws).  Leave-one-out, origin and descent mode:
// sampling's routing with the fast kernel's leave-one-out / origin / descent instantiation
static int sweep_impl(cnf2_ctx* ctx, int ind_begin, int ind_end, double* factors_out, double* loglik_out, double* dosage_out,
                      uint32_t flags, const SweepMode& mode)
{
    RC_TRY(ready(ctx));
    const int n_all = (int)ctx->windows.size();
    if (ind_begin < 0 || ind_end > n_all || ind_begin > ind_end) return fail(ctx, CNF2_ERR_ARG, "individual range out of bounds");
    const bool plain = mode.variant == SW_PLAIN;
    if (!plain) flags &= ~(uint32_t)(CNF2_MERGE_MODES | CNF2_XPOSE | CNF2_FLUSH_TINY | CNF2_NO_TIES | CNF2_RAW_DOSAGE);
    const bool want_dosage = !(flags & CNF2_NO_DOSAGE) && plain;
    if (!factors_out || !loglik_out || (want_dosage && !dosage_out)) return fail(ctx, CNF2_ERR_ARG, "output pointer is NULL");
    const int n = ind_end - ind_begin;
    if (n == 0) return CNF2_OK;
    HIP_TRY(ctx, hipSetDevice(ctx->device));

    if ((size_t)n * ctx->n_chrom > 0x7fffffff) return fail(ctx, CNF2_ERR_ARG, "too many jobs in one call");
    const auto t_plan = std::chrono::steady_clock::now();
    ctx->last_plan_reused = 0;
    memset(ctx->last_lines, 0, sizeof(ctx->last_lines));
    memset(ctx->last_pack, 0, sizeof(ctx->last_pack));
    memset(ctx->last_pack8, 0, sizeof(ctx->last_pack8));

    // the plain half-spill sweep: the fast jobs of uniform windows (slots_uniform: crosses of inbred lines) take the fast
    // kernel's instantiation for them (launch_fb_fast), which has an occupancy of its own; the spill slots cover the larger grid
    // ... and, unless CNF2_NO_LINE_RECORDS, the lines of those windows (numbered once per set of windows, range and cap)
    int        n_lines = 0;
    const bool uni_ok = !(flags & (CNF2_ALL_STATES | CNF2_FULL_SPILL | CNF2_XPOSE)) && (plain || mode.variant == SW_VITERBI);
    int        want_lines = ctx->line_cap >= 0 ? std::min(ctx->line_cap, ctx->lines_fit) : ctx->lines_fit;
    if (uni_ok && !(flags & CNF2_NO_LINE_RECORDS)) RC_TRY(prepare_lines(ctx, ind_begin, n, want_lines, &n_lines));

    // The plan (cnf2_plan.h PlanKey): the job list with the uniform jobs on records four to a wave (group_uniform_jobs: they
    // become the tail of the fast jobs), the counts, the uploads.  The context keeps it: a call with the key of the last one
    // builds, copies and uploads nothing and does not wait for the stream.
    PlanKey key;
    key.windows_gen       = ctx->windows_gen;
    key.map_gen           = ctx->map_gen;
    key.ind_begin         = ind_begin;
    key.n                 = n;
    key.flags             = flags & PLAN_KEY_FLAGS;
    key.uniform_mode      = uni_ok ? 1 : 0;
    key.reserve_blocks    = ctx->reserve_blocks;
    key.uni_blocks_per_cu = ctx->uni_blocks_per_cu;
    auto key_lines = [&]() {
        key.n_lines   = n_lines;
        key.lines_cap = want_lines;
        key.lines_fit = ctx->lines_fit;
    };
    key_lines();
    JobPlan&                jp = ctx->plan_list;
    std::vector<PackedJob>& fours = ctx->plan_fours;
    auto build_jobs = [&]() -> int {
        ctx->plan_valid = false;
        jp = job_plan(ctx, ind_begin, n, flags);
        RC_TRY(ctx->d_jobs.ensure(ctx, jp.jobs.size() + 1));
        if (!jp.pjobs.empty()) {
            RC_TRY(ctx->d_pjobs.ensure(ctx, jp.pjobs.size()));
            HIP_TRY(ctx, hipMemcpyAsync(ctx->d_pjobs, jp.pjobs.data(), sizeof(PackedJob) * jp.pjobs.size(), hipMemcpyHostToDevice, ctx->stream));
        }
        const int32_t* keys = uni_ok && n_lines > 0 ? ctx->h_line_keys.data() : nullptr;
        ctx->plan_n_uniform = ctx->plan_n_on_records = 0;
        for (size_t j = 0; uni_ok && j < jp.n_fast; j++) {
            const int i = jp.jobs[j].ind;
            if (!slots_uniform(ctx->windows[ind_begin + i].flags)) continue;
            ctx->plan_n_uniform++;
            if (keys && keys[2 * (size_t)i] >= 0) ctx->plan_n_on_records++;
        }
        fours.clear();
        size_t n_single = jp.n_fast;   // (the jobs in front of the groups': launch_fb_fast forms it from the groups' number)
        if (keys && !(flags & CNF2_NO_UNIFORM_PACK))
            fours = group_uniform_jobs(jp.jobs, jp.n_fast, ctx->windows.data() + ind_begin, keys, &n_single);
        if (!jp.jobs.empty())
            HIP_TRY(ctx, hipMemcpyAsync(ctx->d_jobs, jp.jobs.data(), sizeof(Job) * jp.jobs.size(), hipMemcpyHostToDevice, ctx->stream));
        HIP_TRY(ctx, hipStreamSynchronize(ctx->stream)); // (the copies have read the lists, which the next plan overwrites)
        return CNF2_OK;
    };
#ifdef CNF2_NO_PLAN_CACHE   /* A/B only: every call plans and uploads anew */
    ctx->plan_valid = false;
#endif
    bool same_jobs = ctx->plan_valid && plan_key_same_jobs(ctx->plan_key, key);
    if (!same_jobs) RC_TRY(build_jobs());
    // (the list's sizes do not depend on the lines: they stand where the lines change below)
    const size_t n_fast = jp.n_fast, n_general = jp.jobs.size() - n_fast, n_packed = jp.pjobs.size();

    // grids and spill: one slot per resident wave, the fast kernel's slots first
    const int    mlen = longest_chrom(ctx);
    const size_t stride = spill_stride(mlen);
    int          grid_fast = 0, grid_gen = 0;
    size_t       free_b = 0, total_b = 0;
    HIP_TRY(ctx, hipMemGetInfo(&free_b, &total_b));
    const size_t n_uniform0 = ctx->plan_n_uniform;
    const int fast_per_cu = n_uniform0 == 0       ? ctx->fast_blocks_per_cu
                            : n_uniform0 < n_fast ? std::max(ctx->fast_blocks_per_cu, ctx->uni_blocks_per_cu)
                                                  : ctx->uni_blocks_per_cu;
    if (!plan_sweep_grids(ctx->n_cu, fast_per_cu, ctx->blocks_per_cu, ctx->reserve_blocks, std::max(n_fast, n_packed),
                          n_general, free_b, ctx->d_spill.cap * sizeof(double), mlen, &grid_fast, &grid_gen))
        return fail(ctx, CNF2_ERR_NOMEM, "a chromosome of %d markers needs %zu MB of spill per block, %zu MB free", mlen,
                    spill_block_bytes(mlen) >> 20, free_b >> 20);
    RC_TRY(ctx->d_spill.ensure(ctx, (size_t)(grid_fast + grid_gen) * CNF2_WAVES_PER_BLOCK * stride));

    double *d_f, *d_l, *d_d = nullptr;
    const size_t nf = (size_t)n * ctx->n_chrom * 8, nl = (size_t)n * ctx->n_chrom, nd = (size_t)n * ctx->n_markers * 3;
    if (flags & CNF2_OUT_DEVICE) {
        d_f = factors_out;
        d_l = loglik_out;
        d_d = dosage_out;
    } else {
        RC_TRY(ctx->d_factors.ensure(ctx, nf));
        RC_TRY(ctx->d_loglik.ensure(ctx, nl));
        if (want_dosage) RC_TRY(ctx->d_dosage.ensure(ctx, nd));
        d_f = ctx->d_factors;
        d_l = ctx->d_loglik;
        d_d = ctx->d_dosage;
    }

    // the records of the call's lines, after the spill slots and the outputs: they take at most half of what is left
    if (ctx->plan_n_on_records == 0) n_lines = 0;
    if (n_lines > 0) {
        const size_t line_bytes = (size_t)ctx->n_markers * LINE_VALUES * 2 * sizeof(LineRec);
        if ((size_t)n_lines * line_bytes > ctx->d_line_rec.cap * sizeof(LineRec)) {
            // the buffer has to grow (not in steady state): lines beyond what fits keep the ordinary producer, from now on
            HIP_TRY(ctx, hipMemGetInfo(&free_b, &total_b));
            const size_t fit = (ctx->d_line_rec.cap * sizeof(LineRec) + free_b / 2) / line_bytes;
            if (fit < (size_t)n_lines) {
                ctx->lines_fit = (int)fit;
                want_lines     = std::min(want_lines, ctx->lines_fit);
                RC_TRY(prepare_lines(ctx, ind_begin, n, want_lines, &n_lines));
                key_lines();
                same_jobs = false;
                RC_TRY(build_jobs());
                if (ctx->plan_n_on_records == 0) n_lines = 0;
            }
        }
        if (n_lines > 0) RC_TRY(ctx->d_line_rec.ensure(ctx, (size_t)n_lines * ctx->n_markers * LINE_VALUES * 2));
    }
    const size_t n_uniform = ctx->plan_n_uniform, n_on_records = ctx->plan_n_on_records;
    ctx->last_lines[0] = n_lines;
    ctx->last_lines[1] = n_lines > 0 ? (int32_t)n_on_records : 0;
    ctx->last_lines[2] = (int32_t)n_uniform - ctx->last_lines[1];
    ctx->last_lines[3] = (int32_t)std::min<size_t>((size_t)n_lines * ctx->n_markers * LINE_VALUES * 2 * sizeof(LineRec), 0x7fffffff);
    const size_t n_groups = n_lines > 0 ? fours.size() : 0;
    ctx->last_pack[0] = (int32_t)(4 * n_groups);
    ctx->last_pack[1] = (int32_t)n_groups;
    // the groups' upload, once the call's lines and the grids stand: pairs of groups whose windows have all eight modes analysed
    // go eight jobs to a wave (pair_uniform_groups: a whole number of rounds of the packed grid's resident waves), in front
    const int pack_cap = std::min(grid_fast, resident_blocks(ctx->n_cu, ctx->uni_blocks_per_cu, ctx->reserve_blocks));
    key.pack_cap = pack_cap;
    if (!(same_jobs && plan_key_same(ctx->plan_key, key))) {
        std::vector<PackedJob>& ugroups = ctx->plan_groups;
        ctx->plan_valid    = false;
        ctx->plan_n_eights = 0;
        ugroups.clear();
        if (n_groups > 0) {
            ugroups = fours;
            if (!(flags & CNF2_NO_UNIFORM_PACK8))
                ctx->plan_n_eights = pair_uniform_groups(ugroups, ctx->windows.data() + ind_begin, (size_t)pack_cap * CNF2_WAVES_PER_BLOCK);
            RC_TRY(ctx->d_upjobs.ensure(ctx, ugroups.size()));
            HIP_TRY(ctx, hipMemcpyAsync(ctx->d_upjobs, ugroups.data(), sizeof(PackedJob) * ugroups.size(), hipMemcpyHostToDevice, ctx->stream));
            HIP_TRY(ctx, hipStreamSynchronize(ctx->stream)); // (the copy has read the vector)
        }
        ctx->plan_key   = key;
        ctx->plan_valid = true;
    } else ctx->last_plan_reused = 1;
    const size_t n_eights = ctx->plan_n_eights;
    ctx->last_pack8[0] = (int32_t)n_eights;
    ctx->last_pack8[1] = (int32_t)(8 * n_eights);

    KernelParams p;
    base_params(ctx, &p);
    p.windows      = ctx->d_windows + ind_begin;
    p.jobs         = ctx->d_jobs;
    p.n_jobs       = (int)n_fast;
    p.spill        = ctx->d_spill;
    p.spill_stride = stride;
    p.factors      = d_f;
    p.loglik       = d_l;
    p.dosage       = d_d;
    p.flags        = (want_dosage ? 0 : KP_NO_DOSAGE) | ((flags & CNF2_RAW_DOSAGE) ? KP_RAW_DOSAGE : 0) |
              ((flags & CNF2_NO_TIES) ? KP_NO_TIES : 0);
    if (flags & CNF2_STATIC_JOBS) p.job_next = nullptr;
    // per mode: the outputs, the flags of its own launches, and the occupancy of the kernel that makes the tied windows'
    // second pass (the general kernel's crossover instantiation; the fast kernel's Viterbi or sampling instantiation)
    int follow_per_cu = 0;
    switch (mode.variant) {
    case SW_CROSSOVERS:
        p.flags  = 0;           // (the crossover instantiations form no rows; KP_NO_DOSAGE would stop them after the forward pass)
        p.xo     = mode.xo;
        p.xo_sum = mode.xo_sum;
        p.xo_cnt = mode.xo_cnt;
        follow_per_cu = ctx->xo_blocks_per_cu;
        break;
    case SW_VITERBI:
        p.flags      = KP_NO_DOSAGE;
        p.vit_logmax = mode.logmax;
        p.vit_state  = mode.state;
        p.vit_shift  = mode.shift;
        follow_per_cu = ctx->fast_blocks_per_cu;
        break;
    case SW_SAMPLING:
        p.flags     = KP_NO_DOSAGE;
        p.smp_state = mode.state;
        p.smp_shift = mode.shift;
        p.smp_logp  = mode.logp;
        p.smp_draws = mode.draws;
        p.smp_seed  = mode.seed;
        p.smp_ind0  = ind_begin;
        follow_per_cu = ctx->fast_blocks_per_cu;
        break;
    case SW_LOO:
        p.flags  = KP_NO_DOSAGE;    // (no rows; the instantiation makes its backward pass all the same)
        p.loo    = mode.loo;
        p.unl    = mode.unl;
        p.xo_cnt = mode.xo_cnt;
        follow_per_cu = ctx->fast_blocks_per_cu;
        break;
    case SW_ORIGINS:
        p.flags  = KP_NO_DOSAGE;    // (no rows; the instantiation makes its backward pass all the same)
        p.org    = mode.org;
        p.obits  = mode.obits;
        p.xo_cnt = mode.xo_cnt;
        follow_per_cu = ctx->fast_blocks_per_cu;
        break;
    case SW_DESCENT:
        p.flags  = KP_NO_DOSAGE;    // (no rows; the instantiation makes its backward pass all the same)
        p.org    = mode.org;
        p.xo_cnt = mode.xo_cnt;
        follow_per_cu = ctx->fast_blocks_per_cu;
        break;
    default: break;
    }
    if (flags & CNF2_LOG_PATHS) {
        RC_TRY(ctx->d_pathlog.ensure(ctx, nl));
        HIP_TRY(ctx, hipMemsetAsync(ctx->d_pathlog, 0xff, nl * sizeof(int32_t), ctx->stream));
        p.path_log     = ctx->d_pathlog;
        ctx->pathlog_n = (int)nl;
    }
    const bool half = !(flags & CNF2_FULL_SPILL);
    // a launch whose likelihoods are not the ones reported (the tied windows' second pass, the Viterbi instantiation)
    auto likelihoods_to_scratch = [&](KernelParams* q) {
        q->factors = ctx->d_xo_f;
        q->loglik  = ctx->d_xo_f + (size_t)n * ctx->n_chrom * 8;
    };

    ctx->last_plan_ms = std::chrono::duration<float, std::milli>(std::chrono::steady_clock::now() - t_plan).count();
    HIP_TRY(ctx, hipEventRecord(ctx->ev0, ctx->stream));
    if (n_general > 0) {
        // the tied windows' kernel on a second stream with its own spill slots (behind the fast kernel's) and its own job
        // counter: no ordering between the two kernels.  It is launched FIRST: its jobs are the long ones (a backward pass
        // per tie combination), and blocks of either kernel that find no room wait and take jobs from their launch's counter
        // once they get on -- the sweep then ends on the short jobs of the untied windows
        KernelParams pt = p;
        HIP_TRY(ctx, hipStreamWaitEvent(ctx->stream2, ctx->ev0, 0));
        pt.jobs   = ctx->d_jobs + n_fast;
        pt.n_jobs = (int)n_general;
        if (pt.job_next) pt.job_next = ctx->d_jobnext + 1;
        pt.spill  = ctx->d_spill + (size_t)((n_fast > 0 || n_packed > 0) ? grid_fast : 0) * CNF2_WAVES_PER_BLOCK * stride;
        // the tile-producer kernel with a pass per tie combination; the general kernel (one lane per table entry, per-marker
        // producer) with the full spill and where asked for
        if (flags & CNF2_FLUSH_TINY) pt.flags |= KP_FLUSH_TINY;
        if (!plain) pt.flags = KP_NO_DOSAGE;    // crossover / Viterbi / sampling mode: likelihoods only here, the rest from the pass below
        if (flags & (CNF2_FULL_SPILL | CNF2_TIES_GENERAL | CNF2_FLUSH_TINY))
            HIP_TRY(ctx, launch_fb(pt, grid_gen, SW_PLAIN, ctx->stream2));
        else HIP_TRY(ctx, launch_fb_fast(pt, grid_gen, {SW_PLAIN, true, false, true}, ctx->stream2));
        if (!plain) {
            // the mode's instantiation over the tied jobs in the same spill slots (after the pass above on this stream): the
            // general kernel's for the crossovers; the fast kernel's for Viterbi, sampling, leave-one-out and origins (the
            // forward pass, the max-product recursion, the draws and alpha beta do not see the tie rule).  Its own likelihoods go to
            // scratch (the ones reported are the tied kernel's); its occupancy is its own
            KernelParams px = pt;
            likelihoods_to_scratch(&px);
            const int gx = std::min(resident_blocks(ctx->n_cu, follow_per_cu, ctx->reserve_blocks), grid_gen);
            if (mode.variant == SW_CROSSOVERS) HIP_TRY(ctx, launch_fb(px, gx, SW_CROSSOVERS, ctx->stream2));
            else HIP_TRY(ctx, launch_fb_fast(px, gx, {mode.variant, half}, ctx->stream2));
        }
        HIP_TRY(ctx, hipEventRecord(ctx->ev2, ctx->stream2));
    }
    if (n_packed > 0) {
        p.pjobs   = ctx->d_pjobs;
        p.n_pjobs = (int)n_packed;
        KernelParams pp = p;
        if (pp.job_next) pp.job_next = ctx->d_jobnext + 2;    // (the fast kernel behind it on the stream zeroes its own)
        launch_fb_packed(pp, std::min(grid_for(n_packed, grid_fast), resident_blocks(ctx->n_cu, ctx->fast_blocks_per_cu, ctx->reserve_blocks)),
                         ctx->stream);
        HIP_TRY(ctx, hipGetLastError());
    }
    if (n_fast > 0) {
        // (grid_fast covers the occupancy of whichever instantiations run; each takes what is resident of its own)
        const int gf = std::min(grid_for(n_fast, grid_fast), resident_blocks(ctx->n_cu, ctx->fast_blocks_per_cu, ctx->reserve_blocks));
        FastVariant plain_half{SW_PLAIN, half, half && (flags & CNF2_XPOSE)};
        // (the packed jobs are uniform jobs on records, the tail of the fast jobs: the UNI launches sweep the others)
        plain_half.n_uniform        = (int)(n_uniform - 4 * n_groups);
        plain_half.grid_uniform     = std::min(grid_for(n_uniform, grid_fast), resident_blocks(ctx->n_cu, ctx->uni_blocks_per_cu, ctx->reserve_blocks));
        plain_half.job_next_uniform = ctx->d_jobnext + 3;
        if (n_lines > 0) {
            plain_half.lines   = ctx->d_lines;
            plain_half.n_lines = n_lines;
            plain_half.n_uniform_rows = ctx->last_lines[2];
            p.line_rec         = ctx->d_line_rec;
            p.line_keys        = ctx->d_line_keys;
            if (n_groups > 0) {
                plain_half.pack_groups   = ctx->d_upjobs;
                plain_half.n_pack_groups = (int)n_groups;
                plain_half.n_pack_eights = (int)n_eights;
                plain_half.grid_pack     = grid_for(n_groups - 2 * n_eights, pack_cap);
                plain_half.grid_pack8    = grid_for(n_eights, pack_cap);
            }
        }
        p.clock_out = ctx->d_clock;
        if (mode.variant == SW_VITERBI) {
            // the likelihoods from cnf2_sweep's own launch without rows (the Viterbi instantiation runs the same recursion,
            // but compiled without the backward pass it does not round every job's factors the same way: DESIGN.md 8c), then
            // the Viterbi instantiation in the same spill slots with its likelihoods to scratch
            KernelParams pl = p;
            pl.flags = KP_NO_DOSAGE;
            HIP_TRY(ctx, launch_fb_fast(pl, gf, plain_half, ctx->stream));
            KernelParams pv = p;
            pv.clock_out = nullptr;
            likelihoods_to_scratch(&pv);
            HIP_TRY(ctx, launch_fb_fast(pv, gf, {SW_VITERBI, half}, ctx->stream));
        } else if (plain) HIP_TRY(ctx, launch_fb_fast(p, gf, plain_half, ctx->stream));
        else HIP_TRY(ctx, launch_fb_fast(p, gf, {mode.variant, half, half && (flags & CNF2_XPOSE)}, ctx->stream));
        p.clock_out = nullptr;
    }
    if (n_general > 0) HIP_TRY(ctx, hipStreamWaitEvent(ctx->stream, ctx->ev2, 0));
    HIP_TRY(ctx, hipEventRecord(ctx->ev1, ctx->stream));
    ctx->timed = true;

    if (!(flags & CNF2_OUT_DEVICE)) {
        HIP_TRY(ctx, hipMemcpyAsync(factors_out, d_f, nf * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
        HIP_TRY(ctx, hipMemcpyAsync(loglik_out, d_l, nl * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
        if (want_dosage)
            HIP_TRY(ctx, hipMemcpyAsync(dosage_out, d_d, nd * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
        HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    }
    return CNF2_OK;
}

int cnf2_sweep(cnf2_ctx* ctx, int ind_begin, int ind_end, double* factors_out, double* loglik_out, double* dosage_out,
               uint32_t flags)
{
    return sweep_impl(ctx, ind_begin, ind_end, factors_out, loglik_out, dosage_out, flags, SweepMode());
}

int cnf2_set_line_records(cnf2_ctx* ctx, int lines)
{
    if (!ctx) return CNF2_ERR_ARG;
    ctx->line_cap = lines;
    return CNF2_OK;
}

int cnf2_last_line_records(cnf2_ctx* ctx, int32_t* out)
{
    if (!ctx || !out) return fail(ctx, CNF2_ERR_ARG, "bad arguments");
    memcpy(out, ctx->last_lines, sizeof(ctx->last_lines));
    return CNF2_OK;
}

int cnf2_last_uniform_pack(cnf2_ctx* ctx, int32_t* out)
{
    if (!ctx || !out) return fail(ctx, CNF2_ERR_ARG, "bad arguments");
    memcpy(out, ctx->last_pack, sizeof(ctx->last_pack));
    return CNF2_OK;
}

int cnf2_last_uniform_pack8(cnf2_ctx* ctx, int32_t* out)
{
    if (!ctx || !out) return fail(ctx, CNF2_ERR_ARG, "bad arguments");
    memcpy(out, ctx->last_pack8, sizeof(ctx->last_pack8));
    return CNF2_OK;
}

int cnf2_last_plan_reused(cnf2_ctx* ctx) { return ctx ? ctx->last_plan_reused : 0; }

float cnf2_last_plan_ms(cnf2_ctx* ctx) { return ctx ? ctx->last_plan_ms : 0.f; }

int cnf2_last_paths(cnf2_ctx* ctx, int32_t* paths_out, int n)
{
    if (!ctx || !paths_out || n < 0) return fail(ctx, CNF2_ERR_ARG, "bad path arguments");
    if (!ctx->d_pathlog || n > ctx->pathlog_n) return fail(ctx, CNF2_ERR_STATE, "no sweep with CNF2_LOG_PATHS covers %d jobs", n);
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    HIP_TRY(ctx, hipMemcpy(paths_out, ctx->d_pathlog, (size_t)n * sizeof(int32_t), hipMemcpyDeviceToHost));
    return CNF2_OK;
}

int cnf2_last_kernel_ms(cnf2_ctx* ctx, float* kernel_ms, int n)
{
    if (!ctx || !kernel_ms || n < 1) return CNF2_ERR_ARG;
    if (!ctx->timed) return fail(ctx, CNF2_ERR_STATE, "no sweep has been launched");
    HIP_TRY(ctx, hipEventSynchronize(ctx->ev1));
    float ms = 0;
    HIP_TRY(ctx, hipEventElapsedTime(&ms, ctx->ev0, ctx->ev1));
    kernel_ms[0] = ms;
    for (int i = 1; i < n; i++) kernel_ms[i] = 0;
    return CNF2_OK;
}

int cnf2_sweep_clock(cnf2_ctx* ctx, double* mhz_out)
{
    if (!ctx || !mhz_out) return fail(ctx, CNF2_ERR_ARG, "bad arguments");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    *mhz_out = 0.0;
    if (!ctx->d_clock) return CNF2_OK;
    unsigned long long t[2] = {0, 0};
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    HIP_TRY(ctx, hipMemcpy(t, ctx->d_clock, sizeof(t), hipMemcpyDeviceToHost));
    int khz = 0;
    HIP_TRY(ctx, hipDeviceGetAttribute(&khz, hipDeviceAttributeWallClockRate, ctx->device));
    if (t[1] > 0 && khz > 0) *mhz_out = (double)t[0] / (double)t[1] * (double)khz * 1e-3;
    return CNF2_OK;
}

int cnf2_clock_probe(cnf2_ctx* ctx, double* mhz_out)
{
    if (!ctx || !mhz_out) return fail(ctx, CNF2_ERR_ARG, "bad arguments");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    RC_TRY(ctx->d_scratch.ensure(ctx, (size_t)8));
    const int iters = 1 << 20;
    hipEvent_t e0, e1;
    HIP_TRY(ctx, hipEventCreate(&e0));
    HIP_TRY(ctx, hipEventCreate(&e1));
    launch_clock_probe(ctx->n_cu, 1 << 14, ctx->d_scratch, ctx->stream);            // warm up
    HIP_TRY(ctx, hipEventRecord(e0, ctx->stream));
    launch_clock_probe(ctx->n_cu, iters, ctx->d_scratch, ctx->stream);
    HIP_TRY(ctx, hipEventRecord(e1, ctx->stream));
    HIP_TRY(ctx, hipEventSynchronize(e1));
    float ms = 0;
    HIP_TRY(ctx, hipEventElapsedTime(&ms, e0, e1));
    (void)hipEventDestroy(e0);
    (void)hipEventDestroy(e1);
    // per SIMD: 4 waves x 8 FMAs x iters, one wave-wide f64 FMA per 4 cycles
    *mhz_out = 4.0 * 8.0 * (double)iters * 4.0 / ((double)ms * 1e-3) / 1e6;
    return CNF2_OK;
}

size_t cnf2_workspace_bytes(cnf2_ctx* ctx)
{
    if (!ctx) return 0;
    const size_t doubles = ctx->d_spill.cap + ctx->d_factors.cap + ctx->d_loglik.cap + ctx->d_dosage.cap + ctx->d_scratch.cap +
                           ctx->d_wbuf.cap;
    return ctx->d_jobs.cap * sizeof(Job) + doubles * sizeof(double);
}

// Runs fb_kernel<true> for one individual x chromosome and leaves the reference-layout store in the
// context's scratch buffer; fills the Stage2Params view of it.  extra = doubles reserved after it.
static int run_store(cnf2_ctx* ctx, int ind, int chrom, Stage2Params* q, size_t extra, double** extra_ptr)
{
    RC_TRY(ready(ctx));
    if (ind < 0 || ind >= (int)ctx->windows.size() || chrom < 0 || chrom >= ctx->n_chrom)
        return fail(ctx, CNF2_ERR_ARG, "individual or chromosome out of range");
    const int    first = ctx->chromstarts[chrom], last = ctx->chromstarts[chrom + 1] - 1, len = last - first + 1;
    const size_t nfw = (size_t)8 * len * 3 * 64, nff = (size_t)8 * len * 3;
    const size_t stride = (size_t)len * 512;
    // scratch: fwbw | factors | spill(4 waves) | out factors(8) | loglik(8) | dosage(n_markers*3) | job(8) | extra
    const size_t total = nfw + nff + stride * CNF2_WAVES_PER_BLOCK + 16 + (size_t)ctx->n_markers * 3 + 8 + extra;
    RC_TRY(ctx->d_scratch.ensure(ctx, total));
    HIP_TRY(ctx, hipMemsetAsync(ctx->d_scratch, 0, (nfw + nff) * sizeof(double), ctx->stream));
    double* d_fw  = ctx->d_scratch;
    double* d_ff  = d_fw + nfw;
    double* d_sp  = d_ff + nff;
    double* d_f   = d_sp + stride * CNF2_WAVES_PER_BLOCK;
    double* d_l   = d_f + 8;
    double* d_d   = d_l + 8;
    Job*    d_job = (Job*)(d_d + (size_t)ctx->n_markers * 3);
    if (extra_ptr) *extra_ptr = d_d + (size_t)ctx->n_markers * 3 + 8;
    Job     jb;
    jb.ind = 0;
    jb.first = first;
    jb.last = last;
    jb.chrom = 0;
    HIP_TRY(ctx, hipMemcpyAsync(d_job, &jb, sizeof(jb), hipMemcpyHostToDevice, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    KernelParams p;
    base_params(ctx, &p);
    p.windows      = ctx->d_windows + ind;
    p.n_chrom      = 1;
    p.jobs         = d_job;
    p.n_jobs       = 1;
    p.spill        = d_sp;
    p.spill_stride = stride;
    p.factors      = d_f;
    p.loglik       = d_l;
    p.dosage       = d_d;   // rows of this individual, indexed by global marker
    p.flags        = KP_NO_DOSAGE;
    p.dbg_fwbw     = d_fw;
    p.dbg_factors  = d_ff;
    HIP_TRY(ctx, launch_fb(p, 1, SW_PLAIN, ctx->stream, true));
    q->kp          = p;
    q->fwbw        = d_fw;
    q->fwbwfactors = d_ff;
    q->factors     = d_f;
    q->loglik      = d_l;
    q->first       = first;
    q->len         = len;
    return CNF2_OK;
}

int cnf2_fwbw_store(cnf2_ctx* ctx, int ind, int chrom, double* fwbw_out, double* fwbwfactors_out)
{
    if (!ctx || !fwbw_out || !fwbwfactors_out) return fail(ctx, CNF2_ERR_ARG, "bad fwbw_store arguments");
    Stage2Params q;
    RC_TRY(run_store(ctx, ind, chrom, &q, 0, nullptr));
    const size_t nfw = (size_t)8 * q.len * 3 * 64, nff = (size_t)8 * q.len * 3;
    HIP_TRY(ctx, hipMemcpyAsync(fwbw_out, q.fwbw, nfw * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipMemcpyAsync(fwbwfactors_out, q.fwbwfactors, nff * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    return CNF2_OK;
}

int cnf2_locked_query(cnf2_ctx* ctx, int ind, int chrom, int marker, double* val_out)
{
    if (!ctx || !val_out) return fail(ctx, CNF2_ERR_ARG, "bad locked_query arguments");
    return stage2_query(ctx, ind, chrom, &marker, (size_t)8 * 64 * 128, val_out,
                        [&](const Stage2Params& q, double* d_out) { launch_locked_query(q, marker, d_out, ctx->stream); });
}

int cnf2_turn_scan(cnf2_ctx* ctx, int ind, int chrom, int marker, double* rawervals_out)
{
    if (!ctx || !rawervals_out) return fail(ctx, CNF2_ERR_ARG, "bad turn_scan arguments");
    return stage2_query(ctx, ind, chrom, &marker, 128 * 8, rawervals_out,
                        [&](const Stage2Params& q, double* d_out) { launch_turn_scan(q, marker, d_out, ctx->stream); });
}

int cnf2_turn_scan_rows(cnf2_ctx* ctx, int ind, int chrom, double* rows_out)
{
    if (!ctx || !rows_out) return fail(ctx, CNF2_ERR_ARG, "bad turn_scan_rows arguments");
    return stage2_rows(ctx, ind, chrom, 1024, rows_out,
                       [&](const Stage2Params& q, double* d_out) { launch_turn_scan_rows(q, d_out, ctx->stream); });
}

int cnf2_state_posterior(cnf2_ctx* ctx, int ind, int chrom, double* rows_out, uint32_t flags)
{
    if (!ctx || !rows_out) return fail(ctx, CNF2_ERR_ARG, "bad state_posterior arguments");
    const uint32_t kp = (flags & CNF2_NO_TIES) ? KP_NO_TIES : 0;
    return stage2_rows(ctx, ind, chrom, 64, rows_out,
                       [&](const Stage2Params& q, double* d_out) { launch_state_rows(q, kp, d_out, ctx->stream); });
}

int cnf2_crossover_rows(cnf2_ctx* ctx, int ind, int chrom, double* rows_out)
{
    if (!ctx || !rows_out) return fail(ctx, CNF2_ERR_ARG, "bad crossover_rows arguments");
    return stage2_rows(ctx, ind, chrom, 6, rows_out,
                       [&](const Stage2Params& q, double* d_out) { launch_crossover_rows(q, d_out, ctx->stream); });
}

// One pass of sweep_impl in a mode, for its three entry points (which have checked their arguments and staged their
// outputs): the scratch of the tied windows' second pass, the crossover sums zeroed (the kernels add to them), the flags
// that mean something to a mode
static int mode_sweep(cnf2_ctx* ctx, int ind_begin, int ind_end, double* factors_out, double* loglik_out, uint32_t flags,
                      const SweepMode& mode)
{
    const size_t n = (size_t)(ind_end - ind_begin);
    RC_TRY(ctx->d_xo_f.ensure(ctx, n * ctx->n_chrom * 9 + 1));
    if (mode.variant == SW_CROSSOVERS)
        HIP_TRY(ctx, hipMemsetAsync(mode.xo_sum, 0, (size_t)ctx->n_markers * 6 * sizeof(double), ctx->stream));
    if (mode.xo_cnt) HIP_TRY(ctx, hipMemsetAsync(mode.xo_cnt, 0, (size_t)ctx->n_chrom * sizeof(int32_t), ctx->stream));
    // (the A/B switches of the plain sweep's route: they reach the Viterbi mode's likelihood launch)
    const uint32_t pass = flags & (CNF2_OUT_DEVICE | CNF2_STATIC_JOBS | CNF2_FULL_SPILL | CNF2_TIES_GENERAL | CNF2_ALL_STATES |
                                   CNF2_NO_LINE_RECORDS | CNF2_NO_UNIFORM_PACK | CNF2_NO_UNIFORM_PACK8);
    return sweep_impl(ctx, ind_begin, ind_end, factors_out, loglik_out, nullptr, pass, mode);
}

static int mode_range(cnf2_ctx* ctx, int ind_begin, int ind_end)
{
    if (ind_begin < 0 || ind_end > (int)ctx->windows.size() || ind_begin > ind_end)
        return fail(ctx, CNF2_ERR_ARG, "individual range out of bounds");
    return CNF2_OK;
}

// one pass of sweep_impl's crossover mode: the sums are zeroed first and added to by the kernels (an empty range reports
// them as zeros)
int cnf2_sweep_crossovers(cnf2_ctx* ctx, int ind_begin, int ind_end, double* factors_out, double* loglik_out,
                          double* xo_out, double* xo_sum_out, int32_t* n_contrib_out, uint32_t flags)
{
    RC_TRY(ready(ctx));
    if (!xo_sum_out || !n_contrib_out) return fail(ctx, CNF2_ERR_ARG, "xo_sum_out and n_contrib_out must not be NULL");
    RC_TRY(mode_range(ctx, ind_begin, ind_end));
    const bool   dev = (flags & CNF2_OUT_DEVICE) != 0;
    const size_t M = ctx->n_markers, C = ctx->n_chrom, nx = (size_t)(ind_end - ind_begin) * M * 6;
    SweepMode    m;
    m.variant = SW_CROSSOVERS;
    RC_TRY(stage_out(ctx, dev, xo_sum_out, ctx->d_xo_sum, M * 6, &m.xo_sum));
    RC_TRY(stage_out(ctx, dev, n_contrib_out, ctx->d_xo_cnt, C, &m.xo_cnt));
    RC_TRY(stage_out(ctx, dev, xo_out, ctx->d_xo, nx, &m.xo));
    RC_TRY(mode_sweep(ctx, ind_begin, ind_end, factors_out, loglik_out, flags, m));
    if (dev) return CNF2_OK;
    RC_TRY(fetch_out(ctx, xo_sum_out, m.xo_sum, M * 6));
    RC_TRY(fetch_out(ctx, n_contrib_out, m.xo_cnt, C));
    RC_TRY(fetch_out(ctx, xo_out, m.xo, nx));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    return CNF2_OK;
}

int cnf2_loo_rows(cnf2_ctx* ctx, int ind, int chrom, double* rows_out)
{
    if (!ctx || !rows_out) return fail(ctx, CNF2_ERR_ARG, "bad loo_rows arguments");
    return stage2_rows(ctx, ind, chrom, 2, rows_out,
                       [&](const Stage2Params& q, double* d_out) { launch_loo_rows(q, d_out, ctx->stream); });
}

// one pass of sweep_impl's leave-one-out mode, then loo_finish_kernel on the context's stream: the logarithms in place and
// the column sums (an empty range reports them as zeros).  The rows the caller gave no device memory for live in the
// context's own buffers
int cnf2_sweep_loo(cnf2_ctx* ctx, int ind_begin, int ind_end, double* factors_out, double* loglik_out, double* loo_out,
                   double* unlinked_out, double* loo_sum_out, double* unlinked_sum_out, int32_t* n_contrib_out, uint32_t flags)
{
    RC_TRY(ready(ctx));
    if (!factors_out || !loglik_out || !loo_sum_out || !unlinked_sum_out || !n_contrib_out)
        return fail(ctx, CNF2_ERR_ARG, "only loo_out and unlinked_out may be NULL");
    RC_TRY(mode_range(ctx, ind_begin, ind_end));
    const bool   dev = (flags & CNF2_OUT_DEVICE) != 0;
    const int    n = ind_end - ind_begin;
    const size_t M = ctx->n_markers, C = ctx->n_chrom, nr = (size_t)n * M;
    SweepMode    m;
    m.variant = SW_LOO;
    double *d_lsum, *d_usum;
    RC_TRY(stage_out(ctx, dev, loo_sum_out, ctx->d_loo_sum, M, &d_lsum));
    RC_TRY(stage_out(ctx, dev, unlinked_sum_out, ctx->d_unl_sum, M, &d_usum));
    RC_TRY(stage_out(ctx, dev, n_contrib_out, ctx->d_xo_cnt, C, &m.xo_cnt));
    m.loo = (dev && loo_out) ? loo_out : nullptr;
    m.unl = (dev && unlinked_out) ? unlinked_out : nullptr;
    if (!m.loo && nr > 0) {
        RC_TRY(ctx->d_loo.ensure(ctx, nr));
        m.loo = ctx->d_loo;
    }
    if (!m.unl && nr > 0) {
        RC_TRY(ctx->d_unl.ensure(ctx, nr));
        m.unl = ctx->d_unl;
    }
    RC_TRY(mode_sweep(ctx, ind_begin, ind_end, factors_out, loglik_out, flags & ~(uint32_t)CNF2_ALL_STATES, m));
    launch_loo_finish(m.loo, m.unl, n, (int)M, d_lsum, d_usum, ctx->stream);
    HIP_TRY(ctx, hipGetLastError());
    HIP_TRY(ctx, hipEventRecord(ctx->ev1, ctx->stream));       // (the timed span of cnf2_last_kernel_ms covers the finish)
    if (dev) return CNF2_OK;
    RC_TRY(fetch_out(ctx, loo_sum_out, d_lsum, M));
    RC_TRY(fetch_out(ctx, unlinked_sum_out, d_usum, M));
    RC_TRY(fetch_out(ctx, n_contrib_out, m.xo_cnt, C));
    if (loo_out) RC_TRY(fetch_out(ctx, loo_out, m.loo, nr));
    if (unlinked_out) RC_TRY(fetch_out(ctx, unlinked_out, m.unl, nr));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    return CNF2_OK;
}

int cnf2_origin_rows(cnf2_ctx* ctx, int ind, int chrom, double* rows_out)
{
    if (!ctx || !rows_out) return fail(ctx, CNF2_ERR_ARG, "bad origin_rows arguments");
    return stage2_rows(ctx, ind, chrom, 10, rows_out,
                       [&](const Stage2Params& q, double* d_out) { launch_origin_rows(q, d_out, ctx->stream); });
}

// one pass of sweep_impl's origin mode, then origin_finish_kernel on the context's stream: the column sums (an empty range
// reports them as zeros).  The rows the caller gave no device memory for live in the context's own buffers
int cnf2_sweep_origins(cnf2_ctx* ctx, int ind_begin, int ind_end, double* factors_out, double* loglik_out, double* origin_out,
                       double* bits_out, double* origin_sum_out, int32_t* n_contrib_out, uint32_t flags)
{
    RC_TRY(ready(ctx));
    if (!factors_out || !loglik_out || !origin_sum_out || !n_contrib_out)
        return fail(ctx, CNF2_ERR_ARG, "only origin_out and bits_out may be NULL");
    RC_TRY(mode_range(ctx, ind_begin, ind_end));
    ctx->qtl_rows_n = 0;
    const bool   dev = (flags & CNF2_OUT_DEVICE) != 0;
    const int    n = ind_end - ind_begin;
    const size_t M = ctx->n_markers, C = ctx->n_chrom, nr = (size_t)n * M;
    SweepMode    m;
    m.variant = SW_ORIGINS;
    double* d_sum;
    RC_TRY(stage_out(ctx, dev, origin_sum_out, ctx->d_org_sum, M * 4, &d_sum));
    RC_TRY(stage_out(ctx, dev, n_contrib_out, ctx->d_xo_cnt, C, &m.xo_cnt));
    m.org   = (dev && origin_out) ? origin_out : nullptr;
    m.obits = (dev && bits_out) ? bits_out : nullptr;
    if (!m.org && nr > 0) {
        RC_TRY(ctx->d_org.ensure(ctx, nr * 4));
        m.org = ctx->d_org;
    }
    if (!m.obits && nr > 0) {
        RC_TRY(ctx->d_obits.ensure(ctx, nr * 6));
        m.obits = ctx->d_obits;
    }
    RC_TRY(mode_sweep(ctx, ind_begin, ind_end, factors_out, loglik_out, flags & ~(uint32_t)CNF2_ALL_STATES, m));
    launch_origin_finish(m.org, n, (int)M, d_sum, ctx->stream);
    HIP_TRY(ctx, hipGetLastError());
    HIP_TRY(ctx, hipEventRecord(ctx->ev1, ctx->stream));       // (the timed span of cnf2_last_kernel_ms covers the finish)
    if (dev) return CNF2_OK;
    RC_TRY(fetch_out(ctx, origin_sum_out, d_sum, M * 4));
    RC_TRY(fetch_out(ctx, n_contrib_out, m.xo_cnt, C));
    if (origin_out) RC_TRY(fetch_out(ctx, origin_out, m.org, nr * 4));
    if (bits_out) RC_TRY(fetch_out(ctx, bits_out, m.obits, nr * 6));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    return CNF2_OK;
}

int cnf2_descent_rows(cnf2_ctx* ctx, int ind, int chrom, double* rows_out)
{
    if (!ctx || !rows_out) return fail(ctx, CNF2_ERR_ARG, "bad descent_rows arguments");
    return stage2_rows(ctx, ind, chrom, 8, rows_out,
                       [&](const Stage2Params& q, double* d_out) { launch_descent_rows(q, d_out, ctx->stream); });
}

// one pass of sweep_impl's descent mode.  The rows the caller gave no device memory for live in the context's own buffer
// (not the origin rows': a scan's kept rows stay what they are)
int cnf2_sweep_descent(cnf2_ctx* ctx, int ind_begin, int ind_end, double* factors_out, double* loglik_out, double* descent_out,
                       int32_t* n_contrib_out, uint32_t flags)
{
    RC_TRY(ready(ctx));
    if (!factors_out || !loglik_out || !n_contrib_out) return fail(ctx, CNF2_ERR_ARG, "only descent_out may be NULL");
    RC_TRY(mode_range(ctx, ind_begin, ind_end));
    const bool   dev = (flags & CNF2_OUT_DEVICE) != 0;
    const int    n = ind_end - ind_begin;
    const size_t M = ctx->n_markers, C = ctx->n_chrom, nr = (size_t)n * M;
    SweepMode    m;
    m.variant = SW_DESCENT;
    RC_TRY(stage_out(ctx, dev, n_contrib_out, ctx->d_xo_cnt, C, &m.xo_cnt));
    m.org = (dev && descent_out) ? descent_out : nullptr;
    if (!m.org && nr > 0) {
        RC_TRY(ctx->d_descent.ensure(ctx, nr * 8));
        m.org = ctx->d_descent;
    }
    RC_TRY(mode_sweep(ctx, ind_begin, ind_end, factors_out, loglik_out, flags & ~(uint32_t)CNF2_ALL_STATES, m));
    if (dev) return CNF2_OK;
    RC_TRY(fetch_out(ctx, n_contrib_out, m.xo_cnt, C));
    if (descent_out) RC_TRY(fetch_out(ctx, descent_out, m.org, nr * 8));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    return CNF2_OK;
}

// ------------------------------------------------------------------------------------------------
// QTL scans (cnf2_qtl.h, cnf2_qtlplan.h, cnf2_qtl_kernels.hip and the scans' own headers and kernels).  Every entry point
// takes the same steps in the same order: the argument checks; the plan (marker map and column tile, cnf2_qtlplan.h); every
// allocation -- the origin buffer, the inputs, the workspace, the staged outputs; the copy of host origin rows; the uploads;
// the launches; the fetches.  So a check or an allocation that fails returns before anything of the caller's is written and
// before the rows a cnf2_sweep_qtl left in the context are touched.
// ------------------------------------------------------------------------------------------------
struct QtlArgs {
    int            n, T, K, P;
    const double*  pheno;
    const uint8_t* use;
    const double*  cov;
    const int32_t* perm;
    double *       lod, *coef, *rss0, *pmax;
    int32_t *      rank, *n_used;
};

// Where a scan's origin rows [n][M][4] come from: the caller's host array, staged in d_org; the caller's device array, read
// in place; or (origin NULL with CNF2_QTL_ORIGIN_DEVICE) the rows the last cnf2_sweep_qtl left in d_org, which stay valid.
struct QtlOrigin {
    bool          staged = false;   // host rows: `host` is copied to d_org (qtl_origin_stage)
    const double* host = nullptr;
    const double* dev = nullptr;    // what the kernels read; for host rows d_org, once they are staged
    size_t        count = 0;        // doubles
};

// the rows kept by the last cnf2_sweep_qtl are those of exactly these n individuals on the map as it is
static int qtl_kept_check(cnf2_ctx* ctx, int n)
{
    if (ctx->qtl_rows_n == 0 || n != ctx->qtl_rows_n || ctx->qtl_rows_m != ctx->n_markers || ctx->d_org.cap < (size_t)n * ctx->n_markers * 4)
        return fail(ctx, CNF2_ERR_STATE, "the context holds the rows of %d individuals from cnf2_sweep_qtl, not of %d", ctx->qtl_rows_n, n);
    return CNF2_OK;
}

static int qtl_origin_source(cnf2_ctx* ctx, int n, const double* origin, uint32_t flags, QtlOrigin* out)
{
    const bool kept = !origin && (flags & CNF2_QTL_ORIGIN_DEVICE);
    if (!origin && !kept) return fail(ctx, CNF2_ERR_ARG, "origin is NULL");
    if (kept) RC_TRY(qtl_kept_check(ctx, n));
    out->staged = !(flags & CNF2_QTL_ORIGIN_DEVICE);
    out->host   = out->staged ? origin : nullptr;
    out->dev    = kept ? ctx->d_org.ptr : out->staged ? nullptr : origin;
    out->count  = (size_t)n * ctx->n_markers * 4;
    if (!out->staged && ((uintptr_t)out->dev & 15)) return fail(ctx, CNF2_ERR_ARG, "device origin rows must be aligned to 16 bytes");
    return CNF2_OK;
}
// room for host rows, with a scan's other allocations (kept rows go with a buffer that has to grow)
static int qtl_origin_reserve(cnf2_ctx* ctx, const QtlOrigin& o)
{
    if (!o.staged) return CNF2_OK;
    if (ctx->d_org.cap < o.count) ctx->qtl_rows_n = 0;
    return ctx->d_org.ensure(ctx, o.count);
}
// ... and the copy, once every allocation has succeeded.  Complete on return: the caller's array is not read after the call,
// whatever its status.  The buffer holds the caller's rows from here on, so it vouches for no sweep's.
static int qtl_origin_stage(cnf2_ctx* ctx, QtlOrigin& o)
{
    if (!o.staged) return CNF2_OK;
    RC_TRY(qtl_origin_reserve(ctx, o));
    ctx->qtl_rows_n = 0;
    HIP_TRY(ctx, hipMemcpyAsync(ctx->d_org.ptr, o.host, o.count * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    o.dev = ctx->d_org;
    return CNF2_OK;
}

// use_out[n] = the mask with NULL expanded; the phenotypes and covariates of the used individuals must be finite
static int qtl_check_values(cnf2_ctx* ctx, const QtlArgs& a, std::vector<uint8_t>* use_out)
{
    std::vector<uint8_t>& use = *use_out;
    use.assign(a.n, 1);
    if (a.use)
        for (int i = 0; i < a.n; i++) use[i] = a.use[i] ? 1 : 0;
    int i = 0, col = 0;
    switch (qtl_check_finite(a.n, a.T, a.pheno, a.K, a.cov, use.data(), &i, &col)) {
    case QTL_PHENO_NOT_FINITE: return fail(ctx, CNF2_ERR_ARG, "phenotype %d of individual %d is used and not finite", col, i);
    case QTL_COV_NOT_FINITE: return fail(ctx, CNF2_ERR_ARG, "covariate %d of individual %d is used and not finite", col, i);
    }
    return CNF2_OK;
}
// the rows of perm[P][n] are permutations that give a used individual (use[n], NULL = all) a used one
static int qtl_check_perm(cnf2_ctx* ctx, int n, int P, const int32_t* perm, const uint8_t* use)
{
    int p = 0, i = 0, j = 0;
    switch (qtl_check_permutations(n, P, perm, use, &p, &i, &j)) {
    case QTL_NOT_A_PERMUTATION: return fail(ctx, CNF2_ERR_ARG, "row %d of perm is not a permutation of 0 .. n-1", p);
    case QTL_PERM_TAKES_UNUSED:
        return fail(ctx, CNF2_ERR_ARG, "permutation %d gives individual %d, which is used, the unused individual %d", p, i, j);
    }
    return CNF2_OK;
}

// every check of the phenotype side, before anything is written; use_out[n] = the mask with NULL expanded
static int qtl_check(cnf2_ctx* ctx, const QtlArgs& a, std::vector<uint8_t>* use_out)
{
    if (ctx->n_markers <= 0) return fail(ctx, CNF2_ERR_STATE, "the map must be uploaded first");
    if (a.n < 1 || a.T < 1 || !a.pheno) return fail(ctx, CNF2_ERR_ARG, "n and n_traits must be at least 1 and pheno not NULL");
    if (a.K < 0 || a.K > QTL_MAXK || (a.K > 0 && !a.cov)) return fail(ctx, CNF2_ERR_ARG, "n_cov must be 0 .. %d, with cov", QTL_MAXK);
    if (a.P < 0 || (a.P > 0) != (a.perm != nullptr) || (a.P > 0) != (a.pmax != nullptr))
        return fail(ctx, CNF2_ERR_ARG, "perm and perm_max_out must be NULL exactly when n_perm is 0");
    if (!a.lod || !a.coef || !a.rank || !a.rss0 || !a.n_used) return fail(ctx, CNF2_ERR_ARG, "an output pointer is NULL");
    if ((size_t)a.T * ((size_t)a.P + 1) > (size_t)1 << 30) return fail(ctx, CNF2_ERR_ARG, "too many columns");
    RC_TRY(qtl_check_values(ctx, a, use_out));
    return qtl_check_perm(ctx, a.n, a.P, a.perm, use_out->data());
}

// The model does not depend on the units and offsets of traits and fixed-effect covariates (include/cnf2hip.h); the sums the
// kernels form -- X0'X0, y'y - b0' S11^-1 b0, A'y - G b0 -- cancel once a column's mean is large against its spread.  So every
// scan works on columns with their mean over the used individuals subtracted: the intercept of X0 takes the mean up, and
// LOD, effects, RSS0 and ranks are those of the raw columns.  A permutation maps used individuals to used ones and keeps a
// column's mean; a constant column becomes exactly 0 (the second pass makes the mean of equal values that value), so a
// constant trait keeps RSS0 = 0 and a constant covariate still leaves X0 without a factor.  The values of unused individuals
// are copied as they are: nothing reads them.  `a` has been validated; its pheno and cov point into `store` afterwards.
struct QtlCentred {
    std::vector<double> pheno, cov;
};
static void qtl_centre_columns(const double* src, int n, int w, const std::vector<uint8_t>& use, std::vector<double>& dst)
{
    dst.assign(src, src + (size_t)n * w);
    for (int k = 0; k < w; k++) {
        const double mean = qtl_column_mean(src + k, n, w, use.data());
        for (int i = 0; i < n; i++)
            if (use[i]) dst[(size_t)i * w + k] = src[(size_t)i * w + k] - mean;
    }
}
// the same with each difference rounded once (qtl_column_mean2): columns that differ by an exact shift give the same bits
static void qtl_centre_columns_once(const double* src, int n, int w, const std::vector<uint8_t>& use, std::vector<double>& dst)
{
    dst.assign(src, src + (size_t)n * w);
    for (int k = 0; k < w; k++) {
        const QtlMean2 mean = qtl_column_mean2(src + k, n, w, use.data());
        for (int i = 0; i < n; i++)
            if (use[i]) dst[(size_t)i * w + k] = qtl_minus_mean2(src[(size_t)i * w + k], mean);
    }
}
static void qtl_centre(QtlArgs& a, const std::vector<uint8_t>& use, QtlCentred& store)
{
    qtl_centre_columns(a.pheno, a.n, a.T, use, store.pheno);
    a.pheno = store.pheno.data();
    if (a.K > 0) {
        qtl_centre_columns(a.cov, a.n, a.K, use, store.cov);
        a.cov = store.cov.data();
    }
}

// what every entry point does with the phenotype side before anything is written or uploaded: the checks, then the centring
static int qtl_validate(cnf2_ctx* ctx, QtlArgs& a, std::vector<uint8_t>* use_out, QtlCentred* store)
{
    RC_TRY(qtl_check(ctx, a, use_out));
    qtl_centre(a, *use_out, *store);
    return CNF2_OK;
}

extern "C++" template <class T>
static int qtl_upload(cnf2_ctx* ctx, DevBuf<T>& buf, const T* src, size_t count)
{
    if (count == 0) return CNF2_OK;
    RC_TRY(buf.ensure(ctx, count));
    // (complete on return: src is caller or local memory, and a later step may fail and return at once)
    HIP_TRY(ctx, hipMemcpyAsync(buf.ptr, src, count * sizeof(T), hipMemcpyHostToDevice, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    return CNF2_OK;
}

// The phenotype-side buffers the scans share: the staged phenotypes, covariates (with room for extra_cov more doubles behind
// them), mask and permutations, the chromosome masks and the column image of a tile of rt columns (rt = 0: a scan without
// one).  First the room for them ...
static int qtl_reserve_inputs(cnf2_ctx* ctx, const QtlArgs& a, size_t rt, size_t extra_cov)
{
    RC_TRY(ctx->d_q_pheno.ensure(ctx, (size_t)a.n * a.T));
    RC_TRY(ctx->d_q_cov.ensure(ctx, std::max<size_t>(1, (size_t)a.n * a.K + extra_cov)));
    RC_TRY(ctx->d_q_use.ensure(ctx, (size_t)a.n));
    RC_TRY(ctx->d_q_perm.ensure(ctx, std::max<size_t>(1, (size_t)a.P * a.n)));
    RC_TRY(ctx->d_q_cmask.ensure(ctx, (size_t)ctx->n_chrom * a.n));
    if (rt > 0) RC_TRY(ctx->d_q_Y.ensure(ctx, (size_t)a.n * rt));
    return CNF2_OK;
}
// ... then what the caller gave, with `use` its expanded mask
static int qtl_upload_inputs(cnf2_ctx* ctx, const QtlArgs& a, const std::vector<uint8_t>& use)
{
    RC_TRY(qtl_upload(ctx, ctx->d_q_pheno, a.pheno, (size_t)a.n * a.T));
    RC_TRY(qtl_upload(ctx, ctx->d_q_cov, a.cov, (size_t)a.n * a.K));
    RC_TRY(qtl_upload(ctx, ctx->d_q_use, use.data(), (size_t)a.n));
    return qtl_upload(ctx, ctx->d_q_perm, a.perm, (size_t)a.P * a.n);
}
// what qtl_gather_kernel reads of them (after qtl_reserve_inputs); r0 and rn are the caller's, per tile
static QtlParams qtl_gather_params(const cnf2_ctx* ctx, const QtlArgs& a, size_t rt)
{
    QtlParams g;
    memset(&g, 0, sizeof(g));
    g.n = a.n, g.T = a.T, g.pheno = ctx->d_q_pheno, g.use = ctx->d_q_use, g.perm = ctx->d_q_perm, g.Y = ctx->d_q_Y, g.rstride = (int)rt;
    return g;
}

// the scan on the rows `org`; `a` has been validated and `use` is its expanded mask
static int qtl_scan_impl(cnf2_ctx* ctx, QtlOrigin& org, const QtlArgs& a, const std::vector<uint8_t>& use, uint32_t flags)
{
    const bool         dev = (flags & CNF2_OUT_DEVICE) != 0;
    const int          M = ctx->n_markers, C = ctx->n_chrom, nx = a.K + 1;
    const size_t       R = (size_t)a.T * ((size_t)a.P + 1);
    const size_t       rt = qtl_column_tile(a.n, R, a.P, 0, ctx->qtl_columns[QTL_CAP_SCAN]);
    const QtlMarkerMap map = qtl_marker_map(ctx->chromstarts.data(), C, 0, C, 16, true, true);

    RC_TRY(qtl_origin_reserve(ctx, org));
    RC_TRY(qtl_reserve_inputs(ctx, a, rt, 0));
    QtlParams q = qtl_gather_params(ctx, a, rt);
    auto outputs = [&](auto each) -> int {
        RC_TRY(each(a.n_used, ctx->d_q_nc, (size_t)C, &q.nc));
        RC_TRY(each(a.rank, ctx->d_q_rank, (size_t)M, &q.rank));
        RC_TRY(each(a.lod, ctx->d_q_lod, (size_t)a.T * M, &q.lod));
        RC_TRY(each(a.coef, ctx->d_q_coef, (size_t)a.T * M * 2, &q.coef));
        RC_TRY(each(a.rss0, ctx->d_q_rss0, (size_t)a.T * C, &q.rss0));
        return each(a.pmax, ctx->d_q_pmax, (size_t)a.P * a.T * C, &q.pmax);
    };
    RC_TRY(ctx->d_q_map.ensure(ctx, map.image.size()));
    RC_TRY(ctx->d_q_chol.ensure(ctx, (size_t)C * QTL_CHOL));
    RC_TRY(ctx->d_q_mk.ensure(ctx, (size_t)M * QTL_MK));
    RC_TRY(ctx->d_q_null.ensure(ctx, (size_t)C * (nx + 1) * rt));
    if (a.P > 0) RC_TRY(ctx->d_q_tilemax.ensure(ctx, map.n_tiles * rt));
    RC_TRY(qtl_stage_outputs(ctx, dev, outputs));
    RC_TRY(qtl_origin_stage(ctx, org));
    RC_TRY(qtl_upload(ctx, ctx->d_q_map, map.image.data(), map.image.size()));
    RC_TRY(qtl_upload_inputs(ctx, a, use));

    q.M = M, q.C = C, q.P = a.P, q.K = a.K, q.nx = nx;
    q.additive = (flags & CNF2_QTL_ADDITIVE) ? 1 : 0;
    q.origin = org.dev, q.cov = ctx->d_q_cov;
    q.cs = ctx->d_q_map, q.mchrom = ctx->d_q_map + map.o_mchrom;
    q.tiles = ctx->d_q_map + map.o_tiles, q.tile_start = ctx->d_q_map + map.o_tstart, q.n_tiles = (int)map.n_tiles;
    q.cmask = ctx->d_q_cmask, q.chol = ctx->d_q_chol, q.mk = ctx->d_q_mk;
    q.nullq = ctx->d_q_null, q.tilemax = ctx->d_q_tilemax;

    launch_qtl_chrom(q, ctx->stream);
    launch_qtl_design(q, ctx->stream);
    for (size_t r0 = 0; r0 < R; r0 += rt) {
        q.r0 = (int)r0;
        q.rn = (int)std::min(rt, R - r0);
        launch_qtl_gather(q, ctx->stream);
        launch_qtl_null(q, ctx->stream);
        launch_qtl_scan(q, ctx->stream);
        if (r0 + q.rn > (size_t)a.T) launch_qtl_finish(q, ctx->stream);
    }
    HIP_TRY(ctx, hipGetLastError());
    return qtl_fetch_outputs(ctx, dev, outputs);
}

int cnf2_qtl_scan(cnf2_ctx* ctx, int n, const double* origin, int n_traits, const double* pheno, const uint8_t* use, int n_cov,
                  const double* cov, int n_perm, const int32_t* perm, double* lod_out, double* coef_out, int32_t* rank_out,
                  double* rss0_out, int32_t* n_used_out, double* perm_max_out, uint32_t flags)
{
    if (!ctx) return CNF2_ERR_ARG;
    QtlOrigin org;
    RC_TRY(qtl_origin_source(ctx, n, origin, flags, &org));
    QtlArgs a = {n, n_traits, n_cov, n_perm, pheno, use, cov, perm, lod_out, coef_out, rss0_out, perm_max_out, rank_out, n_used_out};
    std::vector<uint8_t> mask;
    QtlCentred           centred;
    RC_TRY(qtl_validate(ctx, a, &mask, &centred));
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    return qtl_scan_impl(ctx, org, a, mask, flags);
}

// cnf2_sweep_origins over the range with the rows in the context's buffer, then the scan on them
int cnf2_sweep_qtl(cnf2_ctx* ctx, int ind_begin, int ind_end, double* factors_out, double* loglik_out, int n_traits,
                   const double* pheno, const uint8_t* use, int n_cov, const double* cov, int n_perm, const int32_t* perm,
                   double* lod_out, double* coef_out, int32_t* rank_out, double* rss0_out, int32_t* n_used_out,
                   double* perm_max_out, uint32_t flags)
{
    RC_TRY(ready(ctx));
    if (!factors_out || !loglik_out) return fail(ctx, CNF2_ERR_ARG, "factors_out and loglik_out must not be NULL");
    RC_TRY(mode_range(ctx, ind_begin, ind_end));
    QtlArgs a = {ind_end - ind_begin, n_traits, n_cov, n_perm, pheno, use, cov, perm,
                 lod_out, coef_out, rss0_out, perm_max_out, rank_out, n_used_out};
    std::vector<uint8_t> mask;
    QtlCentred           centred;
    RC_TRY(qtl_validate(ctx, a, &mask, &centred));
    const uint32_t sweep_flags = flags & (CNF2_OUT_DEVICE | CNF2_STATIC_JOBS | CNF2_FULL_SPILL | CNF2_TIES_GENERAL);
    const size_t   M = ctx->n_markers, C = ctx->n_chrom;
    if (flags & CNF2_OUT_DEVICE) {
        RC_TRY(ctx->d_org_sum.ensure(ctx, M * 4));
        RC_TRY(ctx->d_xo_cnt.ensure(ctx, C));
        RC_TRY(cnf2_sweep_origins(ctx, ind_begin, ind_end, factors_out, loglik_out, nullptr, nullptr, ctx->d_org_sum, ctx->d_xo_cnt,
                                  sweep_flags));
    } else {
        std::vector<double>  sum(M * 4);
        std::vector<int32_t> cnt(C);
        RC_TRY(cnf2_sweep_origins(ctx, ind_begin, ind_end, factors_out, loglik_out, nullptr, nullptr, sum.data(), cnt.data(),
                                  sweep_flags));
    }
    ctx->qtl_rows_n = a.n;
    ctx->qtl_rows_m = ctx->n_markers;
    QtlOrigin org;
    org.dev = ctx->d_org;
    return qtl_scan_impl(ctx, org, a, mask, flags);
}

// ------------------------------------------------------------------------------------------------
// Within-family scan (cnf2_qtlfam.h, cnf2_qtlfam_kernels.hip), in the scans' order of steps.  The individuals it uses are
// those of `use` with grp >= 0: that mask is what the checks, the centring and the kernels see.
// ------------------------------------------------------------------------------------------------
int cnf2_qtl_scan_fam(cnf2_ctx* ctx, int n, const double* origin, int side, const int32_t* grp, const int32_t* cell, int n_fam,
                      int n_traits, const double* pheno, const uint8_t* use, int n_cov, const double* cov, int n_perm,
                      const int32_t* perm, double* lod_out, int32_t* df_out, double* slope_out, double* rss0_out,
                      int32_t* n_used_out, int32_t* n_cells_out, double* perm_max_out, uint32_t flags)
{
    if (!ctx) return CNF2_ERR_ARG;
    QtlOrigin org;
    RC_TRY(qtl_origin_source(ctx, n, origin, flags, &org));
    if (ctx->n_markers <= 0) return fail(ctx, CNF2_ERR_STATE, "the map must be uploaded first");
    if (n < 1 || n_traits < 1 || !pheno) return fail(ctx, CNF2_ERR_ARG, "n and n_traits must be at least 1 and pheno not NULL");
    if (side < 0 || side > 1 || !grp || n_fam < 1) return fail(ctx, CNF2_ERR_ARG, "side must be 0 or 1, grp not NULL and n_fam at least 1");
    if (n_cov < 0 || n_cov > QTL_MAXK || (n_cov > 0 && !cov)) return fail(ctx, CNF2_ERR_ARG, "n_cov must be 0 .. %d, with cov", QTL_MAXK);
    if (n_perm < 0 || (n_perm > 0) != (perm != nullptr) || (n_perm > 0) != (perm_max_out != nullptr))
        return fail(ctx, CNF2_ERR_ARG, "perm and perm_max_out must be NULL exactly when n_perm is 0");
    if (!lod_out || !df_out || !rss0_out || !n_used_out || !n_cells_out) return fail(ctx, CNF2_ERR_ARG, "an output pointer is NULL");
    if ((size_t)n_traits * ((size_t)n_perm + 1) > (size_t)1 << 30) return fail(ctx, CNF2_ERR_ARG, "too many columns");
    std::vector<uint8_t> nested(n);
    for (int i = 0; i < n; i++) nested[i] = ((!use || use[i]) && grp[i] >= 0) ? 1 : 0;
    QtlArgs a = {n, n_traits, n_cov, n_perm, pheno, nested.data(), cov, perm, lod_out, nullptr, rss0_out, perm_max_out, df_out, n_used_out};
    std::vector<uint8_t> mask;
    RC_TRY(qtl_check_values(ctx, a, &mask));
    RC_TRY(qtl_check_perm(ctx, n, n_perm, perm, mask.data()));
    QtlFamLayout lay;
    int          bad_i = 0, bad_row = 0;
    switch (qtlfam_layout(n, mask.data(), grp, cell, n_fam, &lay, &bad_i)) {
    case QTLFAM_GRP_RANGE: return fail(ctx, CNF2_ERR_ARG, "grp of individual %d is not below n_fam = %d", bad_i, n_fam);
    case QTLFAM_CELL_NEGATIVE: return fail(ctx, CNF2_ERR_ARG, "cell of individual %d, which is used, is negative", bad_i);
    case QTLFAM_CELL_SPLIT: return fail(ctx, CNF2_ERR_ARG, "the cell of individual %d has members of two slope groups", bad_i);
    }
    if (qtlfam_check_permutations(n, n_perm, perm, lay, &bad_row, &bad_i) != QTLFAM_OK)
        return fail(ctx, CNF2_ERR_ARG, "permutation %d takes individual %d out of its cell", bad_row, bad_i);
    QtlCentred centred;
    qtl_centre(a, mask, centred);
    HIP_TRY(ctx, hipSetDevice(ctx->device));

    const bool   dev = (flags & CNF2_OUT_DEVICE) != 0;
    const int    M = ctx->n_markers, C = ctx->n_chrom, K = n_cov, T = n_traits, F = n_fam, S = lay.S;
    const size_t R = (size_t)T * ((size_t)n_perm + 1), slots = std::max(1, S);
    const size_t rt = qtl_column_tile(slots * C, R, n_perm, 0, ctx->qtl_columns[QTL_CAP_SCAN]);
    QtlMarkerMap map = qtl_marker_map(ctx->chromstarts.data(), C, 0, C, 16, true, true);
    // the gather list behind the marker map: gidx, cellslot, famcell, stepend, folds
    std::vector<int32_t>& img = map.image;
    const size_t o_gidx = img.size();
    img.insert(img.end(), lay.gidx.begin(), lay.gidx.end());
    const size_t o_cellslot = img.size();
    img.insert(img.end(), lay.cellslot.begin(), lay.cellslot.end());
    const size_t o_famcell = img.size();
    img.insert(img.end(), lay.famcell.begin(), lay.famcell.end());
    const size_t o_stepend = img.size();
    img.insert(img.end(), lay.stepend.begin(), lay.stepend.end());
    const size_t o_folds = img.size();
    img.insert(img.end(), lay.folds.begin(), lay.folds.end());

    RC_TRY(qtl_origin_reserve(ctx, org));
    RC_TRY(qtl_reserve_inputs(ctx, a, 0, 0));
    QtlFamParams q;
    memset(&q, 0, sizeof(q));
    auto outputs = [&](auto each) -> int {
        RC_TRY(each(n_used_out, ctx->d_qf_nc, (size_t)C, &q.nc));
        RC_TRY(each(n_cells_out, ctx->d_qf_ncells, (size_t)C, &q.ncells));
        RC_TRY(each(df_out, ctx->d_qf_df, (size_t)M, &q.df));
        RC_TRY(each(lod_out, ctx->d_qf_lod, (size_t)T * M, &q.lod));
        RC_TRY(each(slope_out, ctx->d_qf_slope, (size_t)T * M * F, &q.slope));
        RC_TRY(each(rss0_out, ctx->d_qf_rss0, (size_t)T * C, &q.rss0));
        return each(perm_max_out, ctx->d_qf_pmax, (size_t)n_perm * T * C, &q.pmax);
    };
    const size_t n_tri = (size_t)K * (K + 1) / 2;
    RC_TRY(ctx->d_qf_map.ensure(ctx, img.size()));
    RC_TRY(ctx->d_qf_Z.ensure(ctx, (size_t)C * slots * QTL_MAXK));
    RC_TRY(ctx->d_qf_Y.ensure(ctx, (size_t)C * slots * rt));
    RC_TRY(ctx->d_qf_chrom.ensure(ctx, (size_t)C * QTLFAM_CHROM));
    RC_TRY(ctx->d_qf_rec.ensure(ctx, (size_t)F * (1 + K) * M));
    RC_TRY(ctx->d_qf_hrec.ensure(ctx, (n_tri + 1) * M));
    RC_TRY(ctx->d_qf_null.ensure(ctx, (size_t)C * (K + 2) * rt));
    if (n_perm > 0) RC_TRY(ctx->d_qf_tilemax.ensure(ctx, map.n_tiles * rt));
    if (slope_out) RC_TRY(ctx->d_qf_gamma.ensure(ctx, std::max<size_t>(1, (size_t)T * M * K)));
    RC_TRY(qtl_stage_outputs(ctx, dev, outputs));
    RC_TRY(qtl_origin_stage(ctx, org));
    RC_TRY(qtl_upload(ctx, ctx->d_qf_map, img.data(), img.size()));
    RC_TRY(qtl_upload_inputs(ctx, a, mask));

    q.n = n, q.M = M, q.C = C, q.T = T, q.P = n_perm, q.K = K, q.F = F, q.side = side, q.S = S, q.Q = lay.Q;
    q.origin = org.dev, q.pheno = ctx->d_q_pheno, q.cov = ctx->d_q_cov, q.use = ctx->d_q_use, q.perm = ctx->d_q_perm;
    q.cs = ctx->d_qf_map, q.mchrom = ctx->d_qf_map + map.o_mchrom;
    q.tiles = ctx->d_qf_map + map.o_tiles, q.tile_start = ctx->d_qf_map + map.o_tstart, q.n_tiles = (int)map.n_tiles;
    q.gidx = ctx->d_qf_map + o_gidx, q.cellslot = ctx->d_qf_map + o_cellslot, q.famcell = ctx->d_qf_map + o_famcell;
    q.stepend = ctx->d_qf_map + o_stepend, q.folds = ctx->d_qf_map + o_folds;
    q.cmask = ctx->d_q_cmask, q.Z = ctx->d_qf_Z, q.Y = ctx->d_qf_Y, q.chrom = ctx->d_qf_chrom, q.rec = ctx->d_qf_rec;
    q.hrec = ctx->d_qf_hrec, q.nullq = ctx->d_qf_null, q.tilemax = ctx->d_qf_tilemax;
    q.gamma = slope_out ? ctx->d_qf_gamma.ptr : nullptr;
    q.rstride = (int)rt;

    launch_qtlfam_mask(q, ctx->stream);
    launch_qtlfam_image(q, true, ctx->stream);
    launch_qtlfam_chrom(q, ctx->stream);
    launch_qtlfam_design(q, ctx->stream);
    launch_qtlfam_marker(q, ctx->stream);
    for (size_t r0 = 0; r0 < R; r0 += rt) {
        q.r0 = (int)r0;
        q.rn = (int)std::min(rt, R - r0);
        launch_qtlfam_image(q, false, ctx->stream);
        launch_qtlfam_null(q, ctx->stream);
        launch_qtlfam_scan(q, ctx->stream);
        if (r0 + q.rn > (size_t)T) launch_qtlfam_finish(q, ctx->stream);
    }
    if (q.slope) launch_qtlfam_slope(q, ctx->stream);
    HIP_TRY(ctx, hipGetLastError());
    return qtl_fetch_outputs(ctx, dev, outputs);
}

// ------------------------------------------------------------------------------------------------
// Founder-haplotype scan (cnf2_qtlhap.h, cnf2_qtlhap_kernels.hip), in the scans' order of steps.  The individuals it uses are
// those of `use` with all eight columns in [0, H): that mask is what the checks, the centring and the kernels see.
// ------------------------------------------------------------------------------------------------
int cnf2_qtl_scan_hap(cnf2_ctx* ctx, int n, const double* descent, const int32_t* col, int n_columns, int n_traits,
                      const double* pheno, const uint8_t* use, int n_cov, const double* cov, int n_perm, const int32_t* perm,
                      double* lod_out, int32_t* df_out, double* coef_out, double* rss0_out, int32_t* n_used_out,
                      double* perm_max_out, uint32_t flags)
{
    if (!ctx) return CNF2_ERR_ARG;
    if (ctx->n_markers <= 0) return fail(ctx, CNF2_ERR_STATE, "the map must be uploaded first");
    if (n < 1 || n_traits < 1 || !pheno) return fail(ctx, CNF2_ERR_ARG, "n and n_traits must be at least 1 and pheno not NULL");
    if (!descent || !col) return fail(ctx, CNF2_ERR_ARG, "descent and col must not be NULL");
    if (n_columns < 1 || n_columns > QTLHAP_MAXH) return fail(ctx, CNF2_ERR_ARG, "n_columns must be 1 .. %d", QTLHAP_MAXH);
    if (n_cov < 0 || n_cov > QTL_MAXK || (n_cov > 0 && !cov)) return fail(ctx, CNF2_ERR_ARG, "n_cov must be 0 .. %d, with cov", QTL_MAXK);
    if (n_perm < 0 || (n_perm > 0) != (perm != nullptr) || (n_perm > 0) != (perm_max_out != nullptr))
        return fail(ctx, CNF2_ERR_ARG, "perm and perm_max_out must be NULL exactly when n_perm is 0");
    if (!lod_out || !df_out || !rss0_out || !n_used_out) return fail(ctx, CNF2_ERR_ARG, "an output pointer is NULL");
    if ((size_t)n_traits * ((size_t)n_perm + 1) > (size_t)1 << 30) return fail(ctx, CNF2_ERR_ARG, "too many columns");
    const bool rows_dev = (flags & CNF2_QTL_ORIGIN_DEVICE) != 0;
    if (rows_dev && ((uintptr_t)descent & 15)) return fail(ctx, CNF2_ERR_ARG, "device descent rows must be aligned to 16 bytes");
    std::vector<uint8_t> inmodel(n);
    const int            bad = qtlhap_mask(n, use, col, n_columns, inmodel.data());
    if (bad >= 0) return fail(ctx, CNF2_ERR_ARG, "a column of individual %d is not in -1 .. %d", bad, n_columns - 1);
    QtlArgs a = {n, n_traits, n_cov, n_perm, pheno, inmodel.data(), cov, perm, lod_out, nullptr, rss0_out, perm_max_out, df_out, n_used_out};
    std::vector<uint8_t> mask;
    RC_TRY(qtl_check_values(ctx, a, &mask));
    RC_TRY(qtl_check_perm(ctx, n, n_perm, perm, mask.data()));
    QtlHapLayout lay;
    qtlhap_layout(n, mask.data(), col, &lay);
    QtlCentred centred;
    qtl_centre(a, mask, centred);
    HIP_TRY(ctx, hipSetDevice(ctx->device));

    const bool   dev = (flags & CNF2_OUT_DEVICE) != 0;
    const int    M = ctx->n_markers, C = ctx->n_chrom, K = n_cov, T = n_traits, H = n_columns, nx = K + 1;
    const size_t R = (size_t)T * ((size_t)n_perm + 1);
    const size_t rt = qtl_column_tile(n, R, n_perm, 0, ctx->qtl_columns[QTL_CAP_SCAN]);
    QtlMarkerMap map = qtl_marker_map(ctx->chromstarts.data(), C, 0, C, 2, true, true);
    // col and the gather list behind the marker map: gidx, steppat, stepend, patcol (a word each where they are empty)
    std::vector<int32_t>& img = map.image;
    auto append = [&](const int32_t* v, size_t count) {
        const size_t o = img.size();
        img.insert(img.end(), v, v + count);
        if (count == 0) img.push_back(0);
        return o;
    };
    const size_t o_col = append(col, (size_t)n * 8), o_gidx = append(lay.gidx.data(), lay.gidx.size());
    const size_t o_steppat = append(lay.steppat.data(), lay.steppat.size()), o_stepend = append(lay.stepend.data(), lay.stepend.size());
    const size_t o_patcol = append(lay.patcol.data(), lay.patcol.size());

    const size_t n_rows = (size_t)n * M * 8;
    if (!rows_dev) RC_TRY(ctx->d_descent.ensure(ctx, n_rows));
    RC_TRY(qtl_reserve_inputs(ctx, a, rt, 0));
    QtlHapParams p;
    memset(&p, 0, sizeof(p));
    QtlParams& q = p.q;
    q = qtl_gather_params(ctx, a, rt);
    auto outputs = [&](auto each) -> int {
        RC_TRY(each(n_used_out, ctx->d_qh_nc, (size_t)C, &q.nc));
        RC_TRY(each(df_out, ctx->d_qh_df, (size_t)M, &p.df));
        RC_TRY(each(lod_out, ctx->d_qh_lod, (size_t)T * M, &q.lod));
        RC_TRY(each(coef_out, ctx->d_qh_coef, (size_t)T * M * H, &p.coef));
        RC_TRY(each(rss0_out, ctx->d_qh_rss0, (size_t)T * C, &q.rss0));
        return each(perm_max_out, ctx->d_qh_pmax, (size_t)n_perm * T * C, &q.pmax);
    };
    RC_TRY(ctx->d_qh_map.ensure(ctx, img.size()));
    RC_TRY(ctx->d_q_chol.ensure(ctx, (size_t)C * QTL_CHOL));
    RC_TRY(ctx->d_qh_rec.ensure(ctx, (size_t)M * qtlhap_rec_size(H, nx)));
    RC_TRY(ctx->d_qh_kept.ensure(ctx, (size_t)M));
    RC_TRY(ctx->d_qh_null.ensure(ctx, (size_t)C * (nx + 1) * rt));
    if (n_perm > 0) RC_TRY(ctx->d_qh_tilemax.ensure(ctx, map.n_tiles * rt));
    RC_TRY(qtl_stage_outputs(ctx, dev, outputs));
    if (!rows_dev) {
        // (complete on return: the caller's array is not read after the call)
        HIP_TRY(ctx, hipMemcpyAsync(ctx->d_descent.ptr, descent, n_rows * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
        HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    }
    RC_TRY(qtl_upload(ctx, ctx->d_qh_map, img.data(), img.size()));
    RC_TRY(qtl_upload_inputs(ctx, a, mask));

    q.M = M, q.C = C, q.P = n_perm, q.K = K, q.nx = nx;
    q.cov = ctx->d_q_cov;
    q.cs = ctx->d_qh_map, q.mchrom = ctx->d_qh_map + map.o_mchrom;
    q.tiles = ctx->d_qh_map + map.o_tiles, q.tile_start = ctx->d_qh_map + map.o_tstart, q.n_tiles = (int)map.n_tiles;
    q.cmask = ctx->d_q_cmask, q.chol = ctx->d_q_chol, q.nullq = ctx->d_qh_null, q.tilemax = ctx->d_qh_tilemax;
    p.H = H, p.S = lay.S;
    p.descent = rows_dev ? descent : ctx->d_descent.ptr;
    p.col = ctx->d_qh_map + o_col, p.gidx = ctx->d_qh_map + o_gidx, p.steppat = ctx->d_qh_map + o_steppat;
    p.stepend = ctx->d_qh_map + o_stepend, p.patcol = ctx->d_qh_map + o_patcol;
    p.rec = ctx->d_qh_rec, p.kept = ctx->d_qh_kept;

    launch_qtlhap_chrom(p, ctx->stream);
    launch_qtlhap_design(p, ctx->stream);
    for (size_t r0 = 0; r0 < R; r0 += rt) {
        q.r0 = (int)r0;
        q.rn = (int)std::min(rt, R - r0);
        launch_qtl_gather(q, ctx->stream);
        launch_qtl_null(q, ctx->stream);
        launch_qtlhap_scan(p, ctx->stream);
        if (r0 + q.rn > (size_t)T) launch_qtl_finish(q, ctx->stream);
    }
    HIP_TRY(ctx, hipGetLastError());
    return qtl_fetch_outputs(ctx, dev, outputs);
}

// ------------------------------------------------------------------------------------------------
// Variance-component scan (cnf2_qtlvc.h, cnf2_qtlvc_kernels.hip), in the founder-haplotype scan's order of steps and on its
// mask: the individuals of `use` with all eight columns in [0, H).
// ------------------------------------------------------------------------------------------------
int cnf2_qtl_scan_vc(cnf2_ctx* ctx, int n, const double* descent, const int32_t* col, int n_columns, int n_traits,
                     const double* pheno, const uint8_t* use, int n_cov, const double* cov, int n_perm, const int32_t* perm,
                     double* lod_out, double* h_out, double* sigma2_out, double* blup_out, double* eval_out, int32_t* rank_out,
                     double* rss0_out, int32_t* n_used_out, double* perm_max_out, uint32_t flags)
{
    if (!ctx) return CNF2_ERR_ARG;
    if (ctx->n_markers <= 0) return fail(ctx, CNF2_ERR_STATE, "the map must be uploaded first");
    if (n < 1 || n_traits < 1 || !pheno) return fail(ctx, CNF2_ERR_ARG, "n and n_traits must be at least 1 and pheno not NULL");
    if (!descent || !col) return fail(ctx, CNF2_ERR_ARG, "descent and col must not be NULL");
    if (n_columns < 1 || n_columns > QTLVC_MAXH) return fail(ctx, CNF2_ERR_ARG, "n_columns must be 1 .. %d", QTLVC_MAXH);
    if (n_cov < 0 || n_cov > QTL_MAXK || (n_cov > 0 && !cov)) return fail(ctx, CNF2_ERR_ARG, "n_cov must be 0 .. %d, with cov", QTL_MAXK);
    if (n_perm < 0 || (n_perm > 0) != (perm != nullptr) || (n_perm > 0) != (perm_max_out != nullptr))
        return fail(ctx, CNF2_ERR_ARG, "perm and perm_max_out must be NULL exactly when n_perm is 0");
    if (!lod_out || !h_out || !sigma2_out || !rank_out || !rss0_out || !n_used_out) return fail(ctx, CNF2_ERR_ARG, "an output pointer is NULL");
    if ((size_t)n_traits * ((size_t)n_perm + 1) > (size_t)1 << 30) return fail(ctx, CNF2_ERR_ARG, "too many columns");
    const bool rows_dev = (flags & CNF2_QTL_ORIGIN_DEVICE) != 0;
    if (rows_dev && ((uintptr_t)descent & 15)) return fail(ctx, CNF2_ERR_ARG, "device descent rows must be aligned to 16 bytes");
    std::vector<uint8_t> inmodel(n);
    const int            bad = qtlhap_mask(n, use, col, n_columns, inmodel.data());
    if (bad >= 0) return fail(ctx, CNF2_ERR_ARG, "a column of individual %d is not in -1 .. %d", bad, n_columns - 1);
    QtlArgs a = {n, n_traits, n_cov, n_perm, pheno, inmodel.data(), cov, perm, lod_out, nullptr, rss0_out, perm_max_out, rank_out, n_used_out};
    std::vector<uint8_t> mask;
    RC_TRY(qtl_check_values(ctx, a, &mask));
    RC_TRY(qtl_check_perm(ctx, n, n_perm, perm, mask.data()));
    QtlHapLayout lay;
    qtlhap_layout(n, mask.data(), col, &lay);
    QtlCentred centred;
    qtl_centre(a, mask, centred);
    HIP_TRY(ctx, hipSetDevice(ctx->device));

    const bool   dev = (flags & CNF2_OUT_DEVICE) != 0;
    const int    M = ctx->n_markers, C = ctx->n_chrom, K = n_cov, T = n_traits, H = n_columns, nx = K + 1;
    const size_t R = (size_t)T * ((size_t)n_perm + 1);
    const size_t rt = qtl_column_tile(n, R, n_perm, 0, ctx->qtl_columns[QTL_CAP_SCAN]);
    QtlMarkerMap map = qtl_marker_map(ctx->chromstarts.data(), C, 0, C, 2, true, true);
    // col and the gather list behind the marker map, as the founder-haplotype scan lays them out
    std::vector<int32_t>& img = map.image;
    auto append = [&](const int32_t* v, size_t count) {
        const size_t o = img.size();
        img.insert(img.end(), v, v + count);
        if (count == 0) img.push_back(0);
        return o;
    };
    const size_t o_col = append(col, (size_t)n * 8), o_gidx = append(lay.gidx.data(), lay.gidx.size());
    const size_t o_steppat = append(lay.steppat.data(), lay.steppat.size()), o_stepend = append(lay.stepend.data(), lay.stepend.size());
    const size_t o_patcol = append(lay.patcol.data(), lay.patcol.size());

    const size_t n_rows = (size_t)n * M * 8;
    if (!rows_dev) RC_TRY(ctx->d_descent.ensure(ctx, n_rows));
    RC_TRY(qtl_reserve_inputs(ctx, a, rt, 0));
    QtlVcParams p;
    memset(&p, 0, sizeof(p));
    QtlParams& q = p.q;
    q = qtl_gather_params(ctx, a, rt);
    auto outputs = [&](auto each) -> int {
        RC_TRY(each(n_used_out, ctx->d_qv_nc, (size_t)C, &q.nc));
        RC_TRY(each(rank_out, ctx->d_qv_rank, (size_t)M, &p.rank));
        RC_TRY(each(lod_out, ctx->d_qv_lod, (size_t)T * M, &q.lod));
        RC_TRY(each(h_out, ctx->d_qv_h, (size_t)T * M, &p.h));
        RC_TRY(each(sigma2_out, ctx->d_qv_sigma2, (size_t)T * M, &p.sigma2));
        RC_TRY(each(blup_out, ctx->d_qv_blup, (size_t)T * M * H, &p.blup));
        RC_TRY(each(eval_out, ctx->d_qv_eval, (size_t)M * H, &p.eval));
        RC_TRY(each(rss0_out, ctx->d_qv_rss0, (size_t)T * C, &q.rss0));
        return each(perm_max_out, ctx->d_qv_pmax, (size_t)n_perm * T * C, &q.pmax);
    };
    RC_TRY(ctx->d_qv_map.ensure(ctx, img.size()));
    RC_TRY(ctx->d_q_chol.ensure(ctx, (size_t)C * QTL_CHOL));
    RC_TRY(ctx->d_qv_rec.ensure(ctx, (size_t)M * qtlvc_rec_size(H, nx)));
    RC_TRY(ctx->d_qv_null.ensure(ctx, (size_t)C * (nx + 1) * rt));
    if (n_perm > 0) RC_TRY(ctx->d_qv_tilemax.ensure(ctx, map.n_tiles * rt));
    RC_TRY(qtl_stage_outputs(ctx, dev, outputs));
    if (!rows_dev) {
        // (complete on return: the caller's array is not read after the call)
        HIP_TRY(ctx, hipMemcpyAsync(ctx->d_descent.ptr, descent, n_rows * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
        HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    }
    RC_TRY(qtl_upload(ctx, ctx->d_qv_map, img.data(), img.size()));
    RC_TRY(qtl_upload_inputs(ctx, a, mask));

    q.M = M, q.C = C, q.P = n_perm, q.K = K, q.nx = nx;
    q.cov = ctx->d_q_cov;
    q.cs = ctx->d_qv_map, q.mchrom = ctx->d_qv_map + map.o_mchrom;
    q.tiles = ctx->d_qv_map + map.o_tiles, q.tile_start = ctx->d_qv_map + map.o_tstart, q.n_tiles = (int)map.n_tiles;
    q.cmask = ctx->d_q_cmask, q.chol = ctx->d_q_chol, q.nullq = ctx->d_qv_null, q.tilemax = ctx->d_qv_tilemax;
    p.H = H, p.S = lay.S;
    p.descent = rows_dev ? descent : ctx->d_descent.ptr;
    p.col = ctx->d_qv_map + o_col, p.gidx = ctx->d_qv_map + o_gidx, p.steppat = ctx->d_qv_map + o_steppat;
    p.stepend = ctx->d_qv_map + o_stepend, p.patcol = ctx->d_qv_map + o_patcol;
    p.rec = ctx->d_qv_rec;

    launch_qtlvc_chrom(p, ctx->stream);
    if (!launch_qtlvc_design(p, ctx->stream)) return fail(ctx, CNF2_ERR_NOMEM, "the design kernel's LDS for %d columns was refused", H);
    for (size_t r0 = 0; r0 < R; r0 += rt) {
        q.r0 = (int)r0;
        q.rn = (int)std::min(rt, R - r0);
        launch_qtl_gather(q, ctx->stream);
        launch_qtl_null(q, ctx->stream);
        if (!launch_qtlvc_scan(p, ctx->stream)) return fail(ctx, CNF2_ERR_NOMEM, "the scan kernel's LDS for %d columns was refused", H);
        if (r0 + q.rn > (size_t)T) launch_qtl_finish(q, ctx->stream);
    }
    HIP_TRY(ctx, hipGetLastError());
    return qtl_fetch_outputs(ctx, dev, outputs);
}

// ------------------------------------------------------------------------------------------------
// Multiple-imputation scan (cnf2_qtlimp.h, cnf2_qtlimp_kernels.hip), in the scans' order of steps.  The states are checked
// before anything is written: host states here, device states by a kernel once every allocation has succeeded.
// ------------------------------------------------------------------------------------------------
int cnf2_qtl_scan_imp(cnf2_ctx* ctx, int n, int n_draws, const uint8_t* state, int n_traits, const double* pheno, const uint8_t* use,
                      int n_cov, const double* cov, int n_perm, const int32_t* perm, double* lod_out, double* coef_out,
                      int32_t* rank_out, double* rss0_out, int32_t* n_used_out, double* perm_max_out, double* draw_lod_out,
                      uint32_t flags)
{
    if (!ctx) return CNF2_ERR_ARG;
    QtlArgs a = {n, n_traits, n_cov, n_perm, pheno, use, cov, perm, lod_out, coef_out, rss0_out, perm_max_out, rank_out, n_used_out};
    std::vector<uint8_t> mask;
    QtlCentred           centred;
    RC_TRY(qtl_validate(ctx, a, &mask, &centred));
    if (n_draws < 1 || n_draws > QTLIMP_MAXD) return fail(ctx, CNF2_ERR_ARG, "n_draws must be 1 .. %d", QTLIMP_MAXD);
    if (!state) return fail(ctx, CNF2_ERR_ARG, "state is NULL");
    const bool   dev = (flags & CNF2_OUT_DEVICE) != 0, state_dev = (flags & CNF2_QTL_STATE_DEVICE) != 0;
    const int    M = ctx->n_markers, C = ctx->n_chrom, nx = a.K + 1, D = n_draws;
    const size_t n_state = (size_t)n * D * M;
    if ((size_t)D * a.T * (size_t)M > (size_t)1 << 40) return fail(ctx, CNF2_ERR_ARG, "too many draws, traits or markers");
    if (!state_dev)
        for (int i = 0; i < n; i++)
            for (int c = 0; c < C; c++) {
                const int first = ctx->chromstarts[c];
                switch (qtlimp_check_cells(state + (size_t)i * D * M, D, M, first, ctx->chromstarts[c + 1] - first)) {
                case QTLIMP_STATE_RANGE: return fail(ctx, CNF2_ERR_ARG, "a state of individual %d on chromosome %d is in 64 .. 254", i, c);
                case QTLIMP_STATE_PARTIAL:
                    return fail(ctx, CNF2_ERR_ARG, "individual %d is skipped (0xFF) in some cells of chromosome %d and not in all", i, c);
                }
            }
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    const size_t       R = (size_t)a.T * ((size_t)a.P + 1);
    const size_t       rt = qtl_column_tile(a.n, R, a.P, 0, ctx->qtl_columns[QTL_CAP_IMP]);
    const QtlMarkerMap map = qtl_marker_map(ctx->chromstarts.data(), C, 0, C, 16, true, true);

    RC_TRY(qtl_reserve_inputs(ctx, a, rt, 0));
    QtlImpParams p;
    memset(&p, 0, sizeof(p));
    QtlParams& q = p.q;
    q = qtl_gather_params(ctx, a, rt);
    auto outputs = [&](auto each) -> int {
        RC_TRY(each(a.n_used, ctx->d_qi_nc, (size_t)C, &q.nc));
        RC_TRY(each(a.rank, ctx->d_qi_rank, (size_t)M, &q.rank));
        RC_TRY(each(a.lod, ctx->d_qi_lod, (size_t)a.T * M, &q.lod));
        RC_TRY(each(a.coef, ctx->d_qi_coef, (size_t)a.T * M * 2, &q.coef));
        RC_TRY(each(a.rss0, ctx->d_qi_rss0, (size_t)a.T * C, &q.rss0));
        RC_TRY(each(a.pmax, ctx->d_qi_pmax, (size_t)a.P * a.T * C, &q.pmax));
        return each(draw_lod_out, ctx->d_qi_draw, (size_t)D * a.T * M, &p.draw_lod);
    };
    if (!state_dev) RC_TRY(ctx->d_qi_state.ensure(ctx, n_state));
    RC_TRY(ctx->d_qi_map.ensure(ctx, map.image.size()));
    RC_TRY(ctx->d_qi_bad.ensure(ctx, 2));
    RC_TRY(ctx->d_q_chol.ensure(ctx, (size_t)C * QTL_CHOL));
    RC_TRY(ctx->d_qi_mkd.ensure(ctx, (size_t)D * M * QTL_MK));
    RC_TRY(ctx->d_q_null.ensure(ctx, (size_t)C * (nx + 1) * rt));
    if (a.P > 0) RC_TRY(ctx->d_qi_tilemax.ensure(ctx, map.n_tiles * rt));
    RC_TRY(qtl_stage_outputs(ctx, dev, outputs));
    if (!state_dev) RC_TRY(qtl_upload(ctx, ctx->d_qi_state, state, n_state));
    RC_TRY(qtl_upload(ctx, ctx->d_qi_map, map.image.data(), map.image.size()));

    q.M = M, q.C = C, q.P = a.P, q.K = a.K, q.nx = nx;
    q.additive = (flags & CNF2_QTL_ADDITIVE) ? 1 : 0;
    q.cov = ctx->d_q_cov;
    q.cs = ctx->d_qi_map, q.mchrom = ctx->d_qi_map + map.o_mchrom;
    q.tiles = ctx->d_qi_map + map.o_tiles, q.tile_start = ctx->d_qi_map + map.o_tstart, q.n_tiles = (int)map.n_tiles;
    q.cmask = ctx->d_q_cmask, q.chol = ctx->d_q_chol;
    q.nullq = ctx->d_q_null, q.tilemax = ctx->d_qi_tilemax;
    p.D = D, p.state = state_dev ? state : ctx->d_qi_state.ptr, p.mkd = ctx->d_qi_mkd, p.bad = ctx->d_qi_bad;

    if (state_dev) {
        int32_t bad[2] = {0, 0};
        HIP_TRY(ctx, hipMemsetAsync(p.bad, 0, sizeof(bad), ctx->stream));
        launch_qtlimp_check(p, ctx->stream);
        HIP_TRY(ctx, hipGetLastError());
        HIP_TRY(ctx, hipMemcpyAsync(bad, p.bad, sizeof(bad), hipMemcpyDeviceToHost, ctx->stream));
        HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
        if (bad[0]) return fail(ctx, CNF2_ERR_ARG, "a state is in 64 .. 254");
        if (bad[1]) return fail(ctx, CNF2_ERR_ARG, "an individual is skipped (0xFF) in some cells of a chromosome and not in all");
    }
    RC_TRY(qtl_upload_inputs(ctx, a, mask));

    launch_qtlimp_chrom(p, ctx->stream);
    launch_qtlimp_design(p, ctx->stream);
    launch_qtlimp_rank(p, ctx->stream);
    for (size_t r0 = 0; r0 < R; r0 += rt) {
        q.r0 = (int)r0;
        q.rn = (int)std::min(rt, R - r0);
        launch_qtl_gather(q, ctx->stream);
        launch_qtl_null(q, ctx->stream);
        launch_qtlimp_scan(p, ctx->stream);
        if (r0 + q.rn > (size_t)a.T) launch_qtl_finish(q, ctx->stream);
    }
    HIP_TRY(ctx, hipGetLastError());
    return qtl_fetch_outputs(ctx, dev, outputs);
}

// ------------------------------------------------------------------------------------------------
// Kinship sums (cnf2_kinship.h, cnf2_kinship_kernels.hip), in the scans' order of steps
// ------------------------------------------------------------------------------------------------
int cnf2_kinship_sums(cnf2_ctx* ctx, int n, const double* origin, int chrom_begin, int chrom_end, double* sum_out,
                      int32_t* n_markers_out, uint32_t flags)
{
    if (!ctx) return CNF2_ERR_ARG;
    if (ctx->n_markers <= 0) return fail(ctx, CNF2_ERR_STATE, "the map must be uploaded first");
    QtlOrigin org;
    RC_TRY(qtl_origin_source(ctx, n, origin, flags, &org));
    if (n < 1 || n > 46340) return fail(ctx, CNF2_ERR_ARG, "n must be 1 .. 46340");
    if (chrom_begin < 0 || chrom_end > ctx->n_chrom || chrom_begin >= chrom_end)
        return fail(ctx, CNF2_ERR_ARG, "the chromosome range must be non-empty and within 0 .. %d", ctx->n_chrom);
    if (!sum_out || !n_markers_out) return fail(ctx, CNF2_ERR_ARG, "an output pointer is NULL");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    const bool dev = (flags & CNF2_OUT_DEVICE) != 0;
    KinParams  q;
    memset(&q, 0, sizeof(q));
    q.n = n, q.M = ctx->n_markers;
    q.m_lo   = ctx->chromstarts[chrom_begin];
    q.n_mark = ctx->chromstarts[chrom_end] - q.m_lo;
    q.n_pad  = (n + KIN_TILE - 1) / KIN_TILE * KIN_TILE;
    q.m_pad  = (q.n_mark + KIN_KC - 1) / KIN_KC * KIN_KC;
    const size_t  nn = (size_t)n * n;
    const int32_t n_mark = q.n_mark;
    const bool    split = kin_is_split(n, q.n_mark);
    const int     chunks = split ? (q.m_pad + KIN_CHUNK - 1) / KIN_CHUNK : 1;
    // the chunks summed together in a round: at most KIN_ROUND, their partial sums under 256 MB (the order of the additions
    // does not depend on it)
    const int     round = split ? (int)std::max<size_t>(1, std::min<size_t>(std::min(chunks, KIN_ROUND), ((size_t)256 << 20) / (nn * 8))) : 1;
    auto outputs = [&](auto each) -> int { return each(sum_out, ctx->d_kin_sum, nn, &q.sum); };
    RC_TRY(qtl_origin_reserve(ctx, org));
    RC_TRY(ctx->d_kin_image.ensure(ctx, (size_t)q.m_pad * q.n_pad));
    if (split) RC_TRY(ctx->d_kin_part.ensure(ctx, (size_t)round * nn));
    RC_TRY(qtl_stage_outputs(ctx, dev, outputs));
    RC_TRY(qtl_origin_stage(ctx, org));
    q.origin = org.dev, q.image = ctx->d_kin_image;
    launch_kin_pack(q, ctx->stream);
    if (!split) {
        q.k_lo = 0, q.k_len = q.m_pad, q.out = q.sum;
        launch_kin_syrk(q, 1, ctx->stream);
    } else {
        q.out = ctx->d_kin_part, q.k_len = KIN_CHUNK;
        for (int c0 = 0; c0 < chunks; c0 += round) {
            q.k_lo = c0 * KIN_CHUNK, q.parts = std::min(round, chunks - c0), q.first = c0 == 0;
            launch_kin_syrk(q, q.parts, ctx->stream);
            launch_kin_finish(q, ctx->stream);
        }
    }
    HIP_TRY(ctx, hipGetLastError());
    if (dev) HIP_TRY(ctx, hipMemcpyAsync(n_markers_out, &n_mark, sizeof(int32_t), hipMemcpyHostToDevice, ctx->stream));
    else *n_markers_out = n_mark;
    return qtl_fetch_outputs(ctx, dev, outputs);
}

// ------------------------------------------------------------------------------------------------
// Column scan (cnf2_qtlcols.h, cnf2_qtlcols_kernels.hip), in the scans' order of steps
// ------------------------------------------------------------------------------------------------
int cnf2_qtl_scan_cols(cnf2_ctx* ctx, int n, int n_mark, int ne, const double* reg, const double* scale, int nx, const double* x0,
                       int n_traits, const double* pheno, int n_perm, const int32_t* perm, double* lod_out, double* coef_out,
                       int32_t* rank_out, double* rss0_out, double* perm_max_out, uint32_t flags)
{
    if (!ctx) return CNF2_ERR_ARG;
    if (n < 1 || n_mark < 1 || n_traits < 1) return fail(ctx, CNF2_ERR_ARG, "n, n_mark and n_traits must be at least 1");
    if (ne < 1 || ne > 2) return fail(ctx, CNF2_ERR_ARG, "ne must be 1 or 2");
    if (nx < 1 || nx > QTL_NX) return fail(ctx, CNF2_ERR_ARG, "nx must be 1 .. %d", QTL_NX);
    if (!reg || !x0 || !pheno) return fail(ctx, CNF2_ERR_ARG, "reg, x0 and pheno must not be NULL");
    if (n_perm < 0 || (n_perm > 0) != (perm != nullptr) || (n_perm > 0) != (perm_max_out != nullptr))
        return fail(ctx, CNF2_ERR_ARG, "perm and perm_max_out must be NULL exactly when n_perm is 0");
    if (!lod_out || !coef_out || !rank_out || !rss0_out) return fail(ctx, CNF2_ERR_ARG, "an output pointer is NULL");
    const size_t R = (size_t)n_traits * ((size_t)n_perm + 1);
    if (R > (size_t)1 << 30 || (size_t)n * n_mark * ne > (size_t)1 << 40) return fail(ctx, CNF2_ERR_ARG, "too many columns");
    const bool reg_dev = (flags & CNF2_QTL_REG_DEVICE) != 0;
    if (reg_dev && ((uintptr_t)reg & 15)) return fail(ctx, CNF2_ERR_ARG, "device regressors must be aligned to 16 bytes");
    for (size_t e = 0; e < (size_t)n * n_traits; e++)
        if (!std::isfinite(pheno[e])) return fail(ctx, CNF2_ERR_ARG, "phenotype %d of individual %d is not finite", (int)(e % n_traits), (int)(e / n_traits));
    for (size_t e = 0; e < (size_t)n * nx; e++)
        if (!std::isfinite(x0[e])) return fail(ctx, CNF2_ERR_ARG, "column %d of x0 is not finite at individual %d", (int)(e % nx), (int)(e / nx));
    if (scale)
        for (int i = 0; i < n; i++)
            if (!std::isfinite(scale[i])) return fail(ctx, CNF2_ERR_ARG, "scale is not finite at individual %d", i);
    RC_TRY(qtl_check_perm(ctx, n, n_perm, perm, nullptr));
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    const bool   dev = (flags & CNF2_OUT_DEVICE) != 0;
    const int    M = n_mark, T = n_traits, P = n_perm;
    const size_t rt = qtl_column_tile(n, R, P, 0, ctx->qtl_columns[QTL_CAP_SCAN]), n_tiles = ((size_t)M + 15) / 16;
    const size_t n_reg = reg_dev ? 0 : (size_t)n * M * ne, n_scale = scale ? (size_t)n : 0;

    QtlColsParams q;
    memset(&q, 0, sizeof(q));
    auto outputs = [&](auto each) -> int {
        RC_TRY(each(rank_out, ctx->d_ql_rank, (size_t)M, &q.rank));
        RC_TRY(each(lod_out, ctx->d_ql_lod, (size_t)T * M, &q.lod));
        RC_TRY(each(coef_out, ctx->d_ql_coef, (size_t)T * M * 2, &q.coef));
        RC_TRY(each(rss0_out, ctx->d_ql_rss0, (size_t)T, &q.rss0));
        return each(perm_max_out, ctx->d_ql_pmax, (size_t)P * T, &q.pmax);
    };
    if (n_reg > 0) RC_TRY(ctx->d_ql_reg.ensure(ctx, n_reg));
    if (n_scale > 0) RC_TRY(ctx->d_ql_scale.ensure(ctx, n_scale));
    RC_TRY(ctx->d_ql_x0.ensure(ctx, (size_t)n * nx));
    RC_TRY(ctx->d_ql_pheno.ensure(ctx, (size_t)n * T));
    if (P > 0) RC_TRY(ctx->d_ql_perm.ensure(ctx, (size_t)P * n));
    RC_TRY(ctx->d_ql_chol.ensure(ctx, QTL_CHOL));
    RC_TRY(ctx->d_ql_mk.ensure(ctx, (size_t)M * QTL_MK));
    RC_TRY(ctx->d_ql_Y.ensure(ctx, (size_t)n * rt));
    RC_TRY(ctx->d_ql_null.ensure(ctx, (size_t)(nx + 1) * rt));
    if (P > 0) RC_TRY(ctx->d_ql_tilemax.ensure(ctx, n_tiles * rt));
    RC_TRY(qtl_stage_outputs(ctx, dev, outputs));
    RC_TRY(qtl_upload(ctx, ctx->d_ql_reg, reg, n_reg));
    RC_TRY(qtl_upload(ctx, ctx->d_ql_scale, scale, n_scale));
    RC_TRY(qtl_upload(ctx, ctx->d_ql_x0, x0, (size_t)n * nx));
    RC_TRY(qtl_upload(ctx, ctx->d_ql_pheno, pheno, (size_t)n * T));
    RC_TRY(qtl_upload(ctx, ctx->d_ql_perm, perm, (size_t)P * n));

    q.n = n, q.M = M, q.ne = ne, q.T = T, q.P = P, q.nx = nx;
    q.reg = reg_dev ? reg : ctx->d_ql_reg.ptr, q.scale = scale ? ctx->d_ql_scale.ptr : nullptr;
    q.x0 = ctx->d_ql_x0, q.pheno = ctx->d_ql_pheno, q.perm = ctx->d_ql_perm;
    q.chol = ctx->d_ql_chol, q.mk = ctx->d_ql_mk, q.Y = ctx->d_ql_Y, q.nullq = ctx->d_ql_null, q.tilemax = ctx->d_ql_tilemax;
    q.rstride = (int)rt, q.n_tiles = (int)n_tiles;

    launch_qtlcols_null(q, ctx->stream);
    launch_qtlcols_design(q, ctx->stream);
    for (size_t r0 = 0; r0 < R; r0 += rt) {
        q.r0 = (int)r0;
        q.rn = (int)std::min(rt, R - r0);
        launch_qtlcols_gather(q, ctx->stream);
        launch_qtlcols_colnull(q, ctx->stream);
        launch_qtlcols_scan(q, ctx->stream);
        if (r0 + q.rn > (size_t)T) launch_qtlcols_finish(q, ctx->stream);
    }
    HIP_TRY(ctx, hipGetLastError());
    return qtl_fetch_outputs(ctx, dev, outputs);
}

// ------------------------------------------------------------------------------------------------
// Bootstrap scan (cnf2_qtlboot.h, cnf2_qtlboot_kernels.hip), in the scans' order of steps
// ------------------------------------------------------------------------------------------------
int cnf2_qtl_scan_boot(cnf2_ctx* ctx, int n, const double* origin, int n_traits, const double* pheno, const uint8_t* use, int n_cov,
                       const double* cov, int chrom_begin, int chrom_end, int n_boot, const int32_t* count, double* boot_max_out,
                       int32_t* boot_arg_out, int32_t* n_boot_out, double* boot_lod_out, uint32_t flags)
{
    if (!ctx) return CNF2_ERR_ARG;
    if (ctx->n_markers <= 0) return fail(ctx, CNF2_ERR_STATE, "the map must be uploaded first");
    QtlOrigin org;
    RC_TRY(qtl_origin_source(ctx, n, origin, flags, &org));
    if (n < 1 || n_traits < 1 || !pheno) return fail(ctx, CNF2_ERR_ARG, "n and n_traits must be at least 1 and pheno not NULL");
    if (n_cov < 0 || n_cov > QTL_MAXK || (n_cov > 0 && !cov)) return fail(ctx, CNF2_ERR_ARG, "n_cov must be 0 .. %d, with cov", QTL_MAXK);
    if (chrom_begin < 0 || chrom_end > ctx->n_chrom || chrom_begin >= chrom_end)
        return fail(ctx, CNF2_ERR_ARG, "the chromosome range must be non-empty and within 0 .. %d", ctx->n_chrom);
    if (n_boot < 1 || !count) return fail(ctx, CNF2_ERR_ARG, "n_boot must be at least 1 and count not NULL");
    if (!boot_max_out || !boot_arg_out || !n_boot_out) return fail(ctx, CNF2_ERR_ARG, "an output pointer is NULL");
    const int    T = n_traits, K = n_cov, B = n_boot, nc = chrom_end - chrom_begin;
    const int    m_lo = ctx->chromstarts[chrom_begin], n_mark = ctx->chromstarts[chrom_end] - m_lo;
    if ((size_t)B * T > (size_t)1 << 30 || (size_t)B * T * (size_t)n_mark > (size_t)1 << 40 || T > 65535 || nc > 65535)
        return fail(ctx, CNF2_ERR_ARG, "too many replicates, traits or chromosomes");
    // (the phenotype side is the single scan's without permutations; the scan has its own outputs)
    QtlArgs a = {n, T, K, 0, pheno, use, cov, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
    std::vector<uint8_t> mask;
    RC_TRY(qtl_check_values(ctx, a, &mask));
    for (int b = 0; b < B; b++)
        for (int i = 0; i < n; i++) {
            const int32_t v = count[(size_t)b * n + i];
            if (v < 0) return fail(ctx, CNF2_ERR_ARG, "count of individual %d in replicate %d is negative", i, b);
            if (v > 0 && !mask[i]) return fail(ctx, CNF2_ERR_ARG, "replicate %d draws individual %d, which is not used", b, i);
        }
    // the columns minus their unweighted means over the used individuals, as every scan
    QtlCentred centred;
    qtl_centre(a, mask, centred);

    HIP_TRY(ctx, hipSetDevice(ctx->device));
    const bool dev = (flags & CNF2_OUT_DEVICE) != 0;
    // the map as the kernels read it: the first marker of every scanned chromosome, the marker tiles, the tile starts
    const QtlMarkerMap map = qtl_marker_map(ctx->chromstarts.data(), ctx->n_chrom, chrom_begin, chrom_end, 16, false, false);
    const size_t       n_tiles = map.n_tiles, bt = qtl_replicate_tile(n, B), recd = qtlboot_rec_doubles(T);

    QtlBootParams q;
    memset(&q, 0, sizeof(q));
    auto outputs = [&](auto each) -> int {
        RC_TRY(each(boot_max_out, ctx->d_qo_max, (size_t)B * T * nc, &q.boot_max));
        RC_TRY(each(boot_arg_out, ctx->d_qo_arg, (size_t)B * T * nc, &q.boot_arg));
        RC_TRY(each(n_boot_out, ctx->d_qo_nb, (size_t)B * nc, &q.n_boot));
        return each(boot_lod_out, ctx->d_qo_lod, (size_t)B * T * n_mark, &q.boot_lod);
    };
    RC_TRY(qtl_origin_reserve(ctx, org));
    RC_TRY(qtl_reserve_inputs(ctx, a, 0, 0));
    RC_TRY(ctx->d_qo_map.ensure(ctx, map.image.size()));
    RC_TRY(ctx->d_qo_count.ensure(ctx, (size_t)B * n));
    RC_TRY(ctx->d_qo_cmask.ensure(ctx, (size_t)nc * n));
    RC_TRY(ctx->d_qo_W.ensure(ctx, (size_t)n * bt));
    RC_TRY(ctx->d_qo_rec.ensure(ctx, bt * nc * recd));
    RC_TRY(ctx->d_qo_tilemax.ensure(ctx, n_tiles * bt * T));
    RC_TRY(ctx->d_qo_tilearg.ensure(ctx, n_tiles * bt * T));
    RC_TRY(qtl_stage_outputs(ctx, dev, outputs));
    RC_TRY(qtl_origin_stage(ctx, org));
    RC_TRY(qtl_upload(ctx, ctx->d_qo_map, map.image.data(), map.image.size()));
    RC_TRY(qtl_upload_inputs(ctx, a, mask));
    RC_TRY(qtl_upload(ctx, ctx->d_qo_count, count, (size_t)B * n));

    q.n = n, q.M = ctx->n_markers, q.T = T, q.K = K, q.nx = K + 1;
    q.additive = (flags & CNF2_QTL_ADDITIVE) ? 1 : 0;
    q.nc = nc, q.m_lo = m_lo, q.n_mark = n_mark;
    q.origin = org.dev, q.pheno = ctx->d_q_pheno, q.cov = ctx->d_q_cov, q.use = ctx->d_q_use, q.count = ctx->d_qo_count;
    q.first = ctx->d_qo_map, q.tiles = ctx->d_qo_map + map.o_tiles, q.tile_start = ctx->d_qo_map + map.o_tstart, q.n_tiles = (int)n_tiles;
    q.cmask = ctx->d_qo_cmask, q.W = ctx->d_qo_W, q.rec = ctx->d_qo_rec, q.tilemax = ctx->d_qo_tilemax, q.tilearg = ctx->d_qo_tilearg;

    const int tc = qtlboot_trait_chunk(T);
    launch_qtlboot_mask(q, ctx->stream);
    for (size_t b0 = 0; b0 < (size_t)B; b0 += bt) {
        q.b0 = (int)b0;
        q.bn = (int)std::min(bt, (size_t)B - b0);
        q.bstride = (q.bn + 15) / 16 * 16;
        launch_qtlboot_gather(q, ctx->stream);
        launch_qtlboot_design(q, ctx->stream);
        launch_qtlboot_null(q, ctx->stream);
        // (every trait chunk repeats the design sums: a cell's bits do not depend on the chunk it falls in)
        for (int t0 = 0; t0 < T; t0 += tc) {
            q.t0 = t0, q.tn = std::min(tc, T - t0);
            launch_qtlboot_scan(q, ctx->stream);
        }
        launch_qtlboot_finish(q, ctx->stream);
    }
    HIP_TRY(ctx, hipGetLastError());
    return qtl_fetch_outputs(ctx, dev, outputs);
}

// ------------------------------------------------------------------------------------------------
// Multi-trait scan (cnf2_qtlmv.h, cnf2_qtlmv_kernels.hip), in the scans' order of steps
// ------------------------------------------------------------------------------------------------
int cnf2_qtl_scan_mv(cnf2_ctx* ctx, int n, const double* origin, int n_traits, const double* pheno, const uint8_t* use, int n_cov,
                     const double* cov, int n_perm, const int32_t* perm, double* lod_out, int32_t* rank_out, int32_t* trait_rank_out,
                     int32_t* n_used_out, double* perm_max_out, uint32_t flags)
{
    if (!ctx) return CNF2_ERR_ARG;
    QtlOrigin org;
    RC_TRY(qtl_origin_source(ctx, n, origin, flags, &org));
    if (n_traits > QTLMV_MAXT) return fail(ctx, CNF2_ERR_ARG, "n_traits must be 1 .. %d", QTLMV_MAXT);
    if (!trait_rank_out) return fail(ctx, CNF2_ERR_ARG, "an output pointer is NULL");
    // (the scan has no effects and no RSS0 to report: the common check sees lod_out in their place)
    QtlArgs a = {n, n_traits, n_cov, n_perm, pheno, use, cov, perm, lod_out, lod_out, lod_out, perm_max_out, rank_out, n_used_out};
    std::vector<uint8_t> mask;
    QtlCentred           centred;
    RC_TRY(qtl_validate(ctx, a, &mask, &centred));
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    const bool         dev = (flags & CNF2_OUT_DEVICE) != 0;
    const int          M = ctx->n_markers, C = ctx->n_chrom, T = a.T, T4 = qtlmv_width(T);
    const QtlMarkerMap map = qtl_marker_map(ctx->chromstarts.data(), C, 0, C, 16, true, true);
    const size_t       G = (size_t)a.P + 1, n_tiles = map.n_tiles;
    const size_t       gt = qtl_group_tile(a.n, T, G, a.P, n_tiles, ctx->qtl_columns[QTL_CAP_MV]);
    const size_t       per_wave = 64 / T4, ystride = (gt + per_wave - 1) / per_wave * 64, gstride = ystride / T4;

    QtlMvParams q;
    memset(&q, 0, sizeof(q));
    auto outputs = [&](auto each) -> int {
        RC_TRY(each(n_used_out, ctx->d_qm_nc, (size_t)C, &q.nc));
        RC_TRY(each(rank_out, ctx->d_qm_rank, (size_t)M, &q.rank));
        RC_TRY(each(trait_rank_out, ctx->d_qm_trank, (size_t)C, &q.trait_rank));
        RC_TRY(each(lod_out, ctx->d_qm_lod, (size_t)M, &q.lod));
        return each(perm_max_out, ctx->d_qm_pmax, (size_t)a.P * C, &q.pmax);
    };
    RC_TRY(qtl_origin_reserve(ctx, org));
    RC_TRY(qtl_reserve_inputs(ctx, a, ystride, 0));
    RC_TRY(ctx->d_qm_map.ensure(ctx, map.image.size()));
    RC_TRY(ctx->d_q_chol.ensure(ctx, (size_t)C * QTL_CHOL));
    RC_TRY(ctx->d_q_mk.ensure(ctx, (size_t)M * QTL_MK));
    RC_TRY(ctx->d_q_rank.ensure(ctx, (size_t)M));
    RC_TRY(ctx->d_qm_rec.ensure(ctx, (size_t)C * gstride * qtlmv_rec_doubles(T)));
    if (a.P > 0) RC_TRY(ctx->d_qm_tilemax.ensure(ctx, n_tiles * gstride));
    RC_TRY(qtl_stage_outputs(ctx, dev, outputs));
    RC_TRY(qtl_origin_stage(ctx, org));
    RC_TRY(qtl_upload(ctx, ctx->d_qm_map, map.image.data(), map.image.size()));
    RC_TRY(qtl_upload_inputs(ctx, a, mask));

    // the masks, n_c, the factors of S11 and the marker records: the single scan's kernels (their rank is the design's; the
    // scan's own also says where a chromosome is not scanned)
    QtlParams d;
    memset(&d, 0, sizeof(d));
    d.n = n, d.M = M, d.C = C, d.T = T, d.P = a.P, d.K = a.K, d.nx = a.K + 1;
    d.additive = (flags & CNF2_QTL_ADDITIVE) ? 1 : 0;
    d.origin = org.dev, d.cov = ctx->d_q_cov, d.use = ctx->d_q_use;
    d.cs = ctx->d_qm_map, d.mchrom = ctx->d_qm_map + map.o_mchrom;
    d.cmask = ctx->d_q_cmask, d.nc = q.nc, d.chol = ctx->d_q_chol, d.mk = ctx->d_q_mk, d.rank = ctx->d_q_rank;
    launch_qtl_chrom(d, ctx->stream);
    launch_qtl_design(d, ctx->stream);

    q.n = n, q.M = M, q.C = C, q.T = T, q.T4 = T4, q.P = a.P, q.K = a.K, q.nx = a.K + 1;
    q.ystride = (int)ystride, q.gstride = (int)gstride;
    q.origin = org.dev, q.pheno = ctx->d_q_pheno, q.cov = ctx->d_q_cov, q.use = ctx->d_q_use, q.perm = ctx->d_q_perm;
    q.cmask = ctx->d_q_cmask, q.chol = ctx->d_q_chol, q.mk = ctx->d_q_mk;
    q.tiles = ctx->d_qm_map + map.o_tiles, q.tile_start = ctx->d_qm_map + map.o_tstart, q.n_tiles = (int)n_tiles;
    q.Y = ctx->d_q_Y, q.rec = ctx->d_qm_rec, q.tilemax = ctx->d_qm_tilemax;
    for (size_t g0 = 0; g0 < G; g0 += gt) {
        q.g0 = (int)g0;
        q.gn = (int)std::min(gt, G - g0);
        launch_qtlmv_gather(q, ctx->stream);
        launch_qtlmv_null(q, ctx->stream);
        launch_qtlmv_scan(q, ctx->stream);
        if (g0 + q.gn > 1) launch_qtlmv_finish(q, ctx->stream);
    }
    HIP_TRY(ctx, hipGetLastError());
    return qtl_fetch_outputs(ctx, dev, outputs);
}

// The selection of a pair call as the kernels read it.  sel follows cnf2_qtl_scan2's rules (2 .. QTL2_MAXL strictly ascending
// marker indices); the loci of a chromosome are consecutive in it, so pair (j, k) of one chromosome is row pair_off[j] + k - j - 1
struct PairSel {
    std::vector<int32_t> chrom_sel;    // [C + 1] the chromosomes' ranges in sel
    std::vector<int32_t> pair_off;     // [L]
    int n_pairs = 0, max_anchors = 0;  // max_anchors: the most selected markers of a chromosome, less one
};
static int pair_selection(cnf2_ctx* ctx, int n_sel, const int32_t* sel, PairSel* out)
{
    if (n_sel < 2 || n_sel > QTL2_MAXL || !sel) return fail(ctx, CNF2_ERR_ARG, "n_sel must be 2 .. %d, with sel", QTL2_MAXL);
    const int M = ctx->n_markers, C = ctx->n_chrom;
    for (int j = 0; j < n_sel; j++)
        if (sel[j] < 0 || sel[j] >= M || (j > 0 && sel[j] <= sel[j - 1]))
            return fail(ctx, CNF2_ERR_ARG, "sel must be strictly ascending marker indices below %d", M);
    out->chrom_sel.assign((size_t)C + 1, 0);
    out->pair_off.assign((size_t)n_sel, 0);
    int j = 0, base = 0;
    for (int c = 0; c < C; c++) {
        const int j0 = j;
        while (j < n_sel && sel[j] < ctx->chromstarts[c + 1]) j++;
        const int S = j - j0;
        out->chrom_sel[c + 1] = j;
        for (int a = 0; a < S; a++) out->pair_off[j0 + a] = base + a * (2 * S - a - 1) / 2;
        base += S * (S - 1) / 2;
        out->max_anchors = std::max(out->max_anchors, S - 1);
    }
    out->n_pairs = base;
    return CNF2_OK;
}

// The pair scan on origin rows [n][M][4]: cnf2_qtl2.h, cnf2_qtl2_kernels.hip.  linked (cnf2_qtl_scan2_linked): with the joint
// rows [n][n_pairs][16] of the pairs on one chromosome -- device memory with CNF2_QTL_JOINT_DEVICE, else staged whole in the
// pair sweep's buffer -- the pair kernel's linked form fits those pairs the full design too
static int qtl_scan2_impl(cnf2_ctx* ctx, int n, const double* origin, const double* joint, bool linked, int n_sel,
                          const int32_t* sel, int n_traits, const double* pheno, const uint8_t* use, int n_cov, const double* cov,
                          int n_perm, const int32_t* perm, double* lod_add_out, double* lod_full_out, int32_t* rank_add_out,
                          int32_t* rank_full_out, double* rss0_out, int32_t* n_used_out, double* perm_max_out, uint32_t flags)
{
    if (!ctx) return CNF2_ERR_ARG;
    QtlOrigin org;
    RC_TRY(qtl_origin_source(ctx, n, origin, flags, &org));
    // (the phenotype side is the single scan's; its lod / coef / rank slots stand for this call's four pair outputs)
    QtlArgs a = {n, n_traits, n_cov, n_perm, pheno, use, cov, perm, lod_add_out, lod_full_out, rss0_out, perm_max_out,
                 rank_add_out, n_used_out};
    std::vector<uint8_t> mask;
    QtlCentred           centred;
    RC_TRY(qtl_validate(ctx, a, &mask, &centred));
    if (!rank_full_out) return fail(ctx, CNF2_ERR_ARG, "an output pointer is NULL");
    if (n_cov > QTL2_MAXK) return fail(ctx, CNF2_ERR_ARG, "n_cov must be 0 .. %d for the pair scan", QTL2_MAXK);
    if (n_sel < 2 || n_sel > QTL2_MAXL || !sel) return fail(ctx, CNF2_ERR_ARG, "n_sel must be 2 .. %d, with sel", QTL2_MAXL);
    const int M = ctx->n_markers, C = ctx->n_chrom, L = n_sel;
    for (int j = 0; j < L; j++)
        if (sel[j] < 0 || sel[j] >= M || (j > 0 && sel[j] <= sel[j - 1]))
            return fail(ctx, CNF2_ERR_ARG, "sel must be strictly ascending marker indices below %d", M);
    PairSel ps;
    if (linked) {
        if (!joint) return fail(ctx, CNF2_ERR_ARG, "joint must not be NULL");
        RC_TRY(pair_selection(ctx, n_sel, sel, &ps));
    }
    HIP_TRY(ctx, hipSetDevice(ctx->device));

    const bool   dev = (flags & CNF2_OUT_DEVICE) != 0;
    const bool   joint_host = linked && ps.n_pairs > 0 && !(flags & CNF2_QTL_JOINT_DEVICE);
    const size_t nj = (size_t)n * (size_t)ps.n_pairs * 16;
    const size_t R = (size_t)a.T * ((size_t)a.P + 1), LL = (size_t)L * L;
    const int    n_chunks = (L - 1 + QTL2_CHUNK - 1) / QTL2_CHUNK;
    const size_t rt = qtl_column_tile(a.n, R, a.P, (size_t)3 * L * n_chunks, ctx->qtl_columns[QTL_CAP_SCAN2]);
    // the map as the kernels read it: chromstarts, sel, the chromosomes of sel
    std::vector<int32_t> map(ctx->chromstarts.begin(), ctx->chromstarts.end());
    map.insert(map.end(), sel, sel + L);
    for (int j = 0, c = 0; j < L; j++) {
        while (sel[j] >= ctx->chromstarts[c + 1]) c++;
        map.push_back(c);
    }
    if (linked) map.insert(map.end(), ps.pair_off.begin(), ps.pair_off.end());

    Qtl2Params q;
    memset(&q, 0, sizeof(q));
    auto outputs = [&](auto each) -> int {
        RC_TRY(each(a.n_used, ctx->d_q2_nc, (size_t)C * C, &q.nc));
        RC_TRY(each(rank_add_out, ctx->d_q2_rank_add, LL, &q.rank_add));
        RC_TRY(each(rank_full_out, ctx->d_q2_rank_full, LL, &q.rank_full));
        RC_TRY(each(lod_add_out, ctx->d_q2_lod_add, (size_t)a.T * LL, &q.lod_add));
        RC_TRY(each(lod_full_out, ctx->d_q2_lod_full, (size_t)a.T * LL, &q.lod_full));
        RC_TRY(each(a.rss0, ctx->d_q2_rss0, (size_t)a.T * C * C, &q.rss0));
        return each(a.pmax, ctx->d_q2_pmax, (size_t)a.P * a.T * 3, &q.pmax);
    };
    RC_TRY(qtl_origin_reserve(ctx, org));
    RC_TRY(qtl_reserve_inputs(ctx, a, rt, 0));
    RC_TRY(ctx->d_q2_map.ensure(ctx, map.size()));
    if (joint_host) {
        size_t free_b = 0, total_b = 0;
        HIP_TRY(ctx, hipMemGetInfo(&free_b, &total_b));
        if (nj > ctx->d_pair.cap && nj * sizeof(double) > free_b + ctx->d_pair.cap * sizeof(double))
            return fail(ctx, CNF2_ERR_NOMEM, "the joint rows need %zu MB of device memory", (nj * 8) >> 20);
        RC_TRY(ctx->d_pair.ensure(ctx, nj));
    }
    RC_TRY(ctx->d_q2_yy.ensure(ctx, (size_t)C * C * rt));
    if (a.P > 0) RC_TRY(ctx->d_q2_chunkmax.ensure(ctx, (size_t)L * n_chunks * 3 * rt));
    RC_TRY(qtl_stage_outputs(ctx, dev, outputs));
    RC_TRY(qtl_origin_stage(ctx, org));
    RC_TRY(qtl_upload(ctx, ctx->d_q2_map, map.data(), map.size()));
    RC_TRY(qtl_upload_inputs(ctx, a, mask));
    if (joint_host) HIP_TRY(ctx, hipMemcpyAsync(ctx->d_pair, joint, nj * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
    if (linked && ps.n_pairs > 0) {
        q.joint    = joint_host ? (const double*)ctx->d_pair : joint;
        q.pair_off = ctx->d_q2_map + (C + 1 + 2 * L);
        q.n_pairs  = ps.n_pairs;
    }

    q.n = a.n, q.M = M, q.C = C, q.T = a.T, q.P = a.P, q.K = a.K, q.L = L;
    q.additive = (flags & CNF2_QTL_ADDITIVE) ? 1 : 0;
    q.origin = org.dev, q.pheno = ctx->d_q_pheno, q.cov = ctx->d_q_cov, q.use = ctx->d_q_use, q.perm = ctx->d_q_perm;
    q.cs = ctx->d_q2_map, q.sel = ctx->d_q2_map + (C + 1), q.selchrom = ctx->d_q2_map + (C + 1 + L);
    q.cmask = ctx->d_q_cmask, q.Y = ctx->d_q_Y, q.yy = ctx->d_q2_yy, q.chunkmax = ctx->d_q2_chunkmax;
    q.rstride = (int)rt, q.n_chunks = n_chunks;
    QtlParams g = qtl_gather_params(ctx, a, rt);

    launch_qtl2_mask(q, ctx->stream);
    launch_qtl2_fill(q, ctx->stream);
    for (size_t r0 = 0; r0 < R; r0 += rt) {
        q.r0 = g.r0 = (int)r0;
        q.rn = g.rn = (int)std::min(rt, R - r0);
        launch_qtl_gather(g, ctx->stream);
        launch_qtl2_null(q, ctx->stream);
        launch_qtl2_pairs(q, ctx->stream);
        if (r0 + q.rn > (size_t)a.T) launch_qtl2_finish(q, ctx->stream);
    }
    HIP_TRY(ctx, hipGetLastError());
    return qtl_fetch_outputs(ctx, dev, outputs);
}

int cnf2_qtl_scan2(cnf2_ctx* ctx, int n, const double* origin, int n_sel, const int32_t* sel, int n_traits, const double* pheno,
                   const uint8_t* use, int n_cov, const double* cov, int n_perm, const int32_t* perm, double* lod_add_out,
                   double* lod_full_out, int32_t* rank_add_out, int32_t* rank_full_out, double* rss0_out, int32_t* n_used_out,
                   double* perm_max_out, uint32_t flags)
{
    return qtl_scan2_impl(ctx, n, origin, nullptr, false, n_sel, sel, n_traits, pheno, use, n_cov, cov, n_perm, perm, lod_add_out,
                          lod_full_out, rank_add_out, rank_full_out, rss0_out, n_used_out, perm_max_out, flags);
}

int cnf2_qtl_scan2_linked(cnf2_ctx* ctx, int n, const double* origin, const double* joint, int n_sel, const int32_t* sel,
                          int n_traits, const double* pheno, const uint8_t* use, int n_cov, const double* cov, int n_perm,
                          const int32_t* perm, double* lod_add_out, double* lod_full_out, int32_t* rank_add_out,
                          int32_t* rank_full_out, double* rss0_out, int32_t* n_used_out, double* perm_max_out, uint32_t flags)
{
    return qtl_scan2_impl(ctx, n, origin, joint, true, n_sel, sel, n_traits, pheno, use, n_cov, cov, n_perm, perm, lod_add_out,
                          lod_full_out, rank_add_out, rank_full_out, rss0_out, n_used_out, perm_max_out, flags);
}

// The extended single-locus scan on origin rows [n][M][4]: cnf2_qtlx.h, cnf2_qtlx_kernels.hip
int cnf2_qtl_scanx(cnf2_ctx* ctx, int n, const double* origin, int n_traits, const double* pheno, const uint8_t* use, int n_cov,
                   const double* cov, int n_int, int n_perm, const int32_t* perm, double* lod_out, double* coef_out,
                   int32_t* rank_out, double* rss0_out, int32_t* n_used_out, double* perm_max_out, uint32_t flags)
{
    if (!ctx) return CNF2_ERR_ARG;
    QtlOrigin org;
    RC_TRY(qtl_origin_source(ctx, n, origin, flags, &org));
    QtlArgs a = {n, n_traits, n_cov, n_perm, pheno, use, cov, perm, lod_out, coef_out, rss0_out, perm_max_out, rank_out, n_used_out};
    std::vector<uint8_t> mask;
    QtlCentred           centred;
    RC_TRY(qtl_validate(ctx, a, &mask, &centred));
    if (n_int < 0 || n_int > n_cov) return fail(ctx, CNF2_ERR_ARG, "n_int must be 0 .. n_cov");
    const QtlxDesign ds = qtlx_design(n_cov, n_int, (flags & CNF2_QTL_ADDITIVE) != 0, (flags & CNF2_QTL_IMPRINT) != 0);
    if (ds.w > QTLX_MAXW)
        return fail(ctx, CNF2_ERR_ARG, "the design has %d columns (1 + n_cov + effects x (1 + n_int)); at most %d", ds.w, QTLX_MAXW);
    const int M = ctx->n_markers, C = ctx->n_chrom, ncoef = ds.w - ds.nx;
    HIP_TRY(ctx, hipSetDevice(ctx->device));

    const bool         dev = (flags & CNF2_OUT_DEVICE) != 0;
    const size_t       R = (size_t)a.T * ((size_t)a.P + 1);
    const QtlMarkerMap map = qtl_marker_map(ctx->chromstarts.data(), C, 0, C, QTLX_TILE, false, true);
    const size_t       n_tiles = map.n_tiles;
    const size_t       rt = qtl_column_tile(a.n, R, a.P, QTLX_NSTAT * n_tiles, ctx->qtl_columns[QTL_CAP_SCANX]);
    // (with interactive covariates the raw cov[n][K] follows the centred one: the products are those of the raw values)
    const size_t       n_covs = (size_t)a.n * a.K, n_raw = n_int > 0 ? n_covs : 0;

    QtlxParams q;
    memset(&q, 0, sizeof(q));
    auto outputs = [&](auto each) -> int {
        RC_TRY(each(a.n_used, ctx->d_qx_nc, (size_t)C, &q.nc));
        RC_TRY(each(a.rank, ctx->d_qx_rank, (size_t)M * 3, &q.rank));
        RC_TRY(each(a.lod, ctx->d_qx_lod, (size_t)a.T * M * 3, &q.lod));
        RC_TRY(each(a.coef, ctx->d_qx_coef, (size_t)a.T * M * ncoef, &q.coef));
        RC_TRY(each(a.rss0, ctx->d_qx_rss0, (size_t)a.T * C, &q.rss0));
        return each(a.pmax, ctx->d_qx_pmax, (size_t)a.P * a.T * C * QTLX_NSTAT, &q.pmax);
    };
    RC_TRY(qtl_origin_reserve(ctx, org));
    RC_TRY(qtl_reserve_inputs(ctx, a, rt, n_raw));
    RC_TRY(ctx->d_qx_map.ensure(ctx, map.image.size()));
    RC_TRY(ctx->d_qx_yy.ensure(ctx, (size_t)C * rt));
    if (a.P > 0) RC_TRY(ctx->d_qx_tilemax.ensure(ctx, n_tiles * QTLX_NSTAT * rt));
    RC_TRY(qtl_stage_outputs(ctx, dev, outputs));
    RC_TRY(qtl_origin_stage(ctx, org));
    RC_TRY(qtl_upload(ctx, ctx->d_qx_map, map.image.data(), map.image.size()));
    RC_TRY(qtl_upload_inputs(ctx, a, mask));
    if (n_raw > 0) {
        HIP_TRY(ctx, hipMemcpyAsync(ctx->d_q_cov.ptr + n_covs, cov, n_raw * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
        HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    }

    q.n = a.n, q.M = M, q.C = C, q.T = a.T, q.P = a.P, q.K = a.K, q.Ki = n_int;
    q.additive = (flags & CNF2_QTL_ADDITIVE) ? 1 : 0, q.imprint = (flags & CNF2_QTL_IMPRINT) ? 1 : 0;
    q.origin = org.dev, q.cov = ctx->d_q_cov, q.use = ctx->d_q_use;
    q.cov_raw = ctx->d_q_cov.ptr + n_raw;
    q.cs = ctx->d_qx_map, q.tiles = ctx->d_qx_map + map.o_tiles, q.tile_start = ctx->d_qx_map + map.o_tstart, q.n_tiles = (int)n_tiles;
    q.cmask = ctx->d_q_cmask, q.Y = ctx->d_q_Y, q.yy = ctx->d_qx_yy, q.tilemax = ctx->d_qx_tilemax, q.rstride = (int)rt;
    Qtl2Params k;                          // what qtl2_mask_kernel reads and writes
    memset(&k, 0, sizeof(k));
    k.n = a.n, k.M = M, k.C = C, k.origin = org.dev, k.use = ctx->d_q_use, k.cs = ctx->d_qx_map, k.cmask = ctx->d_q_cmask;
    QtlParams g = qtl_gather_params(ctx, a, rt);

    launch_qtl2_mask(k, ctx->stream);
    for (size_t r0 = 0; r0 < R; r0 += rt) {
        q.r0 = g.r0 = (int)r0;
        q.rn = g.rn = (int)std::min(rt, R - r0);
        launch_qtl_gather(g, ctx->stream);
        launch_qtlx_null(q, ctx->stream);
        launch_qtlx_markers(q, ctx->stream);
        if (r0 + q.rn > (size_t)a.T) launch_qtlx_finish(q, ctx->stream);
    }
    HIP_TRY(ctx, hipGetLastError());
    return qtl_fetch_outputs(ctx, dev, outputs);
}

// rows_out[n_sel][n][4] = the rows the last cnf2_sweep_qtl left in the context at the markers sel: one strided copy per
// marker.  The rows stay valid.
int cnf2_qtl_kept_rows(cnf2_ctx* ctx, int n, int n_sel, const int32_t* sel, double* rows_out)
{
    if (!ctx) return CNF2_ERR_ARG;
    RC_TRY(qtl_kept_check(ctx, n));
    if (n_sel < 0 || (n_sel > 0 && (!sel || !rows_out))) return fail(ctx, CNF2_ERR_ARG, "n_sel must not be negative, with sel and rows_out");
    const int M = ctx->n_markers;
    for (int j = 0; j < n_sel; j++)
        if (sel[j] < 0 || sel[j] >= M) return fail(ctx, CNF2_ERR_ARG, "sel must hold marker indices below %d", M);
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    for (int j = 0; j < n_sel; j++)
        HIP_TRY(ctx, hipMemcpy2DAsync(rows_out + (size_t)j * n * 4, 4 * sizeof(double), ctx->d_org.ptr + (size_t)sel[j] * 4,
                                      (size_t)M * 4 * sizeof(double), 4 * sizeof(double), (size_t)n, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    return CNF2_OK;
}

// The cofactor scan on origin rows [n][M][4]: cnf2_qtlcof.h, cnf2_qtlcof_kernels.hip
int cnf2_qtl_scan_cof(cnf2_ctx* ctx, int n, const double* origin, int n_traits, const double* pheno, const uint8_t* use, int n_cov,
                      const double* cov, int n_cof, const int32_t* cof, const int32_t* excl_lo, const int32_t* excl_hi, int n_perm,
                      const int32_t* perm, double* lod_out, double* lod_base_out, double* coef_out, int32_t* rank_out,
                      int32_t* rank_cof_out, double* rss0_out, int32_t* n_used_out, double* perm_max_out, uint32_t flags)
{
    if (!ctx) return CNF2_ERR_ARG;
    QtlOrigin org;
    RC_TRY(qtl_origin_source(ctx, n, origin, flags, &org));
    QtlArgs a = {n, n_traits, n_cov, n_perm, pheno, use, cov, perm, lod_out, coef_out, rss0_out, perm_max_out, rank_out, n_used_out};
    std::vector<uint8_t> mask;
    QtlCentred           centred;
    RC_TRY(qtl_validate(ctx, a, &mask, &centred));
    if (!lod_base_out || !rank_cof_out) return fail(ctx, CNF2_ERR_ARG, "an output pointer is NULL");
    if (flags & CNF2_QTL_IMPRINT) return fail(ctx, CNF2_ERR_ARG, "the cofactor scan has no imprinting effect");
    if (n_cof < 0 || n_cof > QTLCOF_MAXQ || (n_cof > 0 && (!cof || !excl_lo || !excl_hi)))
        return fail(ctx, CNF2_ERR_ARG, "n_cof must be 0 .. %d, with cof, excl_lo and excl_hi", QTLCOF_MAXQ);
    const QtlcofDesign ds = qtlcof_design(n_cov, n_cof, (flags & CNF2_QTL_ADDITIVE) != 0);
    if (ds.w > QTLCOF_MAXW)
        return fail(ctx, CNF2_ERR_ARG, "the design has %d columns (1 + n_cov + effects x (n_cof + 1)); at most %d", ds.w, QTLCOF_MAXW);
    const int M = ctx->n_markers, C = ctx->n_chrom, Q = n_cof;
    std::vector<int32_t> cofstart(Q);
    for (int k = 0, c = 0; k < Q; k++) {
        if (cof[k] < 0 || cof[k] >= M || (k > 0 && cof[k] <= cof[k - 1]))
            return fail(ctx, CNF2_ERR_ARG, "cof must be strictly ascending marker indices below %d", M);
        while (cof[k] >= ctx->chromstarts[c + 1]) c++;
        cofstart[k] = ctx->chromstarts[c];
        if (excl_lo[k] < ctx->chromstarts[c] || excl_hi[k] >= ctx->chromstarts[c + 1] || excl_lo[k] > cof[k] || excl_hi[k] < cof[k])
            return fail(ctx, CNF2_ERR_ARG, "the range %d .. %d of cofactor %d must lie on its chromosome and contain marker %d", excl_lo[k],
                        excl_hi[k], k, cof[k]);
    }
    HIP_TRY(ctx, hipSetDevice(ctx->device));

    const bool   dev = (flags & CNF2_OUT_DEVICE) != 0;
    const size_t R = (size_t)a.T * ((size_t)a.P + 1);
    // behind the marker map: the cofactors, the first markers of their chromosomes, and per marker the word of the
    // cofactors left out there
    QtlMarkerMap          mm = qtl_marker_map(ctx->chromstarts.data(), C, 0, C, QTLCOF_TILE, false, true);
    std::vector<int32_t>& map = mm.image;
    const size_t          n_tiles = mm.n_tiles, o_cof = map.size();
    map.insert(map.end(), cof, cof + Q);
    const size_t o_cofstart = map.size();
    map.insert(map.end(), cofstart.begin(), cofstart.end());
    const size_t o_skipw = map.size();
    for (int m = 0; m < M; m++) map.push_back((int32_t)qtlcof_skip_word(m, Q, excl_lo, excl_hi));
    const size_t rt = qtl_column_tile(a.n, R, a.P, n_tiles, ctx->qtl_columns[QTL_CAP_COF]);

    QtlcofParams q;
    memset(&q, 0, sizeof(q));
    auto outputs = [&](auto each) -> int {
        RC_TRY(each(a.n_used, ctx->d_qc_nc, (size_t)C, &q.nc));
        RC_TRY(each(a.rank, ctx->d_qc_rank, (size_t)M, &q.rank));
        RC_TRY(each(rank_cof_out, ctx->d_qc_rank_cof, (size_t)M, &q.rank_cof));
        RC_TRY(each(a.lod, ctx->d_qc_lod, (size_t)a.T * M, &q.lod));
        RC_TRY(each(lod_base_out, ctx->d_qc_lod_base, (size_t)a.T * M, &q.lod_base));
        RC_TRY(each(a.coef, ctx->d_qc_coef, (size_t)a.T * M * ds.ne, &q.coef));
        RC_TRY(each(a.rss0, ctx->d_qc_rss0, (size_t)a.T * C, &q.rss0));
        return each(a.pmax, ctx->d_qc_pmax, (size_t)a.P * a.T * C, &q.pmax);
    };
    RC_TRY(qtl_origin_reserve(ctx, org));
    RC_TRY(qtl_reserve_inputs(ctx, a, rt, 0));
    RC_TRY(ctx->d_qc_map.ensure(ctx, map.size()));
    RC_TRY(ctx->d_qc_img.ensure(ctx, std::max<size_t>(1, (size_t)a.n * ds.nc)));
    RC_TRY(ctx->d_qc_yy.ensure(ctx, (size_t)C * rt));
    if (a.P > 0) RC_TRY(ctx->d_qc_tilemax.ensure(ctx, n_tiles * rt));
    RC_TRY(qtl_stage_outputs(ctx, dev, outputs));
    RC_TRY(qtl_origin_stage(ctx, org));
    RC_TRY(qtl_upload(ctx, ctx->d_qc_map, map.data(), map.size()));
    RC_TRY(qtl_upload_inputs(ctx, a, mask));

    q.n = a.n, q.M = M, q.C = C, q.T = a.T, q.P = a.P, q.K = a.K, q.Q = Q;
    q.additive = (flags & CNF2_QTL_ADDITIVE) ? 1 : 0;
    q.origin = org.dev, q.cov = ctx->d_q_cov, q.use = ctx->d_q_use;
    q.cs = ctx->d_qc_map, q.tiles = ctx->d_qc_map + mm.o_tiles, q.tile_start = ctx->d_qc_map + mm.o_tstart, q.n_tiles = (int)n_tiles;
    q.cof = ctx->d_qc_map + o_cof, q.cofstart = ctx->d_qc_map + o_cofstart;
    q.skipw = reinterpret_cast<const uint32_t*>(ctx->d_qc_map.ptr + o_skipw);
    q.cofimg = ctx->d_qc_img, q.cmask = ctx->d_q_cmask, q.Y = ctx->d_q_Y, q.yy = ctx->d_qc_yy, q.tilemax = ctx->d_qc_tilemax;
    q.rstride = (int)rt;
    QtlParams g = qtl_gather_params(ctx, a, rt);

    launch_qtlcof_mask(q, ctx->stream);
    launch_qtlcof_gather(q, ctx->stream);
    for (size_t r0 = 0; r0 < R; r0 += rt) {
        q.r0 = g.r0 = (int)r0;
        q.rn = g.rn = (int)std::min(rt, R - r0);
        launch_qtl_gather(g, ctx->stream);
        launch_qtlcof_null(q, ctx->stream);
        launch_qtlcof_markers(q, ctx->stream);
        if (r0 + q.rn > (size_t)a.T) launch_qtlcof_finish(q, ctx->stream);
    }
    HIP_TRY(ctx, hipGetLastError());
    return qtl_fetch_outputs(ctx, dev, outputs);
}

// The four single-locus scans on origin rows [n][M][4] that fit a model by iteration per (marker, column) -- EM interval
// mapping, logistic, Cox and mean-variance regression -- through one driver, qtl_fit_scan.  What a scan says of itself:
struct QtlFitSpec {
    QtlCap cap;                 // its column cap
    int    tile;                // markers per tile
    int    nfit;                // fits per cell: lod, iters, status, perm_max and the tile maxima carry the factor
    int    nullq;               // doubles of a null fit per (chromosome, column); unused by the EM scan, which reads the single scan's
    bool   image;               // it reads the column image (qtl_gather_kernel)
    bool   extra_behind_coef;   // its one output beyond the shared ones follows coef in its list (else ll0)
};
// ... and what the driver tells it of the plan
struct QtlFitPlan {
    size_t rt, n_tiles, cells, ne;   // columns per tile, marker tiles, T x M, effects
};
static int qtl_fit_reserve_nothing(const QtlFitPlan&) { return CNF2_OK; }

static int qtl_fit_check_iter(cnf2_ctx* ctx, int max_iter, int most, double tol)
{
    if (max_iter < 1 || max_iter > most) return fail(ctx, CNF2_ERR_ARG, "max_iter must be 1 .. %d", most);
    if (!std::isfinite(tol)) return fail(ctx, CNF2_ERR_ARG, "tol must be finite");
    return CNF2_OK;
}
// the values v[n][T] (`what`: "phenotype", "status") of the used individuals are 0 or 1
static int qtl_fit_check_01(cnf2_ctx* ctx, const QtlArgs& a, const std::vector<uint8_t>& use, const double* v, const char* what)
{
    for (int i = 0; i < a.n; i++) {
        if (!use[i]) continue;
        for (int t = 0; t < a.T; t++) {
            const double y = v[(size_t)i * a.T + t];
            if (!(y == 0.0 || y == 1.0)) return fail(ctx, CNF2_ERR_ARG, "%s %d of individual %d is used and neither 0 nor 1", what, t, i);
        }
    }
    return CNF2_OK;
}
// qtl_centre with each difference rounded once (qtl_centre_columns_once: a shifted column gives the same bits, which a fit
// of a nearly collinear marker needs for the same printed effects); the covariates, and with `traits` the traits too
static void qtl_centre_once(QtlArgs& a, const std::vector<uint8_t>& use, QtlCentred& store, bool traits)
{
    if (traits) {
        qtl_centre_columns_once(a.pheno, a.n, a.T, use, store.pheno);
        a.pheno = store.pheno.data();
    }
    if (a.K > 0) {
        qtl_centre_columns_once(a.cov, a.n, a.K, use, store.cov);
        a.cov = store.cov.data();
    }
}

// The driver.  q: the scan's QtlemParams (the EM scan: the factor and the null fit are the single scan's, qtl_null_kernel
// runs per tile, and there are no scan words) or QtlbinParams (the null fits and scan words are the scan's own), zeroed by
// the caller, who may hold it inside a larger struct.  The callables are the scan's own part of a step: check(a, use,
// centred) its argument checks behind qtl_check's and its centring; extra(each, plan) its extra output; start() and
// tile(last), with q.r0 and q.rn set, its launches before the column tiles and per tile; reserve(plan) its own allocations.
// The masks, n_c, the column image and the EM scan's null fit are launched here (cnf2_qtl_kernels.hip).
extern "C++" template <class Q, class Check, class Extra, class Start, class Tile, class Reserve = int (*)(const QtlFitPlan&)>
static int qtl_fit_scan(cnf2_ctx* ctx, const QtlFitSpec& s, QtlFitBufs& b, int n, const double* origin, QtlArgs a, int max_iter,
                        double tol, int32_t* iters_out, int32_t* status_out, uint32_t flags, Q& q, Check check, Extra extra,
                        Start start, Tile tile, Reserve reserve = qtl_fit_reserve_nothing)
{
    constexpr bool em = std::is_same<Q, QtlemParams>::value;
    QtlOrigin      org;
    RC_TRY(qtl_origin_source(ctx, n, origin, flags, &org));
    std::vector<uint8_t> mask;
    QtlCentred           centred;
    RC_TRY(qtl_check(ctx, a, &mask));
    RC_TRY(check(a, mask, centred));
    const QtlemDesign ds = qtlem_design(a.K, (flags & CNF2_QTL_ADDITIVE) != 0, (flags & CNF2_QTL_IMPRINT) != 0);
    const int M = ctx->n_markers, C = ctx->n_chrom;
    HIP_TRY(ctx, hipSetDevice(ctx->device));

    const bool         dev = (flags & CNF2_OUT_DEVICE) != 0;
    const size_t       R = (size_t)a.T * ((size_t)a.P + 1), TC = (size_t)a.T * C;
    const QtlMarkerMap map = qtl_marker_map(ctx->chromstarts.data(), C, 0, C, s.tile, true, true);
    const size_t       n_tiles = map.n_tiles, cells = (size_t)a.T * M;
    const size_t       rt = qtl_column_tile(a.n, R, a.P, s.nfit * n_tiles, ctx->qtl_columns[s.cap]);
    const QtlFitPlan   plan = {rt, n_tiles, cells, (size_t)ds.ne};

    RC_TRY(qtl_origin_reserve(ctx, org));
    RC_TRY(qtl_reserve_inputs(ctx, a, s.image ? rt : 0, 0));
    QtlParams g = qtl_gather_params(ctx, a, rt);   // ... and the other kernels of cnf2_qtl_kernels.hip read and write
    double**  ll0;
    if constexpr (em) ll0 = &q.rss0;
    else ll0 = &q.ll0;
    auto outputs = [&](auto each) -> int {
        RC_TRY(each(a.n_used, b.nc, (size_t)C, &g.nc));
        RC_TRY(each(a.rank, b.rank, (size_t)M, &q.rank));
        RC_TRY(each(a.lod, b.lod, cells * s.nfit, &q.lod));
        RC_TRY(each(a.coef, b.coef, cells * ds.ne, &q.coef));
        if (s.extra_behind_coef) RC_TRY(extra(each, plan));
        RC_TRY(each(iters_out, b.iters, cells * s.nfit, &q.iters));
        RC_TRY(each(status_out, b.status, cells * s.nfit, &q.status));
        RC_TRY(each(a.rss0, b.ll0, TC, ll0));
        if (!s.extra_behind_coef) RC_TRY(extra(each, plan));
        return each(a.pmax, b.pmax, (size_t)a.P * TC * s.nfit, &q.pmax);
    };
    RC_TRY(b.map.ensure(ctx, map.image.size()));
    RC_TRY(ctx->d_q_chol.ensure(ctx, (size_t)C * QTL_CHOL));
    RC_TRY(b.keep.ensure(ctx, (size_t)M));
    if constexpr (em) {
        RC_TRY(ctx->d_q_null.ensure(ctx, (size_t)C * (ds.nx + 1) * rt));
        RC_TRY(ctx->d_qe_rss0_null.ensure(ctx, TC));
    } else {
        RC_TRY(b.scan.ensure(ctx, (size_t)C));
        RC_TRY(b.null.ensure(ctx, (size_t)C * s.nullq * rt));
    }
    RC_TRY(reserve(plan));
    if (a.P > 0) RC_TRY(b.tilemax.ensure(ctx, n_tiles * s.nfit * rt));
    RC_TRY(qtl_stage_outputs(ctx, dev, outputs));
    RC_TRY(qtl_origin_stage(ctx, org));
    RC_TRY(qtl_upload(ctx, b.map, map.image.data(), map.image.size()));
    RC_TRY(qtl_upload_inputs(ctx, a, mask));

    g.M = M, g.C = C, g.P = a.P, g.K = a.K, g.nx = ds.nx;
    g.origin = org.dev, g.cov = ctx->d_q_cov;
    g.cs = b.map, g.mchrom = b.map + map.o_mchrom;
    g.cmask = ctx->d_q_cmask, g.chol = ctx->d_q_chol;
    q.n = a.n, q.M = M, q.C = C, q.T = a.T, q.P = a.P, q.K = a.K;
    q.additive = (flags & CNF2_QTL_ADDITIVE) ? 1 : 0, q.imprint = (flags & CNF2_QTL_IMPRINT) ? 1 : 0;
    q.max_iter = max_iter, q.tol = tol;
    q.origin = org.dev, q.cov = ctx->d_q_cov, q.cs = g.cs, q.mchrom = g.mchrom;
    q.tiles = b.map + map.o_tiles, q.tile_start = b.map + map.o_tstart, q.n_tiles = (int)n_tiles;
    q.cmask = ctx->d_q_cmask, q.nc = g.nc, q.keep = b.keep;
    q.Y = s.image ? ctx->d_q_Y.ptr : nullptr, q.tilemax = b.tilemax, q.rstride = (int)rt;
    if constexpr (em) {
        g.nullq = ctx->d_q_null, g.rss0 = ctx->d_qe_rss0_null;
        q.chol = ctx->d_q_chol, q.nullq = ctx->d_q_null;
    } else {
        q.scan = b.scan, q.nullq = b.null;
        HIP_TRY(ctx, hipMemsetAsync(b.scan.ptr, 0, (size_t)C * sizeof(int32_t), ctx->stream));     // (a chromosome without markers has no thread to say so)
    }

    launch_qtl_chrom(g, ctx->stream);
    start();
    for (size_t r0 = 0; r0 < R; r0 += rt) {
        q.r0 = g.r0 = (int)r0;
        q.rn = g.rn = (int)std::min(rt, R - r0);
        if (s.image) launch_qtl_gather(g, ctx->stream);
        if constexpr (em) launch_qtl_null(g, ctx->stream);
        RC_TRY(tile(r0 + q.rn > (size_t)a.T));
    }
    HIP_TRY(ctx, hipGetLastError());
    return qtl_fetch_outputs(ctx, dev, outputs);
}

// The maximum-likelihood scan: cnf2_qtlem.h, cnf2_qtlem_kernels.hip.  Traits and covariates are centred as in the single scan.
int cnf2_qtl_scan_em(cnf2_ctx* ctx, int n, const double* origin, int n_traits, const double* pheno, const uint8_t* use, int n_cov,
                     const double* cov, int n_perm, const int32_t* perm, int max_iter, double tol, double* lod_out,
                     double* coef_out, double* sigma2_out, int32_t* iters_out, int32_t* status_out, int32_t* rank_out,
                     double* rss0_out, int32_t* n_used_out, double* perm_max_out, uint32_t flags)
{
    if (!ctx) return CNF2_ERR_ARG;
    const QtlArgs args = {n, n_traits, n_cov, n_perm, pheno, use, cov, perm, lod_out, coef_out, rss0_out, perm_max_out, rank_out, n_used_out};
    QtlemParams   q;
    memset(&q, 0, sizeof(q));
    return qtl_fit_scan(
        ctx, {QTL_CAP_EM, QTLEM_TILE, 1, 0, true, true}, ctx->qe, n, origin, args, max_iter, tol, iters_out, status_out, flags, q,
        [&](QtlArgs& a, const std::vector<uint8_t>& mask, QtlCentred& centred) -> int {
            if (!sigma2_out || !iters_out || !status_out) return fail(ctx, CNF2_ERR_ARG, "an output pointer is NULL");
            RC_TRY(qtl_fit_check_iter(ctx, max_iter, QTLEM_MAX_ITER, tol));
            qtl_centre(a, mask, centred);
            return CNF2_OK;
        },
        [&](auto each, const QtlFitPlan& plan) -> int { return each(sigma2_out, ctx->d_qe_sigma2, plan.cells, &q.sigma2); },
        [&] { launch_qtlem_rank(q, ctx->stream); },
        [&](bool last) -> int {
            launch_qtlem_fit(q, ctx->stream);
            if (last) launch_qtlem_finish(q, ctx->stream);
            return CNF2_OK;
        });
}

// The binary-trait scan: cnf2_qtlbin.h, cnf2_qtlbin_kernels.hip.  The covariates are centred, rounded once; the 0/1 trait is not.
int cnf2_qtl_scan_binary(cnf2_ctx* ctx, int n, const double* origin, int n_traits, const double* pheno, const uint8_t* use, int n_cov,
                         const double* cov, int n_perm, const int32_t* perm, int max_iter, double tol, double* lod_out,
                         double* coef_out, int32_t* iters_out, int32_t* status_out, int32_t* rank_out, double* ll0_out,
                         int32_t* n_ones_out, int32_t* n_used_out, double* perm_max_out, uint32_t flags)
{
    if (!ctx) return CNF2_ERR_ARG;
    const QtlArgs args = {n, n_traits, n_cov, n_perm, pheno, use, cov, perm, lod_out, coef_out, ll0_out, perm_max_out, rank_out, n_used_out};
    QtlbinParams  q;
    memset(&q, 0, sizeof(q));
    return qtl_fit_scan(
        ctx, {QTL_CAP_BIN, QTLBIN_TILE, 1, QTLBIN_NULLQ, true, false}, ctx->qb, n, origin, args, max_iter, tol, iters_out, status_out,
        flags, q,
        [&](QtlArgs& a, const std::vector<uint8_t>& mask, QtlCentred& centred) -> int {
            if (!iters_out || !status_out || !n_ones_out) return fail(ctx, CNF2_ERR_ARG, "an output pointer is NULL");
            RC_TRY(qtl_fit_check_iter(ctx, max_iter, QTLBIN_MAX_ITER, tol));
            RC_TRY(qtl_fit_check_01(ctx, a, mask, a.pheno, "phenotype"));
            qtl_centre_once(a, mask, centred, false);
            return CNF2_OK;
        },
        [&](auto each, const QtlFitPlan&) -> int { return each(n_ones_out, ctx->d_qb_ones, (size_t)n_traits * ctx->n_chrom, &q.n_ones); },
        [&] { launch_qtlbin_rank(q, ctx->stream); },
        [&](bool last) -> int {
            launch_qtlbin_null(q, ctx->stream);
            launch_qtlbin_fit(q, ctx->stream);
            if (last) launch_qtlbin_finish(q, ctx->stream);
            return CNF2_OK;
        });
}

// The survival-trait scan: cnf2_qtlsurv.h, cnf2_qtlsurv_kernels.hip.  The rank rule and the maxima of the permuted columns are
// the binary scan's kernels.  No kernel reads a time (they are checked as the phenotypes: a used time must be finite): the
// host puts every column of a tile in risk order (qtlsurv_order, the permuted columns as permuted) and the kernels walk the
// order words, so there is no column image.  The covariates are centred as in the binary scan.
int cnf2_qtl_scan_surv(cnf2_ctx* ctx, int n, const double* origin, int n_traits, const double* time, const double* status,
                       const uint8_t* use, int n_cov, const double* cov, int n_perm, const int32_t* perm, int max_iter, double tol,
                       double* lod_out, double* coef_out, int32_t* iters_out, int32_t* status_out, int32_t* rank_out, double* ll0_out,
                       int32_t* n_events_out, int32_t* n_used_out, double* perm_max_out, uint32_t flags)
{
    if (!ctx) return CNF2_ERR_ARG;
    const QtlArgs args = {n, n_traits, n_cov, n_perm, time, use, cov, perm, lod_out, coef_out, ll0_out, perm_max_out, rank_out, n_used_out};
    QtlsurvParams p;
    memset(&p, 0, sizeof(p));
    QtlbinParams&         q = p.b;
    const int             C = ctx->n_chrom;
    const uint8_t*        used = nullptr;        // the expanded mask, once it is checked
    size_t                fit_blocks = 0, null_blocks = 0, n_tiles = 0;
    std::vector<uint32_t> ord;
    return qtl_fit_scan(
        ctx, {QTL_CAP_SURV, QTLBIN_TILE, 1, QTLBIN_NULLQ, false, false}, ctx->qs, n, origin, args, max_iter, tol, iters_out, status_out,
        flags, q,
        [&](QtlArgs& a, const std::vector<uint8_t>& mask, QtlCentred& centred) -> int {
            if (!status || !iters_out || !status_out || !n_events_out) return fail(ctx, CNF2_ERR_ARG, "status or an output pointer is NULL");
            if ((uint32_t)a.n > QTLSURV_IND) return fail(ctx, CNF2_ERR_ARG, "too many individuals");
            RC_TRY(qtl_fit_check_iter(ctx, max_iter, QTLSURV_MAX_ITER, tol));
            RC_TRY(qtl_fit_check_01(ctx, a, mask, status, "status"));
            qtl_centre_once(a, mask, centred, false);
            used = mask.data();
            return CNF2_OK;
        },
        [&](auto each, const QtlFitPlan&) -> int { return each(n_events_out, ctx->d_qs_events, (size_t)n_traits * C, &q.n_ones); },
        [&] { launch_qtlbin_rank(q, ctx->stream); },
        [&](bool last) -> int {
            for (int rr = 0; rr < q.rn; rr++) {
                const size_t gr = (size_t)q.r0 + rr, pq = gr / n_traits, t = gr % n_traits;
                qtlsurv_order(n, time + t, status + t, (size_t)n_traits, pq ? perm + (pq - 1) * (size_t)n : nullptr, used,
                              ord.data() + (size_t)rr * n);
            }
            RC_TRY(qtl_upload(ctx, ctx->d_qs_ord, ord.data(), (size_t)q.rn * n));       // (complete on return: the tile before has been read)
            p.fit_blocks  = (int)std::min(fit_blocks, n_tiles * (size_t)q.rn);
            p.null_blocks = (int)std::min(null_blocks, ((size_t)C * q.rn + QTLSURV_WAVES - 1) / QTLSURV_WAVES);
            launch_qtlsurv_null(p, ctx->stream);
            launch_qtlsurv_fit(p, ctx->stream);
            if (last) launch_qtlbin_finish(q, ctx->stream);
            return CNF2_OK;
        },
        [&](const QtlFitPlan& plan) -> int {
            // (the order words of a tile, 4 bytes each, stay under the column image's bound)
            // The blocks of a launch: as many as it has cells, at most the cap, and no more than keep the work rows under 256 MB
            const size_t cap = ctx->qtlsurv_blocks > 0 ? (size_t)ctx->qtlsurv_blocks : 1024;
            n_tiles     = plan.n_tiles;
            fit_blocks  = std::max<size_t>(1, std::min(std::min(cap, n_tiles * plan.rt), ((size_t)1 << 28) / (64 * (size_t)n)));
            null_blocks = std::max<size_t>(1, std::min(fit_blocks, ((size_t)C * plan.rt + QTLSURV_WAVES - 1) / QTLSURV_WAVES));
            ord.resize(plan.rt * (size_t)n);
            RC_TRY(ctx->d_qs_ord.ensure(ctx, plan.rt * (size_t)n));
            RC_TRY(ctx->d_qs_work.ensure(ctx, fit_blocks * QTLSURV_WAVES * 2 * (size_t)n));
            p.ord = ctx->d_qs_ord, p.work = ctx->d_qs_work;
            return CNF2_OK;
        });
}

// The variance-QTL scan: cnf2_qtlvar.h, cnf2_qtlvar_kernels.hip.  The rank rule is the binary scan's kernel.  The traits and the
// covariates are centred, rounded once.
int cnf2_qtl_scan_var(cnf2_ctx* ctx, int n, const double* origin, int n_traits, const double* pheno, const uint8_t* use, int n_cov,
                      const double* cov, int n_var, int n_perm, const int32_t* perm, int max_iter, double tol, double* lod_out,
                      double* coef_mean_out, double* coef_var_out, int32_t* iters_out, int32_t* status_out, int32_t* rank_out,
                      double* ll0_out, int32_t* n_used_out, double* perm_max_out, uint32_t flags)
{
    if (!ctx) return CNF2_ERR_ARG;
    const QtlArgs args = {n, n_traits, n_cov, n_perm, pheno, use, cov, perm, lod_out, coef_mean_out, ll0_out, perm_max_out, rank_out, n_used_out};
    QtlvarParams  p;
    memset(&p, 0, sizeof(p));
    p.n_var = n_var;
    return qtl_fit_scan(
        ctx, {QTL_CAP_VAR, QTLBIN_TILE, QTLVAR_NFIT, QTLVAR_NULLQ, true, true}, ctx->qv, n, origin, args, max_iter, tol, iters_out,
        status_out, flags, p.b,
        [&](QtlArgs& a, const std::vector<uint8_t>& mask, QtlCentred& centred) -> int {
            if (!coef_var_out || !iters_out || !status_out) return fail(ctx, CNF2_ERR_ARG, "an output pointer is NULL");
            if (n_var < 0 || n_var > std::min(a.K, QTLVAR_MAXV))
                return fail(ctx, CNF2_ERR_ARG, "n_var must be 0 .. min(n_cov, %d)", QTLVAR_MAXV);
            RC_TRY(qtl_fit_check_iter(ctx, max_iter, QTLVAR_MAX_ITER, tol));
            qtl_centre_once(a, mask, centred, true);
            return CNF2_OK;
        },
        [&](auto each, const QtlFitPlan& plan) -> int { return each(coef_var_out, ctx->d_qv_coefv, plan.cells * plan.ne, &p.coef_var); },
        [&] {
            launch_qtlbin_rank(p.b, ctx->stream);
            launch_qtlvar_threshold(p, ctx->stream);
        },
        [&](bool last) -> int {
            launch_qtlvar_null(p, ctx->stream);
            launch_qtlvar_fit(p, ctx->stream);
            if (last) launch_qtlvar_finish(p, ctx->stream);
            return CNF2_OK;
        });
}

// one pass of sweep_impl's Viterbi mode
int cnf2_sweep_viterbi(cnf2_ctx* ctx, int ind_begin, int ind_end, double* factors_out, double* loglik_out, double* logmax_out,
                       uint8_t* state_out, int32_t* shift_out, uint32_t flags)
{
    RC_TRY(ready(ctx));
    if (!logmax_out || !state_out || !shift_out) return fail(ctx, CNF2_ERR_ARG, "logmax_out, state_out and shift_out must not be NULL");
    RC_TRY(mode_range(ctx, ind_begin, ind_end));
    const bool   dev = (flags & CNF2_OUT_DEVICE) != 0;
    const size_t n   = (size_t)(ind_end - ind_begin);
    if (n == 0) return CNF2_OK;
    const size_t nlm = n * ctx->n_chrom * 8, nst = n * ctx->n_markers, nsh = n * ctx->n_chrom;
    SweepMode    m;
    m.variant = SW_VITERBI;
    RC_TRY(stage_out(ctx, dev, logmax_out, ctx->d_vit_lm, nlm, &m.logmax));
    RC_TRY(stage_out(ctx, dev, state_out, ctx->d_vit_st, nst, &m.state));
    RC_TRY(stage_out(ctx, dev, shift_out, ctx->d_vit_sh, nsh, &m.shift));
    RC_TRY(mode_sweep(ctx, ind_begin, ind_end, factors_out, loglik_out, flags, m));
    if (dev) return CNF2_OK;
    RC_TRY(fetch_out(ctx, logmax_out, m.logmax, nlm));
    RC_TRY(fetch_out(ctx, state_out, m.state, nst));
    RC_TRY(fetch_out(ctx, shift_out, m.shift, nsh));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    return CNF2_OK;
}

// one pass of sweep_impl's sampling mode
int cnf2_sweep_sample(cnf2_ctx* ctx, int ind_begin, int ind_end, int n_draws, uint64_t seed, double* factors_out,
                      double* loglik_out, uint8_t* state_out, int32_t* shift_out, double* logp_out, uint32_t flags)
{
    RC_TRY(ready(ctx));
    if (n_draws < 1 || n_draws > 1024) return fail(ctx, CNF2_ERR_ARG, "n_draws must be in 1 .. 1024, not %d", n_draws);
    if (!state_out || !shift_out) return fail(ctx, CNF2_ERR_ARG, "state_out and shift_out must not be NULL");
    RC_TRY(mode_range(ctx, ind_begin, ind_end));
    const bool   dev = (flags & CNF2_OUT_DEVICE) != 0;
    const size_t nd  = (size_t)(ind_end - ind_begin) * n_draws;
    if (nd == 0) return CNF2_OK;
    const size_t nst = nd * ctx->n_markers, nsh = nd * ctx->n_chrom;
    SweepMode    m;
    m.variant = SW_SAMPLING;
    m.draws   = n_draws;
    m.seed    = (unsigned long long)seed;
    // host outputs are staged whole (callers with many draws split the individual range: the draws do not change)
    RC_TRY(stage_out(ctx, dev, state_out, ctx->d_smp_st, nst, &m.state));
    RC_TRY(stage_out(ctx, dev, shift_out, ctx->d_smp_sh, nsh, &m.shift));
    RC_TRY(stage_out(ctx, dev, logp_out, ctx->d_smp_lp, nsh, &m.logp));
    RC_TRY(mode_sweep(ctx, ind_begin, ind_end, factors_out, loglik_out, flags, m));
    if (dev) return CNF2_OK;
    RC_TRY(fetch_out(ctx, state_out, m.state, nst));
    RC_TRY(fetch_out(ctx, shift_out, m.shift, nsh));
    RC_TRY(fetch_out(ctx, logp_out, m.logp, nsh));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    return CNF2_OK;
}

int cnf2_haplos(cnf2_ctx* ctx, int ind, int chrom, double* rows_out, uint32_t flags)
{
    if (!ctx || !rows_out) return fail(ctx, CNF2_ERR_ARG, "bad haplos arguments");
    const uint32_t kp = (flags & CNF2_NO_TIES) ? KP_NO_TIES : 0;
    return stage2_rows(ctx, ind, chrom, 14, rows_out,
                       [&](const Stage2Params& q, double* d_out) { launch_haplos_rows(q, kp, d_out, ctx->stream); });
}

int cnf2_infprobs(cnf2_ctx* ctx, int ind, int chrom, int marker, double* inf_out, double* hz_out, uint32_t flags)
{
    if (!ctx || !inf_out || !hz_out) return fail(ctx, CNF2_ERR_ARG, "bad infprobs arguments");
    Stage2Params q;
    double*      d_out = nullptr;
    RC_TRY(ready(ctx));
    if (chrom < 0 || chrom >= ctx->n_chrom) return fail(ctx, CNF2_ERR_ARG, "chromosome out of range");
    if (marker < ctx->chromstarts[chrom] || marker >= ctx->chromstarts[chrom + 1])
        return fail(ctx, CNF2_ERR_ARG, "marker not on the chromosome");
    RC_TRY(run_store(ctx, ind, chrom, &q, 32, &d_out));
    launch_infprobs(q, marker, (flags & CNF2_NO_TIES) ? KP_NO_TIES : 0, d_out, ctx->stream);
    HIP_TRY(ctx, hipGetLastError());
    double h[30];
    HIP_TRY(ctx, hipMemcpyAsync(h, d_out, 30 * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    for (int k = 0; k < 28; k++) inf_out[k] = h[k];
    hz_out[0] = h[28];
    hz_out[1] = h[29];
    return CNF2_OK;
}

int cnf2_infprobs_rows(cnf2_ctx* ctx, int ind, int chrom, double* rows_out, uint32_t flags)
{
    if (!ctx || !rows_out) return fail(ctx, CNF2_ERR_ARG, "bad infprobs_rows arguments");
    const uint32_t kp = (flags & CNF2_NO_TIES) ? KP_NO_TIES : 0;
    return stage2_rows(ctx, ind, chrom, 30, rows_out,
                       [&](const Stage2Params& q, double* d_out) { launch_infprobs_rows(q, kp, d_out, ctx->stream); });
}

int cnf2_descendants(cnf2_ctx* ctx, int32_t* desc_out)
{
    if (!ctx || !desc_out) return fail(ctx, CNF2_ERR_ARG, "bad descendants arguments");
    if (ctx->ped.n_rec == 0) return fail(ctx, CNF2_ERR_STATE, "no pedigree uploaded");
    derive_descendants(ctx->ped, desc_out);
    return CNF2_OK;
}

// Entries of the list the update scouts set flows aside on: a chunk of the pass's flows, at most 2^26
static size_t todo_chunk(size_t n_rec, size_t chrom_len, size_t markers_upto)
{
    const size_t n1 = n_rec * chrom_len * 4, n3 = n_rec * markers_upto;
    size_t       want = n1 > n3 ? n1 : n3;
    if (want < 4096) want = 4096;
    const size_t cap = (size_t)1 << 26;        // x 48 B for the two lists: 3.2 GB
    return want < cap ? want : cap;
}

// ... in doubles: two lists of 24-byte entries (the scouts' and the packed one of the guided kernel; a third for the experiment with
// a second lock-step kernel) and the packing's counts
#ifdef CNF2_X_GUIDED_ROUNDS
#define TODO_LISTS 3
#else
#define TODO_LISTS 2
#endif
static size_t todo_doubles(size_t chunk) { return chunk * 3 * TODO_LISTS + chunk / 256 + 8; }

// row_doubles: doubles of the batch buffer per job and marker; part_need: doubles the caller allocates for itself between
// the spill and the batch buffer.  Leaves plan.fit to the caller where it is BATCH_NO_PART or BATCH_NO_ROWS.
static int batched_setup(cnf2_ctx* ctx, int ind_begin, int n, uint32_t flags, size_t row_doubles, size_t part_need, Batched* b)
{
    b->list = job_plan(ctx, ind_begin, n, flags & CNF2_NO_TIES);
    const std::vector<Job>& jobs = b->list.jobs;
    ctx->plan_valid = false;           // (d_jobs no longer holds the last sweep's list)
    RC_TRY(ctx->d_jobs.ensure(ctx, jobs.size() + 1));
    HIP_TRY(ctx, hipMemcpy(ctx->d_jobs, jobs.data(), sizeof(Job) * jobs.size(), hipMemcpyHostToDevice));
    b->max_len = longest_chrom(ctx);
    size_t free_b = 0, total_b = 0;
    HIP_TRY(ctx, hipMemGetInfo(&free_b, &total_b));
    const size_t held_b = (ctx->d_spill.cap + ctx->d_wbuf.cap) * sizeof(double);
    b->plan = plan_batches(ctx->n_cu, ctx->fast_blocks_per_cu, ctx->reserve_blocks, free_b, held_b, b->max_len, row_doubles, jobs.size(), ctx->batch_jobs, part_need, ctx->d_part.cap);
    if (b->plan.fit == BATCH_NO_SPILL) return fail(ctx, CNF2_ERR_NOMEM, "not enough memory for the spill of one block");
    return ctx->d_spill.ensure(ctx, (size_t)b->plan.grid_cap * CNF2_WAVES_PER_BLOCK * spill_stride(b->max_len));
}

enum : uint32_t { ACC_RESERVE_ONLY = 1u << 31 };     // internal flag of cnf2_sweep_accumulate (not in the header)
// internal flags of cnf2_sweep_place (not in the header; A/B of its two routes to the likelihoods, see there)
enum : uint32_t { PLACE_SWEEP_LIKELIHOODS = 1u << 30, PLACE_OWN_LIKELIHOODS = 1u << 29 };

// Batched HOT LOOP 2 with its reductions (cnF2freq.cpp:5416-5577, 5876-5902 with moveinfprobs / movehaplos
// 3577-3616) for the analysed individuals [ind_begin, ind_end): the sweep kernels run in their accumulate
// instantiation (they leave the posterior weights wg(s, g) of every marker in a batch buffer next to the usual
// outputs), acc_rows_kernel turns them into the per-record accumulators on the device.  Jobs go in batches sized
// to the memory that is free (4 KB per individual x marker of weights).
int cnf2_sweep_accumulate(cnf2_ctx* ctx, int ind_begin, int ind_end, const int32_t* descendants, double* factors_out,
                          double* loglik_out, double* dosage_out, double* infprobs, double* haplobase,
                          double* haplocount, double* homozyg, uint32_t flags)
{
    RC_TRY(ready(ctx));
    const int n_all = (int)ctx->windows.size();
    const bool out_dev = (flags & CNF2_OUT_DEVICE) != 0, acc_dev = (flags & CNF2_ACC_DEVICE) != 0;
    const bool acc_given = infprobs && haplobase && haplocount && homozyg;
    const bool acc_none = !infprobs && !haplobase && !haplocount && !homozyg;    // keep them in the context
    const bool reserve_only = (flags & ACC_RESERVE_ONLY) != 0;      // cnf2_reserve_accumulate: allocations only
    if ((!descendants && !reserve_only) || (!acc_given && !(acc_none && !acc_dev)) || ind_begin < 0 || ind_end > n_all || ind_begin > ind_end)
        return fail(ctx, CNF2_ERR_ARG, "bad accumulate arguments");
    if (out_dev && (!factors_out || !loglik_out || !dosage_out)) return fail(ctx, CNF2_ERR_ARG, "output pointer is NULL");
    const HostPedigree& P = ctx->ped;
    const int    n = ind_end - ind_begin;
    const size_t M = (size_t)ctx->n_markers, R = (size_t)P.n_rec;
    HIP_TRY(ctx, hipSetDevice(ctx->device));

    // per-record tables
    RC_TRY(ensure_rec_tables(ctx, R));
    if (descendants) HIP_TRY(ctx, hipMemcpy(ctx->d_desc, descendants, sizeof(int32_t) * R, hipMemcpyHostToDevice));
    HIP_TRY(ctx, hipMemcpy(ctx->d_rec_empty, P.empty.data(), R, hipMemcpyHostToDevice));

    // accumulators and sweep outputs
    double *a_inf = infprobs, *a_hb = haplobase, *a_hc = haplocount, *a_hz = homozyg;
    if (!acc_dev) {
        RC_TRY(ctx->d_acc_inf.ensure(ctx, R * M * 4));
        RC_TRY(ctx->d_acc_hb.ensure(ctx, R * M));
        RC_TRY(ctx->d_acc_hc.ensure(ctx, R * M));
        RC_TRY(ctx->d_acc_hz.ensure(ctx, (size_t)(n > 0 ? n : 1) * M * 2));
        a_inf = ctx->d_acc_inf;
        a_hb  = ctx->d_acc_hb;
        a_hc  = ctx->d_acc_hc;
        a_hz  = ctx->d_acc_hz;
    }
    if (!(flags & CNF2_ACC_KEEP)) {
        HIP_TRY(ctx, hipMemsetAsync(a_inf, 0, R * M * 4 * sizeof(double), ctx->stream));
        HIP_TRY(ctx, hipMemsetAsync(a_hb, 0, R * M * sizeof(double), ctx->stream));
        HIP_TRY(ctx, hipMemsetAsync(a_hc, 0, R * M * sizeof(double), ctx->stream));
    }
    HIP_TRY(ctx, hipMemsetAsync(a_hz, 0, (size_t)n * M * 2 * sizeof(double), ctx->stream));
    const size_t nf = (size_t)n * ctx->n_chrom * 8, nl = (size_t)n * ctx->n_chrom, nd = (size_t)n * M * 3;
    double *d_f = factors_out, *d_l = loglik_out, *d_d = dosage_out;
    if (!out_dev) {
        RC_TRY(ctx->d_factors.ensure(ctx, nf ? nf : 1));
        RC_TRY(ctx->d_loglik.ensure(ctx, nl ? nl : 1));
        RC_TRY(ctx->d_dosage.ensure(ctx, nd ? nd : 1));
        d_f = ctx->d_factors;
        d_l = ctx->d_loglik;
        d_d = ctx->d_dosage;
    }
    // A caller that passes no dosage pointer gets no per-locus rows (an iteration that prints none: all but the last of a
    // run): the sweep then runs in the instantiation that forms none -- no class sums, no restricted tables, no tile
    // epilogue -- and, since the posterior weights do not see the tie rule, the sweep of the windows with tie groups takes it
    // as well (their accumulators do see the rule: they stay a pass of their own).
    const bool want_rows = dosage_out != nullptr;
    if (n > 0) {
        // CNF2_DETERMINISTIC: the per-individual rows (336 B per individual x marker) are taken out of what is free BEFORE the
        // batch buffer is sized -- and allocated now, also by cnf2_reserve_accumulate -- so that the batch buffer cannot
        // leave them without memory
        const size_t part_need = (flags & CNF2_DETERMINISTIC) ? (size_t)n * M * 42 : 0;
        Batched      b;
        RC_TRY(batched_setup(ctx, ind_begin, n, flags, 512, part_need, &b));     // weights: 512 doubles per (job, marker)
        if (b.plan.fit == BATCH_NO_PART)
            return fail(ctx, CNF2_ERR_NOMEM, "CNF2_DETERMINISTIC needs %zu MB for the per-individual rows", (part_need * 8) >> 20);
        if (part_need) RC_TRY(ctx->d_part.ensure(ctx, part_need));
        const int    mlen = b.max_len;
        const size_t stride = spill_stride(mlen), per_job = (size_t)mlen * 512, batch = b.plan.batch;
        if (b.plan.fit == BATCH_NO_ROWS)
            return fail(ctx, CNF2_ERR_NOMEM, "not enough memory for the weights of one job (%zu MB)", per_job >> 17);
        {
            // CNF2_TIMING: the first call of a run allocates the batch buffer (up to half the free memory) -- seconds
            const bool timing = getenv("CNF2_TIMING") != nullptr && ctx->d_wbuf.cap < batch * per_job;
            const auto t0 = std::chrono::steady_clock::now();
            RC_TRY(ctx->d_wbuf.ensure(ctx, batch * per_job));
            if (timing)
                fprintf(stderr, "  [sweep_accumulate] batch buffer of %.1f GB allocated in %.3f s (%zu jobs per batch of %zu)\n",
                        batch * per_job * 8 / 1e9, std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count(), batch,
                        b.list.jobs.size());
        }
        if (reserve_only) {
            // ... and the buffers of the update passes (cnf2_update_pass): results of a chromosome's flows, the scouts' list
            RC_TRY(ctx->d_flow_next.ensure(ctx, 32));
            RC_TRY(ctx->d_flow_out.ensure(ctx, R * (size_t)mlen * 4));
            RC_TRY(ctx->d_todo.ensure(ctx, todo_doubles(todo_chunk(R, (size_t)mlen, M))));
            HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
            return CNF2_OK;
        }

        KernelParams p;
        base_params(ctx, &p);
        if (flags & CNF2_STATIC_JOBS) p.job_next = nullptr;
        p.windows      = ctx->d_windows + ind_begin;
        p.spill        = ctx->d_spill;
        p.spill_stride = stride;
        p.factors      = d_f;
        p.loglik       = d_l;
        p.dosage       = d_d;
        p.flags        = ((flags & CNF2_RAW_DOSAGE) ? KP_RAW_DOSAGE : 0) | ((flags & CNF2_NO_TIES) ? KP_NO_TIES : 0);
        p.wbuf         = ctx->d_wbuf;
        p.wstride      = (size_t)mlen;
        AccParams q;
        memset(&q, 0, sizeof(q));
        q.flags     = ((flags & CNF2_NO_TIES) ? KP_NO_TIES : 0) | ((flags & CNF2_ACC_TABLE) ? KP_ACC_TABLE : 0);
        for (int j = 0; j < n; j++)
            if (ctx->windows[ind_begin + j].flags[0] & SLOT_FOUNDER) q.flags |= KP_ACC_ATTOP;
        q.slot_rec  = ctx->d_slot_rec + (size_t)ind_begin * 7;
        q.desc      = ctx->d_desc;
        q.rec_empty = ctx->d_rec_empty;
        q.acc_inf   = a_inf;
        q.acc_hb    = a_hb;
        q.acc_hc    = a_hc;
        q.acc_hz    = a_hz;
        q.max_len   = mlen;
        std::vector<int32_t> gather;               // CNF2_DETERMINISTIC: rec_start[R + 1], then ind * 8 + slot per record
        if (flags & CNF2_DETERMINISTIC) {
            const size_t need = part_need;                    // allocated above, before the batch buffer was sized
            HIP_TRY(ctx, hipMemsetAsync(ctx->d_part, 0, need * sizeof(double), ctx->stream));
            q.part = ctx->d_part;
            std::vector<int32_t> count(R + 1, 0);
            auto first_slots = [&](int j, auto&& f) {         // the slots that emit: first occurrence of their record
                const int32_t* sr = &ctx->slot_rec[(size_t)(ind_begin + j) * 7];
                for (int k = 0; k < 7; k++) {
                    if (sr[k] < 0) continue;
                    bool first = true;
                    for (int k2 = 0; k2 < k; k2++) first = first && sr[k2] != sr[k];
                    if (first) f(sr[k], k);
                }
            };
            for (int j = 0; j < n; j++) first_slots(j, [&](int r, int) { count[r + 1]++; });
            for (size_t r = 0; r < R; r++) count[r + 1] += count[r];
            gather.assign(R + 1 + (size_t)count[R], 0);
            std::copy(count.begin(), count.end(), gather.begin());
            std::vector<int32_t> fill(count.begin(), count.end() - 1);
            for (int j = 0; j < n; j++) first_slots(j, [&](int r, int k) { gather[R + 1 + fill[r]++] = j * 8 + k; });
            RC_TRY(ctx->d_gather.ensure(ctx, gather.size()));
            HIP_TRY(ctx, hipMemcpyAsync(ctx->d_gather, gather.data(), gather.size() * sizeof(int32_t), hipMemcpyHostToDevice, ctx->stream));
        }
        HIP_TRY(ctx, hipEventRecord(ctx->ev0, ctx->stream));
        RC_TRY(for_each_batch(ctx, b, &p, [&](int pass, int grid, int max_len) -> int {
            // tied windows: the general kernel where asked for; without rows the untied instantiation; else the tied one
            const FastVariant v = {want_rows ? SW_WEIGHTS_ROWS : SW_WEIGHTS, true, false, pass == 1 && want_rows};
            if (pass == 1 && (flags & CNF2_TIES_GENERAL)) HIP_TRY(ctx, launch_fb(p, grid, SW_WEIGHTS_ROWS, ctx->stream));
            else HIP_TRY(ctx, launch_fb_fast(p, grid, v, ctx->stream));
            q.kp      = p;
            q.n_jobs  = p.n_jobs;
            q.max_len = max_len;
            q.flags   = (q.flags & ~(uint32_t)KP_ACC_LANES) | ((pass == 1 || (flags & CNF2_ACC_LANES)) ? KP_ACC_LANES : 0);
            launch_acc_rows(q, ctx->stream);
            HIP_TRY(ctx, hipGetLastError());
            return CNF2_OK;
        }));
        if (q.part) {
            launch_acc_gather(q, ctx->d_gather, ctx->d_gather + R + 1, (int)R, ctx->stream);
            HIP_TRY(ctx, hipGetLastError());
            HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));     // `gather` (host staging of the lists) goes out of scope
        }
        HIP_TRY(ctx, hipEventRecord(ctx->ev1, ctx->stream));
        ctx->timed = true;
    }
    if (!out_dev) {
        if (factors_out) HIP_TRY(ctx, hipMemcpyAsync(factors_out, d_f, nf * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
        if (loglik_out) HIP_TRY(ctx, hipMemcpyAsync(loglik_out, d_l, nl * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
        if (dosage_out) HIP_TRY(ctx, hipMemcpyAsync(dosage_out, d_d, nd * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    }
    if (!acc_dev && acc_given) {
        HIP_TRY(ctx, hipMemcpyAsync(infprobs, a_inf, R * M * 4 * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
        HIP_TRY(ctx, hipMemcpyAsync(haplobase, a_hb, R * M * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
        HIP_TRY(ctx, hipMemcpyAsync(haplocount, a_hc, R * M * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
        HIP_TRY(ctx, hipMemcpyAsync(homozyg, a_hz, (size_t)n * M * 2 * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    }
    if (!out_dev || !acc_dev) HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    return CNF2_OK;
}

// The allocations of cnf2_sweep_accumulate for [ind_begin, ind_end) without the sweep: accumulators, outputs, spill and the
// batch buffer of posterior weights (up to half of the free memory: a first hipMalloc of that size takes seconds on a
// fresh device, 4.3 s for 125 GB measured).  A run calls this once after its uploads, so that its first iteration costs
// what the others cost.
int cnf2_reserve_accumulate(cnf2_ctx* ctx, int ind_begin, int ind_end, uint32_t flags)
{
    const uint32_t keep = flags & (CNF2_NO_TIES | CNF2_DETERMINISTIC | CNF2_TIES_GENERAL);
    return cnf2_sweep_accumulate(ctx, ind_begin, ind_end, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr,
                                 keep | ACC_RESERVE_ONLY);
}

// Batched turn scan (HOT LOOP 3, cnF2freq.cpp:5686-5752) for the analysed individuals [ind_begin, ind_end): the sweep
// kernels run in their turn-scan instantiation (alpha after emission and beta of every marker, with scales, into a
// batch buffer), turn_rows_kernel forms rawervals[turn][s] for all 128 turns and 8 shift modes of every marker.
int cnf2_sweep_turn_scan(cnf2_ctx* ctx, int ind_begin, int ind_end, double* rawervals_out, double* turn_lse_out,
                         uint32_t flags)
{
    RC_TRY(ready(ctx));
    const int n_all = (int)ctx->windows.size();
    if ((!rawervals_out && !turn_lse_out) || ind_begin < 0 || ind_end > n_all || ind_begin > ind_end)
        return fail(ctx, CNF2_ERR_ARG, "bad turn scan arguments");
    const bool out_dev = (flags & CNF2_OUT_DEVICE) != 0;
    const int    n = ind_end - ind_begin;
    const size_t M = (size_t)ctx->n_markers;
    if (n == 0) return CNF2_OK;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    const size_t nf = (size_t)n * ctx->n_chrom * 8, nl = (size_t)n * ctx->n_chrom, nd = (size_t)n * M * 3;
    RC_TRY(ctx->d_factors.ensure(ctx, nf));
    RC_TRY(ctx->d_loglik.ensure(ctx, nl));
    RC_TRY(ctx->d_dosage.ensure(ctx, nd));
    double *d_full = rawervals_out, *d_lse = turn_lse_out;
    if (!out_dev) {
        // staging for the whole range: 9 KB per individual x marker -- callers with large ranges use device buffers
        d_full = d_lse = nullptr;
        const size_t need = (rawervals_out ? (size_t)n * M * 1024 : 0) + (turn_lse_out ? (size_t)n * M * 128 : 0);
        RC_TRY(ctx->d_scratch.ensure(ctx, need));
        double* q0 = ctx->d_scratch;
        if (rawervals_out) {
            d_full = q0;
            q0 += (size_t)n * M * 1024;
        }
        if (turn_lse_out) d_lse = q0;
    }
    Batched b;
    RC_TRY(batched_setup(ctx, ind_begin, n, flags, CNF2_TURN_ROW, 0, &b));
    if (b.plan.fit == BATCH_NO_ROWS) return fail(ctx, CNF2_ERR_NOMEM, "not enough memory for the alpha/beta rows of one job");
    const int mlen = b.max_len;
    RC_TRY(ctx->d_wbuf.ensure(ctx, b.plan.batch * (size_t)mlen * CNF2_TURN_ROW));
    KernelParams p;
    base_params(ctx, &p);
    if (flags & CNF2_STATIC_JOBS) p.job_next = nullptr;
    p.windows      = ctx->d_windows + ind_begin;
    p.spill        = ctx->d_spill;
    p.spill_stride = spill_stride(mlen);
    p.factors      = ctx->d_factors;
    p.loglik       = ctx->d_loglik;
    p.dosage       = ctx->d_dosage;
    p.flags        = (flags & CNF2_NO_TIES) ? KP_NO_TIES : 0;
    p.wbuf         = ctx->d_wbuf;
    p.wstride      = (size_t)mlen;
    TurnParams q;
    memset(&q, 0, sizeof(q));
    q.max_len   = mlen;
    q.rawervals = d_full;
    q.turn_lse  = d_lse;
    q.valu_form = (flags & CNF2_TURN_VALU) ? 1 : 0;
    HIP_TRY(ctx, hipEventRecord(ctx->ev0, ctx->stream));
    RC_TRY(for_each_batch(ctx, b, &p, [&](int pass, int grid, int max_len) -> int {
        // alpha and beta do not see the tie rule: tied windows take the tile-producer kernel too (its rows, which
        // would need the rule, go to the context's scratch and are not an output of this call)
        const bool fast = pass == 0 || !(flags & CNF2_TIES_GENERAL);
        if (fast) HIP_TRY(ctx, launch_fb_fast(p, grid, {SW_ALPHA_BETA}, ctx->stream));
        else HIP_TRY(ctx, launch_fb(p, grid, SW_ALPHA_BETA, ctx->stream));
        q.kp      = p;
        q.n_jobs  = p.n_jobs;
        q.max_len = max_len;
        q.scaled_transitions = fast;
        launch_turn_rows(q, ctx->stream);
        HIP_TRY(ctx, hipGetLastError());
        return CNF2_OK;
    }));
    HIP_TRY(ctx, hipEventRecord(ctx->ev1, ctx->stream));
    ctx->timed = true;
    if (!out_dev) {
        if (rawervals_out) HIP_TRY(ctx, hipMemcpyAsync(rawervals_out, d_full, (size_t)n * M * 1024 * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
        if (turn_lse_out) HIP_TRY(ctx, hipMemcpyAsync(turn_lse_out, d_lse, (size_t)n * M * 128 * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
        HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    }
    return CNF2_OK;
}

// The pairs of a selection that lie on one chromosome, in the order of cnf2_sweep_pairs' rows
int cnf2_linked_pairs(cnf2_ctx* ctx, int n_sel, const int32_t* sel, int32_t* pairs_out, int32_t* n_pairs_out)
{
    RC_TRY(ready(ctx));
    if (!n_pairs_out) return fail(ctx, CNF2_ERR_ARG, "n_pairs_out must not be NULL");
    PairSel ps;
    RC_TRY(pair_selection(ctx, n_sel, sel, &ps));
    if (pairs_out)
        for (int c = 0; c < ctx->n_chrom; c++)
            for (int j = ps.chrom_sel[c]; j < ps.chrom_sel[c + 1]; j++)
                for (int k = j + 1; k < ps.chrom_sel[c + 1]; k++) {
                    int32_t* o = pairs_out + (size_t)(ps.pair_off[j] + k - j - 1) * 2;
                    o[0] = j;
                    o[1] = k;
                }
    *n_pairs_out = ps.n_pairs;
    return CNF2_OK;
}

// Pair posteriors of the analysed individuals [ind_begin, ind_end): in batches, the sweep kernels in their turn-scan
// instantiation (alpha after the emission and beta of every marker into the batch buffer), then pair_sweep_kernel on the
// batch; the column sums by origin_finish_kernel.  The rows the caller gave no device memory for live whole in the context.
int cnf2_sweep_pairs(cnf2_ctx* ctx, int ind_begin, int ind_end, int n_sel, const int32_t* sel, double* factors_out,
                     double* loglik_out, double* joint_out, double* joint_sum_out, int32_t* n_contrib_out, uint32_t flags)
{
    RC_TRY(ready(ctx));
    if (!factors_out || !loglik_out || !joint_sum_out || !n_contrib_out)
        return fail(ctx, CNF2_ERR_ARG, "only joint_out may be NULL");
    RC_TRY(mode_range(ctx, ind_begin, ind_end));
    PairSel ps;
    RC_TRY(pair_selection(ctx, n_sel, sel, &ps));
    if (ps.n_pairs == 0) return fail(ctx, CNF2_ERR_ARG, "no two selected markers share a chromosome");
    const bool   dev = (flags & CNF2_OUT_DEVICE) != 0;
    const int    n = ind_end - ind_begin;
    const size_t M = (size_t)ctx->n_markers, C = (size_t)ctx->n_chrom, L = (size_t)n_sel, NP = (size_t)ps.n_pairs;
    const size_t nf = (size_t)n * C * 8, nl = (size_t)n * C, nr = (size_t)n * NP * 16;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    double *d_f, *d_l, *d_sum, *d_joint = (dev && joint_out) ? joint_out : nullptr;
    int32_t* d_cnt;
    if (!d_joint && nr > ctx->d_pair.cap) {
        size_t free_b = 0, total_b = 0;
        HIP_TRY(ctx, hipMemGetInfo(&free_b, &total_b));
        if (nr * sizeof(double) > free_b + ctx->d_pair.cap * sizeof(double))
            return fail(ctx, CNF2_ERR_NOMEM, "the pair rows of the range need %zu MB: split the range", (nr * 8) >> 20);
    }
    RC_TRY(stage_out(ctx, dev, factors_out, ctx->d_factors, nf ? nf : 1, &d_f));
    RC_TRY(stage_out(ctx, dev, loglik_out, ctx->d_loglik, nl ? nl : 1, &d_l));
    RC_TRY(stage_out(ctx, dev, joint_sum_out, ctx->d_pair_sum, NP * 16, &d_sum));
    RC_TRY(stage_out(ctx, dev, n_contrib_out, ctx->d_xo_cnt, C, &d_cnt));
    RC_TRY(ctx->d_dosage.ensure(ctx, (size_t)(n > 0 ? n : 1) * M * 3));
    if (!d_joint && nr > 0) {
        RC_TRY(ctx->d_pair.ensure(ctx, nr));
        d_joint = ctx->d_pair;
    }
    std::vector<int32_t> map(sel, sel + L);
    map.insert(map.end(), ps.chrom_sel.begin(), ps.chrom_sel.end());
    map.insert(map.end(), ps.pair_off.begin(), ps.pair_off.end());
    RC_TRY(ctx->d_pair_map.ensure(ctx, map.size()));
    HIP_TRY(ctx, hipMemcpy(ctx->d_pair_map, map.data(), map.size() * sizeof(int32_t), hipMemcpyHostToDevice));
    if (n > 0) {
        Batched b;
        RC_TRY(batched_setup(ctx, ind_begin, n, flags, CNF2_TURN_ROW, 0, &b));
        if (b.plan.fit == BATCH_NO_ROWS) return fail(ctx, CNF2_ERR_NOMEM, "not enough memory for the alpha/beta rows of one job");
        const int mlen = b.max_len;
        RC_TRY(ctx->d_wbuf.ensure(ctx, b.plan.batch * (size_t)mlen * CNF2_TURN_ROW));
        KernelParams p;
        base_params(ctx, &p);
        if (flags & CNF2_STATIC_JOBS) p.job_next = nullptr;
        p.windows      = ctx->d_windows + ind_begin;
        p.spill        = ctx->d_spill;
        p.spill_stride = spill_stride(mlen);
        p.factors      = d_f;
        p.loglik       = d_l;
        p.dosage       = ctx->d_dosage;
        p.flags        = 0;
        p.wbuf         = ctx->d_wbuf;
        p.wstride      = (size_t)mlen;
        PairParams q;
        memset(&q, 0, sizeof(q));
        q.max_anchors = ps.max_anchors;
        q.n_pairs     = ps.n_pairs;
        q.sel         = ctx->d_pair_map;
        q.chrom_sel   = ctx->d_pair_map + L;
        q.pair_off    = ctx->d_pair_map + L + C + 1;
        q.joint       = d_joint;
        HIP_TRY(ctx, hipMemsetAsync(d_joint, 0, nr * sizeof(double), ctx->stream));
        HIP_TRY(ctx, hipEventRecord(ctx->ev0, ctx->stream));
        RC_TRY(for_each_batch(ctx, b, &p, [&](int pass, int grid, int) -> int {
            // alpha and beta do not see the tie rule: tied windows take the tile-producer kernel too (cnf2_sweep_turn_scan)
            if (pass == 0 || !(flags & CNF2_TIES_GENERAL)) HIP_TRY(ctx, launch_fb_fast(p, grid, {SW_ALPHA_BETA}, ctx->stream));
            else HIP_TRY(ctx, launch_fb(p, grid, SW_ALPHA_BETA, ctx->stream));
            q.kp     = p;
            q.n_jobs = p.n_jobs;
            launch_pair_sweep(q, ctx->stream);
            HIP_TRY(ctx, hipGetLastError());
            return CNF2_OK;
        }));
    }
    launch_pair_count(d_f, d_l, n, (int)C, d_cnt, ctx->stream);
    if (n > 0) launch_origin_finish(d_joint, n, (int)(NP * 4), d_sum, ctx->stream);
    else HIP_TRY(ctx, hipMemsetAsync(d_sum, 0, NP * 16 * sizeof(double), ctx->stream));
    HIP_TRY(ctx, hipGetLastError());
    if (n > 0) {
        HIP_TRY(ctx, hipEventRecord(ctx->ev1, ctx->stream));
        ctx->timed = true;
    }
    if (dev) return CNF2_OK;
    RC_TRY(fetch_out(ctx, factors_out, d_f, nf));
    RC_TRY(fetch_out(ctx, loglik_out, d_l, nl));
    RC_TRY(fetch_out(ctx, joint_sum_out, d_sum, NP * 16));
    RC_TRY(fetch_out(ctx, n_contrib_out, d_cnt, C));
    if (joint_out && nr > 0) RC_TRY(fetch_out(ctx, joint_out, d_joint, nr));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    return CNF2_OK;
}

// The pair rows of one individual and chromosome from the reference-layout store, brute force: rows_out[S (S - 1) / 2][16] for
// the S markers of sel on the chromosome, pairs in ascending first, then ascending second locus (nothing where S < 2)
int cnf2_pair_rows(cnf2_ctx* ctx, int ind, int chrom, int n_sel, const int32_t* sel, double* rows_out)
{
    if (!ctx || !rows_out) return fail(ctx, CNF2_ERR_ARG, "bad pair_rows arguments");
    RC_TRY(ready(ctx));
    if (ind < 0 || ind >= (int)ctx->windows.size() || chrom < 0 || chrom >= ctx->n_chrom)
        return fail(ctx, CNF2_ERR_ARG, "individual or chromosome out of range");
    PairSel ps;
    RC_TRY(pair_selection(ctx, n_sel, sel, &ps));
    const int j0 = ps.chrom_sel[chrom], S = ps.chrom_sel[chrom + 1] - j0;
    if (S < 2) return CNF2_OK;
    std::vector<int32_t> local((size_t)S);
    for (int a = 0; a < S; a++) local[a] = sel[j0 + a] - ctx->chromstarts[chrom];
    const size_t nr = (size_t)S * (S - 1) / 2 * 16;
    Stage2Params q;
    double*      d_out = nullptr;
    RC_TRY(run_store(ctx, ind, chrom, &q, nr + (size_t)(S + 1) / 2, &d_out));
    int32_t* d_sel = (int32_t*)(d_out + nr);
    HIP_TRY(ctx, hipMemcpyAsync(d_sel, local.data(), sizeof(int32_t) * S, hipMemcpyHostToDevice, ctx->stream));
    launch_pair_rows(q, d_sel, S, d_out, ctx->stream);
    HIP_TRY(ctx, hipGetLastError());
    HIP_TRY(ctx, hipMemcpyAsync(rows_out, d_out, nr * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    return CNF2_OK;
}

// Candidates whose emission tables are held at once (a multiple of 16): more are processed in tiles over the same weights
#define CNF2_PLACE_TILE 256
// Whether a range without tied windows reports the placement instantiation's own likelihoods (one forward pass fewer)
#ifndef PLACE_OWN_DEFAULT
#define PLACE_OWN_DEFAULT true
#endif

// Marker placement: in batches, the placement sweep (the fast kernel's SW_POSTERIOR instantiation for every window: alpha
// and beta do not see the tie rule) and, per tile of candidates, place_rows_kernel over the batch's state posteriors.  The
// sweep runs once per batch, not once per tile.  The likelihoods: see below.
int cnf2_sweep_place(cnf2_ctx* ctx, int ind_begin, int ind_end, int n_cand, const uint8_t* cand_allele, const double* cand_sure,
                     const double* cand_hw, double* factors_out, double* loglik_out, double* place_out, double* place_sum_out,
                     int32_t* n_zero_out, double* null_out, int32_t* n_contrib_out, uint32_t flags)
{
    RC_TRY(ready(ctx));
    if (n_cand < 1 || !cand_allele || !cand_sure) return fail(ctx, CNF2_ERR_ARG, "n_cand must be >= 1 and cand_allele / cand_sure not NULL");
    if (!factors_out || !loglik_out || !place_sum_out || !n_zero_out || !null_out || !n_contrib_out)
        return fail(ctx, CNF2_ERR_ARG, "only place_out may be NULL");
    RC_TRY(mode_range(ctx, ind_begin, ind_end));
    const bool   dev = (flags & CNF2_OUT_DEVICE) != 0;
    const int    n = ind_end - ind_begin;
    const size_t M = ctx->n_markers, C = ctx->n_chrom, Q = (size_t)n_cand, R = (size_t)ctx->n_rows;
    if (Q * M > 0x7fffffff) return fail(ctx, CNF2_ERR_ARG, "too many candidates x markers in one call");
    HIP_TRY(ctx, hipSetDevice(ctx->device));

    // the candidate rows, in the row index space of cnf2_upload_rows
    {
        std::vector<uint8_t> packed(R * Q);
        for (size_t i = 0; i < R * Q; i++) {
            const uint8_t a0 = cand_allele[2 * i], a1 = cand_allele[2 * i + 1];
            if (a0 > 15 || a1 > 15) return fail(ctx, CNF2_ERR_ARG, "allele value out of range");
            packed[i] = (uint8_t)(a0 | (a1 << 4));
        }
        RC_TRY(ctx->d_pl_allele8.ensure(ctx, R * Q));
        RC_TRY(ctx->d_pl_sure.ensure(ctx, R * Q));
        RC_TRY(ctx->d_pl_hw.ensure(ctx, R * Q));
        HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));     // (an earlier call's kernels may still read the buffers)
        HIP_TRY(ctx, hipMemcpy(ctx->d_pl_allele8, packed.data(), R * Q, hipMemcpyHostToDevice));
        HIP_TRY(ctx, hipMemcpy(ctx->d_pl_sure, cand_sure, R * Q * sizeof(double2), hipMemcpyHostToDevice));
        if (cand_hw) HIP_TRY(ctx, hipMemcpy(ctx->d_pl_hw, cand_hw, R * Q * sizeof(double), hipMemcpyHostToDevice));
        else {
            const std::vector<double> half(R * Q, 0.5);
            HIP_TRY(ctx, hipMemcpy(ctx->d_pl_hw, half.data(), R * Q * sizeof(double), hipMemcpyHostToDevice));
        }
    }

    double * d_place, *d_sum, *d_null;
    int32_t *d_nz, *d_cnt;
    const size_t np = (size_t)n * Q * M;
    RC_TRY(stage_out(ctx, dev, place_out, ctx->d_pl_out, np, &d_place));
    RC_TRY(stage_out(ctx, dev, place_sum_out, ctx->d_pl_sum, Q * M, &d_sum));
    RC_TRY(stage_out(ctx, dev, n_zero_out, ctx->d_pl_nz, Q * M, &d_nz));
    RC_TRY(stage_out(ctx, dev, null_out, ctx->d_pl_null, Q, &d_null));
    RC_TRY(stage_out(ctx, dev, n_contrib_out, ctx->d_xo_cnt, C, &d_cnt));
    HIP_TRY(ctx, hipMemsetAsync(d_sum, 0, Q * M * sizeof(double), ctx->stream));
    HIP_TRY(ctx, hipMemsetAsync(d_nz, 0, Q * M * sizeof(int32_t), ctx->stream));
    HIP_TRY(ctx, hipMemsetAsync(d_null, 0, Q * sizeof(double), ctx->stream));
    HIP_TRY(ctx, hipMemsetAsync(d_cnt, 0, C * sizeof(int32_t), ctx->stream));

    if (n > 0) {
        // The likelihoods.  A range without tied windows: the placement instantiation's own (its forward pass is the plain sweep's: bit-equal).  With tied windows,
        // or with PLACE_SWEEP_LIKELIHOODS: cnf2_sweep's launches without rows first, the placement instantiation's to scratch
        bool tied_any = false;
        for (int j = 0; j < n && !tied_any; j++) tied_any = ctx->windows[ind_begin + j].n_groups > 0;
        const bool own = !tied_any && ((flags & PLACE_OWN_LIKELIHOODS) || (PLACE_OWN_DEFAULT && !(flags & PLACE_SWEEP_LIKELIHOODS)));
        const size_t nf = (size_t)n * C * 8, nl = (size_t)n * C;
        if (!own) {
            const uint32_t pass = flags & (CNF2_OUT_DEVICE | CNF2_STATIC_JOBS | CNF2_FULL_SPILL | CNF2_TIES_GENERAL | CNF2_ALL_STATES);
            RC_TRY(sweep_impl(ctx, ind_begin, ind_end, factors_out, loglik_out, nullptr, pass | CNF2_NO_DOSAGE, SweepMode()));
            HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));     // (the job list and the spill are replaced below)
        } else if (!dev) {
            RC_TRY(ctx->d_factors.ensure(ctx, nf));
            RC_TRY(ctx->d_loglik.ensure(ctx, nl));
        }
        RC_TRY(ctx->d_xo_f.ensure(ctx, nf + nl + 1));

        // the candidates' emission tables: all of them at once up to CNF2_PLACE_TILE, and an eighth of what is free
        size_t free_b = 0, total_b = 0;
        HIP_TRY(ctx, hipMemGetInfo(&free_b, &total_b));
        const size_t per16 = (size_t)n * 16 * 512 * sizeof(double);
        size_t       qcap = std::min((Q + 15) / 16 * 16, (size_t)CNF2_PLACE_TILE);
        qcap = std::min(qcap, std::max((size_t)1, (free_b + ctx->d_pl_emis.cap * sizeof(double)) / 8 / per16) * 16);
        RC_TRY(ctx->d_pl_emis.ensure(ctx, (size_t)n * qcap * 512));
        const int n_tiles = (int)((Q + qcap - 1) / qcap);

        // every window takes the untied instantiation: one list, by chromosome
        Batched b;
        RC_TRY(batched_setup(ctx, ind_begin, n, CNF2_NO_TIES, 512, 0, &b));
        const int    mlen = b.max_len;
        const size_t per_job = (size_t)mlen * 512;
        if (b.plan.fit == BATCH_NO_ROWS)
            return fail(ctx, CNF2_ERR_NOMEM, "not enough memory for the state posteriors of one job (%zu MB)", per_job >> 17);
        RC_TRY(ctx->d_wbuf.ensure(ctx, b.plan.batch * per_job));

        KernelParams p;
        base_params(ctx, &p);
        if (flags & CNF2_STATIC_JOBS) p.job_next = nullptr;
        p.windows      = ctx->d_windows + ind_begin;
        p.spill        = ctx->d_spill;
        p.spill_stride = spill_stride(mlen);
        p.factors      = own ? (dev ? factors_out : (double*)ctx->d_factors) : (double*)ctx->d_xo_f;
        p.loglik       = own ? (dev ? loglik_out : (double*)ctx->d_loglik) : ctx->d_xo_f + nf;
        p.wbuf         = ctx->d_wbuf;
        p.wstride      = (size_t)mlen;
        p.xo_cnt       = d_cnt;
        KernelParams pc = p;             // the candidate rows: Q "markers"
        pc.allele8   = ctx->d_pl_allele8;
        pc.sure      = ctx->d_pl_sure;
        pc.hw        = ctx->d_pl_hw;
        pc.n_markers = n_cand;
        PlaceParams q;
        memset(&q, 0, sizeof(q));
        q.n_cand    = n_cand;
        q.qcap      = (int)qcap;
        q.emis      = ctx->d_pl_emis;
        q.place     = d_place;
        q.place_sum = d_sum;
        q.n_zero    = d_nz;
        const bool half = !(flags & CNF2_FULL_SPILL);
        HIP_TRY(ctx, hipEventRecord(ctx->ev0, ctx->stream));
        if (n_tiles == 1) launch_place_emission(pc, n, 0, n_cand, (int)qcap, ctx->d_pl_emis, d_null, ctx->stream);
        bool first_batch = true;
        RC_TRY(for_each_batch(ctx, b, &p, [&](int, int grid, int max_len) -> int {
            HIP_TRY(ctx, launch_fb_fast(p, grid, {SW_POSTERIOR, half}, ctx->stream));
            q.kp      = p;
            q.n_jobs  = p.n_jobs;
            q.max_len = max_len;
            for (int t = 0; t < n_tiles; t++) {
                q.q0 = t * (int)qcap;
                q.qn = std::min((int)qcap, n_cand - q.q0);
                // (more than one tile: the tables of this tile for the whole range again; the baseline only once)
                if (n_tiles > 1)
                    launch_place_emission(pc, n, q.q0, q.qn, (int)qcap, ctx->d_pl_emis, first_batch ? d_null : nullptr, ctx->stream);
                // jobs a block walks with its tile's sums in registers: as many as still leave the device some thousand blocks
                const size_t units = (size_t)p.n_jobs * ((max_len + 63) / 64) * ((q.qn + 31) / 32);
                q.group = (int)std::max((size_t)1, std::min((size_t)256, units / 8192));
                launch_place_rows(q, ctx->stream);
            }
            HIP_TRY(ctx, hipGetLastError());
            first_batch = false;
            return CNF2_OK;
        }));
        HIP_TRY(ctx, hipEventRecord(ctx->ev1, ctx->stream));
        ctx->timed = true;
        if (own && !dev) {
            RC_TRY(fetch_out(ctx, factors_out, (const double*)ctx->d_factors, nf));
            RC_TRY(fetch_out(ctx, loglik_out, (const double*)ctx->d_loglik, nl));
        }
    }
    if (dev) return CNF2_OK;
    RC_TRY(fetch_out(ctx, place_out, d_place, np));
    RC_TRY(fetch_out(ctx, place_sum_out, d_sum, Q * M));
    RC_TRY(fetch_out(ctx, n_zero_out, d_nz, Q * M));
    RC_TRY(fetch_out(ctx, null_out, d_null, Q));
    RC_TRY(fetch_out(ctx, n_contrib_out, d_cnt, C));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    return CNF2_OK;
}

// The accumulators alone, into host arrays (zeroed first): the form the parity tests use.
int cnf2_accumulate(cnf2_ctx* ctx, int ind_begin, int ind_end, const int32_t* descendants, double* infprobs_out,
                    double* haplobase_out, double* haplocount_out, double* homozyg_out, uint32_t flags)
{
    return cnf2_sweep_accumulate(ctx, ind_begin, ind_end, descendants, nullptr, nullptr, nullptr, infprobs_out,
                                 haplobase_out, haplocount_out, homozyg_out,
                                 flags & ~(uint32_t)(CNF2_OUT_DEVICE | CNF2_ACC_DEVICE | CNF2_ACC_KEEP));
}

// ------------------------------------------------------------------------------------------------
// Per-iteration parameter updates on the device
// ------------------------------------------------------------------------------------------------
int cnf2_snapshot_priors(cnf2_ctx* ctx, const uint8_t* has_prior)
{
    if (!ctx || !has_prior) return fail(ctx, CNF2_ERR_ARG, "bad prior arguments");
    if (!ctx->d_allele8 || ctx->ped.n_rec == 0) return fail(ctx, CNF2_ERR_STATE, "rows and pedigree must be uploaded first");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    const size_t cnt = (size_t)ctx->n_rows * ctx->n_markers;
    RC_TRY(ctx->d_prior_allele8.release(ctx));
    RC_TRY(ctx->d_prior_sure.release(ctx));
    RC_TRY(ctx->d_has_prior.release(ctx));
    ctx->priors_set = false;
    RC_TRY(ctx->d_prior_allele8.alloc(ctx, cnt));
    RC_TRY(ctx->d_prior_sure.alloc(ctx, cnt));
    RC_TRY(ctx->d_has_prior.alloc(ctx, ctx->ped.n_rec));
    HIP_TRY(ctx, hipMemcpy(ctx->d_prior_allele8, ctx->d_allele8, cnt, hipMemcpyDeviceToDevice));
    HIP_TRY(ctx, hipMemcpy(ctx->d_prior_sure, ctx->d_sure, cnt * sizeof(double2), hipMemcpyDeviceToDevice));
    HIP_TRY(ctx, hipMemcpy(ctx->d_has_prior, has_prior, ctx->ped.n_rec, hipMemcpyHostToDevice));
    ctx->priors_set = true;
    return CNF2_OK;
}

static int update_pass_impl(cnf2_ctx* ctx, int chrom, const int32_t* recs, int n_recs, const int32_t* children,
                            const int32_t* descendants, double* infprobs, double* haplobase, double* haplocount, double scalefactor,
                            double entropyfactor, int* hits_out, uint32_t flags)
{
    if (!ctx || !children || !descendants || !hits_out) return fail(ctx, CNF2_ERR_ARG, "bad update arguments");
    if (recs) {
        if (n_recs < 0) return fail(ctx, CNF2_ERR_ARG, "bad record list");
        for (int i = 0; i < n_recs; i++)
            if (recs[i] < 0 || recs[i] >= ctx->ped.n_rec || (i > 0 && recs[i] <= recs[i - 1]))
                return fail(ctx, CNF2_ERR_ARG, "the record list must be ascending and within the pedigree (position %d)", i);
    }
    if (!ctx->d_allele8 || ctx->ped.n_rec == 0 || !ctx->d_rho) return fail(ctx, CNF2_ERR_STATE, "map, rows and pedigree must be uploaded first");
    if (!ctx->priors_set) return fail(ctx, CNF2_ERR_STATE, "cnf2_snapshot_priors must be called after the rows were uploaded");
    if (chrom < 0 || chrom >= ctx->n_chrom) return fail(ctx, CNF2_ERR_ARG, "chromosome out of range");
    const bool acc_dev = (flags & CNF2_ACC_DEVICE) != 0;
    const bool given = infprobs && haplobase && haplocount;
    if (acc_dev && !given) return fail(ctx, CNF2_ERR_ARG, "accumulator pointers are NULL");
    const HostPedigree& P = ctx->ped;
    const size_t R = (size_t)P.n_rec, M = (size_t)ctx->n_markers;
    // a row that is written must belong to one record.  Row 0 is the shared blank row of a de-duplicated upload: the
    // kernels never write it (a record on it keeps haplotype weight 1/2); every other row has exactly one owner, empty
    // records included (updatehaploweights moves their weights too).
    {
        std::vector<int32_t> owner(ctx->n_rows, -1);
        for (int r = 0; r < P.n_rec; r++) {
            if (P.row_of[r] == 0) {
                if (!P.empty[r]) return fail(ctx, CNF2_ERR_ARG, "record %d has data but sits on the blank row 0", r);
                continue;
            }
            if (owner[P.row_of[r]] >= 0) return fail(ctx, CNF2_ERR_ARG, "records %d and %d share genotype row %d: updates need one row per record (or the blank row 0)", owner[P.row_of[r]], r, P.row_of[r]);
            owner[P.row_of[r]] = r;
        }
    }
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    if (ctx->d_row_of.cap < R || ctx->d_children.cap < R) {
        RC_TRY(ctx->d_row_of.release(ctx));
        RC_TRY(ctx->d_children.release(ctx));
        RC_TRY(ctx->d_row_of.alloc(ctx, R));
        RC_TRY(ctx->d_children.alloc(ctx, R));
    }
    RC_TRY(ensure_rec_tables(ctx, R));
    RC_TRY(ctx->d_chromstarts.ensure(ctx, 65536));
    if (ctx->n_chrom + 1 > 65536) return fail(ctx, CNF2_ERR_ARG, "too many chromosomes");
    RC_TRY(ctx->d_hits.ensure(ctx, 1));
    HIP_TRY(ctx, hipMemcpyAsync(ctx->d_row_of, P.row_of.data(), sizeof(int32_t) * R, hipMemcpyHostToDevice, ctx->stream));
    HIP_TRY(ctx, hipMemcpyAsync(ctx->d_children, children, sizeof(int32_t) * R, hipMemcpyHostToDevice, ctx->stream));
    HIP_TRY(ctx, hipMemcpyAsync(ctx->d_desc, descendants, sizeof(int32_t) * R, hipMemcpyHostToDevice, ctx->stream));
    HIP_TRY(ctx, hipMemcpyAsync(ctx->d_rec_empty, P.empty.data(), R, hipMemcpyHostToDevice, ctx->stream));
    HIP_TRY(ctx, hipMemcpyAsync(ctx->d_chromstarts, ctx->chromstarts.data(), sizeof(int32_t) * (ctx->n_chrom + 1),
                                hipMemcpyHostToDevice, ctx->stream));
    HIP_TRY(ctx, hipMemsetAsync(ctx->d_hits, 0, sizeof(int), ctx->stream));
    RC_TRY(ctx->d_anyinfo.ensure(ctx, R * ctx->n_chrom));
    RC_TRY(ctx->d_fw.ensure(ctx, R * M * 2));
    RC_TRY(ctx->d_ratio.ensure(ctx, R * M));
    double *a_inf = infprobs, *a_hb = haplobase, *a_hc = haplocount;
    if (!acc_dev) {
        RC_TRY(ctx->d_acc_inf.ensure(ctx, R * M * 4));
        RC_TRY(ctx->d_acc_hb.ensure(ctx, R * M));
        RC_TRY(ctx->d_acc_hc.ensure(ctx, R * M));
        a_inf = ctx->d_acc_inf;
        a_hb  = ctx->d_acc_hb;
        a_hc  = ctx->d_acc_hc;
        if (given) {
            HIP_TRY(ctx, hipMemcpyAsync(a_inf, infprobs, R * M * 4 * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
            HIP_TRY(ctx, hipMemcpyAsync(a_hb, haplobase, R * M * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
            HIP_TRY(ctx, hipMemcpyAsync(a_hc, haplocount, R * M * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
        }
    }
    UpdateParams u;
    memset(&u, 0, sizeof(u));
    u.n_rec = P.n_rec;
    if (recs) {
        RC_TRY(ctx->d_updrecs.ensure(ctx, (size_t)(n_recs > 0 ? n_recs : 1)));
        HIP_TRY(ctx, hipMemcpyAsync(ctx->d_updrecs, recs, sizeof(int32_t) * n_recs, hipMemcpyHostToDevice, ctx->stream));
        u.n_rec = n_recs;
        u.rec_list = ctx->d_updrecs;
    }
    const size_t RU = (size_t)u.n_rec;         // records this pass updates
    u.n_markers = ctx->n_markers;
    u.n_chrom = ctx->n_chrom;
    u.chrom = chrom;
    u.first = ctx->chromstarts[chrom];
    u.last = ctx->chromstarts[chrom + 1] - 1;
    u.chromstarts_host_upto = ctx->chromstarts[chrom + 1];
    u.chromstarts = ctx->d_chromstarts;
    u.row_of = ctx->d_row_of;
    u.rec_empty = ctx->d_rec_empty;
    u.has_prior = ctx->d_has_prior;
    u.children = ctx->d_children;
    u.descendants = ctx->d_desc;
    u.allele8 = ctx->d_allele8;
    u.sure = ctx->d_sure;
    u.hw = ctx->d_hw;
    u.prior_allele8 = ctx->d_prior_allele8;
    u.prior_sure = ctx->d_prior_sure;
    u.acc_inf = a_inf;
    u.acc_hb = a_hb;
    u.acc_hc = a_hc;
    u.anyinfo = ctx->d_anyinfo;
    u.fw = ctx->d_fw;
    u.ratio = ctx->d_ratio;
    u.relhaplo = 0.5;
    u.scalefactor = scalefactor;
    u.entropyfactor = entropyfactor;
    u.hits = ctx->d_hits;
    if (!(flags & CNF2_UPDATE_PLAIN)) {
        RC_TRY(ctx->d_flow_next.ensure(ctx, 32));
        RC_TRY(ctx->d_flow_out.ensure(ctx, (RU ? RU : 1) * (size_t)(u.last - u.first + 1) * 4));
        // the scouts work through their flows in chunks; a chunk's worth of set-aside entries (24 bytes each), no more
        // than the pass has flows (certainties: 4 per record and marker of the chromosome; weights: 1 per record and marker
        // of the chromosomes so far)
        const size_t chunk = todo_chunk(RU, (size_t)(u.last - u.first + 1), (size_t)u.chromstarts_host_upto);
        RC_TRY(ctx->d_todo.ensure(ctx, todo_doubles(chunk)));
        u.flow_next = ctx->d_flow_next;
        u.flow_out = ctx->d_flow_out;
        u.stats = getenv("CNF2_UPDATE_STATS") ? ctx->d_flow_next + 2 : nullptr;     // diagnostics only (no effect on results): a few atomics per wavefront
        u.todo = ctx->d_todo;
        u.todo_cap = chunk;
        u.todo2 = ctx->d_todo + chunk * 3;
        u.todo3 = TODO_LISTS > 2 ? ctx->d_todo + chunk * 6 : nullptr;
        u.todo_counts = (unsigned long long*)(ctx->d_todo + chunk * 3 * TODO_LISTS);
        u.scout_passes = (flags & CNF2_UPDATE_ONE_SCOUT) ? 1 : 2;
        u.mirror = (flags & CNF2_UPDATE_BOTH_FLOWS) ? 0 : 1;
        u.literal_finish = (flags & CNF2_UPDATE_LITERAL_FINISH) ? 1 : 0;
    }
    if (u.n_rec > 0) launch_update_pass(u, ctx->stream);
    HIP_TRY(ctx, hipGetLastError());
    ctx->qtl_rows_n = 0;               // (the rows a cnf2_sweep_qtl left are no longer this state's)
    ctx->windows_dirty = true;          // rows changed: the "homozygous everywhere" flags must be derived again
    HIP_TRY(ctx, hipMemcpyAsync(hits_out, ctx->d_hits, sizeof(int), hipMemcpyDeviceToHost, ctx->stream));
    if (!acc_dev && given) {
        HIP_TRY(ctx, hipMemcpyAsync(infprobs, a_inf, R * M * 4 * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
        HIP_TRY(ctx, hipMemcpyAsync(haplobase, a_hb, R * M * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
        HIP_TRY(ctx, hipMemcpyAsync(haplocount, a_hc, R * M * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    }
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    return CNF2_OK;
}

int cnf2_update_pass(cnf2_ctx* ctx, int chrom, const int32_t* children, const int32_t* descendants, double* infprobs,
                     double* haplobase, double* haplocount, double scalefactor, double entropyfactor, int* hits_out,
                     uint32_t flags)
{
    return update_pass_impl(ctx, chrom, nullptr, 0, children, descendants, infprobs, haplobase, haplocount, scalefactor, entropyfactor,
                            hits_out, flags);
}

int cnf2_update_pass_records(cnf2_ctx* ctx, int chrom, const int32_t* recs, int n_recs, const int32_t* children,
                             const int32_t* descendants, double scalefactor, double entropyfactor, int* hits_out, uint32_t flags)
{
    if (!recs && n_recs != 0) return fail(ctx, CNF2_ERR_ARG, "bad record list");
    static const int32_t none = 0;
    return update_pass_impl(ctx, chrom, recs ? recs : &none, n_recs, children, descendants, nullptr, nullptr, nullptr, scalefactor,
                            entropyfactor, hits_out, flags & ~(uint32_t)CNF2_ACC_DEVICE);
}

// ------------------------------------------------------------------------------------------------
// Exchange support of multi-process runs: listed records' accumulators / rows to and from a packed device buffer
// ------------------------------------------------------------------------------------------------
int cnf2_exchange_buffer(cnf2_ctx* ctx, size_t bytes, void** d_buf)
{
    if (!ctx || !d_buf) return fail(ctx, CNF2_ERR_ARG, "bad arguments");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    RC_TRY(ctx->d_xbuf.ensure(ctx, bytes ? bytes : 1));
    *d_buf = ctx->d_xbuf;
    return CNF2_OK;
}

int cnf2_exchange_read(cnf2_ctx* ctx, size_t offset, void* host_dst, size_t bytes)
{
    if (!ctx || (!host_dst && bytes)) return fail(ctx, CNF2_ERR_ARG, "bad arguments");
    if (offset + bytes > ctx->d_xbuf.cap || !ctx->d_xbuf) return fail(ctx, CNF2_ERR_ARG, "beyond the exchange buffer");
    if (!bytes) return CNF2_OK;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    HIP_TRY(ctx, hipMemcpy(host_dst, ctx->d_xbuf + offset, bytes, hipMemcpyDeviceToHost));
    return CNF2_OK;
}

int cnf2_exchange_write(cnf2_ctx* ctx, size_t offset, const void* host_src, size_t bytes)
{
    if (!ctx || (!host_src && bytes)) return fail(ctx, CNF2_ERR_ARG, "bad arguments");
    if (offset + bytes > ctx->d_xbuf.cap || !ctx->d_xbuf) return fail(ctx, CNF2_ERR_ARG, "beyond the exchange buffer");
    if (!bytes) return CNF2_OK;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    HIP_TRY(ctx, hipMemcpy(ctx->d_xbuf + offset, host_src, bytes, hipMemcpyHostToDevice));
    return CNF2_OK;
}

int cnf2_exchange_download(cnf2_ctx* ctx, void* host_dst, size_t bytes) { return cnf2_exchange_read(ctx, 0, host_dst, bytes); }
int cnf2_exchange_upload(cnf2_ctx* ctx, const void* host_src, size_t bytes) { return cnf2_exchange_write(ctx, 0, host_src, bytes); }

size_t cnf2_packed_accumulator_doubles(const cnf2_ctx* ctx) { return ctx ? (size_t)ctx->n_markers * 6 : 0; }
size_t cnf2_packed_row_bytes(const cnf2_ctx* ctx) { return ctx ? (((size_t)ctx->n_markers * 25 + 7) & ~(size_t)7) : 0; }

// uploads recs (and, with rows, the rows they sit on) as index lists: d_xidx = [recs | rows]
static int exchange_lists(cnf2_ctx* ctx, const int32_t* recs, int n, bool rows)
{
    if (!ctx || (!recs && n > 0) || n < 0) return fail(ctx, CNF2_ERR_ARG, "bad record list");
    if (ctx->ped.n_rec == 0 || !ctx->d_allele8) return fail(ctx, CNF2_ERR_STATE, "rows and pedigree must be uploaded first");
    std::vector<int32_t> idx((size_t)n * 2);
    for (int i = 0; i < n; i++) {
        if (recs[i] < 0 || recs[i] >= ctx->ped.n_rec) return fail(ctx, CNF2_ERR_ARG, "record out of range at %d", i);
        idx[i] = recs[i];
        idx[(size_t)n + i] = ctx->ped.row_of[recs[i]];
        if (rows && idx[(size_t)n + i] == 0) return fail(ctx, CNF2_ERR_ARG, "record %d sits on the shared blank row", recs[i]);
    }
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    RC_TRY(ctx->d_xidx.ensure(ctx, (size_t)(n > 0 ? n : 1) * 2));
    if (n > 0) {
        HIP_TRY(ctx, hipMemcpyAsync(ctx->d_xidx, idx.data(), sizeof(int32_t) * idx.size(), hipMemcpyHostToDevice, ctx->stream));
        HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));          // idx goes out of scope
    }
    return CNF2_OK;
}

static int have_accumulators(cnf2_ctx* ctx)
{
    const size_t R = (size_t)ctx->ped.n_rec, M = (size_t)ctx->n_markers;
    if (!ctx->d_acc_inf || !ctx->d_acc_hb || !ctx->d_acc_hc || ctx->d_acc_inf.cap < R * M * 4 || ctx->d_acc_hb.cap < R * M ||
        ctx->d_acc_hc.cap < R * M)
        return fail(ctx, CNF2_ERR_STATE, "the context holds no accumulators (cnf2_sweep_accumulate with NULL accumulator pointers first)");
    return CNF2_OK;
}

int cnf2_pack_accumulators(cnf2_ctx* ctx, const int32_t* recs, int n, double* d_packed)
{
    RC_TRY(exchange_lists(ctx, recs, n, false));
    if (n == 0) return CNF2_OK;
    if (!d_packed) return fail(ctx, CNF2_ERR_ARG, "packed buffer is NULL");
    RC_TRY(have_accumulators(ctx));
    const size_t M = (size_t)ctx->n_markers, S = M * 6;
    launch_copy_rows_f64(ctx->d_acc_inf, M * 4, ctx->d_xidx, d_packed, S, nullptr, n, M * 4, ctx->stream);
    launch_copy_rows_f64(ctx->d_acc_hb, M, ctx->d_xidx, d_packed + M * 4, S, nullptr, n, M, ctx->stream);
    launch_copy_rows_f64(ctx->d_acc_hc, M, ctx->d_xidx, d_packed + M * 5, S, nullptr, n, M, ctx->stream);
    HIP_TRY(ctx, hipGetLastError());
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    return CNF2_OK;
}

int cnf2_unpack_accumulators(cnf2_ctx* ctx, const int32_t* recs, int n, const double* d_packed)
{
    RC_TRY(exchange_lists(ctx, recs, n, false));
    if (n == 0) return CNF2_OK;
    if (!d_packed) return fail(ctx, CNF2_ERR_ARG, "packed buffer is NULL");
    RC_TRY(have_accumulators(ctx));
    const size_t M = (size_t)ctx->n_markers, S = M * 6;
    launch_copy_rows_f64(d_packed, S, nullptr, ctx->d_acc_inf, M * 4, ctx->d_xidx, n, M * 4, ctx->stream);
    launch_copy_rows_f64(d_packed + M * 4, S, nullptr, ctx->d_acc_hb, M, ctx->d_xidx, n, M, ctx->stream);
    launch_copy_rows_f64(d_packed + M * 5, S, nullptr, ctx->d_acc_hc, M, ctx->d_xidx, n, M, ctx->stream);
    HIP_TRY(ctx, hipGetLastError());
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    return CNF2_OK;
}

int cnf2_pack_rows(cnf2_ctx* ctx, const int32_t* recs, int n, void* d_packed)
{
    RC_TRY(exchange_lists(ctx, recs, n, true));
    if (n == 0) return CNF2_OK;
    if (!d_packed) return fail(ctx, CNF2_ERR_ARG, "packed buffer is NULL");
    const size_t   M = (size_t)ctx->n_markers, B = cnf2_packed_row_bytes(ctx);
    const int32_t* rows = ctx->d_xidx + n;
    uint8_t*       q = (uint8_t*)d_packed;
    launch_copy_rows_f64((const double*)ctx->d_sure.ptr, M * 2, rows, (double*)q, B / 8, nullptr, n, M * 2, ctx->stream);
    launch_copy_rows_f64(ctx->d_hw, M, rows, (double*)(q + M * 16), B / 8, nullptr, n, M, ctx->stream);
    launch_copy_rows_u8(ctx->d_allele8, M, rows, q + M * 24, B, nullptr, n, M, ctx->stream);
    HIP_TRY(ctx, hipGetLastError());
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    return CNF2_OK;
}

int cnf2_unpack_rows(cnf2_ctx* ctx, const int32_t* recs, int n, const void* d_packed)
{
    RC_TRY(exchange_lists(ctx, recs, n, true));
    if (n == 0) return CNF2_OK;
    if (!d_packed) return fail(ctx, CNF2_ERR_ARG, "packed buffer is NULL");
    const size_t   M = (size_t)ctx->n_markers, B = cnf2_packed_row_bytes(ctx);
    const int32_t* rows = ctx->d_xidx + n;
    const uint8_t* q = (const uint8_t*)d_packed;
    launch_copy_rows_f64((const double*)q, B / 8, nullptr, (double*)ctx->d_sure.ptr, M * 2, rows, n, M * 2, ctx->stream);
    launch_copy_rows_f64((const double*)(q + M * 16), B / 8, nullptr, ctx->d_hw, M, rows, n, M, ctx->stream);
    launch_copy_rows_u8(q + M * 24, B, nullptr, ctx->d_allele8, M, rows, n, M, ctx->stream);
    HIP_TRY(ctx, hipGetLastError());
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    ctx->qtl_rows_n = 0;               // (the rows a cnf2_sweep_qtl left are no longer this state's)
    ctx->windows_dirty = true;          // rows changed: the "homozygous everywhere" flags must be derived again
    return CNF2_OK;
}

int cnf2_download_accumulators(cnf2_ctx* ctx, double* infprobs, double* haplobase, double* haplocount)
{
    if (!ctx) return fail(ctx, CNF2_ERR_ARG, "ctx is NULL");
    const size_t R = (size_t)ctx->ped.n_rec, M = (size_t)ctx->n_markers;
    if (!ctx->d_acc_inf || !ctx->d_acc_hb || !ctx->d_acc_hc || ctx->d_acc_inf.cap < R * M * 4 || ctx->d_acc_hb.cap < R * M ||
        ctx->d_acc_hc.cap < R * M)
        return fail(ctx, CNF2_ERR_STATE, "the context holds no accumulators (cnf2_sweep_accumulate with NULL accumulator pointers first)");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    if (infprobs) HIP_TRY(ctx, hipMemcpy(infprobs, ctx->d_acc_inf, R * M * 4 * sizeof(double), hipMemcpyDeviceToHost));
    if (haplobase) HIP_TRY(ctx, hipMemcpy(haplobase, ctx->d_acc_hb, R * M * sizeof(double), hipMemcpyDeviceToHost));
    if (haplocount) HIP_TRY(ctx, hipMemcpy(haplocount, ctx->d_acc_hc, R * M * sizeof(double), hipMemcpyDeviceToHost));
    return CNF2_OK;
}

int cnf2_accumulator_ptrs(cnf2_ctx* ctx, double** infprobs, double** haplobase, double** haplocount)
{
    if (!ctx || !infprobs || !haplobase || !haplocount) return fail(ctx, CNF2_ERR_ARG, "bad arguments");
    const size_t R = (size_t)ctx->ped.n_rec, M = (size_t)ctx->n_markers;
    if (!ctx->d_acc_inf || !ctx->d_acc_hb || !ctx->d_acc_hc || ctx->d_acc_inf.cap < R * M * 4 || ctx->d_acc_hb.cap < R * M ||
        ctx->d_acc_hc.cap < R * M)
        return fail(ctx, CNF2_ERR_STATE, "the context holds no accumulators (cnf2_sweep_accumulate with NULL accumulator pointers first)");
    *infprobs = ctx->d_acc_inf;
    *haplobase = ctx->d_acc_hb;
    *haplocount = ctx->d_acc_hc;
    return CNF2_OK;
}

int cnf2_upload_accumulators(cnf2_ctx* ctx, const double* infprobs, const double* haplobase, const double* haplocount)
{
    if (!ctx) return fail(ctx, CNF2_ERR_ARG, "ctx is NULL");
    const size_t R = (size_t)ctx->ped.n_rec, M = (size_t)ctx->n_markers;
    if (R == 0 || M == 0) return fail(ctx, CNF2_ERR_STATE, "map and pedigree must be uploaded first");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    RC_TRY(ctx->d_acc_inf.ensure(ctx, R * M * 4));
    RC_TRY(ctx->d_acc_hb.ensure(ctx, R * M));
    RC_TRY(ctx->d_acc_hc.ensure(ctx, R * M));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    if (infprobs) HIP_TRY(ctx, hipMemcpy(ctx->d_acc_inf, infprobs, R * M * 4 * sizeof(double), hipMemcpyHostToDevice));
    if (haplobase) HIP_TRY(ctx, hipMemcpy(ctx->d_acc_hb, haplobase, R * M * sizeof(double), hipMemcpyHostToDevice));
    if (haplocount) HIP_TRY(ctx, hipMemcpy(ctx->d_acc_hc, haplocount, R * M * sizeof(double), hipMemcpyHostToDevice));
    return CNF2_OK;
}

int cnf2_update_stats(cnf2_ctx* ctx, uint64_t* out16)
{
    if (!ctx || !out16) return fail(ctx, CNF2_ERR_ARG, "bad arguments");
    if (!ctx->d_flow_next) return fail(ctx, CNF2_ERR_STATE, "no update pass has run");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    HIP_TRY(ctx, hipMemcpy(out16, ctx->d_flow_next + 2, 16 * sizeof(uint64_t), hipMemcpyDeviceToHost));
    return CNF2_OK;
}

int cnf2_update_stats_guided(cnf2_ctx* ctx, uint64_t* out8)
{
    if (!ctx || !out8) return fail(ctx, CNF2_ERR_ARG, "bad arguments");
    if (!ctx->d_flow_next) return fail(ctx, CNF2_ERR_STATE, "no update pass has run");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    HIP_TRY(ctx, hipMemcpy(out8, ctx->d_flow_next + 18, 8 * sizeof(uint64_t), hipMemcpyDeviceToHost));
    return CNF2_OK;
}

int cnf2_download_rows(cnf2_ctx* ctx, int row0, int n, uint8_t* allele, double* sure, double* hw)
{
    if (!ctx || !allele || !sure || !hw) return fail(ctx, CNF2_ERR_ARG, "bad row arguments");
    if (!ctx->d_allele8) return fail(ctx, CNF2_ERR_STATE, "no rows uploaded");
    if (row0 < 0 || n < 0 || row0 + n > ctx->n_rows) return fail(ctx, CNF2_ERR_ARG, "row range out of bounds");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    const size_t M = ctx->n_markers, cnt = (size_t)n * M;
    std::vector<uint8_t> packed(cnt);
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    HIP_TRY(ctx, hipMemcpy(packed.data(), ctx->d_allele8 + (size_t)row0 * M, cnt, hipMemcpyDeviceToHost));
    for (size_t i = 0; i < cnt; i++) {
        allele[i * 2]     = packed[i] & 15;
        allele[i * 2 + 1] = packed[i] >> 4;
    }
    HIP_TRY(ctx, hipMemcpy(sure, ctx->d_sure + (size_t)row0 * M, cnt * sizeof(double2), hipMemcpyDeviceToHost));
    HIP_TRY(ctx, hipMemcpy(hw, ctx->d_hw + (size_t)row0 * M, cnt * sizeof(double), hipMemcpyDeviceToHost));
    return CNF2_OK;
}

// ------------------------------------------------------------------------------------------------
// Pre-processing users of the emission for ARBITRARY records (postmarkerdata, cnF2freq.cpp:3190-3412)
// ------------------------------------------------------------------------------------------------
// windows of the records recs[0..n): mode 0 = no founder flag anywhere (the state in which main() calls
// postmarkerdata: fixtrees has not run), mode 1 = the flags fixtrees has left when the records are processed in
// ascending order (a member's flag counts if its record index is <= the record's own, cnF2freq.cpp:3373-3389),
// mode 2 = every flag (fixtrees has run on everybody)
static int scan_windows(cnf2_ctx* ctx, const int32_t* recs, int n, int mode)
{
    const HostPedigree& P = ctx->ped;
    std::vector<Window> ws(n);
    for (int i = 0; i < n; i++) {
        if (recs[i] < 0 || recs[i] >= P.n_rec) return fail(ctx, CNF2_ERR_ARG, "record out of range at %d", i);
        int32_t slot_rec[7];
        derive_window(P, recs[i], &ws[i], slot_rec);
        for (int k = 0; k < 7; k++) {
            if (slot_rec[k] < 0) continue;
            if (mode == 0 || (mode == 1 && slot_rec[k] > recs[i])) ws[i].flags[k] &= (uint8_t)~SLOT_FOUNDER;
        }
    }
    RC_TRY(ctx->d_scanwin.ensure(ctx, (size_t)n));
    HIP_TRY(ctx, hipMemcpy(ctx->d_scanwin, ws.data(), sizeof(Window) * n, hipMemcpyHostToDevice));
    return CNF2_OK;
}

int cnf2_fixparents_scan(cnf2_ctx* ctx, const int32_t* recs, int n, uint8_t* ok_out)
{
    if (!ctx || !recs || !ok_out || n < 0) return fail(ctx, CNF2_ERR_ARG, "bad scan arguments");
    if (!ctx->d_rho || !ctx->d_allele8 || ctx->ped.n_rec == 0) return fail(ctx, CNF2_ERR_STATE, "map, rows and pedigree must be uploaded first");
    if (n == 0) return CNF2_OK;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    // grid.y holds the record index: slabs of at most 65 535 records (a pedigree of config 4's size has ~300 000)
    const int    slab = 65535;
    const size_t per = (size_t)ctx->n_markers * 2;
    RC_TRY(ctx->d_okout.ensure(ctx, (size_t)(n < slab ? n : slab) * per));
    for (int i0 = 0; i0 < n; i0 += slab) {
        const int k = n - i0 < slab ? n - i0 : slab;
        RC_TRY(scan_windows(ctx, recs + i0, k, 0));
        KernelParams p;
        base_params(ctx, &p);
        p.windows = ctx->d_scanwin;
        launch_okvals(p, k, ctx->d_okout, ctx->stream);
        HIP_TRY(ctx, hipGetLastError());
        HIP_TRY(ctx, hipMemcpyAsync(ok_out + (size_t)i0 * per, ctx->d_okout, (size_t)k * per, hipMemcpyDeviceToHost, ctx->stream));
        HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    }
    return CNF2_OK;
}

// ordered: bit 0 = founder flags as fixtrees has assigned them in ascending order; bit 1 = evaluate by brute force
// (the 65 536 emission calls of the reference's loops) instead of the closed form -- cross-check only
int cnf2_variances(cnf2_ctx* ctx, const int32_t* recs, int n, int ordered, double* var_out)
{
    if (!ctx || !recs || !var_out || n < 0) return fail(ctx, CNF2_ERR_ARG, "bad scan arguments");
    if (!ctx->d_rho || !ctx->d_allele8 || ctx->ped.n_rec == 0) return fail(ctx, CNF2_ERR_STATE, "map, rows and pedigree must be uploaded first");
    if (n == 0) return CNF2_OK;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    const size_t M = ctx->n_markers;
    const bool brute = (ordered & 2) != 0;
    ordered &= 1;
    const int slab = brute ? 4096 : 65535;       // grid.y
    RC_TRY(ctx->d_scratch.ensure(ctx, (size_t)(n < slab ? n : slab) * M));
    for (int i0 = 0; i0 < n; i0 += slab) {
        const int k = n - i0 < slab ? n - i0 : slab;
        RC_TRY(scan_windows(ctx, recs + i0, k, ordered ? 1 : 2));
        KernelParams p;
        base_params(ctx, &p);
        p.windows = ctx->d_scanwin;
        if (brute) launch_addvariance_batch(p, k, ctx->d_scratch, ctx->stream);
        else launch_variance_closed(p, k, ctx->d_scratch, ctx->stream);
        HIP_TRY(ctx, hipGetLastError());
        HIP_TRY(ctx, hipMemcpyAsync(var_out + (size_t)i0 * M, ctx->d_scratch, (size_t)k * M * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
        HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    }
    return CNF2_OK;
}

// var_out[q] = addvariance of record recs[q] at marker markers[q] with the reference's own rounding (variance_exact)
int cnf2_variances_exact(cnf2_ctx* ctx, const int32_t* recs, const int32_t* markers, int n, int ordered, double* var_out)
{
    if (!ctx || !recs || !markers || !var_out || n < 0) return fail(ctx, CNF2_ERR_ARG, "bad scan arguments");
    if (!ctx->d_rho || !ctx->d_allele8 || ctx->ped.n_rec == 0) return fail(ctx, CNF2_ERR_STATE, "map, rows and pedigree must be uploaded first");
    if (n == 0) return CNF2_OK;
    for (int q = 0; q < n; q++)
        if (markers[q] < 0 || markers[q] >= ctx->n_markers) return fail(ctx, CNF2_ERR_ARG, "marker out of range at %d", q);
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    const int slab = 1 << 20;
    // per entry: the result, then (behind all results) its marker
    RC_TRY(ctx->d_scratch.ensure(ctx, (size_t)(n < slab ? n : slab) * 2));
    for (int i0 = 0; i0 < n; i0 += slab) {
        const int k = n - i0 < slab ? n - i0 : slab;
        RC_TRY(scan_windows(ctx, recs + i0, k, (ordered & 1) ? 1 : 2));
        int32_t* d_markers = (int32_t*)(ctx->d_scratch + k);
        HIP_TRY(ctx, hipMemcpyAsync(d_markers, markers + i0, (size_t)k * sizeof(int32_t), hipMemcpyHostToDevice, ctx->stream));
        KernelParams p;
        base_params(ctx, &p);
        p.windows = ctx->d_scanwin;
        launch_variance_exact(p, d_markers, k, ctx->d_scratch, ctx->stream);
        HIP_TRY(ctx, hipGetLastError());
        HIP_TRY(ctx, hipMemcpyAsync(var_out + i0, ctx->d_scratch, (size_t)k * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
        HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    }
    return CNF2_OK;
}

int cnf2_addvariance(cnf2_ctx* ctx, int ind, int chrom, double* var_out)
{
    RC_TRY(ready(ctx));
    if (!var_out || ind < 0 || ind >= (int)ctx->windows.size() || chrom < 0 || chrom >= ctx->n_chrom)
        return fail(ctx, CNF2_ERR_ARG, "bad addvariance arguments");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    const int first = ctx->chromstarts[chrom], len = ctx->chromstarts[chrom + 1] - first;
    RC_TRY(ctx->d_scratch.ensure(ctx, (size_t)len));
    KernelParams p;
    base_params(ctx, &p);
    p.windows = ctx->d_windows + ind;
    launch_addvariance(p, first, len, ctx->d_scratch, ctx->stream);
    HIP_TRY(ctx, hipGetLastError());
    HIP_TRY(ctx, hipMemcpyAsync(var_out, ctx->d_scratch, (size_t)len * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    return CNF2_OK;
}

int cnf2_emission(cnf2_ctx* ctx, int ind, int marker, double* e_out)
{
    RC_TRY(ready(ctx));
    if (ind < 0 || ind >= (int)ctx->windows.size() || marker < 0 || marker >= ctx->n_markers || !e_out)
        return fail(ctx, CNF2_ERR_ARG, "bad emission arguments");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    RC_TRY(ctx->d_scratch.ensure(ctx, (size_t)512));
    KernelParams p;
    base_params(ctx, &p);
    launch_emission(p, ind, marker, ctx->d_scratch, ctx->stream);
    HIP_TRY(ctx, hipGetLastError());
    HIP_TRY(ctx, hipMemcpyAsync(e_out, ctx->d_scratch, 512 * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    return CNF2_OK;
}

int cnf2_emission_paths(cnf2_ctx* ctx, int ind, int marker, double* e_out)
{
    RC_TRY(ready(ctx));
    if (ind < 0 || ind >= (int)ctx->windows.size() || marker < 0 || marker >= ctx->n_markers || !e_out)
        return fail(ctx, CNF2_ERR_ARG, "bad emission arguments");
    const size_t n = (size_t)8 * 64 * 128;
    RC_TRY(ctx->d_scratch.ensure(ctx, n));
    KernelParams p;
    base_params(ctx, &p);
    p.windows = ctx->d_windows + ind;
    launch_emission_paths(p, marker, ctx->d_scratch, ctx->stream);
    HIP_TRY(ctx, hipGetLastError());
    HIP_TRY(ctx, hipMemcpyAsync(e_out, ctx->d_scratch, n * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    return CNF2_OK;
}

int cnf2_selftest_lane_xor(cnf2_ctx* ctx, double* out384)
{
    if (!ctx || !out384) return CNF2_ERR_ARG;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    RC_TRY(ctx->d_scratch.ensure(ctx, (size_t)512));
    launch_xor_selftest(ctx->d_scratch, ctx->stream);
    HIP_TRY(ctx, hipGetLastError());
    HIP_TRY(ctx, hipMemcpyAsync(out384, ctx->d_scratch, 384 * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    return CNF2_OK;
}

} // extern "C"
