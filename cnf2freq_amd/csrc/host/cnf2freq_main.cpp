// cnf2freq_main.cpp -- drop-in command line for the PlantImpute invocation of the reference
// (demo.sh:37):
//   cnF2freq --mapfile F --pedfile F --genfile F --output F --count N [--limit n] [--capmarker n] [--tmppath d]
//            [--deserialize F] [--gpus N] [--crossovers F] [--viterbi F] [--sample F [--draws K] [--seed S]]
//            [--place F --place-genfile G --place-markers Q] [--loo F [--loo-threshold X]] [--origins F] [--descent F]
//            [--qtl F --phenofile P [--qtl-covariates name,name] [--qtl-permutations K] [--qtl-seed S] [--qtl-additive]]
//            [--qtl2 F [--qtl2-every S] [--qtl2-linked] --phenofile P [the --qtl-* options]]
//            [--qtlx F --phenofile P [--qtl-imprint] [--qtl-interactive name,name] [the --qtl-* options]]
//            [--qtlem F --phenofile P [--qtl-em-iterations N] [--qtl-em-tol X] [--qtl-imprint] [the --qtl-* options]]
//            [--qtlvar F --phenofile P [--qtl-var-covariates name,name] [--qtl-var-iterations N] [--qtl-var-tol X] [--qtl-imprint] [the --qtl-* options]]
//            [--qtlbin F --phenofile P [--qtl-binary-iterations N] [--qtl-binary-tol X] [--qtl-imprint] [the --qtl-* options]]
//            [--qtlsurv F --phenofile P --qtl-surv-time NAME --qtl-surv-status NAME [--qtl-surv-iterations N] [--qtl-surv-tol X]
//             [--qtl-imprint] [the --qtl-* options]]
//            [--qtlcof F --phenofile P --qtl-cofactors i,j,k [--qtl-window X] [the --qtl-* options]]
//            [--qtlboot F --phenofile P --qtl-boot-chrom C [--qtl-boot-replicates B] [--qtl-covariates, --qtl-seed, --qtl-additive]]
//            [--qtlmv F --phenofile P [--qtl-traits name,name,..] [--qtl-covariates, --qtl-permutations, --qtl-seed, --qtl-additive]]
//            [--qtlfam F --phenofile P [--qtl-fam-side first|second|both] [--qtl-cell parent|pair] [--qtl-covariates, --qtl-permutations, --qtl-seed]]
//            [--qtlhap F --phenofile P [--qtl-hap-by haplotype|founder|line] [--qtl-covariates, --qtl-permutations, --qtl-seed]]
//            [--qtlvc F --phenofile P [--qtl-vc-by haplotype|founder|line] [--qtl-covariates, --qtl-permutations, --qtl-seed]]
//            [--qtlimp F --phenofile P [--qtl-imp-draws D] [--qtl-imp-seed S] [--qtl-covariates, --qtl-permutations, --qtl-seed, --qtl-additive]]
//            [--remap F [--remap-iterations K]]
// Flag names and semantics follow main() (cnF2freq.cpp:7954-7972, 8083-8195): postmarkerdata, an optional
// --deserialize of an earlier dump, then --count rounds of which the first only dumps and every later one runs a
// haplotyping sweep (doit) before its dump.  Rows of the last round go to --output, earlier ones to stdout; every
// round's dump, and the FIRST PASS / SKEWNESS PASS lines of the last one, go to --output (cnF2freq.cpp:8166-8186,
// 6259, 6351).  Per chromosome and analysed individual the output is "name:chrom", one row per marker of the
// allele-2 dosage posterior ("%.5lf" tab separated, genotypereporter, cnF2freq.cpp:3499-3538) and a blank line
// (cnF2freq.cpp:6183-6188).
//
// --gpus N (not a flag of the reference, whose MPI code is dead: cnF2freq.cpp:5297-5299, 6245-6254): the process reads the
// files, forks N ranks -- before anything has touched a GPU --, rank r takes GPU r, its block of the analysed individuals and
// the records it owns (cnf2_partition.h), the ranks exchange through shared memory (cnf2_shm_transport.h), and rank 0
// writes ONE output in the order of a single-GPU run: the other ranks' rows reach it through files in --tmppath.
//
// --crossovers F / --remap F (not flags of the reference, whose DOREMAPDISTANCES path is compiled out): after the last round,
// the crossover posteriors of every analysed individual (cnf2_sweep_crossovers; per chromosome and individual "name:chrom",
// one "%.5lf" tab-separated line of the 6 meioses per marker, a blank line) and / or K EM steps of the marker map
// (cnf2_remap.h) written as a .map file that is read back and checked.  The summed log-likelihood of every step goes to
// stderr; --output is the same with or without these flags.  Single GPU only.
//
// --viterbi F (not a flag of the reference): after the last round, and before a --remap changes the map, the MAP
// inheritance path of every analysed individual (cnf2_sweep_viterbi): per chromosome and individual a header
// "name:chrom<TAB>s*<TAB>log posterior of the path" ("%.6lf"; "-<TAB>-" where the individual is skipped), one line per
// marker of the 6 state bits as 0 / 1 in the column order of --crossovers ("-" where skipped), a blank line.  --output is
// the same with or without it.  Single GPU only.
//
// --sample F [--draws K] [--seed S] (not flags of the reference): after the last round, and before a --remap changes the
// map, K (1 .. 1024, default 1) inheritance paths of every analysed individual drawn from the posterior with seed S
// (default 0; cnf2_sweep_sample).  Per chromosome, individual and draw a header "name:chrom<TAB>k<TAB>s<TAB>logp" (s the
// drawn shift mode, logp "%.6lf" the log posterior probability of the drawn (mode, path); "-<TAB>-" where the individual is
// skipped), one line per marker of the 6 state bits as for --viterbi, a blank line.  --output is the same with or without
// it.  Single GPU only.
//
// --place F --place-genfile G --place-markers Q (not flags of the reference): after the last round, and before a --remap
// changes the map, where Q markers that are not on the map go (cnf2_sweep_place).  G is a genotype file in the readers'
// format with Q markers per individual, read against the same pedfile.  F holds one line per candidate,
// "index<TAB>chrom<TAB>marker<TAB>pos<TAB>LOD<TAB>support_lo<TAB>support_hi<TAB>n_zero": the candidate (from 0), the
// chromosome (from 1), map index (from 0) and position of the best marker among those at which the fewest individuals are
// impossible, the LOD there against "unlinked", the positions that bound the contiguous stretch within 1 LOD of it on that
// chromosome, and that fewest number; after a blank line the LOD at every marker of the map, one "%.5lf" tab-separated
// line per candidate.  --output is the same with or without it.  Single GPU only.
//
// --loo F [--loo-threshold X] (not flags of the reference): after the last round, and before a --remap changes the map,
// the leave-one-marker-out costs of the last round's state (cnf2_sweep_loo).  F holds one line per marker,
// "chrom<TAB>pos<TAB>contributors<TAB>mean cost<TAB>LOD": the chromosome (from 1), the position, the individuals with a
// likelihood on that chromosome, the mean over them of the cost in nats of their data at the marker given the rest of the
// chromosome ("%.5lf"; "-" where nobody contributes), and the LOD of the marker's own position against "off the map"; after
// a blank line the cells whose cost is at least X nats (default 5), "name<TAB>chrom<TAB>marker<TAB>pos<TAB>cost<TAB>unlinked"
// with the marker's map index (from 0) and the cost of the same data with the marker off the map, by individual, then
// marker.  --output is the same with or without it.  Single GPU only.
//
// --descent F (not a flag of the reference): after the last round, like --origins, the descent rows of the last round's state
// (cnf2_sweep_descent): from which grandparent and which of its strands each allele descends.  Per chromosome and analysed
// individual a header "name:chrom", then one line per marker of the eight probabilities ("%.6lf", tab separated: the first
// parent's side, classes 2 w + b = 0..3 -- that parent's par[.][w], strand b as the grandparent's record labels it -- then
// the second parent's side; eight "-" where the individual is skipped on the chromosome), then a blank line.  After the last
// individual one line per chromosome, "chrom<TAB>contributors".  --output is the same with or without it.  Single GPU only.
//
// --origins F (not a flag of the reference): after the last round, and before a --remap changes the map, the grandparental
// origin probabilities of the last round's state (cnf2_sweep_origins).  Per chromosome and analysed individual a header
// "name:chrom", then one line per marker of the four probabilities ("%.6lf", tab separated, k = 0..3: the alleles from the
// first / second parent descend from those parents' first-first, second-first, first-second, second-second parent; four
// "-" where the individual is skipped on the chromosome), then a blank line.  After the last individual one line per marker,
// "chrom<TAB>pos<TAB>contributors<TAB>" and the four column sums ("%.5lf"): the expected class counts.  --output is the
// same with or without it.  Single GPU only.
//
// --qtl F --phenofile P (not flags of the reference): after the last round, and before a --remap changes the map, a QTL scan
// of the last round's state (cnf2_sweep_qtl: Haley-Knott regression on the origin rows).  P is a whitespace table: a header
// "id name...", then one line per individual keyed by the pedigree file's names; NA or - is a missing value.  Every column
// is a trait unless --qtl-covariates names it (fixed effects, at most 8).  Analysed individuals that are absent from P, or
// lack a covariate, are not used; a trait's missing values leave their individuals out of that trait's scan.  A name in P
// that the pedigree does not know, or a covariate that P does not have, is an error that names it.  F: per marker
// "chrom<TAB>pos<TAB>n<TAB>rank" (n and rank of the first trait's individuals), then per trait "<TAB>LOD<TAB>a<TAB>d" ("%.5lf",
// "-" for the effect of a dropped column); with --qtl-permutations K > 0, after a blank line, per trait
// "name<TAB>5 %<TAB>1 %": the genome-wide thresholds from K permutations of the null model's residuals, made from
// --qtl-seed by the rule of cnf2freq_amd/qtl.py (cnf2h_qtl_permutations).  --qtl-additive drops the dominance column.
// --qtl2 F [--qtl2-every S] (with --phenofile and the --qtl-* options; not flags of the reference): the two-QTL pair scan
// (cnf2_qtl_scan2) of every S-th marker of each chromosome, from its first (S = 1 by default; at most 4096 loci), after
// --qtl where both are given and on the same sweep's rows.  Covariates: at most 6.  F is described at qtl2_scan below.
// --qtl2-linked (only with --qtl2): the full model on the pairs of one chromosome too, from one pair sweep of the selected
// loci (cnf2_sweep_pairs, cnf2_qtl_scan2_linked).
// --qtlx F [--qtl-imprint] [--qtl-interactive name,name] (with --phenofile and the --qtl-* options; not flags of the
// reference): the extended single-locus scan (cnf2_qtl_scanx) -- per marker the nested models Mendelian (a, d), imprinting
// (+ i, with --qtl-imprint) and interaction (+ the products of the effects with the named covariates, which must be among
// --qtl-covariates and are moved to the front of them) -- after --qtl and --qtl2 where they are given, on the same sweep's
// rows.  The design takes at most 15 columns.  F is described at qtlx_scan below.
// --qtlcof F --qtl-cofactors i,j,k [--qtl-window X] (with --phenofile and the --qtl-* options; not flags of the reference):
// the cofactor scan (cnf2_qtl_scan_cof: composite interval mapping) -- every marker fitted together with the markers i, j, k
// (map indices from 0, as the other files print them), each of which is left out of the design within X map units of itself
// (default 0: at its own position only) -- after the other scans where they are given, on the same sweep's rows.  The design
// takes at most 15 columns: six cofactors less one per two covariates, thirteen with --qtl-additive.  F is described at
// qtlcof_scan below.
// --qtlboot F --qtl-boot-chrom C [--qtl-boot-replicates B] (with --phenofile, --qtl-covariates, --qtl-seed and
// --qtl-additive; not flags of the reference): the bootstrap of the scan on chromosome C (from 1, as the files print it) with
// B replicates (default 1000; cnf2_qtl_scan_boot) for the confidence interval of a QTL's position, after the other scans
// where they are given, on the same sweep's rows.  F is described at qtlboot_scan below.
// --qtlmv F [--qtl-traits name,name,..] (with --phenofile and --qtl-covariates, --qtl-permutations, --qtl-seed, --qtl-additive;
// not flags of the reference): the multi-trait scan (cnf2_qtl_scan_mv) -- the joint LOD of the named traits (default: every
// trait of the table; 16 at most) at every marker, on the individuals that have all of them -- after the other scans where
// they are given, on the same sweep's rows.  F is described at qtlmv_scan below.
// --qtlfam F [--qtl-fam-side first|second|both] [--qtl-cell parent|pair] (with --phenofile and --qtl-covariates,
// --qtl-permutations, --qtl-seed; not flags of the reference): the within-family scan (cnf2_qtl_scan_fam) -- a mean per
// cell and a substitution effect per F1 parent on the side -- after the scans above where they are given, on the same
// sweep's rows.  F is described at qtlfam_scan below.
// --qtlimp F [--qtl-imp-draws D] [--qtl-imp-seed S] (with --phenofile and --qtl-covariates, --qtl-permutations, --qtl-seed,
// --qtl-additive; not flags of the reference): the multiple-imputation scan (cnf2_qtl_scan_imp) -- --qtl's model on D
// (default 16, at most 1024) inheritance paths per individual drawn from the posterior with seed S (default 0;
// cnf2_sweep_sample), combined on the likelihood scale -- after the other scans, on a sampling sweep of its own.  F has the
// format of --qtl's file.
// --output is the same with or without it.  Single GPU only.
//
// Everything numeric goes through the C ABI of include/cnf2hip.h (host bookkeeping in cnf2_engine.cpp); this program
// has no compute path of its own and fails if no GPU is present.  Out of scope: the toulbar2
// bridge and the haplotype inversions it decides, all non-PlantImpute readers.
#include <signal.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <dirent.h>
#include <sys/prctl.h>
#include <sys/wait.h>
#include <unistd.h>

#include <algorithm>
#include <chrono>
#include <string>
#include <vector>

#include "cnf2_engine.h"
#include "cnf2_qtl_host.h"
#include "../cnf2_qtlx.h"
#include "../cnf2_qtlem.h"
#include "../cnf2_qtlbin.h"
#include "../cnf2_qtlvar.h"
#include "../cnf2_qtlsurv.h"
#include "../cnf2_qtlmv.h"
#include "cnf2_readers.h"
#include "cnf2_rccl_transport.h"
#include "cnf2_remap.h"
#include "cnf2_shm_transport.h"
#include "cnf2hip.h"

using namespace cnf2host;

struct Options {
    std::string mapfile, pedfile, genfile, output, deserialize, tmppath = ".";
    int         count = 3;          // cnF2freq.cpp:7961
    int         limit = 1000000;    // INDCOUNT (settings.h:9)
    int         capmarker = 0;
    bool        quiet = false;
    bool        merge_modes = true;   // CNF2_MERGE_MODES: exact, faster for F2-type pedigrees (include/cnf2hip.h)
    bool        normalise = false;    // rows as the reporter leaves them: raw class sums (cnF2freq.cpp:3523 has the
                                      // division by probsum commented out); --normalise divides each row by its sum
    bool        preprocess = true;    // --no-preprocess: skip postmarkerdata      } parity aids, not reference modes:
    bool        update = true;        // --no-update: sweeps without the updates    } every round repeats the same sweep
    bool        dump_all = true;      // --dump-last-only: large runs
    bool        rows_all = true;      // --rows-last-only: large runs (rows of non-final rounds are not formatted)
    bool        parse_only = false;   // print the parsed tables and stop (no GPU needed; used by tests)
    int         gpus = 1;             // --gpus N: N ranks, one GPU each
    bool        single_device = false;   // --single-device: every rank on GPU 0 (rehearsal of --gpus N on a one-GPU box)
    std::string transport;               // --transport rccl|shm: what the ranks exchange through (default: rccl when every rank has
                                         // a GPU of its own, shm -- staging through a shared region on the host -- with --single-device)
    bool        rccl_selftest = false;   // --rccl-selftest: the RCCL transport's collectives with a world of one on GPU 0, then stop
    std::string crossovers;              // --crossovers F: crossover posteriors of the last round's state
    std::string viterbi;                 // --viterbi F: MAP inheritance paths of the last round's state
    std::string sample;                  // --sample F: inheritance paths drawn from the posterior of the last round's state
    int         draws = 1;               // --draws K
    unsigned long long seed = 0;         // --seed S
    bool        draws_set = false, seed_set = false;
    std::string place, place_genfile;    // --place F --place-genfile G: where the Q markers of G go on the map
    int         place_markers = 0;       // --place-markers Q
    std::string loo;                     // --loo F: leave-one-marker-out costs of the last round's state
    double      loo_threshold = 5.0;     // --loo-threshold X: cells at or above X nats are listed
    bool        loo_threshold_set = false;
    std::string origins;                 // --origins F: grandparental origin probabilities of the last round's state
    std::string descent;                 // --descent F: descent rows (grandparent and strand) of the last round's state
    std::string qtl, phenofile;          // --qtl F --phenofile P: QTL scan of the last round's state
    std::string qtl_covariates;          // --qtl-covariates name,name
    int         qtl_permutations = 0;    // --qtl-permutations K
    unsigned long long qtl_seed = 0;     // --qtl-seed S
    bool        qtl_additive = false;    // --qtl-additive
    bool        qtl_extra_set = false;   // one of the four above was given
    std::string qtl2;                    // --qtl2 F: pair scan of the last round's state (with --phenofile and the --qtl-* options)
    int         qtl2_every = 1;          // --qtl2-every S: every S-th marker of each chromosome, from its first
    bool        qtl2_every_set = false;
    bool        qtl2_linked = false;     // --qtl2-linked: the full model on the pairs of one chromosome too (cnf2_sweep_pairs, cnf2_qtl_scan2_linked)
    std::string qtlx;                    // --qtlx F: extended single-locus scan (with --phenofile and the --qtl-* options)
    bool        qtl_imprint = false;     // --qtl-imprint
    std::string qtl_interactive;         // --qtl-interactive name,name
    bool        qtlx_extra_set = false;  // one of the two above was given
    bool        qtl_interactive_set = false;
    std::string qtlem;                   // --qtlem F: maximum-likelihood scan (with --phenofile and the --qtl-* options, --qtl-imprint)
    int         qtlem_iterations = 1000; // --qtl-em-iterations
    double      qtlem_tol = 1e-6;        // --qtl-em-tol
    bool        qtlem_extra_set = false; // one of the two above was given
    std::string qtlbin;                  // --qtlbin F: binary-trait scan (with --phenofile and the --qtl-* options, --qtl-imprint)
    int         qtlbin_iterations = 50;  // --qtl-binary-iterations
    double      qtlbin_tol = 1e-7;       // --qtl-binary-tol
    bool        qtlbin_extra_set = false; // one of the two above was given
    std::string qtlvar;                  // --qtlvar F: variance-QTL scan (with --phenofile and the --qtl-* options, --qtl-imprint)
    std::string qtlvar_covariates;       // --qtl-var-covariates: names among --qtl-covariates, the variance design's
    int         qtlvar_iterations = 50;  // --qtl-var-iterations
    double      qtlvar_tol = 1e-7;       // --qtl-var-tol
    bool        qtlvar_extra_set = false; // one of the three above was given
    std::vector<int> qtlvar_cov_cols;    // columns of pheno: the variance covariates first, then the other covariates
    int         qtlvar_n_var = 0;
    std::vector<int> qtlbin_trait_cols;  // columns of pheno: the traits whose values are all 0 or 1
    std::string qtlsurv;                 // --qtlsurv F: survival-trait scan (with --phenofile, the two column names and the --qtl-* options)
    std::string qtlsurv_time, qtlsurv_status;   // --qtl-surv-time, --qtl-surv-status: column names
    int         qtlsurv_iterations = 50; // --qtl-surv-iterations
    double      qtlsurv_tol = 1e-7;      // --qtl-surv-tol
    bool        qtlsurv_extra_set = false; // one of the four above was given
    int         qtlsurv_time_col = -1, qtlsurv_status_col = -1;   // columns of pheno
    std::string qtlcof;                  // --qtlcof F: cofactor scan (with --phenofile and the --qtl-* options)
    std::string qtl_cofactors;           // --qtl-cofactors i,j,k: map indices, from 0
    double      qtl_window = 0.0;        // --qtl-window X: a cofactor is left out within X map units of itself
    bool        qtlcof_extra_set = false; // one of the two above was given
    std::vector<int32_t> qtlcof_cof;     // the cofactors, ascending
    std::string qtlboot;                 // --qtlboot F: bootstrap of the scan (with --phenofile, --qtl-covariates, --qtl-seed, --qtl-additive)
    int         qtl_boot_chrom = 0;      // --qtl-boot-chrom C: the chromosome, from 1
    int         qtl_boot_replicates = 1000;   // --qtl-boot-replicates B
    bool        qtlboot_extra_set = false; // one of the two above was given
    std::string qtlmv;                   // --qtlmv F: multi-trait scan (with --phenofile and the shared --qtl-* options)
    std::string qtl_traits;              // --qtl-traits name,name,..: the traits scanned jointly (default: all)
    bool        qtl_traits_set = false;
    std::vector<int> qtlmv_trait_cols;   // columns of pheno, in the order they are scanned
    std::string qtlfam;                  // --qtlfam F: within-family scan (with --phenofile, --qtl-covariates, --qtl-permutations, --qtl-seed)
    std::string qtlhap;                  // --qtlhap F: founder-haplotype scan (with --phenofile, --qtl-covariates, --qtl-permutations, --qtl-seed)
    std::string qtl_hap_by = "haplotype"; // --qtl-hap-by haplotype|founder|line: what a model column stands for
    bool        qtlhap_extra_set = false;
    std::string qtlvc;                   // --qtlvc F: variance-component scan (with --phenofile, --qtl-covariates, --qtl-permutations, --qtl-seed)
    std::string qtl_vc_by = "haplotype"; // --qtl-vc-by haplotype|founder|line: what a random effect stands for
    bool        qtlvc_extra_set = false;
    std::string qtl_fam_side = "both";   // --qtl-fam-side first|second|both
    std::string qtl_cell = "pair";       // --qtl-cell parent|pair: a mean per parent on the side, or per pair of parents
    bool        qtlfam_extra_set = false; // one of the two above was given
    std::string qtlimp;                  // --qtlimp F: multiple-imputation scan (with --phenofile and the shared --qtl-* options)
    int         qtl_imp_draws = 16;      // --qtl-imp-draws D
    unsigned long long qtl_imp_seed = 0; // --qtl-imp-seed S
    bool        qtlimp_extra_set = false; // one of the two above was given
    std::vector<int> qtlx_cov_cols;      // columns of pheno: the interactive covariates first, then the others
    int         qtlx_n_int = 0;
    PhenoTable  pheno;                   // P as read (main, before any rank starts)
    std::vector<int> qtl_cov_cols, qtl_trait_cols;     // columns of pheno
    std::string remap;                   // --remap F: the map after --remap-iterations EM steps
    int         remap_iterations = 1;
    bool        remap_iterations_set = false;
};

static bool parse(int argc, char** argv, Options& o)
{
    for (int i = 1; i < argc; i++) {
        std::string a = argv[i], v;
        bool        has = false;
        size_t      eq = a.find('=');
        if (a.rfind("--", 0) == 0 && eq != std::string::npos) {
            v   = a.substr(eq + 1);
            a   = a.substr(0, eq);
            has = true;
        }
        auto val = [&]() -> std::string {
            if (has) return v;
            if (i + 1 >= argc) {
                fprintf(stderr, "missing value for %s\n", a.c_str());
                exit(2);
            }
            return argv[++i];
        };
        if (a == "--mapfile") o.mapfile = val();
        else if (a == "--pedfile") o.pedfile = val();
        else if (a == "--genfile") o.genfile = val();
        else if (a == "--output") o.output = val();
        else if (a == "--deserialize") o.deserialize = val();
        else if (a == "--tmppath") o.tmppath = val();
        else if (a == "--count") o.count = atoi(val().c_str());
        else if (a == "--limit") o.limit = atoi(val().c_str());
        else if (a == "--capmarker") o.capmarker = atoi(val().c_str());
        else if (a == "--quiet") o.quiet = true;
        else if (a == "--no-merge-modes") o.merge_modes = false;
        else if (a == "--normalise") o.normalise = true;
        else if (a == "--no-preprocess") o.preprocess = false;
        else if (a == "--no-update") o.update = false;
        else if (a == "--dump-last-only") o.dump_all = false;
        else if (a == "--rows-last-only") o.rows_all = false;
        else if (a == "--parse-only") o.parse_only = true;
        else if (a == "--gpus") o.gpus = atoi(val().c_str());
        else if (a == "--single-device") o.single_device = true;
        else if (a == "--transport") o.transport = val();
        else if (a == "--rccl-selftest") o.rccl_selftest = true;
        else if (a == "--crossovers") o.crossovers = val();
        else if (a == "--viterbi") o.viterbi = val();
        else if (a == "--sample") o.sample = val();
        else if (a == "--draws") {
            o.draws     = atoi(val().c_str());
            o.draws_set = true;
        }
        else if (a == "--seed") {
            o.seed     = strtoull(val().c_str(), nullptr, 0);
            o.seed_set = true;
        }
        else if (a == "--place") o.place = val();
        else if (a == "--place-genfile") o.place_genfile = val();
        else if (a == "--place-markers") o.place_markers = atoi(val().c_str());
        else if (a == "--loo") o.loo = val();
        else if (a == "--loo-threshold") {
            const std::string t = val();
            char*             end = nullptr;
            o.loo_threshold     = strtod(t.c_str(), &end);
            o.loo_threshold_set = true;
            if (t.empty() || *end != 0 || o.loo_threshold != o.loo_threshold) {
                fprintf(stderr, "--loo-threshold needs a number, not \"%s\"\n", t.c_str());
                exit(2);
            }
        }
        else if (a == "--origins") o.origins = val();
        else if (a == "--descent") o.descent = val();
        else if (a == "--qtl") o.qtl = val();
        else if (a == "--qtl2") o.qtl2 = val();
        else if (a == "--qtlx") o.qtlx = val();
        else if (a == "--qtl-imprint") o.qtl_imprint = o.qtlx_extra_set = true;
        else if (a == "--qtl-interactive") {
            o.qtl_interactive = val();
            o.qtlx_extra_set  = o.qtl_interactive_set = true;
        }
        else if (a == "--qtlem") o.qtlem = val();
        else if (a == "--qtl-em-iterations") {
            o.qtlem_iterations = atoi(val().c_str());
            o.qtlem_extra_set  = true;
        }
        else if (a == "--qtl-em-tol") {
            const std::string t = val();
            char*             end = nullptr;
            o.qtlem_tol       = strtod(t.c_str(), &end);
            o.qtlem_extra_set = true;
            if (t.empty() || *end != 0 || !std::isfinite(o.qtlem_tol)) {
                fprintf(stderr, "--qtl-em-tol needs a finite number, not \"%s\"\n", t.c_str());
                exit(2);
            }
        }
        else if (a == "--qtlcof") o.qtlcof = val();
        else if (a == "--qtl-cofactors") {
            o.qtl_cofactors    = val();
            o.qtlcof_extra_set = true;
        }
        else if (a == "--qtl-window") {
            const std::string t = val();
            char*             end = nullptr;
            o.qtl_window       = strtod(t.c_str(), &end);
            o.qtlcof_extra_set = true;
            if (t.empty() || *end != 0 || !std::isfinite(o.qtl_window)) {
                fprintf(stderr, "--qtl-window needs a finite number, not \"%s\"\n", t.c_str());
                exit(2);
            }
        }
        else if (a == "--qtlboot") o.qtlboot = val();
        else if (a == "--qtlmv") o.qtlmv = val();
        else if (a == "--qtlimp") o.qtlimp = val();
        else if (a == "--qtlfam") o.qtlfam = val();
        else if (a == "--qtlhap") o.qtlhap = val();
        else if (a == "--qtlvc") o.qtlvc = val();
        else if (a == "--qtl-vc-by") {
            o.qtl_vc_by       = val();
            o.qtlvc_extra_set = true;
        }
        else if (a == "--qtl-hap-by") {
            o.qtl_hap_by       = val();
            o.qtlhap_extra_set = true;
        }
        else if (a == "--qtl-fam-side") {
            o.qtl_fam_side     = val();
            o.qtlfam_extra_set = true;
        }
        else if (a == "--qtl-cell") {
            o.qtl_cell         = val();
            o.qtlfam_extra_set = true;
        }
        else if (a == "--qtl-imp-draws") {
            o.qtl_imp_draws    = atoi(val().c_str());
            o.qtlimp_extra_set = true;
        }
        else if (a == "--qtl-imp-seed") {
            o.qtl_imp_seed     = strtoull(val().c_str(), nullptr, 0);
            o.qtlimp_extra_set = true;
        }
        else if (a == "--qtl-traits") {
            o.qtl_traits     = val();
            o.qtl_traits_set = true;
        }
        else if (a == "--qtl-boot-chrom") {
            o.qtl_boot_chrom    = atoi(val().c_str());
            o.qtlboot_extra_set = true;
        }
        else if (a == "--qtl-boot-replicates") {
            o.qtl_boot_replicates = atoi(val().c_str());
            o.qtlboot_extra_set   = true;
        }
        else if (a == "--qtlbin") o.qtlbin = val();
        else if (a == "--qtl-binary-iterations") {
            o.qtlbin_iterations = atoi(val().c_str());
            o.qtlbin_extra_set  = true;
        }
        else if (a == "--qtl-binary-tol") {
            const std::string t = val();
            char*             end = nullptr;
            o.qtlbin_tol       = strtod(t.c_str(), &end);
            o.qtlbin_extra_set = true;
            if (t.empty() || *end != 0 || !std::isfinite(o.qtlbin_tol)) {
                fprintf(stderr, "--qtl-binary-tol needs a finite number, not \"%s\"\n", t.c_str());
                exit(2);
            }
        }
        else if (a == "--qtlvar") o.qtlvar = val();
        else if (a == "--qtl-var-covariates") {
            o.qtlvar_covariates = val();
            o.qtlvar_extra_set  = true;
        }
        else if (a == "--qtl-var-iterations") {
            o.qtlvar_iterations = atoi(val().c_str());
            o.qtlvar_extra_set  = true;
        }
        else if (a == "--qtl-var-tol") {
            const std::string t = val();
            char*             end = nullptr;
            o.qtlvar_tol       = strtod(t.c_str(), &end);
            o.qtlvar_extra_set = true;
            if (t.empty() || *end != 0 || !std::isfinite(o.qtlvar_tol)) {
                fprintf(stderr, "--qtl-var-tol needs a finite number, not \"%s\"\n", t.c_str());
                exit(2);
            }
        }
        else if (a == "--qtlsurv") o.qtlsurv = val();
        else if (a == "--qtl-surv-time") {
            o.qtlsurv_time      = val();
            o.qtlsurv_extra_set = true;
        }
        else if (a == "--qtl-surv-status") {
            o.qtlsurv_status    = val();
            o.qtlsurv_extra_set = true;
        }
        else if (a == "--qtl-surv-iterations") {
            o.qtlsurv_iterations = atoi(val().c_str());
            o.qtlsurv_extra_set  = true;
        }
        else if (a == "--qtl-surv-tol") {
            const std::string t = val();
            char*             end = nullptr;
            o.qtlsurv_tol       = strtod(t.c_str(), &end);
            o.qtlsurv_extra_set = true;
            if (t.empty() || *end != 0 || !std::isfinite(o.qtlsurv_tol)) {
                fprintf(stderr, "--qtl-surv-tol needs a finite number, not \"%s\"\n", t.c_str());
                exit(2);
            }
        }
        else if (a == "--qtl2-linked") o.qtl2_linked = true;
        else if (a == "--qtl2-every") {
            o.qtl2_every     = atoi(val().c_str());
            o.qtl2_every_set = true;
        }
        else if (a == "--phenofile") o.phenofile = val();
        else if (a == "--qtl-covariates") {
            o.qtl_covariates = val();
            o.qtl_extra_set  = true;
        }
        else if (a == "--qtl-permutations") {
            o.qtl_permutations = atoi(val().c_str());
            o.qtl_extra_set    = true;
        }
        else if (a == "--qtl-seed") {
            o.qtl_seed      = strtoull(val().c_str(), nullptr, 0);
            o.qtl_extra_set = true;
        }
        else if (a == "--qtl-additive") o.qtl_additive = o.qtl_extra_set = true;
        else if (a == "--remap") o.remap = val();
        else if (a == "--remap-iterations") {
            o.remap_iterations = atoi(val().c_str());
            o.remap_iterations_set = true;
        }
        else {
            fprintf(stderr, "unsupported option %s (this build covers the PlantImpute path only)\n", a.c_str());
            return false;
        }
    }
    return true;
}

static void crossovers_and_remap(const Options& opt, Pedigree& P, cnf2_ctx* ctx);
static void viterbi_paths(const Options& opt, Pedigree& P, cnf2_ctx* ctx);
static void sample_paths(const Options& opt, Pedigree& P, cnf2_ctx* ctx);
static void place_markers(const Options& opt, Pedigree& P, cnf2_ctx* ctx);
static void loo_costs(const Options& opt, Pedigree& P, cnf2_ctx* ctx);
static void origin_rows(const Options& opt, Pedigree& P, cnf2_ctx* ctx);
static void descent_rows(const Options& opt, Pedigree& P, cnf2_ctx* ctx);
static void qtl_scan(const Options& opt, Pedigree& P, cnf2_ctx* ctx);
static void qtl2_scan(const Options& opt, Pedigree& P, cnf2_ctx* ctx, bool rows_kept);
static void qtlx_scan(const Options& opt, Pedigree& P, cnf2_ctx* ctx, bool rows_kept);
static void qtlem_scan(const Options& opt, Pedigree& P, cnf2_ctx* ctx, bool rows_kept);
static void qtlbin_scan(const Options& opt, Pedigree& P, cnf2_ctx* ctx, bool rows_kept);
static void qtlvar_scan(const Options& opt, Pedigree& P, cnf2_ctx* ctx, bool rows_kept);
static void qtlsurv_scan(const Options& opt, Pedigree& P, cnf2_ctx* ctx, bool rows_kept);
static void qtlcof_scan(const Options& opt, Pedigree& P, cnf2_ctx* ctx, bool rows_kept);
static void qtlboot_scan(const Options& opt, Pedigree& P, cnf2_ctx* ctx, bool rows_kept);
static void qtlmv_scan(const Options& opt, Pedigree& P, cnf2_ctx* ctx, bool rows_kept);
static void qtlimp_scan(const Options& opt, Pedigree& P, cnf2_ctx* ctx);
static void qtlfam_scan(const Options& opt, Pedigree& P, cnf2_ctx* ctx, bool rows_kept);
static void qtlhap_scan(const Options& opt, Pedigree& P, cnf2_ctx* ctx);
static void qtlvc_scan(const Options& opt, Pedigree& P, cnf2_ctx* ctx);

// One rank of a run: GPU `rank` (or 0), the whole pedigree, its block of the analysed individuals.  rank 0 writes the output.
static int run_rank(const Options& opt, Pedigree& P, int rank, int world, ShmRegion* region)
{
    if (rank > 0) {
        // what is identical on every rank (progress lines, pass lines, dumps) is written by rank 0 only
        if (!freopen("/dev/null", "w", stdout)) return 3;
    }
    cnf2_ctx* ctx = nullptr;
    const int device = (world > 1 && !opt.single_device) ? rank : 0;
    if (cnf2_ctx_create(device, &ctx) != CNF2_OK) {
        fprintf(stderr, "cnf2_ctx_create(device %d): %s%s\n", device, cnf2_last_error(nullptr),
                world > 1 ? " (--gpus N needs N GPUs; --single-device rehearses it on one)" : "");
        if (world > 1) return 3;
        abort();
    }
    EngineOptions eo;
    eo.quiet = opt.quiet;
    eo.merge_modes = opt.merge_modes;
    eo.normalise = opt.normalise;
    eo.update = opt.update;
    eo.dump_all = opt.dump_all;
    if (world > 1) {
        eo.spool_dir = opt.tmppath;
        eo.spool_tag = "run" + std::to_string((long)getppid());       // every rank is a child of the process that read the files
    }
    ShmTransport  T;
    RcclTransport TR;
    const bool    use_rccl = world > 1 && (opt.transport.empty() ? !opt.single_device : opt.transport == "rccl");
    // any failure below the C ABI ends the run the way the reference ends on every failure (cnF2freq.cpp:21-25)
    try {
    Engine E(P, ctx, eo);
    E.upload();
    if (world > 1) {
        T.R = region;
        T.ctx = ctx;
        T.rank = rank;
        if (use_rccl) {
            if (TR.init(region, ctx, rank, world) != 0) return 4;
            E.set_partition(rank, world, RcclTransport::call, &TR);
        } else
            E.set_partition(rank, world, ShmTransport::call, &T);
        E.set_root_threads(host_threads() * world);          // rank 0 infers the genotypes for all while the others wait
    }
    if (opt.preprocess) E.postmarkerdata(opt.limit);                 // cnF2freq.cpp:8083-8085
    if (!opt.deserialize.empty() && !E.deserialize(opt.deserialize.c_str())) {
        fprintf(stderr, "cannot open %s\n", opt.deserialize.c_str());
        abort();
    }
    if (world > 1) {
        const Partition& Q = E.partition();
        if (rank == 0) fprintf(stderr, "transport: %s\n", use_rccl ? "RCCL in place on the exchange buffer" : "shared memory on the host");
        if (rank == 0) {
            size_t xb[4];
            E.exchange_bytes(xb);
            fprintf(stderr, "%d ranks: blocks", world);
            for (int r = 0; r < world; r++) fprintf(stderr, " [%d, %d)", Q.bounds[r], Q.bounds[r + 1]);
            fprintf(stderr, "; %zu shared records, %zu bytes exchanged per iteration\n", Q.n_shared, xb[3]);
        }
    }

    FILE* out = stdout;
    if (rank > 0) out = fopen("/dev/null", "w");
    else if (!opt.output.empty()) out = fopen(opt.output.c_str(), "w");
    if (!out) { fprintf(stderr, "cannot open output\n"); abort(); }

    for (int it = 0; it < opt.count; it++) {
        const bool early = it < 1;                       // cnF2freq.cpp:8131
        if (!early) {
            E.set_print_rows(opt.rows_all || it == opt.count - 1);
            E.iteration((it == opt.count - 1) ? out : stdout);
        }
        fflush(stdout);
        fflush(out);
        if (opt.dump_all || it == opt.count - 1) {
            const auto t0 = std::chrono::steady_clock::now();
            E.dump(out, opt.limit);                                              // (gathers the ranks' rows: every rank calls it)
            if (getenv("CNF2_TIMING") && rank == 0)
                fprintf(stderr, "  [write] dump of round %-3d                  %.3f s\n", it,
                        std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count());
        }
        fflush(stdout);
        fflush(out);
    }
    if (out != stdout) fclose(out);
    if (world == 1 && !opt.viterbi.empty()) viterbi_paths(opt, P, ctx);
    if (world == 1 && !opt.sample.empty()) sample_paths(opt, P, ctx);
    if (world == 1 && !opt.place.empty()) place_markers(opt, P, ctx);
    if (world == 1 && !opt.loo.empty()) loo_costs(opt, P, ctx);
    if (world == 1 && !opt.origins.empty()) origin_rows(opt, P, ctx);
    if (world == 1 && !opt.descent.empty()) descent_rows(opt, P, ctx);
    if (world == 1 && !opt.qtl.empty()) qtl_scan(opt, P, ctx);
    if (world == 1 && !opt.qtl2.empty()) qtl2_scan(opt, P, ctx, !opt.qtl.empty());
    if (world == 1 && !opt.qtlx.empty()) qtlx_scan(opt, P, ctx, !opt.qtl.empty() || !opt.qtl2.empty());
    if (world == 1 && !opt.qtlem.empty()) qtlem_scan(opt, P, ctx, !opt.qtl.empty() || !opt.qtl2.empty() || !opt.qtlx.empty());
    if (world == 1 && !opt.qtlbin.empty())
        qtlbin_scan(opt, P, ctx, !opt.qtl.empty() || !opt.qtl2.empty() || !opt.qtlx.empty() || !opt.qtlem.empty());
    if (world == 1 && !opt.qtlcof.empty())
        qtlcof_scan(opt, P, ctx, !opt.qtl.empty() || !opt.qtl2.empty() || !opt.qtlx.empty() || !opt.qtlem.empty() || !opt.qtlbin.empty());
    if (world == 1 && !opt.qtlboot.empty())
        qtlboot_scan(opt, P, ctx, !opt.qtl.empty() || !opt.qtl2.empty() || !opt.qtlx.empty() || !opt.qtlem.empty() || !opt.qtlbin.empty() ||
                                      !opt.qtlcof.empty());
    if (world == 1 && !opt.qtlmv.empty())
        qtlmv_scan(opt, P, ctx, !opt.qtl.empty() || !opt.qtl2.empty() || !opt.qtlx.empty() || !opt.qtlem.empty() || !opt.qtlbin.empty() ||
                                    !opt.qtlcof.empty() || !opt.qtlboot.empty());
    if (world == 1 && !opt.qtlsurv.empty())
        qtlsurv_scan(opt, P, ctx, !opt.qtl.empty() || !opt.qtl2.empty() || !opt.qtlx.empty() || !opt.qtlem.empty() || !opt.qtlbin.empty() ||
                                      !opt.qtlcof.empty() || !opt.qtlboot.empty() || !opt.qtlmv.empty());
    if (world == 1 && !opt.qtlvar.empty())
        qtlvar_scan(opt, P, ctx, !opt.qtl.empty() || !opt.qtl2.empty() || !opt.qtlx.empty() || !opt.qtlem.empty() || !opt.qtlbin.empty() ||
                                     !opt.qtlcof.empty() || !opt.qtlboot.empty() || !opt.qtlmv.empty() || !opt.qtlsurv.empty());
    if (world == 1 && !opt.qtlfam.empty())
        qtlfam_scan(opt, P, ctx, !opt.qtl.empty() || !opt.qtl2.empty() || !opt.qtlx.empty() || !opt.qtlem.empty() || !opt.qtlbin.empty() ||
                                     !opt.qtlcof.empty() || !opt.qtlboot.empty() || !opt.qtlmv.empty() || !opt.qtlsurv.empty() || !opt.qtlvar.empty());
    if (world == 1 && !opt.qtlhap.empty()) qtlhap_scan(opt, P, ctx);
    if (world == 1 && !opt.qtlvc.empty()) qtlvc_scan(opt, P, ctx);
    if (world == 1 && !opt.qtlimp.empty()) qtlimp_scan(opt, P, ctx);
    if (world == 1 && (!opt.crossovers.empty() || !opt.remap.empty())) crossovers_and_remap(opt, P, ctx);
    } catch (const EngineError& e) {
        fprintf(stderr, "%s\n", e.what());
        if (world > 1) return 4;                          // the parent stops the other ranks and aborts
        abort();
    }
    cnf2_ctx_destroy(ctx);
    return 0;
}

// summed window log-likelihood of a sweep (the quantity an EM step of the map cannot decrease): loglik of every
// (individual, chromosome) that is not skipped (cnF2freq.cpp:5403)
static double summed_loglik(const std::vector<double>& ll)
{
    double s = 0.0;
    for (double v : ll)
        if (!(v != v) && !(v < (double)CNF2_MINFACTOR)) s += v;
    return s;
}

// --crossovers / --remap after the last round (single GPU): the context holds the last round's rows
static void crossovers_and_remap(const Options& opt, Pedigree& P, cnf2_ctx* ctx)
{
    const int N = (int)P.dous.size(), M = P.n_markers(), C = (int)P.chromstarts.size() - 1;
    std::vector<double>  f((size_t)N * C * 8), ll((size_t)N * C), xs((size_t)M * 6);
    std::vector<int32_t> cnt(C);
    auto sweep = [&](double* xo) {
        if (cnf2_sweep_crossovers(ctx, 0, N, f.data(), ll.data(), xo, xs.data(), cnt.data(), 0) != CNF2_OK)
            throw EngineError(CNF2_ERR_STATE, std::string("cnf2_sweep_crossovers: ") + cnf2_last_error(ctx));
    };
    if (!opt.crossovers.empty()) {
        std::vector<double> xo((size_t)N * M * 6);
        sweep(xo.data());
        FILE* out = fopen(opt.crossovers.c_str(), "w");
        if (!out) throw EngineError(CNF2_ERR_STATE, "cannot write " + opt.crossovers);
        for (int c = 0; c < C; c++)
            for (int j = 0; j < N; j++) {
                fprintf(out, "%s:%d\n", P.inds[P.dous[j]].name.c_str(), c + 1);
                for (int m = P.chromstarts[c]; m < P.chromstarts[c + 1]; m++) {
                    const double* r = &xo[((size_t)j * M + m) * 6];
                    fprintf(out, "%.5lf\t%.5lf\t%.5lf\t%.5lf\t%.5lf\t%.5lf\n", r[0], r[1], r[2], r[3], r[4], r[5]);
                }
                fprintf(out, "\n");
            }
        if (fclose(out) != 0) throw EngineError(CNF2_ERR_STATE, "cannot write " + opt.crossovers);
    }
    if (opt.remap.empty()) return;
    std::vector<double> pos(P.pos.begin(), P.pos.end()), npos(M);
    const double genrec[3] = {-0.02, -0.02, -0.02};       // what the engine uploads (cnf2_upload_map with NULL)
    for (int k = 0; k <= opt.remap_iterations; k++) {
        sweep(nullptr);
        fprintf(stderr, "remap step %d: summed loglik %.10f\n", k, summed_loglik(ll));
        if (k == opt.remap_iterations) break;
        map_mstep(pos.data(), M, P.chromstarts.data(), C, genrec, xs.data(), cnt.data(), npos.data());
        pos.swap(npos);
        if (cnf2_upload_map(ctx, pos.data(), M, P.chromstarts.data(), C, nullptr) != CNF2_OK)
            throw EngineError(CNF2_ERR_STATE, std::string("cnf2_upload_map: ") + cnf2_last_error(ctx));
    }
    std::string err;
    if (!write_map_checked(opt.remap.c_str(), pos.data(), M, P.chromstarts.data(), C, &err)) throw EngineError(CNF2_ERR_STATE, err);
}

// --viterbi after the last round (single GPU): the context holds the last round's rows and the map they were swept with
static void viterbi_paths(const Options& opt, Pedigree& P, cnf2_ctx* ctx)
{
    const int N = (int)P.dous.size(), M = P.n_markers(), C = (int)P.chromstarts.size() - 1;
    std::vector<double>  f((size_t)N * C * 8), ll((size_t)N * C), lm((size_t)N * C * 8);
    std::vector<uint8_t> st((size_t)N * M);
    std::vector<int32_t> sh((size_t)N * C);
    if (cnf2_sweep_viterbi(ctx, 0, N, f.data(), ll.data(), lm.data(), st.data(), sh.data(), 0) != CNF2_OK)
        throw EngineError(CNF2_ERR_STATE, std::string("cnf2_sweep_viterbi: ") + cnf2_last_error(ctx));
    FILE* out = fopen(opt.viterbi.c_str(), "w");
    if (!out) throw EngineError(CNF2_ERR_STATE, "cannot write " + opt.viterbi);
    for (int c = 0; c < C; c++)
        for (int j = 0; j < N; j++) {
            const size_t e = (size_t)j * C + c;
            const int    s = sh[e];
            if (s < 0) fprintf(out, "%s:%d\t-\t-\n", P.inds[P.dous[j]].name.c_str(), c + 1);
            else fprintf(out, "%s:%d\t%d\t%.6lf\n", P.inds[P.dous[j]].name.c_str(), c + 1, s, lm[e * 8 + s] - ll[e]);
            for (int m = P.chromstarts[c]; m < P.chromstarts[c + 1]; m++) {
                const int g = st[(size_t)j * M + m];
                if (s < 0) fprintf(out, "-\t-\t-\t-\t-\t-\n");
                else fprintf(out, "%d\t%d\t%d\t%d\t%d\t%d\n", g & 1, (g >> 1) & 1, (g >> 2) & 1, (g >> 3) & 1, (g >> 4) & 1, (g >> 5) & 1);
            }
            fprintf(out, "\n");
        }
    if (fclose(out) != 0) throw EngineError(CNF2_ERR_STATE, "cannot write " + opt.viterbi);
}

// --sample after the last round (single GPU), like --viterbi
static void sample_paths(const Options& opt, Pedigree& P, cnf2_ctx* ctx)
{
    const int N = (int)P.dous.size(), M = P.n_markers(), C = (int)P.chromstarts.size() - 1, K = opt.draws;
    std::vector<double>  f((size_t)N * C * 8), ll((size_t)N * C), lp((size_t)N * K * C);
    std::vector<uint8_t> st((size_t)N * K * M);
    std::vector<int32_t> sh((size_t)N * K * C);
    if (cnf2_sweep_sample(ctx, 0, N, K, (uint64_t)opt.seed, f.data(), ll.data(), st.data(), sh.data(), lp.data(), 0) != CNF2_OK)
        throw EngineError(CNF2_ERR_STATE, std::string("cnf2_sweep_sample: ") + cnf2_last_error(ctx));
    FILE* out = fopen(opt.sample.c_str(), "w");
    if (!out) throw EngineError(CNF2_ERR_STATE, "cannot write " + opt.sample);
    for (int c = 0; c < C; c++)
        for (int j = 0; j < N; j++)
            for (int k = 0; k < K; k++) {
                const size_t d = (size_t)j * K + k, e = d * C + c;
                const int    s = sh[e];
                if (s < 0) fprintf(out, "%s:%d\t%d\t-\t-\n", P.inds[P.dous[j]].name.c_str(), c + 1, k);
                else fprintf(out, "%s:%d\t%d\t%d\t%.6lf\n", P.inds[P.dous[j]].name.c_str(), c + 1, k, s, lp[e]);
                for (int m = P.chromstarts[c]; m < P.chromstarts[c + 1]; m++) {
                    const int g = st[d * M + m];
                    if (s < 0) fprintf(out, "-\t-\t-\t-\t-\t-\n");
                    else fprintf(out, "%d\t%d\t%d\t%d\t%d\t%d\n", g & 1, (g >> 1) & 1, (g >> 2) & 1, (g >> 3) & 1, (g >> 4) & 1, (g >> 5) & 1);
                }
                fprintf(out, "\n");
            }
    if (fclose(out) != 0) throw EngineError(CNF2_ERR_STATE, "cannot write " + opt.sample);
}

// --place after the last round (single GPU), like --viterbi: the candidates' genotypes are read against the same pedfile
// into a pedigree of their own, whose individuals are matched to the run's by name (the context's rows: record r in row
// r + 1, row 0 blank; an individual the file does not mention has no data at the candidates)
static void place_markers(const Options& opt, Pedigree& P, cnf2_ctx* ctx)
{
    const int N = (int)P.dous.size(), M = P.n_markers(), C = (int)P.chromstarts.size() - 1, Q = opt.place_markers;
    Pedigree G;
    for (int q = 0; q < Q; q++) G.pos.push_back((double)q);
    G.chromstarts = {0, Q};
    FILE* f = fopen(opt.pedfile.c_str(), "rt");
    if (!read_alpha_ped(f, G)) throw EngineError(CNF2_ERR_STATE, "cannot read " + opt.pedfile);
    fclose(f);
    f = fopen(opt.place_genfile.c_str(), "rt");
    if (!read_alpha_gen(f, G)) throw EngineError(CNF2_ERR_STATE, "cannot read " + opt.place_genfile);
    fclose(f);
    const size_t R = P.inds.size(), per = (size_t)Q * 2;
    std::vector<uint8_t> ca((R + 1) * per, 0);
    std::vector<double>  cs((R + 1) * per, 0.0);
    for (size_t r = 0; r < R; r++) {
        const auto it = G.index.find(P.inds[r].name);
        if (it == G.index.end() || it->second < 0) continue;
        const Individual& I = G.inds[it->second];
        std::copy(I.allele.begin(), I.allele.end(), ca.begin() + (r + 1) * per);
        std::copy(I.sure.begin(), I.sure.end(), cs.begin() + (r + 1) * per);
    }
    std::vector<double>  fa((size_t)N * C * 8), ll((size_t)N * C), ps((size_t)Q * M), null(Q);
    std::vector<int32_t> nz((size_t)Q * M), cnt(C);
    if (cnf2_sweep_place(ctx, 0, N, Q, ca.data(), cs.data(), nullptr, fa.data(), ll.data(), nullptr, ps.data(), nz.data(),
                         null.data(), cnt.data(), 0) != CNF2_OK)
        throw EngineError(CNF2_ERR_STATE, std::string("cnf2_sweep_place: ") + cnf2_last_error(ctx));
    FILE* out = fopen(opt.place.c_str(), "w");
    if (!out) throw EngineError(CNF2_ERR_STATE, "cannot write " + opt.place);
    const double ln10 = 2.30258509299404568402, drop = 1.0;
    std::vector<double> lod((size_t)Q * M);
    for (int q = 0; q < Q; q++) {
        double*        L = &lod[(size_t)q * M];
        const int32_t* Z = &nz[(size_t)q * M];
        for (int m = 0; m < M; m++) L[m] = (ps[(size_t)q * M + m] - null[q]) / ln10;
        const int32_t fewest = *std::min_element(Z, Z + M);
        int best = -1, c = 0;
        for (int m = 0; m < M; m++)
            if (Z[m] == fewest && (best < 0 || L[m] > L[best])) best = m;
        while (P.chromstarts[c + 1] <= best) c++;
        auto inside = [&](int m) { return Z[m] == fewest && L[m] >= L[best] - drop; };
        int lo = best, hi = best;
        while (lo - 1 >= P.chromstarts[c] && inside(lo - 1)) lo--;
        while (hi + 1 < P.chromstarts[c + 1] && inside(hi + 1)) hi++;
        fprintf(out, "%d\t%d\t%d\t%.5lf\t%.5lf\t%.5lf\t%.5lf\t%d\n", q, c + 1, best, P.pos[best], L[best], P.pos[lo], P.pos[hi], (int)fewest);
    }
    fprintf(out, "\n");
    for (int q = 0; q < Q; q++)
        for (int m = 0; m < M; m++) fprintf(out, "%.5lf%c", lod[(size_t)q * M + m], m + 1 < M ? '\t' : '\n');
    if (fclose(out) != 0) throw EngineError(CNF2_ERR_STATE, "cannot write " + opt.place);
}

// --loo after the last round (single GPU), like --viterbi
static void loo_costs(const Options& opt, Pedigree& P, cnf2_ctx* ctx)
{
    const int N = (int)P.dous.size(), M = P.n_markers(), C = (int)P.chromstarts.size() - 1;
    std::vector<double>  f((size_t)N * C * 8), ll((size_t)N * C), loo((size_t)N * M), unl((size_t)N * M), ls(M), us(M);
    std::vector<int32_t> cnt(C);
    if (cnf2_sweep_loo(ctx, 0, N, f.data(), ll.data(), loo.data(), unl.data(), ls.data(), us.data(), cnt.data(), 0) != CNF2_OK)
        throw EngineError(CNF2_ERR_STATE, std::string("cnf2_sweep_loo: ") + cnf2_last_error(ctx));
    FILE* out = fopen(opt.loo.c_str(), "w");
    if (!out) throw EngineError(CNF2_ERR_STATE, "cannot write " + opt.loo);
    const double ln10 = 2.30258509299404568402;
    for (int c = 0; c < C; c++)
        for (int m = P.chromstarts[c]; m < P.chromstarts[c + 1]; m++) {
            if (cnt[c] > 0) fprintf(out, "%d\t%.5lf\t%d\t%.5lf\t%.5lf\n", c + 1, P.pos[m], (int)cnt[c], ls[m] / cnt[c], (us[m] - ls[m]) / ln10);
            else fprintf(out, "%d\t%.5lf\t0\t-\t%.5lf\n", c + 1, P.pos[m], (us[m] - ls[m]) / ln10);
        }
    fprintf(out, "\n");
    for (int j = 0; j < N; j++)
        for (int c = 0; c < C; c++)
            for (int m = P.chromstarts[c]; m < P.chromstarts[c + 1]; m++) {
                const double v = loo[(size_t)j * M + m];
                if (v != (double)CNF2_IGNORED && v >= opt.loo_threshold)
                    fprintf(out, "%s\t%d\t%d\t%.5lf\t%.5lf\t%.5lf\n", P.inds[P.dous[j]].name.c_str(), c + 1, m, P.pos[m], v, unl[(size_t)j * M + m]);
            }
    if (fclose(out) != 0) throw EngineError(CNF2_ERR_STATE, "cannot write " + opt.loo);
}

// --origins after the last round (single GPU), like --viterbi
static void origin_rows(const Options& opt, Pedigree& P, cnf2_ctx* ctx)
{
    const int N = (int)P.dous.size(), M = P.n_markers(), C = (int)P.chromstarts.size() - 1;
    std::vector<double>  f((size_t)N * C * 8), ll((size_t)N * C), og((size_t)N * M * 4), os((size_t)M * 4);
    std::vector<int32_t> cnt(C);
    if (cnf2_sweep_origins(ctx, 0, N, f.data(), ll.data(), og.data(), nullptr, os.data(), cnt.data(), 0) != CNF2_OK)
        throw EngineError(CNF2_ERR_STATE, std::string("cnf2_sweep_origins: ") + cnf2_last_error(ctx));
    FILE* out = fopen(opt.origins.c_str(), "w");
    if (!out) throw EngineError(CNF2_ERR_STATE, "cannot write " + opt.origins);
    for (int c = 0; c < C; c++)
        for (int j = 0; j < N; j++) {
            fprintf(out, "%s:%d\n", P.inds[P.dous[j]].name.c_str(), c + 1);
            for (int m = P.chromstarts[c]; m < P.chromstarts[c + 1]; m++) {
                const double* r = &og[((size_t)j * M + m) * 4];
                // (a skipped individual's rows are all zero; every other row sums to 1)
                if (r[0] == 0.0 && r[1] == 0.0 && r[2] == 0.0 && r[3] == 0.0) fprintf(out, "-\t-\t-\t-\n");
                else fprintf(out, "%.6lf\t%.6lf\t%.6lf\t%.6lf\n", r[0], r[1], r[2], r[3]);
            }
            fprintf(out, "\n");
        }
    for (int c = 0; c < C; c++)
        for (int m = P.chromstarts[c]; m < P.chromstarts[c + 1]; m++)
            fprintf(out, "%d\t%.5lf\t%d\t%.5lf\t%.5lf\t%.5lf\t%.5lf\n", c + 1, P.pos[m], (int)cnt[c], os[(size_t)m * 4], os[(size_t)m * 4 + 1],
                    os[(size_t)m * 4 + 2], os[(size_t)m * 4 + 3]);
    if (fclose(out) != 0) throw EngineError(CNF2_ERR_STATE, "cannot write " + opt.origins);
}

// --descent after the last round (single GPU), like --origins
static void descent_rows(const Options& opt, Pedigree& P, cnf2_ctx* ctx)
{
    const int N = (int)P.dous.size(), M = P.n_markers(), C = (int)P.chromstarts.size() - 1;
    std::vector<double>  f((size_t)N * C * 8), ll((size_t)N * C), ds((size_t)N * M * 8);
    std::vector<int32_t> cnt(C);
    if (cnf2_sweep_descent(ctx, 0, N, f.data(), ll.data(), ds.data(), cnt.data(), 0) != CNF2_OK)
        throw EngineError(CNF2_ERR_STATE, std::string("cnf2_sweep_descent: ") + cnf2_last_error(ctx));
    FILE* out = fopen(opt.descent.c_str(), "w");
    if (!out) throw EngineError(CNF2_ERR_STATE, "cannot write " + opt.descent);
    for (int c = 0; c < C; c++)
        for (int j = 0; j < N; j++) {
            fprintf(out, "%s:%d\n", P.inds[P.dous[j]].name.c_str(), c + 1);
            for (int m = P.chromstarts[c]; m < P.chromstarts[c + 1]; m++) {
                const double* r = &ds[((size_t)j * M + m) * 8];
                // (a skipped individual's rows are all zero; every other row's sides sum to 1 each)
                bool zero = true;
                for (int k = 0; k < 8; k++) zero = zero && r[k] == 0.0;
                for (int k = 0; k < 8; k++) {
                    if (zero) fprintf(out, "-%c", k == 7 ? '\n' : '\t');
                    else fprintf(out, "%.6lf%c", r[k], k == 7 ? '\n' : '\t');
                }
            }
            fprintf(out, "\n");
        }
    for (int c = 0; c < C; c++) fprintf(out, "%d\t%d\n", c + 1, (int)cnt[c]);
    if (fclose(out) != 0) throw EngineError(CNF2_ERR_STATE, "cannot write " + opt.descent);
}

// --qtlx after the last round (single GPU), and after --qtl / --qtl2 where they are given: the extended single-locus scan
// (cnf2_qtl_scanx) on the rows a cnf2_sweep_qtl left in the context -- theirs, or one of this function's own.  Traits are
// grouped by their pattern of missing values as for --qtl.  The file holds one table per trait, the tables separated by a
// blank line: a line "trait" and the name; per marker chromosome, position, n, the three nested LODs (Mendelian, +
// imprinting, + interaction), lod_imprint = the second less the first, lod_interaction = the third less the second, the three
// cumulative ranks and the effects of the full model in the design's column order ("-" for a dropped column); with
// --qtl-permutations K > 0 five lines "threshold", the statistic's name and its 5 % and 1 % genome-wide thresholds.
static void qtlx_scan(const Options& opt, Pedigree& P, cnf2_ctx* ctx, bool rows_kept)
{
    const int N = (int)P.dous.size(), M = P.n_markers(), C = (int)P.chromstarts.size() - 1;
    const int T = (int)opt.qtl_trait_cols.size(), K = (int)opt.qtlx_cov_cols.size(), Ki = opt.qtlx_n_int, NP = opt.qtl_permutations;
    const cnf2::QtlxDesign ds = cnf2::qtlx_design(K, Ki, opt.qtl_additive, opt.qtl_imprint);
    const int NC = ds.w - ds.nx;
    std::map<std::string, int> row_of;
    for (size_t r = 0; r < opt.pheno.ids.size(); r++) row_of[opt.pheno.ids[r]] = (int)r;
    std::vector<double>  y((size_t)N * T, NAN), cov((size_t)N * K, 0.0);
    std::vector<uint8_t> base(N, 0);
    for (int j = 0; j < N; j++) {
        const auto it = row_of.find(P.inds[P.dous[j]].name);
        if (it == row_of.end()) continue;
        const std::vector<double>& row = opt.pheno.rows[it->second];
        base[j] = 1;
        for (int k = 0; k < K; k++) {
            cov[(size_t)j * K + k] = row[opt.qtlx_cov_cols[k]];
            if (row[opt.qtlx_cov_cols[k]] != row[opt.qtlx_cov_cols[k]]) base[j] = 0;
        }
        for (int t = 0; t < T; t++) y[(size_t)j * T + t] = row[opt.qtl_trait_cols[t]];
    }
    std::map<std::vector<uint8_t>, std::vector<int>> groups;      // pattern of use -> traits
    for (int t = 0; t < T; t++) {
        std::vector<uint8_t> u(N);
        for (int j = 0; j < N; j++) u[j] = base[j] && y[(size_t)j * T + t] == y[(size_t)j * T + t];
        groups[u].push_back(t);
    }
    const uint32_t flags = (opt.qtl_additive ? CNF2_QTL_ADDITIVE : 0) | (opt.qtl_imprint ? CNF2_QTL_IMPRINT : 0) | CNF2_QTL_ORIGIN_DEVICE;
    std::vector<double>  lod((size_t)T * M * 3), coef((size_t)T * M * NC), thr((size_t)T * 10, 0.0);
    std::vector<int32_t> rank((size_t)T * M * 3), nused((size_t)T * C);
    for (const auto& g : groups) {
        const std::vector<int>&     tr = g.second;
        const std::vector<uint8_t>& u  = g.first;
        const int                   Tg = (int)tr.size();
        std::vector<double>  yg((size_t)N * Tg), l((size_t)Tg * M * 3), cf((size_t)Tg * M * NC), rss((size_t)Tg * C);
        std::vector<int32_t> rk((size_t)M * 3), nu(C);
        for (int j = 0; j < N; j++)
            for (int t = 0; t < Tg; t++) yg[(size_t)j * Tg + t] = u[j] ? y[(size_t)j * T + tr[t]] : 0.0;
        int rc;
        if (!rows_kept) {          // the sweep, with the rows left in the context; its single-locus scan is not reported
            std::vector<double>  fa((size_t)N * C * 8), ll((size_t)N * C), l1((size_t)Tg * M), c1((size_t)Tg * M * 2), r1((size_t)Tg * C);
            std::vector<int32_t> k1(M), n1(C);
            rc = cnf2_sweep_qtl(ctx, 0, N, fa.data(), ll.data(), Tg, yg.data(), u.data(), K, K ? cov.data() : nullptr, 0, nullptr,
                                l1.data(), c1.data(), k1.data(), r1.data(), n1.data(), nullptr, flags & CNF2_QTL_ADDITIVE);
            if (rc != CNF2_OK) throw EngineError(CNF2_ERR_STATE, std::string("--qtlx: ") + cnf2_last_error(ctx));
            rows_kept = true;
        }
        rc = cnf2_qtl_scanx(ctx, N, nullptr, Tg, yg.data(), u.data(), K, K ? cov.data() : nullptr, Ki, 0, nullptr, l.data(), cf.data(),
                            rk.data(), rss.data(), nu.data(), nullptr, flags);
        if (rc != CNF2_OK) throw EngineError(CNF2_ERR_STATE, std::string("--qtlx: ") + cnf2_last_error(ctx));
        for (int t = 0; t < Tg; t++) {
            std::copy(l.begin() + (size_t)t * M * 3, l.begin() + (size_t)(t + 1) * M * 3, lod.begin() + (size_t)tr[t] * M * 3);
            std::copy(cf.begin() + (size_t)t * M * NC, cf.begin() + (size_t)(t + 1) * M * NC, coef.begin() + (size_t)tr[t] * M * NC);
            std::copy(rk.begin(), rk.end(), rank.begin() + (size_t)tr[t] * M * 3);
            std::copy(nu.begin(), nu.end(), nused.begin() + (size_t)tr[t] * C);
        }
        if (NP > 0) {
            std::vector<int32_t> perm((size_t)NP * N);
            std::vector<double>  res((size_t)N * Tg, 0.0), pm((size_t)NP * Tg * C * 5);
            qtl_permutations(N, NP, opt.qtl_seed, u.data(), nullptr, perm.data());
            // (as for --qtl: with too few individuals nothing is scanned and the residuals stay 0; with enough of them a null
            // design without full rank is an error)
            const int n_u = (int)std::count(u.begin(), u.end(), (uint8_t)1);
            if (n_u >= ds.w + 1 && !qtl_null_residuals(N, Tg, yg.data(), K, K ? cov.data() : nullptr, u.data(), res.data()))
                throw EngineError(CNF2_ERR_ARG, "--qtl-permutations: the null design (intercept and covariates) of the individuals used for " +
                                                    opt.pheno.columns[opt.qtl_trait_cols[tr[0]]] + " has no full rank");
            rc = cnf2_qtl_scanx(ctx, N, nullptr, Tg, res.data(), u.data(), K, K ? cov.data() : nullptr, Ki, NP, perm.data(), l.data(),
                                cf.data(), rk.data(), rss.data(), nu.data(), pm.data(), flags);
            if (rc != CNF2_OK) throw EngineError(CNF2_ERR_STATE, std::string("--qtlx permutations: ") + cnf2_last_error(ctx));
            for (int t = 0; t < Tg; t++)
                for (int s = 0; s < 5; s++) {
                    std::vector<double> mx(NP, 0.0);
                    for (int p = 0; p < NP; p++)
                        for (int c = 0; c < C; c++) mx[p] = std::max(mx[p], pm[(((size_t)p * Tg + t) * C + c) * 5 + s]);
                    thr[(size_t)tr[t] * 10 + 2 * s]     = qtl_threshold(mx, 0.05);
                    thr[(size_t)tr[t] * 10 + 2 * s + 1] = qtl_threshold(mx, 0.01);
                }
        }
    }
    FILE* out = fopen(opt.qtlx.c_str(), "w");
    if (!out) throw EngineError(CNF2_ERR_STATE, "cannot write " + opt.qtlx);
    static const char* const stat[5] = {"lod_mendelian", "lod_imprinting", "lod_full", "lod_imprint", "lod_interaction"};
    for (int t = 0; t < T; t++) {
        fprintf(out, "%strait\t%s\n", t ? "\n" : "", opt.pheno.columns[opt.qtl_trait_cols[t]].c_str());
        for (int c = 0; c < C; c++)
            for (int m = P.chromstarts[c]; m < P.chromstarts[c + 1]; m++) {
                const double*  l = &lod[((size_t)t * M + m) * 3];
                const int32_t* r = &rank[((size_t)t * M + m) * 3];
                fprintf(out, "%d\t%.5lf\t%d\t%.5lf\t%.5lf\t%.5lf\t%.5lf\t%.5lf\t%d\t%d\t%d", c + 1, P.pos[m], (int)nused[(size_t)t * C + c], l[0],
                        l[1], l[2], l[1] - l[0], l[2] - l[1], (int)r[0], (int)r[1], (int)r[2]);
                for (int e = 0; e < NC; e++) {
                    const double v = coef[((size_t)t * M + m) * NC + e];
                    if (v != v) fprintf(out, "\t-");
                    else fprintf(out, "\t%.5lf", v);
                }
                fprintf(out, "\n");
            }
        if (NP > 0)
            for (int s = 0; s < 5; s++) fprintf(out, "threshold\t%s\t%.5lf\t%.5lf\n", stat[s], thr[(size_t)t * 10 + 2 * s], thr[(size_t)t * 10 + 2 * s + 1]);
    }
    if (fclose(out) != 0) throw EngineError(CNF2_ERR_STATE, "cannot write " + opt.qtlx);
}

// --qtlem after the last round (single GPU), and after --qtl / --qtl2 / --qtlx where they are given: the maximum-likelihood
// scan (cnf2_qtl_scan_em) on the rows a cnf2_sweep_qtl left in the context -- theirs, or one of this function's own.  Traits
// are grouped by their pattern of missing values as for --qtl.  The file holds one table per trait, the tables separated by a
// blank line: a line "trait" and the name; per marker chromosome, position, n, the rank, the LOD, sigma^2, the iterations, the
// status (0 = stopped by --qtl-em-tol, 1 = by --qtl-em-iterations, 2 = breakdown) and the effects a, d (not with
// --qtl-additive), i (with --qtl-imprint), "-" for a dropped one or a cell without a fit; with --qtl-permutations K > 0 a line
// "threshold", "lod" and the 5 % and 1 % genome-wide thresholds.
static void qtlem_scan(const Options& opt, Pedigree& P, cnf2_ctx* ctx, bool rows_kept)
{
    const int N = (int)P.dous.size(), M = P.n_markers(), C = (int)P.chromstarts.size() - 1;
    const int T = (int)opt.qtl_trait_cols.size(), K = (int)opt.qtl_cov_cols.size(), NP = opt.qtl_permutations;
    const cnf2::QtlemDesign ds = cnf2::qtlem_design(K, opt.qtl_additive, opt.qtl_imprint);
    const int NC = ds.ne;
    std::map<std::string, int> row_of;
    for (size_t r = 0; r < opt.pheno.ids.size(); r++) row_of[opt.pheno.ids[r]] = (int)r;
    std::vector<double>  y((size_t)N * T, NAN), cov((size_t)N * K, 0.0);
    std::vector<uint8_t> base(N, 0);
    for (int j = 0; j < N; j++) {
        const auto it = row_of.find(P.inds[P.dous[j]].name);
        if (it == row_of.end()) continue;
        const std::vector<double>& row = opt.pheno.rows[it->second];
        base[j] = 1;
        for (int k = 0; k < K; k++) {
            cov[(size_t)j * K + k] = row[opt.qtl_cov_cols[k]];
            if (row[opt.qtl_cov_cols[k]] != row[opt.qtl_cov_cols[k]]) base[j] = 0;
        }
        for (int t = 0; t < T; t++) y[(size_t)j * T + t] = row[opt.qtl_trait_cols[t]];
    }
    std::map<std::vector<uint8_t>, std::vector<int>> groups;      // pattern of use -> traits
    for (int t = 0; t < T; t++) {
        std::vector<uint8_t> u(N);
        for (int j = 0; j < N; j++) u[j] = base[j] && y[(size_t)j * T + t] == y[(size_t)j * T + t];
        groups[u].push_back(t);
    }
    const uint32_t flags = (opt.qtl_additive ? CNF2_QTL_ADDITIVE : 0) | (opt.qtl_imprint ? CNF2_QTL_IMPRINT : 0) | CNF2_QTL_ORIGIN_DEVICE;
    std::vector<double>  lod((size_t)T * M), coef((size_t)T * M * NC), s2((size_t)T * M), thr((size_t)T * 2, 0.0);
    std::vector<int32_t> rank((size_t)T * M), nused((size_t)T * C), iters((size_t)T * M), status((size_t)T * M);
    for (const auto& g : groups) {
        const std::vector<int>&     tr = g.second;
        const std::vector<uint8_t>& u  = g.first;
        const int                   Tg = (int)tr.size();
        std::vector<double>  yg((size_t)N * Tg), l((size_t)Tg * M), cf((size_t)Tg * M * NC), sg((size_t)Tg * M), rss((size_t)Tg * C);
        std::vector<int32_t> rk(M), nu(C), it((size_t)Tg * M), st((size_t)Tg * M);
        for (int j = 0; j < N; j++)
            for (int t = 0; t < Tg; t++) yg[(size_t)j * Tg + t] = u[j] ? y[(size_t)j * T + tr[t]] : 0.0;
        int rc;
        if (!rows_kept) {          // the sweep, with the rows left in the context; its Haley-Knott scan is not reported
            std::vector<double>  fa((size_t)N * C * 8), ll((size_t)N * C), l1((size_t)Tg * M), c1((size_t)Tg * M * 2), r1((size_t)Tg * C);
            std::vector<int32_t> k1(M), n1(C);
            rc = cnf2_sweep_qtl(ctx, 0, N, fa.data(), ll.data(), Tg, yg.data(), u.data(), K, K ? cov.data() : nullptr, 0, nullptr,
                                l1.data(), c1.data(), k1.data(), r1.data(), n1.data(), nullptr, flags & CNF2_QTL_ADDITIVE);
            if (rc != CNF2_OK) throw EngineError(CNF2_ERR_STATE, std::string("--qtlem: ") + cnf2_last_error(ctx));
            rows_kept = true;
        }
        rc = cnf2_qtl_scan_em(ctx, N, nullptr, Tg, yg.data(), u.data(), K, K ? cov.data() : nullptr, 0, nullptr, opt.qtlem_iterations,
                              opt.qtlem_tol, l.data(), cf.data(), sg.data(), it.data(), st.data(), rk.data(), rss.data(), nu.data(), nullptr,
                              flags);
        if (rc != CNF2_OK) throw EngineError(CNF2_ERR_STATE, std::string("--qtlem: ") + cnf2_last_error(ctx));
        for (int t = 0; t < Tg; t++) {
            const size_t from = (size_t)t * M, to = (size_t)tr[t] * M;
            std::copy(l.begin() + from, l.begin() + from + M, lod.begin() + to);
            std::copy(sg.begin() + from, sg.begin() + from + M, s2.begin() + to);
            std::copy(it.begin() + from, it.begin() + from + M, iters.begin() + to);
            std::copy(st.begin() + from, st.begin() + from + M, status.begin() + to);
            std::copy(cf.begin() + from * NC, cf.begin() + (from + M) * NC, coef.begin() + to * NC);
            std::copy(rk.begin(), rk.end(), rank.begin() + to);
            std::copy(nu.begin(), nu.end(), nused.begin() + (size_t)tr[t] * C);
        }
        if (NP > 0) {
            std::vector<int32_t> perm((size_t)NP * N);
            std::vector<double>  res((size_t)N * Tg, 0.0), pm((size_t)NP * Tg * C);
            qtl_permutations(N, NP, opt.qtl_seed, u.data(), nullptr, perm.data());
            // (as for --qtl: with too few individuals nothing is scanned and the residuals stay 0; with enough of them a null
            // design without full rank is an error)
            const int n_u = (int)std::count(u.begin(), u.end(), (uint8_t)1);
            if (n_u >= std::max(ds.w + 1, K + 4) && !qtl_null_residuals(N, Tg, yg.data(), K, K ? cov.data() : nullptr, u.data(), res.data()))
                throw EngineError(CNF2_ERR_ARG, "--qtl-permutations: the null design (intercept and covariates) of the individuals used for " +
                                                    opt.pheno.columns[opt.qtl_trait_cols[tr[0]]] + " has no full rank");
            rc = cnf2_qtl_scan_em(ctx, N, nullptr, Tg, res.data(), u.data(), K, K ? cov.data() : nullptr, NP, perm.data(),
                                  opt.qtlem_iterations, opt.qtlem_tol, l.data(), cf.data(), sg.data(), it.data(), st.data(), rk.data(),
                                  rss.data(), nu.data(), pm.data(), flags);
            if (rc != CNF2_OK) throw EngineError(CNF2_ERR_STATE, std::string("--qtlem permutations: ") + cnf2_last_error(ctx));
            for (int t = 0; t < Tg; t++) {
                std::vector<double> mx(NP, 0.0);
                for (int p = 0; p < NP; p++)
                    for (int c = 0; c < C; c++) mx[p] = std::max(mx[p], pm[((size_t)p * Tg + t) * C + c]);
                thr[(size_t)tr[t] * 2]     = qtl_threshold(mx, 0.05);
                thr[(size_t)tr[t] * 2 + 1] = qtl_threshold(mx, 0.01);
            }
        }
    }
    FILE* out = fopen(opt.qtlem.c_str(), "w");
    if (!out) throw EngineError(CNF2_ERR_STATE, "cannot write " + opt.qtlem);
    auto number = [&](double v) {
        if (v != v) fprintf(out, "\t-");
        else fprintf(out, "\t%.5lf", v);
    };
    for (int t = 0; t < T; t++) {
        fprintf(out, "%strait\t%s\n", t ? "\n" : "", opt.pheno.columns[opt.qtl_trait_cols[t]].c_str());
        for (int c = 0; c < C; c++)
            for (int m = P.chromstarts[c]; m < P.chromstarts[c + 1]; m++) {
                const size_t at = (size_t)t * M + m;
                fprintf(out, "%d\t%.5lf\t%d\t%d\t%.5lf", c + 1, P.pos[m], (int)nused[(size_t)t * C + c], (int)rank[at], lod[at]);
                number(s2[at]);
                fprintf(out, "\t%d\t%d", (int)iters[at], (int)status[at]);
                for (int e = 0; e < NC; e++) number(coef[at * NC + e]);
                fprintf(out, "\n");
            }
        if (NP > 0) fprintf(out, "threshold\tlod\t%.5lf\t%.5lf\n", thr[(size_t)t * 2], thr[(size_t)t * 2 + 1]);
    }
    if (fclose(out) != 0) throw EngineError(CNF2_ERR_STATE, "cannot write " + opt.qtlem);
}

// --qtlbin after the last round (single GPU), and after the other scans where they are given: the binary-trait scan
// (cnf2_qtl_scan_binary) of the traits whose values are all 0 or 1, on the rows a cnf2_sweep_qtl left in the context -- theirs,
// or one of this function's own.  Traits are grouped by their pattern of missing values as for --qtl; permutations permute the
// 0/1 values themselves.  The file holds one table per trait, the tables separated by a blank line: a line "trait" and the
// name; per marker chromosome, position, n, the rank, the LOD, the iterations, the status (0 = stopped by --qtl-binary-tol,
// 1 = by --qtl-binary-iterations, 2 = breakdown) and the effects a, d (not with --qtl-additive), i (with --qtl-imprint), "-" for
// a dropped one or a cell without a fit; with --qtl-permutations K > 0 a line "threshold", "lod" and the 5 % and 1 %
// genome-wide thresholds.
static void qtlbin_scan(const Options& opt, Pedigree& P, cnf2_ctx* ctx, bool rows_kept)
{
    const int N = (int)P.dous.size(), M = P.n_markers(), C = (int)P.chromstarts.size() - 1;
    const int T = (int)opt.qtlbin_trait_cols.size(), K = (int)opt.qtl_cov_cols.size(), NP = opt.qtl_permutations;
    const int NC = cnf2::qtlem_design(K, opt.qtl_additive, opt.qtl_imprint).ne;
    std::map<std::string, int> row_of;
    for (size_t r = 0; r < opt.pheno.ids.size(); r++) row_of[opt.pheno.ids[r]] = (int)r;
    std::vector<double>  y((size_t)N * T, NAN), cov((size_t)N * K, 0.0);
    std::vector<uint8_t> base(N, 0);
    for (int j = 0; j < N; j++) {
        const auto it = row_of.find(P.inds[P.dous[j]].name);
        if (it == row_of.end()) continue;
        const std::vector<double>& row = opt.pheno.rows[it->second];
        base[j] = 1;
        for (int k = 0; k < K; k++) {
            cov[(size_t)j * K + k] = row[opt.qtl_cov_cols[k]];
            if (row[opt.qtl_cov_cols[k]] != row[opt.qtl_cov_cols[k]]) base[j] = 0;
        }
        for (int t = 0; t < T; t++) y[(size_t)j * T + t] = row[opt.qtlbin_trait_cols[t]];
    }
    std::map<std::vector<uint8_t>, std::vector<int>> groups;      // pattern of use -> traits
    for (int t = 0; t < T; t++) {
        std::vector<uint8_t> u(N);
        for (int j = 0; j < N; j++) u[j] = base[j] && y[(size_t)j * T + t] == y[(size_t)j * T + t];
        groups[u].push_back(t);
    }
    const uint32_t flags = (opt.qtl_additive ? CNF2_QTL_ADDITIVE : 0) | (opt.qtl_imprint ? CNF2_QTL_IMPRINT : 0) | CNF2_QTL_ORIGIN_DEVICE;
    std::vector<double>  lod((size_t)T * M), coef((size_t)T * M * NC), thr((size_t)T * 2, 0.0);
    std::vector<int32_t> rank((size_t)T * M), nused((size_t)T * C), iters((size_t)T * M), status((size_t)T * M);
    for (const auto& g : groups) {
        const std::vector<int>&     tr = g.second;
        const std::vector<uint8_t>& u  = g.first;
        const int                   Tg = (int)tr.size();
        std::vector<double>  yg((size_t)N * Tg), l((size_t)Tg * M), cf((size_t)Tg * M * NC), l0((size_t)Tg * C), pm((size_t)NP * Tg * C);
        std::vector<int32_t> rk(M), nu(C), it((size_t)Tg * M), st((size_t)Tg * M), n1((size_t)Tg * C), perm((size_t)NP * N);
        for (int j = 0; j < N; j++)
            for (int t = 0; t < Tg; t++) yg[(size_t)j * Tg + t] = u[j] ? y[(size_t)j * T + tr[t]] : 0.0;
        int rc;
        if (!rows_kept) {          // the sweep, with the rows left in the context; its Haley-Knott scan is not reported
            std::vector<double>  fa((size_t)N * C * 8), ll((size_t)N * C), l1((size_t)Tg * M), c1((size_t)Tg * M * 2), r1((size_t)Tg * C);
            std::vector<int32_t> k1(M), m1(C);
            rc = cnf2_sweep_qtl(ctx, 0, N, fa.data(), ll.data(), Tg, yg.data(), u.data(), K, K ? cov.data() : nullptr, 0, nullptr,
                                l1.data(), c1.data(), k1.data(), r1.data(), m1.data(), nullptr, flags & CNF2_QTL_ADDITIVE);
            if (rc != CNF2_OK) throw EngineError(CNF2_ERR_STATE, std::string("--qtlbin: ") + cnf2_last_error(ctx));
            rows_kept = true;
        }
        if (NP > 0) qtl_permutations(N, NP, opt.qtl_seed, u.data(), nullptr, perm.data());
        rc = cnf2_qtl_scan_binary(ctx, N, nullptr, Tg, yg.data(), u.data(), K, K ? cov.data() : nullptr, NP, NP ? perm.data() : nullptr,
                                  opt.qtlbin_iterations, opt.qtlbin_tol, l.data(), cf.data(), it.data(), st.data(), rk.data(), l0.data(),
                                  n1.data(), nu.data(), NP ? pm.data() : nullptr, flags);
        if (rc != CNF2_OK) throw EngineError(CNF2_ERR_STATE, std::string("--qtlbin: ") + cnf2_last_error(ctx));
        for (int t = 0; t < Tg; t++) {
            const size_t from = (size_t)t * M, to = (size_t)tr[t] * M;
            std::copy(l.begin() + from, l.begin() + from + M, lod.begin() + to);
            std::copy(it.begin() + from, it.begin() + from + M, iters.begin() + to);
            std::copy(st.begin() + from, st.begin() + from + M, status.begin() + to);
            std::copy(cf.begin() + from * NC, cf.begin() + (from + M) * NC, coef.begin() + to * NC);
            std::copy(rk.begin(), rk.end(), rank.begin() + to);
            std::copy(nu.begin(), nu.end(), nused.begin() + (size_t)tr[t] * C);
            if (NP > 0) {
                std::vector<double> mx(NP, 0.0);
                for (int p = 0; p < NP; p++)
                    for (int c = 0; c < C; c++) mx[p] = std::max(mx[p], pm[((size_t)p * Tg + t) * C + c]);
                thr[(size_t)tr[t] * 2]     = qtl_threshold(mx, 0.05);
                thr[(size_t)tr[t] * 2 + 1] = qtl_threshold(mx, 0.01);
            }
        }
    }
    FILE* out = fopen(opt.qtlbin.c_str(), "w");
    if (!out) throw EngineError(CNF2_ERR_STATE, "cannot write " + opt.qtlbin);
    for (int t = 0; t < T; t++) {
        fprintf(out, "%strait\t%s\n", t ? "\n" : "", opt.pheno.columns[opt.qtlbin_trait_cols[t]].c_str());
        for (int c = 0; c < C; c++)
            for (int m = P.chromstarts[c]; m < P.chromstarts[c + 1]; m++) {
                const size_t at = (size_t)t * M + m;
                fprintf(out, "%d\t%.5lf\t%d\t%d\t%.5lf\t%d\t%d", c + 1, P.pos[m], (int)nused[(size_t)t * C + c], (int)rank[at], lod[at],
                        (int)iters[at], (int)status[at]);
                for (int e = 0; e < NC; e++) {
                    const double v = coef[at * NC + e];
                    if (v != v) fprintf(out, "\t-");
                    else fprintf(out, "\t%.5lf", v);
                }
                fprintf(out, "\n");
            }
        if (NP > 0) fprintf(out, "threshold\tlod\t%.5lf\t%.5lf\n", thr[(size_t)t * 2], thr[(size_t)t * 2 + 1]);
    }
    if (fclose(out) != 0) throw EngineError(CNF2_ERR_STATE, "cannot write " + opt.qtlbin);
}

// --qtlvar after the last round (single GPU), and after the other scans where they are given: the variance-QTL scan
// (cnf2_qtl_scan_var) of every trait, on the rows a cnf2_sweep_qtl left in the context -- theirs, or one of this function's own.
// Traits are grouped by their pattern of missing values as for --qtl; permutations permute the phenotypes themselves.  The
// file holds one table per trait, the tables separated by a blank line: a line "trait" and the name; per marker chromosome,
// position, n, the rank, the joint, the mean and the variance LOD, the iterations and the status (0 = stopped by
// --qtl-var-tol, 1 = by --qtl-var-iterations, 2 = breakdown) of the mean-only, the variance-only and the full fit, the full
// fit's mean effects a, d (not with --qtl-additive), i (with --qtl-imprint) and then its log-variance effects in the same
// order, "-" for a dropped one or a cell without a fit; with --qtl-permutations K > 0 three lines "threshold", the LOD's name
// and its 5 % and 1 % genome-wide thresholds.
static void qtlvar_scan(const Options& opt, Pedigree& P, cnf2_ctx* ctx, bool rows_kept)
{
    const int N = (int)P.dous.size(), M = P.n_markers(), C = (int)P.chromstarts.size() - 1;
    const int T = (int)opt.qtl_trait_cols.size(), K = (int)opt.qtlvar_cov_cols.size(), NP = opt.qtl_permutations;
    const int NC = cnf2::qtlem_design(K, opt.qtl_additive, opt.qtl_imprint).ne, NF = cnf2::QTLVAR_NFIT;
    std::map<std::string, int> row_of;
    for (size_t r = 0; r < opt.pheno.ids.size(); r++) row_of[opt.pheno.ids[r]] = (int)r;
    std::vector<double>  y((size_t)N * T, NAN), cov((size_t)N * K, 0.0);
    std::vector<uint8_t> base(N, 0);
    for (int j = 0; j < N; j++) {
        const auto it = row_of.find(P.inds[P.dous[j]].name);
        if (it == row_of.end()) continue;
        const std::vector<double>& row = opt.pheno.rows[it->second];
        base[j] = 1;
        for (int k = 0; k < K; k++) {
            cov[(size_t)j * K + k] = row[opt.qtlvar_cov_cols[k]];
            if (row[opt.qtlvar_cov_cols[k]] != row[opt.qtlvar_cov_cols[k]]) base[j] = 0;
        }
        for (int t = 0; t < T; t++) y[(size_t)j * T + t] = row[opt.qtl_trait_cols[t]];
    }
    std::map<std::vector<uint8_t>, std::vector<int>> groups;      // pattern of use -> traits
    for (int t = 0; t < T; t++) {
        std::vector<uint8_t> u(N);
        for (int j = 0; j < N; j++) u[j] = base[j] && y[(size_t)j * T + t] == y[(size_t)j * T + t];
        groups[u].push_back(t);
    }
    const uint32_t flags = (opt.qtl_additive ? CNF2_QTL_ADDITIVE : 0) | (opt.qtl_imprint ? CNF2_QTL_IMPRINT : 0) | CNF2_QTL_ORIGIN_DEVICE;
    std::vector<double>  lod((size_t)T * M * NF), cm((size_t)T * M * NC), cv((size_t)T * M * NC), thr((size_t)T * NF * 2, 0.0);
    std::vector<int32_t> rank((size_t)T * M), nused((size_t)T * C), iters((size_t)T * M * NF), status((size_t)T * M * NF);
    for (const auto& g : groups) {
        const std::vector<int>&     tr = g.second;
        const std::vector<uint8_t>& u  = g.first;
        const int                   Tg = (int)tr.size();
        std::vector<double>  yg((size_t)N * Tg), l((size_t)Tg * M * NF), fm((size_t)Tg * M * NC), fv((size_t)Tg * M * NC), l0((size_t)Tg * C),
            pm((size_t)NP * Tg * C * NF);
        std::vector<int32_t> rk(M), nu(C), it((size_t)Tg * M * NF), st((size_t)Tg * M * NF), perm((size_t)NP * N);
        for (int j = 0; j < N; j++)
            for (int t = 0; t < Tg; t++) yg[(size_t)j * Tg + t] = u[j] ? y[(size_t)j * T + tr[t]] : 0.0;
        int rc;
        if (!rows_kept) {          // the sweep, with the rows left in the context; its Haley-Knott scan is not reported
            std::vector<double>  fa((size_t)N * C * 8), ll((size_t)N * C), l1((size_t)Tg * M), c1((size_t)Tg * M * 2), r1((size_t)Tg * C);
            std::vector<int32_t> k1(M), m1(C);
            rc = cnf2_sweep_qtl(ctx, 0, N, fa.data(), ll.data(), Tg, yg.data(), u.data(), K, K ? cov.data() : nullptr, 0, nullptr,
                                l1.data(), c1.data(), k1.data(), r1.data(), m1.data(), nullptr, flags & CNF2_QTL_ADDITIVE);
            if (rc != CNF2_OK) throw EngineError(CNF2_ERR_STATE, std::string("--qtlvar: ") + cnf2_last_error(ctx));
            rows_kept = true;
        }
        if (NP > 0) qtl_permutations(N, NP, opt.qtl_seed, u.data(), nullptr, perm.data());
        rc = cnf2_qtl_scan_var(ctx, N, nullptr, Tg, yg.data(), u.data(), K, K ? cov.data() : nullptr, opt.qtlvar_n_var, NP,
                               NP ? perm.data() : nullptr, opt.qtlvar_iterations, opt.qtlvar_tol, l.data(), fm.data(), fv.data(), it.data(),
                               st.data(), rk.data(), l0.data(), nu.data(), NP ? pm.data() : nullptr, flags);
        if (rc != CNF2_OK) throw EngineError(CNF2_ERR_STATE, std::string("--qtlvar: ") + cnf2_last_error(ctx));
        for (int t = 0; t < Tg; t++) {
            const size_t from = (size_t)t * M, to = (size_t)tr[t] * M;
            std::copy(l.begin() + from * NF, l.begin() + (from + M) * NF, lod.begin() + to * NF);
            std::copy(it.begin() + from * NF, it.begin() + (from + M) * NF, iters.begin() + to * NF);
            std::copy(st.begin() + from * NF, st.begin() + (from + M) * NF, status.begin() + to * NF);
            std::copy(fm.begin() + from * NC, fm.begin() + (from + M) * NC, cm.begin() + to * NC);
            std::copy(fv.begin() + from * NC, fv.begin() + (from + M) * NC, cv.begin() + to * NC);
            std::copy(rk.begin(), rk.end(), rank.begin() + to);
            std::copy(nu.begin(), nu.end(), nused.begin() + (size_t)tr[t] * C);
            for (int f = 0; f < NF && NP > 0; f++) {
                std::vector<double> mx(NP, 0.0);
                for (int p = 0; p < NP; p++)
                    for (int c = 0; c < C; c++) mx[p] = std::max(mx[p], pm[(((size_t)p * Tg + t) * C + c) * NF + f]);
                thr[((size_t)tr[t] * NF + f) * 2]     = qtl_threshold(mx, 0.05);
                thr[((size_t)tr[t] * NF + f) * 2 + 1] = qtl_threshold(mx, 0.01);
            }
        }
    }
    FILE* out = fopen(opt.qtlvar.c_str(), "w");
    if (!out) throw EngineError(CNF2_ERR_STATE, "cannot write " + opt.qtlvar);
    static const char* const lod_names[3] = {"joint", "mean", "variance"};
    for (int t = 0; t < T; t++) {
        fprintf(out, "%strait\t%s\n", t ? "\n" : "", opt.pheno.columns[opt.qtl_trait_cols[t]].c_str());
        for (int c = 0; c < C; c++)
            for (int m = P.chromstarts[c]; m < P.chromstarts[c + 1]; m++) {
                const size_t at = (size_t)t * M + m;
                fprintf(out, "%d\t%.5lf\t%d\t%d", c + 1, P.pos[m], (int)nused[(size_t)t * C + c], (int)rank[at]);
                for (int f = 0; f < NF; f++) fprintf(out, "\t%.5lf", lod[at * NF + f]);
                for (int f = 0; f < NF; f++) fprintf(out, "\t%d", (int)iters[at * NF + f]);
                for (int f = 0; f < NF; f++) fprintf(out, "\t%d", (int)status[at * NF + f]);
                for (int e = 0; e < 2 * NC; e++) {
                    const double v = e < NC ? cm[at * NC + e] : cv[at * NC + e - NC];
                    if (v != v) fprintf(out, "\t-");
                    else fprintf(out, "\t%.5lf", v);
                }
                fprintf(out, "\n");
            }
        for (int f = 0; f < NF && NP > 0; f++)
            fprintf(out, "threshold\t%s\t%.5lf\t%.5lf\n", lod_names[f], thr[((size_t)t * NF + f) * 2], thr[((size_t)t * NF + f) * 2 + 1]);
    }
    if (fclose(out) != 0) throw EngineError(CNF2_ERR_STATE, "cannot write " + opt.qtlvar);
}

// --qtlsurv after the last round (single GPU), and after the other scans where they are given: the survival-trait scan
// (cnf2_qtl_scan_surv) of the pair of columns --qtl-surv-time and --qtl-surv-status (1 = the event was observed at the time,
// 0 = censored then), on the rows a cnf2_sweep_qtl left in the context -- theirs, or one of this function's own.  An individual
// is used when its covariates, its time and its status are there; permutations permute the pairs.  The file has --qtlbin's
// layout: a line "trait", the time's and the status's name; per marker chromosome, position, n, the rank, the LOD, the
// iterations, the status of the fit (0 = stopped by --qtl-surv-tol, 1 = by --qtl-surv-iterations, 2 = breakdown) and the
// effects on the log hazard a, d (not with --qtl-additive), i (with --qtl-imprint), "-" for a dropped one or a cell without a
// fit; with --qtl-permutations K > 0 a line "threshold", "lod" and the 5 % and 1 % genome-wide thresholds.
static void qtlsurv_scan(const Options& opt, Pedigree& P, cnf2_ctx* ctx, bool rows_kept)
{
    const int N = (int)P.dous.size(), M = P.n_markers(), C = (int)P.chromstarts.size() - 1;
    const int K = (int)opt.qtl_cov_cols.size(), NP = opt.qtl_permutations;
    const int NC = cnf2::qtlem_design(K, opt.qtl_additive, opt.qtl_imprint).ne;
    std::map<std::string, int> row_of;
    for (size_t r = 0; r < opt.pheno.ids.size(); r++) row_of[opt.pheno.ids[r]] = (int)r;
    std::vector<double>  tm(N, 0.0), ev(N, 0.0), cov((size_t)N * K, 0.0);
    std::vector<uint8_t> u(N, 0);
    for (int j = 0; j < N; j++) {
        const auto it = row_of.find(P.inds[P.dous[j]].name);
        if (it == row_of.end()) continue;
        const std::vector<double>& row = opt.pheno.rows[it->second];
        const double t = row[opt.qtlsurv_time_col], d = row[opt.qtlsurv_status_col];
        bool on = t == t && d == d;
        for (int k = 0; k < K; k++) {
            cov[(size_t)j * K + k] = row[opt.qtl_cov_cols[k]];
            if (row[opt.qtl_cov_cols[k]] != row[opt.qtl_cov_cols[k]]) on = false;
        }
        u[j] = on ? 1 : 0;
        if (on) tm[j] = t, ev[j] = d;
    }
    const uint32_t flags = (opt.qtl_additive ? CNF2_QTL_ADDITIVE : 0) | (opt.qtl_imprint ? CNF2_QTL_IMPRINT : 0) | CNF2_QTL_ORIGIN_DEVICE;
    std::vector<double>  lod(M), coef((size_t)M * NC), l0(C), pm((size_t)NP * C);
    std::vector<int32_t> rank(M), nused(C), iters(M), status(M), nev(C), perm((size_t)NP * N);
    int rc;
    if (!rows_kept) {          // the sweep, with the rows left in the context; its Haley-Knott scan is not reported
        std::vector<double>  fa((size_t)N * C * 8), ll((size_t)N * C), l1(M), c1((size_t)M * 2), r1(C);
        std::vector<int32_t> k1(M), m1(C);
        rc = cnf2_sweep_qtl(ctx, 0, N, fa.data(), ll.data(), 1, tm.data(), u.data(), K, K ? cov.data() : nullptr, 0, nullptr, l1.data(),
                            c1.data(), k1.data(), r1.data(), m1.data(), nullptr, flags & CNF2_QTL_ADDITIVE);
        if (rc != CNF2_OK) throw EngineError(CNF2_ERR_STATE, std::string("--qtlsurv: ") + cnf2_last_error(ctx));
    }
    if (NP > 0) qtl_permutations(N, NP, opt.qtl_seed, u.data(), nullptr, perm.data());
    rc = cnf2_qtl_scan_surv(ctx, N, nullptr, 1, tm.data(), ev.data(), u.data(), K, K ? cov.data() : nullptr, NP, NP ? perm.data() : nullptr,
                            opt.qtlsurv_iterations, opt.qtlsurv_tol, lod.data(), coef.data(), iters.data(), status.data(), rank.data(),
                            l0.data(), nev.data(), nused.data(), NP ? pm.data() : nullptr, flags);
    if (rc != CNF2_OK) throw EngineError(CNF2_ERR_STATE, std::string("--qtlsurv: ") + cnf2_last_error(ctx));
    FILE* out = fopen(opt.qtlsurv.c_str(), "w");
    if (!out) throw EngineError(CNF2_ERR_STATE, "cannot write " + opt.qtlsurv);
    fprintf(out, "trait\t%s\t%s\n", opt.qtlsurv_time.c_str(), opt.qtlsurv_status.c_str());
    for (int c = 0; c < C; c++)
        for (int m = P.chromstarts[c]; m < P.chromstarts[c + 1]; m++) {
            fprintf(out, "%d\t%.5lf\t%d\t%d\t%.5lf\t%d\t%d", c + 1, P.pos[m], (int)nused[c], (int)rank[m], lod[m], (int)iters[m], (int)status[m]);
            for (int e = 0; e < NC; e++) {
                const double v = coef[(size_t)m * NC + e];
                if (v != v) fprintf(out, "\t-");
                else fprintf(out, "\t%.5lf", v);
            }
            fprintf(out, "\n");
        }
    if (NP > 0) {
        std::vector<double> mx(NP, 0.0);
        for (int p = 0; p < NP; p++)
            for (int c = 0; c < C; c++) mx[p] = std::max(mx[p], pm[(size_t)p * C + c]);
        fprintf(out, "threshold\tlod\t%.5lf\t%.5lf\n", qtl_threshold(mx, 0.05), qtl_threshold(mx, 0.01));
    }
    if (fclose(out) != 0) throw EngineError(CNF2_ERR_STATE, "cannot write " + opt.qtlsurv);
}

// res[n][T]: the residuals of every phenotype column on the columns X[n][W] and the intercept over the used individuals, 0 for
// the others -- qtl.null_residuals of the Python package for a null model that holds the cofactors: the columns minus their
// means, orthogonalised one after the other (twice, for the rounding); a column of which less than QTL_PIVOT of its own
// length is left depends on those before it and is passed over, as least squares of minimal norm passes over it
static void qtlcof_null_residuals(int n, int T, const double* pheno, int W, const double* X, const uint8_t* use, double* res)
{
    std::vector<int> idx;
    for (int i = 0; i < n; i++)
        if (use[i]) idx.push_back(i);
    const size_t nu = idx.size();
    std::fill(res, res + (size_t)n * T, 0.0);
    if (nu == 0) return;
    auto dot = [&](const std::vector<double>& a, const std::vector<double>& b) {
        double s = 0.0;
        for (size_t i = 0; i < nu; i++) s += a[i] * b[i];
        return s;
    };
    auto centre = [&](std::vector<double>& v) {
        double mean = 0.0;
        for (double x : v) mean += x;
        mean /= (double)nu;
        for (double& x : v) x -= mean;
    };
    std::vector<std::vector<double>> basis;
    for (int k = 0; k < W; k++) {
        std::vector<double> v(nu);
        for (size_t i = 0; i < nu; i++) v[i] = X[(size_t)idx[i] * W + k];
        centre(v);
        const double raw = dot(v, v);
        for (int pass = 0; pass < 2; pass++)
            for (const auto& b : basis) {
                const double s = dot(b, v);
                for (size_t i = 0; i < nu; i++) v[i] -= s * b[i];
            }
        const double left = dot(v, v);
        if (!(raw > 0.0) || left < cnf2::QTL_PIVOT * raw) continue;
        const double inv = 1.0 / sqrt(left);
        for (double& x : v) x *= inv;
        basis.push_back(v);
    }
    for (int t = 0; t < T; t++) {
        std::vector<double> v(nu);
        for (size_t i = 0; i < nu; i++) v[i] = pheno[(size_t)idx[i] * T + t];
        centre(v);
        for (int pass = 0; pass < 2; pass++)
            for (const auto& b : basis) {
                const double s = dot(b, v);
                for (size_t i = 0; i < nu; i++) v[i] -= s * b[i];
            }
        for (size_t i = 0; i < nu; i++) res[(size_t)idx[i] * T + t] = v[i];
    }
}

// --qtlcof after the last round (single GPU), and after the other scans where they are given: the cofactor scan
// (cnf2_qtl_scan_cof: composite interval mapping) with the markers of --qtl-cofactors as cofactors, each left out of the
// design within --qtl-window map units of itself, on the rows a cnf2_sweep_qtl left in the context -- theirs, or one of this
// function's own.  Traits are grouped by their pattern of missing values as for --qtl; with --qtl-permutations K > 0 the
// residuals of the null model [1, covariates, every cofactor's columns] are permuted, the cofactors' columns coming from the
// context's rows (cnf2_qtl_kept_rows).  The file holds one table per trait, the tables separated by a blank line: a line
// "trait" and the name; with permutations a line "threshold", "lod" and the 5 % and 1 % genome-wide thresholds of the
// conditional LOD over the markers in no cofactor's range; per marker chromosome, position, n, the kept cofactor columns,
// the LOD of the cofactors against the null model, the rank, the conditional LOD of the marker given the cofactors and its
// effects a, d (not with --qtl-additive) in the full model, "-" for a dropped one.
static void qtlcof_scan(const Options& opt, Pedigree& P, cnf2_ctx* ctx, bool rows_kept)
{
    const int N = (int)P.dous.size(), M = P.n_markers(), C = (int)P.chromstarts.size() - 1;
    const int T = (int)opt.qtl_trait_cols.size(), K = (int)opt.qtl_cov_cols.size(), NP = opt.qtl_permutations;
    const int Q = (int)opt.qtlcof_cof.size(), NC = opt.qtl_additive ? 1 : 2;
    // the ranges: the markers of the cofactor's chromosome within --qtl-window of it (qtl.cofactor_windows)
    std::vector<int32_t> lo(Q), hi(Q);
    for (int q = 0, c = 0; q < Q; q++) {
        const int m = opt.qtlcof_cof[q];
        while (P.chromstarts[c + 1] <= m) c++;
        lo[q] = hi[q] = m;
        for (int k = P.chromstarts[c]; k < P.chromstarts[c + 1]; k++)
            if (fabs(P.pos[k] - P.pos[m]) <= opt.qtl_window) {
                lo[q] = std::min(lo[q], (int32_t)k);
                hi[q] = std::max(hi[q], (int32_t)k);
            }
    }
    std::map<std::string, int> row_of;
    for (size_t r = 0; r < opt.pheno.ids.size(); r++) row_of[opt.pheno.ids[r]] = (int)r;
    std::vector<double>  y((size_t)N * T, NAN), cov((size_t)N * K, 0.0);
    std::vector<uint8_t> base(N, 0);
    for (int j = 0; j < N; j++) {
        const auto it = row_of.find(P.inds[P.dous[j]].name);
        if (it == row_of.end()) continue;
        const std::vector<double>& row = opt.pheno.rows[it->second];
        base[j] = 1;
        for (int k = 0; k < K; k++) {
            cov[(size_t)j * K + k] = row[opt.qtl_cov_cols[k]];
            if (row[opt.qtl_cov_cols[k]] != row[opt.qtl_cov_cols[k]]) base[j] = 0;
        }
        for (int t = 0; t < T; t++) y[(size_t)j * T + t] = row[opt.qtl_trait_cols[t]];
    }
    std::map<std::vector<uint8_t>, std::vector<int>> groups;      // pattern of use -> traits
    for (int t = 0; t < T; t++) {
        std::vector<uint8_t> u(N);
        for (int j = 0; j < N; j++) u[j] = base[j] && y[(size_t)j * T + t] == y[(size_t)j * T + t];
        groups[u].push_back(t);
    }
    const uint32_t flags = (opt.qtl_additive ? CNF2_QTL_ADDITIVE : 0) | CNF2_QTL_ORIGIN_DEVICE;
    std::vector<double>  lod((size_t)T * M), lodb((size_t)T * M), coef((size_t)T * M * NC), thr((size_t)T * 2, 0.0);
    std::vector<int32_t> rank((size_t)T * M), rankc((size_t)T * M), nused((size_t)T * C);
    std::vector<double>  nullx;            // [N][K + NC Q]: the covariates and the cofactors' columns
    const int            WN = K + NC * Q;
    for (const auto& g : groups) {
        const std::vector<int>&     tr = g.second;
        const std::vector<uint8_t>& u  = g.first;
        const int                   Tg = (int)tr.size();
        std::vector<double>  yg((size_t)N * Tg), l((size_t)Tg * M), lb((size_t)Tg * M), cf((size_t)Tg * M * NC), rss((size_t)Tg * C);
        std::vector<int32_t> rk(M), rkc(M), nu(C);
        for (int j = 0; j < N; j++)
            for (int t = 0; t < Tg; t++) yg[(size_t)j * Tg + t] = u[j] ? y[(size_t)j * T + tr[t]] : 0.0;
        int rc;
        if (!rows_kept) {          // the sweep, with the rows left in the context; its single-locus scan is not reported
            std::vector<double>  fa((size_t)N * C * 8), ll((size_t)N * C), l1((size_t)Tg * M), c1((size_t)Tg * M * 2), r1((size_t)Tg * C);
            std::vector<int32_t> k1(M), n1(C);
            rc = cnf2_sweep_qtl(ctx, 0, N, fa.data(), ll.data(), Tg, yg.data(), u.data(), K, K ? cov.data() : nullptr, 0, nullptr,
                                l1.data(), c1.data(), k1.data(), r1.data(), n1.data(), nullptr, flags & CNF2_QTL_ADDITIVE);
            if (rc != CNF2_OK) throw EngineError(CNF2_ERR_STATE, std::string("--qtlcof: ") + cnf2_last_error(ctx));
            rows_kept = true;
        }
        rc = cnf2_qtl_scan_cof(ctx, N, nullptr, Tg, yg.data(), u.data(), K, K ? cov.data() : nullptr, Q, opt.qtlcof_cof.data(), lo.data(),
                               hi.data(), 0, nullptr, l.data(), lb.data(), cf.data(), rk.data(), rkc.data(), rss.data(), nu.data(), nullptr,
                               flags);
        if (rc != CNF2_OK) throw EngineError(CNF2_ERR_STATE, std::string("--qtlcof: ") + cnf2_last_error(ctx));
        for (int t = 0; t < Tg; t++) {
            const size_t from = (size_t)t * M, to = (size_t)tr[t] * M;
            std::copy(l.begin() + from, l.begin() + from + M, lod.begin() + to);
            std::copy(lb.begin() + from, lb.begin() + from + M, lodb.begin() + to);
            std::copy(cf.begin() + from * NC, cf.begin() + (from + M) * NC, coef.begin() + to * NC);
            std::copy(rk.begin(), rk.end(), rank.begin() + to);
            std::copy(rkc.begin(), rkc.end(), rankc.begin() + to);
            std::copy(nu.begin(), nu.end(), nused.begin() + (size_t)tr[t] * C);
        }
        if (NP > 0) {
            if (nullx.empty() && WN > 0) {
                std::vector<double> rows((size_t)Q * N * 4);
                if (cnf2_qtl_kept_rows(ctx, N, Q, opt.qtlcof_cof.data(), rows.data()) != CNF2_OK)
                    throw EngineError(CNF2_ERR_STATE, std::string("--qtlcof: ") + cnf2_last_error(ctx));
                nullx.assign((size_t)N * WN, 0.0);
                for (int j = 0; j < N; j++) {
                    for (int k = 0; k < K; k++) nullx[(size_t)j * WN + k] = cov[(size_t)j * K + k];
                    for (int q = 0; q < Q; q++) {
                        const double* o = &rows[((size_t)q * N + j) * 4];
                        nullx[(size_t)j * WN + K + NC * q] = o[3] - o[0];
                        if (NC == 2) nullx[(size_t)j * WN + K + NC * q + 1] = o[1] + o[2];
                    }
                }
            }
            std::vector<int32_t> perm((size_t)NP * N);
            std::vector<double>  res((size_t)N * Tg, 0.0), pm((size_t)NP * Tg * C);
            qtl_permutations(N, NP, opt.qtl_seed, u.data(), nullptr, perm.data());
            qtlcof_null_residuals(N, Tg, yg.data(), WN, nullx.data(), u.data(), res.data());
            rc = cnf2_qtl_scan_cof(ctx, N, nullptr, Tg, res.data(), u.data(), K, K ? cov.data() : nullptr, Q, opt.qtlcof_cof.data(),
                                   lo.data(), hi.data(), NP, perm.data(), l.data(), lb.data(), cf.data(), rk.data(), rkc.data(), rss.data(),
                                   nu.data(), pm.data(), flags);
            if (rc != CNF2_OK) throw EngineError(CNF2_ERR_STATE, std::string("--qtlcof permutations: ") + cnf2_last_error(ctx));
            for (int t = 0; t < Tg; t++) {
                std::vector<double> mx(NP, 0.0);
                for (int p = 0; p < NP; p++)
                    for (int c = 0; c < C; c++) mx[p] = std::max(mx[p], pm[((size_t)p * Tg + t) * C + c]);
                thr[(size_t)tr[t] * 2]     = qtl_threshold(mx, 0.05);
                thr[(size_t)tr[t] * 2 + 1] = qtl_threshold(mx, 0.01);
            }
        }
    }
    FILE* out = fopen(opt.qtlcof.c_str(), "w");
    if (!out) throw EngineError(CNF2_ERR_STATE, "cannot write " + opt.qtlcof);
    for (int t = 0; t < T; t++) {
        fprintf(out, "%strait\t%s\n", t ? "\n" : "", opt.pheno.columns[opt.qtl_trait_cols[t]].c_str());
        if (NP > 0) fprintf(out, "threshold\tlod\t%.5lf\t%.5lf\n", thr[(size_t)t * 2], thr[(size_t)t * 2 + 1]);
        for (int c = 0; c < C; c++)
            for (int m = P.chromstarts[c]; m < P.chromstarts[c + 1]; m++) {
                const size_t at = (size_t)t * M + m;
                fprintf(out, "%d\t%.5lf\t%d\t%d\t%.5lf\t%d\t%.5lf", c + 1, P.pos[m], (int)nused[(size_t)t * C + c], (int)rankc[at], lodb[at],
                        (int)rank[at], lod[at]);
                for (int e = 0; e < NC; e++) {
                    const double v = coef[at * NC + e];
                    if (v != v) fprintf(out, "\t-");
                    else fprintf(out, "\t%.5lf", v);
                }
                fprintf(out, "\n");
            }
    }
    if (fclose(out) != 0) throw EngineError(CNF2_ERR_STATE, "cannot write " + opt.qtlcof);
}

// --qtlboot after the last round (single GPU), and after the other scans where they are given: the non-parametric bootstrap
// of the scan on chromosome --qtl-boot-chrom (cnf2_qtl_scan_boot) on the rows a cnf2_sweep_qtl left in the context -- theirs,
// or one of this function's own.  Traits are grouped by their pattern of missing values as for --qtl; a group's replicates
// draw among its own individuals (cnf2h_qtl_bootstrap_counts' rule with --qtl-seed), and one more replicate, everybody once,
// is the observed scan.  The file: per trait "name<TAB>marker<TAB>pos<TAB>pos_lo<TAB>pos_hi<TAB>lo<TAB>hi<TAB>V" -- the marker
// (map index from 0; "-" and "-" where the observed scan cannot be fitted) and position of the observed scan's largest LOD on
// the chromosome, the 95 % bootstrap interval (qtl.boot_interval: the positions number floor(0.025 V) and ceil(0.975 V) - 1
// of the V usable replicates' best positions in ascending order) as positions and as markers, four "-" when V is 0, and V;
// after a blank line per marker of the chromosome "chrom<TAB>pos" and per trait the share of the V replicates that chose it
// ("%.5lf").
static void qtlboot_scan(const Options& opt, Pedigree& P, cnf2_ctx* ctx, bool rows_kept)
{
    const int N = (int)P.dous.size(), C = (int)P.chromstarts.size() - 1;
    const int T = (int)opt.qtl_trait_cols.size(), K = (int)opt.qtl_cov_cols.size(), B = opt.qtl_boot_replicates;
    const int chrom = opt.qtl_boot_chrom - 1, first = P.chromstarts[chrom], L = P.chromstarts[chrom + 1] - first;
    std::map<std::string, int> row_of;
    for (size_t r = 0; r < opt.pheno.ids.size(); r++) row_of[opt.pheno.ids[r]] = (int)r;
    std::vector<double>  y((size_t)N * T, NAN), cov((size_t)N * K, 0.0);
    std::vector<uint8_t> base(N, 0);
    for (int j = 0; j < N; j++) {
        const auto it = row_of.find(P.inds[P.dous[j]].name);
        if (it == row_of.end()) continue;
        const std::vector<double>& row = opt.pheno.rows[it->second];
        base[j] = 1;
        for (int k = 0; k < K; k++) {
            cov[(size_t)j * K + k] = row[opt.qtl_cov_cols[k]];
            if (row[opt.qtl_cov_cols[k]] != row[opt.qtl_cov_cols[k]]) base[j] = 0;
        }
        for (int t = 0; t < T; t++) y[(size_t)j * T + t] = row[opt.qtl_trait_cols[t]];
    }
    std::map<std::vector<uint8_t>, std::vector<int>> groups;      // pattern of use -> traits
    for (int t = 0; t < T; t++) {
        std::vector<uint8_t> u(N);
        for (int j = 0; j < N; j++) u[j] = base[j] && y[(size_t)j * T + t] == y[(size_t)j * T + t];
        groups[u].push_back(t);
    }
    const uint32_t flags = (opt.qtl_additive ? CNF2_QTL_ADDITIVE : 0) | CNF2_QTL_ORIGIN_DEVICE;
    std::vector<int32_t> peak(T, -1), lo(T, -1), hi(T, -1), V(T, 0);
    std::vector<double>  share((size_t)T * L, 0.0);
    for (const auto& g : groups) {
        const std::vector<int>&     tr = g.second;
        const std::vector<uint8_t>& u  = g.first;
        const int                   Tg = (int)tr.size();
        std::vector<double> yg((size_t)N * Tg);
        for (int j = 0; j < N; j++)
            for (int t = 0; t < Tg; t++) yg[(size_t)j * Tg + t] = u[j] ? y[(size_t)j * T + tr[t]] : 0.0;
        int rc;
        if (!rows_kept) {          // the sweep, with the rows left in the context; its single-locus scan is not reported
            const int            M = P.n_markers();
            std::vector<double>  fa((size_t)N * C * 8), ll((size_t)N * C), l1((size_t)Tg * M), c1((size_t)Tg * M * 2), r1((size_t)Tg * C);
            std::vector<int32_t> k1(M), n1(C);
            rc = cnf2_sweep_qtl(ctx, 0, N, fa.data(), ll.data(), Tg, yg.data(), u.data(), K, K ? cov.data() : nullptr, 0, nullptr,
                                l1.data(), c1.data(), k1.data(), r1.data(), n1.data(), nullptr, flags & CNF2_QTL_ADDITIVE);
            if (rc != CNF2_OK) throw EngineError(CNF2_ERR_STATE, std::string("--qtlboot: ") + cnf2_last_error(ctx));
            rows_kept = true;
        }
        // replicate 0 draws everybody once: the observed scan; the B others follow
        std::vector<int32_t> count((size_t)(B + 1) * N);
        for (int j = 0; j < N; j++) count[j] = u[j] ? 1 : 0;
        qtl_bootstrap_counts(N, B, opt.qtl_seed, u.data(), nullptr, count.data() + N);
        std::vector<double>  bmax((size_t)(B + 1) * Tg);
        std::vector<int32_t> barg((size_t)(B + 1) * Tg), nb(B + 1);
        rc = cnf2_qtl_scan_boot(ctx, N, nullptr, Tg, yg.data(), u.data(), K, K ? cov.data() : nullptr, chrom, chrom + 1, B + 1,
                                count.data(), bmax.data(), barg.data(), nb.data(), nullptr, flags);
        if (rc != CNF2_OK) throw EngineError(CNF2_ERR_STATE, std::string("--qtlboot: ") + cnf2_last_error(ctx));
        for (int t = 0; t < Tg; t++) {
            const int gt = tr[t];
            peak[gt] = barg[t];
            std::vector<int32_t> kept;
            for (int b = 1; b <= B; b++)
                if (barg[(size_t)b * Tg + t] >= 0) kept.push_back(barg[(size_t)b * Tg + t]);
            V[gt] = (int32_t)kept.size();
            if (kept.empty()) continue;
            std::stable_sort(kept.begin(), kept.end(), [&](int32_t a, int32_t b) { return P.pos[a] < P.pos[b] || (P.pos[a] == P.pos[b] && a < b); });
            const int n = V[gt];
            const int k_lo = std::min(n - 1, std::max(0, (int)floor(0.025 * n + 1e-9)));
            const int k_hi = std::max(k_lo, std::min(n - 1, std::max(0, (int)ceil(0.975 * n - 1e-9) - 1)));
            lo[gt] = kept[k_lo], hi[gt] = kept[k_hi];
            for (int32_t m : kept) share[(size_t)gt * L + (m - first)] += 1.0 / n;
        }
    }
    FILE* out = fopen(opt.qtlboot.c_str(), "w");
    if (!out) throw EngineError(CNF2_ERR_STATE, "cannot write " + opt.qtlboot);
    for (int t = 0; t < T; t++) {
        fprintf(out, "%s", opt.pheno.columns[opt.qtl_trait_cols[t]].c_str());
        if (peak[t] >= 0) fprintf(out, "\t%d\t%.5lf", (int)peak[t], P.pos[peak[t]]);
        else fprintf(out, "\t-\t-");
        if (V[t] > 0) fprintf(out, "\t%.5lf\t%.5lf\t%d\t%d", P.pos[lo[t]], P.pos[hi[t]], (int)lo[t], (int)hi[t]);
        else fprintf(out, "\t-\t-\t-\t-");
        fprintf(out, "\t%d\n", (int)V[t]);
    }
    fprintf(out, "\n");
    for (int k = 0; k < L; k++) {
        fprintf(out, "%d\t%.5lf", chrom + 1, P.pos[first + k]);
        for (int t = 0; t < T; t++) fprintf(out, "\t%.5lf", share[(size_t)t * L + k]);
        fprintf(out, "\n");
    }
    if (fclose(out) != 0) throw EngineError(CNF2_ERR_STATE, "cannot write " + opt.qtlboot);
}

// --qtl-cofactors against the map, and the design's width, before anything runs: false with a message
static bool prepare_qtlcof(Options& opt, const Pedigree& P)
{
    const int          M = P.n_markers();
    std::istringstream ss(opt.qtl_cofactors);
    for (std::string tok; std::getline(ss, tok, ',');) {
        if (tok.empty()) continue;
        char*      end = nullptr;
        const long m   = strtol(tok.c_str(), &end, 10);
        if (*end != 0) {
            fprintf(stderr, "--qtl-cofactors: not a marker index: %s\n", tok.c_str());
            return false;
        }
        if (m < 0 || m >= M) {
            fprintf(stderr, "--qtl-cofactors: marker %ld is not on the map (0 .. %d)\n", m, M - 1);
            return false;
        }
        if (std::find(opt.qtlcof_cof.begin(), opt.qtlcof_cof.end(), (int32_t)m) != opt.qtlcof_cof.end()) {
            fprintf(stderr, "--qtl-cofactors: marker %ld is given twice\n", m);
            return false;
        }
        opt.qtlcof_cof.push_back((int32_t)m);
    }
    std::sort(opt.qtlcof_cof.begin(), opt.qtlcof_cof.end());
    if (opt.qtlcof_cof.empty()) {
        fprintf(stderr, "--qtlcof FILE needs --qtl-cofactors LIST\n");
        return false;
    }
    const int W = 1 + (int)opt.qtl_cov_cols.size() + (opt.qtl_additive ? 1 : 2) * ((int)opt.qtlcof_cof.size() + 1);
    if (W > cnf2::QTLX_MAXW) {
        fprintf(stderr, "--qtlcof: the design has %d columns (1 + covariates + effects x (cofactors + 1)); at most %d\n", W, cnf2::QTLX_MAXW);
        return false;
    }
    return true;
}

// the traits --qtlbin scans: the non-covariate columns whose values, where not missing, are all 0 or 1 (and not all missing)
static bool prepare_qtlbin(Options& opt)
{
    for (int col : opt.qtl_trait_cols) {
        bool binary = true, any = false;
        for (const std::vector<double>& row : opt.pheno.rows) {
            const double v = row[col];
            if (v != v) continue;
            any = true;
            if (!(v == 0.0 || v == 1.0)) binary = false;
        }
        if (binary && any) opt.qtlbin_trait_cols.push_back(col);
    }
    if (opt.qtlbin_trait_cols.empty()) {
        fprintf(stderr, "--qtlbin: no column of %s that is not a covariate holds only 0 and 1\n", opt.phenofile.c_str());
        return false;
    }
    return true;
}

// the two columns --qtlsurv scans: both named, in the table, no covariates, and the status 0 or 1 wherever it is there
static bool prepare_qtlsurv(Options& opt)
{
    const struct { const char* flag; const std::string& name; int* col; } want[2] = {
        {"--qtl-surv-time", opt.qtlsurv_time, &opt.qtlsurv_time_col}, {"--qtl-surv-status", opt.qtlsurv_status, &opt.qtlsurv_status_col}};
    for (const auto& w : want) {
        const auto it = std::find(opt.pheno.columns.begin(), opt.pheno.columns.end(), w.name);
        if (it == opt.pheno.columns.end()) {
            fprintf(stderr, "%s: \"%s\" is not a column of %s\n", w.flag, w.name.c_str(), opt.phenofile.c_str());
            return false;
        }
        *w.col = (int)(it - opt.pheno.columns.begin());
        if (std::find(opt.qtl_cov_cols.begin(), opt.qtl_cov_cols.end(), *w.col) != opt.qtl_cov_cols.end()) {
            fprintf(stderr, "%s: \"%s\" is a covariate\n", w.flag, w.name.c_str());
            return false;
        }
    }
    if (opt.qtlsurv_time_col == opt.qtlsurv_status_col) {
        fprintf(stderr, "--qtl-surv-time and --qtl-surv-status name the same column\n");
        return false;
    }
    for (const std::vector<double>& row : opt.pheno.rows) {
        const double v = row[opt.qtlsurv_status_col];
        if (v == v && !(v == 0.0 || v == 1.0)) {
            fprintf(stderr, "--qtl-surv-status: column \"%s\" holds a value that is neither 0 nor 1\n", opt.qtlsurv_status.c_str());
            return false;
        }
    }
    return true;
}

// --qtl2-every S: every S-th marker of each chromosome from its first (cnf2freq_amd/qtl.py's select_every)
static std::vector<int32_t> qtl2_select(const std::vector<int32_t>& chromstarts, int every)
{
    std::vector<int32_t> sel;
    for (size_t c = 0; c + 1 < chromstarts.size(); c++)
        for (int m = chromstarts[c]; m < chromstarts[c + 1]; m += every) sel.push_back(m);
    return sel;
}

// --phenofile against the pedigree and --qtl-covariates, before anything runs: false with a message that names what is wrong
static bool prepare_qtl(Options& opt, const Pedigree& P)
{
    std::string err;
    if (!read_pheno_table(opt.phenofile, opt.pheno, &err)) {
        fprintf(stderr, "%s\n", err.c_str());
        return false;
    }
    std::string unknown;
    for (const std::string& id : opt.pheno.ids) {
        const auto it = P.index.find(id);
        if (it == P.index.end() || it->second < 0) unknown += " " + id;
    }
    if (!unknown.empty()) {
        fprintf(stderr, "%s: not in the pedigree:%s\n", opt.phenofile.c_str(), unknown.c_str());
        return false;
    }
    std::vector<std::string> want;
    std::istringstream       ss(opt.qtl_covariates);
    for (std::string tok; std::getline(ss, tok, ',');)
        if (!tok.empty()) want.push_back(tok);
    std::string missing;
    for (const std::string& w : want) {
        const auto it = std::find(opt.pheno.columns.begin(), opt.pheno.columns.end(), w);
        if (it == opt.pheno.columns.end()) missing += " " + w;
        else opt.qtl_cov_cols.push_back((int)(it - opt.pheno.columns.begin()));
    }
    if (!missing.empty()) {
        fprintf(stderr, "--qtl-covariates: not a column of %s:%s\n", opt.phenofile.c_str(), missing.c_str());
        return false;
    }
    if (opt.qtl_cov_cols.size() > 8) {
        fprintf(stderr, "--qtl-covariates: at most 8\n");
        return false;
    }
    for (int k = 0; k < (int)opt.pheno.columns.size(); k++)
        if (std::find(opt.qtl_cov_cols.begin(), opt.qtl_cov_cols.end(), k) == opt.qtl_cov_cols.end()) opt.qtl_trait_cols.push_back(k);
    if (opt.qtl_trait_cols.empty()) {
        fprintf(stderr, "%s: every column is a covariate, no trait is left\n", opt.phenofile.c_str());
        return false;
    }
    return true;
}

// --qtl-traits against the traits of the table, and their number, before anything runs: false with a message
static bool prepare_qtlmv(Options& opt)
{
    if (!opt.qtl_traits_set) opt.qtlmv_trait_cols = opt.qtl_trait_cols;
    std::istringstream ss(opt.qtl_traits);
    for (std::string tok; std::getline(ss, tok, ',');) {
        if (tok.empty()) continue;
        const auto it = std::find(opt.pheno.columns.begin(), opt.pheno.columns.end(), tok);
        const int  k  = it == opt.pheno.columns.end() ? -1 : (int)(it - opt.pheno.columns.begin());
        if (k < 0 || std::find(opt.qtl_trait_cols.begin(), opt.qtl_trait_cols.end(), k) == opt.qtl_trait_cols.end()) {
            fprintf(stderr, "--qtl-traits: the phenotype file has no trait %s\n", tok.c_str());
            return false;
        }
        if (std::find(opt.qtlmv_trait_cols.begin(), opt.qtlmv_trait_cols.end(), k) == opt.qtlmv_trait_cols.end()) opt.qtlmv_trait_cols.push_back(k);
    }
    if (opt.qtlmv_trait_cols.empty() || (int)opt.qtlmv_trait_cols.size() > cnf2::QTLMV_MAXT) {
        fprintf(stderr, "--qtlmv takes 1 .. %d traits, not %zu\n", cnf2::QTLMV_MAXT, opt.qtlmv_trait_cols.size());
        return false;
    }
    return true;
}

// --qtlmv after the last round (single GPU), and after the other scans where they are given: the multi-trait scan
// (cnf2_qtl_scan_mv) of the traits of --qtl-traits on the rows a cnf2_sweep_qtl left in the context -- theirs, or one of this
// function's own.  Complete cases only: an individual is used when the table has it with every covariate and every one of
// the traits.  The file has the form of --qtl's: per marker "marker<TAB>chrom<TAB>pos<TAB>lod<TAB>rank" -- the map index from 0,
// the chromosome from 1, the joint LOD and the marker's rank -- and with --qtl-permutations K > 0, after a blank line,
// "joint<TAB>t5<TAB>t1", the 5 % and 1 % genome-wide thresholds of the joint LOD (the permutations move all traits of an
// individual together; with covariates the residuals of the null model are permuted, as for --qtl).
static void qtlmv_scan(const Options& opt, Pedigree& P, cnf2_ctx* ctx, bool rows_kept)
{
    const int N = (int)P.dous.size(), M = P.n_markers(), C = (int)P.chromstarts.size() - 1;
    const int T = (int)opt.qtlmv_trait_cols.size(), K = (int)opt.qtl_cov_cols.size(), NP = opt.qtl_permutations;
    std::map<std::string, int> row_of;
    for (size_t r = 0; r < opt.pheno.ids.size(); r++) row_of[opt.pheno.ids[r]] = (int)r;
    std::vector<double>  y((size_t)N * T, 0.0), cov((size_t)N * K, 0.0);
    std::vector<uint8_t> u(N, 0);
    for (int j = 0; j < N; j++) {
        const auto it = row_of.find(P.inds[P.dous[j]].name);
        if (it == row_of.end()) continue;
        const std::vector<double>& row = opt.pheno.rows[it->second];
        u[j] = 1;
        for (int k = 0; k < K; k++) {
            cov[(size_t)j * K + k] = row[opt.qtl_cov_cols[k]];
            if (!std::isfinite(row[opt.qtl_cov_cols[k]])) u[j] = 0;
        }
        for (int t = 0; t < T; t++)
            if (!std::isfinite(row[opt.qtlmv_trait_cols[t]])) u[j] = 0;
        for (int t = 0; t < T; t++) y[(size_t)j * T + t] = u[j] ? row[opt.qtlmv_trait_cols[t]] : 0.0;
    }
    const uint32_t flags = (opt.qtl_additive ? CNF2_QTL_ADDITIVE : 0) | CNF2_QTL_ORIGIN_DEVICE;
    int rc;
    if (!rows_kept) {          // the sweep, with the rows left in the context; its single-locus scan is not reported
        std::vector<double>  fa((size_t)N * C * 8), ll((size_t)N * C), y1(N), l1(M), c1((size_t)M * 2), r1(C);
        std::vector<int32_t> k1(M), n1(C);
        for (int j = 0; j < N; j++) y1[j] = y[(size_t)j * T];
        rc = cnf2_sweep_qtl(ctx, 0, N, fa.data(), ll.data(), 1, y1.data(), u.data(), K, K ? cov.data() : nullptr, 0, nullptr, l1.data(),
                            c1.data(), k1.data(), r1.data(), n1.data(), nullptr, flags & CNF2_QTL_ADDITIVE);
        if (rc != CNF2_OK) throw EngineError(CNF2_ERR_STATE, std::string("--qtlmv: ") + cnf2_last_error(ctx));
    }
    std::vector<double>  lod(M, 0.0), thr(2, 0.0);
    std::vector<int32_t> rank(M, 0), trank(C, 0), nused(C, 0);
    rc = cnf2_qtl_scan_mv(ctx, N, nullptr, T, y.data(), u.data(), K, K ? cov.data() : nullptr, 0, nullptr, lod.data(), rank.data(),
                          trank.data(), nused.data(), nullptr, flags);
    if (rc != CNF2_OK) throw EngineError(CNF2_ERR_STATE, std::string("--qtlmv: ") + cnf2_last_error(ctx));
    if (NP > 0) {
        std::vector<int32_t> perm((size_t)NP * N), rk(M), tr(C), nu(C);
        std::vector<double>  res(y), l(M), pm((size_t)NP * C);
        qtl_permutations(N, NP, opt.qtl_seed, u.data(), nullptr, perm.data());
        // (as for --qtl: with too few individuals nothing is scanned, whatever is permuted; with enough of them a null design
        // without full rank is an error, not thresholds of 0)
        const int n_u = (int)std::count(u.begin(), u.end(), (uint8_t)1);
        if (K > 0 && n_u >= K + 4 && !qtl_null_residuals(N, T, y.data(), K, cov.data(), u.data(), res.data()))
            throw EngineError(CNF2_ERR_ARG, "--qtl-permutations: the null design (intercept and covariates) of the individuals used for --qtlmv has no full rank");
        rc = cnf2_qtl_scan_mv(ctx, N, nullptr, T, res.data(), u.data(), K, K ? cov.data() : nullptr, NP, perm.data(), l.data(), rk.data(),
                              tr.data(), nu.data(), pm.data(), flags);
        if (rc != CNF2_OK) throw EngineError(CNF2_ERR_STATE, std::string("--qtlmv permutations: ") + cnf2_last_error(ctx));
        std::vector<double> mx(NP, 0.0);
        for (int p = 0; p < NP; p++)
            for (int c = 0; c < C; c++) mx[p] = std::max(mx[p], pm[(size_t)p * C + c]);
        thr[0] = qtl_threshold(mx, 0.05);
        thr[1] = qtl_threshold(mx, 0.01);
    }
    FILE* out = fopen(opt.qtlmv.c_str(), "w");
    if (!out) throw EngineError(CNF2_ERR_STATE, "cannot write " + opt.qtlmv);
    for (int c = 0; c < C; c++)
        for (int m = P.chromstarts[c]; m < P.chromstarts[c + 1]; m++)
            fprintf(out, "%d\t%d\t%.5lf\t%.5lf\t%d\n", m, c + 1, P.pos[m], lod[m], (int)rank[m]);
    if (NP > 0) fprintf(out, "\njoint\t%.5lf\t%.5lf\n", thr[0], thr[1]);
    if (fclose(out) != 0) throw EngineError(CNF2_ERR_STATE, "cannot write " + opt.qtlmv);
}

// --qtl-var-covariates against --qtl-covariates, before anything runs: false with a message.  The variance covariates come
// first in the order given, then the other covariates.
static bool prepare_qtlvar(Options& opt)
{
    std::istringstream ss(opt.qtlvar_covariates);
    std::string        missing;
    for (std::string tok; std::getline(ss, tok, ',');) {
        if (tok.empty()) continue;
        const auto it = std::find(opt.pheno.columns.begin(), opt.pheno.columns.end(), tok);
        const int  k  = it == opt.pheno.columns.end() ? -1 : (int)(it - opt.pheno.columns.begin());
        if (k < 0 || std::find(opt.qtl_cov_cols.begin(), opt.qtl_cov_cols.end(), k) == opt.qtl_cov_cols.end()) missing += " " + tok;
        else if (std::find(opt.qtlvar_cov_cols.begin(), opt.qtlvar_cov_cols.end(), k) == opt.qtlvar_cov_cols.end()) opt.qtlvar_cov_cols.push_back(k);
    }
    if (!missing.empty()) {
        fprintf(stderr, "--qtl-var-covariates: not among --qtl-covariates:%s\n", missing.c_str());
        return false;
    }
    opt.qtlvar_n_var = (int)opt.qtlvar_cov_cols.size();
    if (opt.qtlvar_n_var > cnf2::QTLVAR_MAXV) {
        fprintf(stderr, "--qtl-var-covariates: at most %d\n", cnf2::QTLVAR_MAXV);
        return false;
    }
    for (int k : opt.qtl_cov_cols)
        if (std::find(opt.qtlvar_cov_cols.begin(), opt.qtlvar_cov_cols.end(), k) == opt.qtlvar_cov_cols.end()) opt.qtlvar_cov_cols.push_back(k);
    return true;
}

// --qtl-interactive against --qtl-covariates, and the design's width, before anything runs: false with a message
static bool prepare_qtlx(Options& opt)
{
    std::istringstream ss(opt.qtl_interactive);
    std::string        missing;
    for (std::string tok; std::getline(ss, tok, ',');) {
        if (tok.empty()) continue;
        const auto it = std::find(opt.pheno.columns.begin(), opt.pheno.columns.end(), tok);
        const int  k  = it == opt.pheno.columns.end() ? -1 : (int)(it - opt.pheno.columns.begin());
        if (k < 0 || std::find(opt.qtl_cov_cols.begin(), opt.qtl_cov_cols.end(), k) == opt.qtl_cov_cols.end()) missing += " " + tok;
        else if (std::find(opt.qtlx_cov_cols.begin(), opt.qtlx_cov_cols.end(), k) == opt.qtlx_cov_cols.end()) opt.qtlx_cov_cols.push_back(k);
    }
    if (!missing.empty()) {
        fprintf(stderr, "--qtl-interactive: not among --qtl-covariates:%s\n", missing.c_str());
        return false;
    }
    opt.qtlx_n_int = (int)opt.qtlx_cov_cols.size();
    for (int k : opt.qtl_cov_cols)
        if (std::find(opt.qtlx_cov_cols.begin(), opt.qtlx_cov_cols.end(), k) == opt.qtlx_cov_cols.end()) opt.qtlx_cov_cols.push_back(k);
    const cnf2::QtlxDesign ds = cnf2::qtlx_design((int)opt.qtlx_cov_cols.size(), opt.qtlx_n_int, opt.qtl_additive, opt.qtl_imprint);
    if (ds.w > cnf2::QTLX_MAXW) {
        fprintf(stderr, "--qtlx: the design has %d columns (1 + covariates + effects x (1 + interactive covariates)); at most %d\n", ds.w,
                cnf2::QTLX_MAXW);
        return false;
    }
    return true;
}

// --qtl after the last round (single GPU), like --origins: the traits grouped by their pattern of missing values, the first
// group through cnf2_sweep_qtl, the others and the permutations on the rows that call left in the context
static void qtl_scan(const Options& opt, Pedigree& P, cnf2_ctx* ctx)
{
    const int N = (int)P.dous.size(), M = P.n_markers(), C = (int)P.chromstarts.size() - 1;
    const int T = (int)opt.qtl_trait_cols.size(), K = (int)opt.qtl_cov_cols.size(), NP = opt.qtl_permutations;
    std::map<std::string, int> row_of;
    for (size_t r = 0; r < opt.pheno.ids.size(); r++) row_of[opt.pheno.ids[r]] = (int)r;
    std::vector<double>  y((size_t)N * T, NAN), cov((size_t)N * K, 0.0);
    std::vector<uint8_t> base(N, 0);
    for (int j = 0; j < N; j++) {
        const auto it = row_of.find(P.inds[P.dous[j]].name);
        if (it == row_of.end()) continue;
        const std::vector<double>& row = opt.pheno.rows[it->second];
        base[j] = 1;
        for (int k = 0; k < K; k++) {
            cov[(size_t)j * K + k] = row[opt.qtl_cov_cols[k]];
            if (row[opt.qtl_cov_cols[k]] != row[opt.qtl_cov_cols[k]]) base[j] = 0;
        }
        for (int t = 0; t < T; t++) y[(size_t)j * T + t] = row[opt.qtl_trait_cols[t]];
    }
    std::vector<double>  lod((size_t)T * M, 0.0), coef((size_t)T * M * 2, NAN), thr((size_t)T * 2, 0.0);
    std::vector<int32_t> rank0(M, 0), nused0(C, 0);
    std::map<std::vector<uint8_t>, std::vector<int>> groups;      // pattern of use -> traits
    for (int t = 0; t < T; t++) {
        std::vector<uint8_t> u(N);
        for (int j = 0; j < N; j++) u[j] = base[j] && y[(size_t)j * T + t] == y[(size_t)j * T + t];
        groups[u].push_back(t);
    }
    std::vector<std::vector<int>> order;                           // the first trait's group first
    std::vector<std::vector<uint8_t>> uses;
    for (const auto& g : groups)
        if (g.second[0] == 0) order.insert(order.begin(), g.second), uses.insert(uses.begin(), g.first);
        else order.push_back(g.second), uses.push_back(g.first);
    const uint32_t flags = opt.qtl_additive ? CNF2_QTL_ADDITIVE : 0;
    bool swept = false;
    for (size_t g = 0; g < order.size(); g++) {
        const std::vector<int>&     tr = order[g];
        const std::vector<uint8_t>& u  = uses[g];
        const int                   Tg = (int)tr.size();
        std::vector<double>  yg((size_t)N * Tg), l((size_t)Tg * M), cf((size_t)Tg * M * 2), rss((size_t)Tg * C);
        std::vector<int32_t> rk(M), nu(C);
        for (int j = 0; j < N; j++)
            for (int t = 0; t < Tg; t++) yg[(size_t)j * Tg + t] = u[j] ? y[(size_t)j * T + tr[t]] : 0.0;
        int rc;
        if (!swept) {
            std::vector<double> f((size_t)N * C * 8), ll((size_t)N * C);
            rc = cnf2_sweep_qtl(ctx, 0, N, f.data(), ll.data(), Tg, yg.data(), u.data(), K, K ? cov.data() : nullptr, 0, nullptr,
                                l.data(), cf.data(), rk.data(), rss.data(), nu.data(), nullptr, flags);
            swept = true;
        } else
            rc = cnf2_qtl_scan(ctx, N, nullptr, Tg, yg.data(), u.data(), K, K ? cov.data() : nullptr, 0, nullptr, l.data(), cf.data(),
                               rk.data(), rss.data(), nu.data(), nullptr, flags | CNF2_QTL_ORIGIN_DEVICE);
        if (rc != CNF2_OK) throw EngineError(CNF2_ERR_STATE, std::string("--qtl: ") + cnf2_last_error(ctx));
        if (g == 0) rank0 = rk, nused0 = nu;
        for (int t = 0; t < Tg; t++) {
            std::copy(l.begin() + (size_t)t * M, l.begin() + (size_t)(t + 1) * M, lod.begin() + (size_t)tr[t] * M);
            std::copy(cf.begin() + (size_t)t * M * 2, cf.begin() + (size_t)(t + 1) * M * 2, coef.begin() + (size_t)tr[t] * M * 2);
        }
        if (NP > 0) {
            std::vector<int32_t> perm((size_t)NP * N);
            std::vector<double>  res((size_t)N * Tg, 0.0), pm((size_t)NP * Tg * C);
            qtl_permutations(N, NP, opt.qtl_seed, u.data(), nullptr, perm.data());
            // (with fewer than K + 4 individuals nothing is scanned and every maximum is 0, whatever is permuted: the residuals
            // stay 0; with enough of them a null design without full rank -- a constant covariate -- is an error, not zeros)
            const int n_u = (int)std::count(u.begin(), u.end(), (uint8_t)1);
            if (n_u >= K + 4 && !qtl_null_residuals(N, Tg, yg.data(), K, K ? cov.data() : nullptr, u.data(), res.data()))
                throw EngineError(CNF2_ERR_ARG, "--qtl-permutations: the null design (intercept and covariates) of the individuals used for " +
                                                    opt.pheno.columns[opt.qtl_trait_cols[tr[0]]] + " has no full rank");
            rc = cnf2_qtl_scan(ctx, N, nullptr, Tg, res.data(), u.data(), K, K ? cov.data() : nullptr, NP, perm.data(), l.data(),
                               cf.data(), rk.data(), rss.data(), nu.data(), pm.data(), flags | CNF2_QTL_ORIGIN_DEVICE);
            if (rc != CNF2_OK) throw EngineError(CNF2_ERR_STATE, std::string("--qtl permutations: ") + cnf2_last_error(ctx));
            for (int t = 0; t < Tg; t++) {
                std::vector<double> mx(NP, 0.0);
                for (int p = 0; p < NP; p++)
                    for (int c = 0; c < C; c++) mx[p] = std::max(mx[p], pm[((size_t)p * Tg + t) * C + c]);
                thr[(size_t)tr[t] * 2]     = qtl_threshold(mx, 0.05);
                thr[(size_t)tr[t] * 2 + 1] = qtl_threshold(mx, 0.01);
            }
        }
    }
    FILE* out = fopen(opt.qtl.c_str(), "w");
    if (!out) throw EngineError(CNF2_ERR_STATE, "cannot write " + opt.qtl);
    auto effect = [&](double v) {
        if (v != v) fprintf(out, "\t-");
        else fprintf(out, "\t%.5lf", v);
    };
    for (int c = 0; c < C; c++)
        for (int m = P.chromstarts[c]; m < P.chromstarts[c + 1]; m++) {
            fprintf(out, "%d\t%.5lf\t%d\t%d", c + 1, P.pos[m], (int)nused0[c], (int)rank0[m]);
            for (int t = 0; t < T; t++) {
                fprintf(out, "\t%.5lf", lod[(size_t)t * M + m]);
                effect(coef[((size_t)t * M + m) * 2]);
                effect(coef[((size_t)t * M + m) * 2 + 1]);
            }
            fprintf(out, "\n");
        }
    if (NP > 0) {
        fprintf(out, "\n");
        for (int t = 0; t < T; t++)
            fprintf(out, "%s\t%.5lf\t%.5lf\n", opt.pheno.columns[opt.qtl_trait_cols[t]].c_str(), thr[(size_t)t * 2], thr[(size_t)t * 2 + 1]);
    }
    if (fclose(out) != 0) throw EngineError(CNF2_ERR_STATE, "cannot write " + opt.qtl);
}

// --qtlfam after the last round (single GPU) and after the scans above: per side of --qtl-fam-side and per pattern of missing
// values the within-family scan (cnf2_qtl_scan_fam) of its traits on the rows a cnf2_sweep_qtl left in the context -- theirs,
// or one of this function's own.  The slope group of an individual is its parent on the side and its mean cell that parent
// (--qtl-cell parent) or its pair of parents (--qtl-cell pair, the default), by cnf2h_qtl_families' rule; an individual whose
// parent on the side has no recorded parents is not used.  With --qtl-permutations the residuals of the null model -- cell
// means and covariates -- are permuted inside the cells.  The file has the form of --qtl's: per marker
// "chrom<TAB>pos", then per side "n_used<TAB>n_cells<TAB>df" of the first trait's pattern -- the individuals used on the
// chromosome, the cells among them, the fitted families -- and per trait its LOD; after a blank line per trait
// "name<TAB>t5<TAB>t1" per side.  The table and the grouping are --qtl's (qtl_scan above).
static void qtlfam_scan(const Options& opt, Pedigree& P, cnf2_ctx* ctx, bool rows_kept)
{
    const int N = (int)P.dous.size(), M = P.n_markers(), C = (int)P.chromstarts.size() - 1;
    const int T = (int)opt.qtl_trait_cols.size(), K = (int)opt.qtl_cov_cols.size(), NP = opt.qtl_permutations;
    std::map<std::string, int> row_of;
    for (size_t r = 0; r < opt.pheno.ids.size(); r++) row_of[opt.pheno.ids[r]] = (int)r;
    std::vector<double>  y((size_t)N * T, NAN), cov((size_t)N * K, 0.0);
    std::vector<uint8_t> base(N, 0);
    for (int j = 0; j < N; j++) {
        const auto it = row_of.find(P.inds[P.dous[j]].name);
        if (it == row_of.end()) continue;
        const std::vector<double>& row = opt.pheno.rows[it->second];
        base[j] = 1;
        for (int k = 0; k < K; k++) {
            cov[(size_t)j * K + k] = row[opt.qtl_cov_cols[k]];
            if (row[opt.qtl_cov_cols[k]] != row[opt.qtl_cov_cols[k]]) base[j] = 0;
        }
        for (int t = 0; t < T; t++) y[(size_t)j * T + t] = row[opt.qtl_trait_cols[t]];
    }
    if (!rows_kept) {          // the sweep, with the rows left in the context; its single-locus scan is not reported
        std::vector<double>  fa((size_t)N * C * 8), ll((size_t)N * C), y1(N, 0.0), l1(M), c1((size_t)M * 2), r1(C);
        std::vector<int32_t> k1(M), n1(C);
        if (cnf2_sweep_qtl(ctx, 0, N, fa.data(), ll.data(), 1, y1.data(), nullptr, 0, nullptr, 0, nullptr, l1.data(), c1.data(), k1.data(),
                           r1.data(), n1.data(), nullptr, 0) != CNF2_OK)
            throw EngineError(CNF2_ERR_STATE, std::string("--qtlfam: ") + cnf2_last_error(ctx));
    }
    std::vector<int32_t> par((size_t)P.inds.size() * 2), dous(P.dous.begin(), P.dous.end());
    for (size_t r = 0; r < P.inds.size(); r++) par[2 * r] = P.inds[r].pars[0], par[2 * r + 1] = P.inds[r].pars[1];
    std::vector<int> sides;
    if (opt.qtl_fam_side != "second") sides.push_back(0);
    if (opt.qtl_fam_side != "first") sides.push_back(1);
    const int NS = (int)sides.size();
    std::vector<double>  lod((size_t)NS * T * M, 0.0), thr((size_t)NS * T * 2, 0.0);
    std::vector<int32_t> df0((size_t)NS * M, 0), nused0((size_t)NS * C, 0), ncells0((size_t)NS * C, 0);
    for (int s = 0; s < NS; s++) {
        std::vector<int32_t> grp(N), pairs(N);
        const int            F = std::max(1, qtl_families(par.data(), N, dous.data(), sides[s], grp.data(), pairs.data()));
        const std::vector<int32_t>& cell = opt.qtl_cell == "pair" ? pairs : grp;
        std::map<std::vector<uint8_t>, std::vector<int>> groups;      // pattern of use -> traits
        for (int t = 0; t < T; t++) {
            std::vector<uint8_t> u(N);
            for (int j = 0; j < N; j++) u[j] = base[j] && grp[j] >= 0 && y[(size_t)j * T + t] == y[(size_t)j * T + t];
            groups[u].push_back(t);
        }
        for (const auto& g : groups) {
            const std::vector<int>&     tr = g.second;
            const std::vector<uint8_t>& u  = g.first;
            const int                   Tg = (int)tr.size();
            std::vector<double>  yg((size_t)N * Tg), l((size_t)Tg * M), rss((size_t)Tg * C);
            std::vector<int32_t> df(M), nu(C), nq(C);
            for (int j = 0; j < N; j++)
                for (int t = 0; t < Tg; t++) yg[(size_t)j * Tg + t] = u[j] ? y[(size_t)j * T + tr[t]] : 0.0;
            int rc = cnf2_qtl_scan_fam(ctx, N, nullptr, sides[s], grp.data(), cell.data(), F, Tg, yg.data(), u.data(), K, K ? cov.data() : nullptr,
                                       0, nullptr, l.data(), df.data(), nullptr, rss.data(), nu.data(), nq.data(), nullptr, CNF2_QTL_ORIGIN_DEVICE);
            if (rc != CNF2_OK) throw EngineError(CNF2_ERR_STATE, std::string("--qtlfam: ") + cnf2_last_error(ctx));
            if (tr[0] == 0) {
                std::copy(df.begin(), df.end(), df0.begin() + (size_t)s * M);
                std::copy(nu.begin(), nu.end(), nused0.begin() + (size_t)s * C);
                std::copy(nq.begin(), nq.end(), ncells0.begin() + (size_t)s * C);
            }
            for (int t = 0; t < Tg; t++) std::copy(l.begin() + (size_t)t * M, l.begin() + (size_t)(t + 1) * M, lod.begin() + ((size_t)s * T + tr[t]) * M);
            if (NP > 0) {
                std::vector<int32_t> perm((size_t)NP * N);
                std::vector<double>  res((size_t)N * Tg, 0.0), pm((size_t)NP * Tg * C);
                qtl_permutations(N, NP, opt.qtl_seed, u.data(), cell.data(), perm.data());
                // (a null design without full rank -- a covariate constant within every cell -- leaves the residuals 0: nothing
                // is scanned then, and every maximum is 0 whatever is permuted)
                qtl_cell_residuals(N, Tg, yg.data(), K, cov.data(), u.data(), cell.data(), res.data());
                rc = cnf2_qtl_scan_fam(ctx, N, nullptr, sides[s], grp.data(), cell.data(), F, Tg, res.data(), u.data(), K, K ? cov.data() : nullptr,
                                       NP, perm.data(), l.data(), df.data(), nullptr, rss.data(), nu.data(), nq.data(), pm.data(),
                                       CNF2_QTL_ORIGIN_DEVICE);
                if (rc != CNF2_OK) throw EngineError(CNF2_ERR_STATE, std::string("--qtlfam permutations: ") + cnf2_last_error(ctx));
                for (int t = 0; t < Tg; t++) {
                    std::vector<double> mx(NP, 0.0);
                    for (int p = 0; p < NP; p++)
                        for (int c = 0; c < C; c++) mx[p] = std::max(mx[p], pm[((size_t)p * Tg + t) * C + c]);
                    thr[((size_t)s * T + tr[t]) * 2]     = qtl_threshold(mx, 0.05);
                    thr[((size_t)s * T + tr[t]) * 2 + 1] = qtl_threshold(mx, 0.01);
                }
            }
        }
    }
    FILE* out = fopen(opt.qtlfam.c_str(), "w");
    if (!out) throw EngineError(CNF2_ERR_STATE, "cannot write " + opt.qtlfam);
    for (int c = 0; c < C; c++)
        for (int m = P.chromstarts[c]; m < P.chromstarts[c + 1]; m++) {
            fprintf(out, "%d\t%.5lf", c + 1, P.pos[m]);
            for (int s = 0; s < NS; s++) {
                fprintf(out, "\t%d\t%d\t%d", (int)nused0[(size_t)s * C + c], (int)ncells0[(size_t)s * C + c], (int)df0[(size_t)s * M + m]);
                for (int t = 0; t < T; t++) fprintf(out, "\t%.5lf", lod[((size_t)s * T + t) * M + m]);
            }
            fprintf(out, "\n");
        }
    if (NP > 0) {
        fprintf(out, "\n");
        for (int t = 0; t < T; t++) {
            fprintf(out, "%s", opt.pheno.columns[opt.qtl_trait_cols[t]].c_str());
            for (int s = 0; s < NS; s++) fprintf(out, "\t%.5lf\t%.5lf", thr[((size_t)s * T + t) * 2], thr[((size_t)s * T + t) * 2 + 1]);
            fprintf(out, "\n");
        }
    }
    if (fclose(out) != 0) throw EngineError(CNF2_ERR_STATE, "cannot write " + opt.qtlfam);
}

// --qtlhap after the last round (single GPU) and after the scans above: one descent sweep (cnf2_sweep_descent), the column map
// of --qtl-hap-by (cnf2h_descent_columns' rule: haplotype, the default, an effect per founder haplotype; founder; line), then
// per pattern of missing values the founder-haplotype scan (cnf2_qtl_scan_hap) of its traits, and with --qtl-permutations one
// more on the permuted residuals of the null model.  An individual with a parent without two recorded parents is not used.
// More than 16 phased grandparents (32 columns) are refused: the within-family scan (--qtlfam) is the tool then.  The file
// has the form of --qtl's: per marker "chrom<TAB>pos<TAB>n_used<TAB>df" of the first trait's pattern -- the individuals used
// on the chromosome, the columns kept -- and per trait its LOD; after a blank line per trait "name<TAB>t5<TAB>t1".
static void qtlhap_scan(const Options& opt, Pedigree& P, cnf2_ctx* ctx)
{
    const int N = (int)P.dous.size(), M = P.n_markers(), C = (int)P.chromstarts.size() - 1;
    const int T = (int)opt.qtl_trait_cols.size(), K = (int)opt.qtl_cov_cols.size(), NP = opt.qtl_permutations;
    std::map<std::string, int> row_of;
    for (size_t r = 0; r < opt.pheno.ids.size(); r++) row_of[opt.pheno.ids[r]] = (int)r;
    std::vector<double>  y((size_t)N * T, NAN), cov((size_t)N * K, 0.0);
    std::vector<uint8_t> base(N, 0);
    for (int j = 0; j < N; j++) {
        const auto it = row_of.find(P.inds[P.dous[j]].name);
        if (it == row_of.end()) continue;
        const std::vector<double>& row = opt.pheno.rows[it->second];
        base[j] = 1;
        for (int k = 0; k < K; k++) {
            cov[(size_t)j * K + k] = row[opt.qtl_cov_cols[k]];
            if (row[opt.qtl_cov_cols[k]] != row[opt.qtl_cov_cols[k]]) base[j] = 0;
        }
        for (int t = 0; t < T; t++) y[(size_t)j * T + t] = row[opt.qtl_trait_cols[t]];
    }
    std::vector<double> rows((size_t)N * M * 8);
    {
        std::vector<double>  fa((size_t)N * C * 8), ll((size_t)N * C);
        std::vector<int32_t> cnt(C);
        if (cnf2_sweep_descent(ctx, 0, N, fa.data(), ll.data(), rows.data(), cnt.data(), 0) != CNF2_OK)
            throw EngineError(CNF2_ERR_STATE, std::string("--qtlhap: ") + cnf2_last_error(ctx));
    }
    std::vector<int32_t> par((size_t)P.inds.size() * 2), dous(P.dous.begin(), P.dous.end()), col((size_t)N * 8);
    for (size_t r = 0; r < P.inds.size(); r++) par[2 * r] = P.inds[r].pars[0], par[2 * r + 1] = P.inds[r].pars[1];
    const int by = opt.qtl_hap_by == "haplotype" ? 0 : opt.qtl_hap_by == "founder" ? 1 : 2;
    const int G  = descent_columns(par.data(), N, dous.data(), by, col.data());
    const int H  = std::max(1, by == 0 ? 2 * G : by == 1 ? G : 2);
    if (H > 32)
        throw EngineError(CNF2_ERR_STATE, "--qtlhap: " + std::to_string(G) + " grandparents give " + std::to_string(H) +
                                              " columns, and the scan takes 32: use --qtl-hap-by founder or line, or --qtlfam");
    std::vector<uint8_t> inmodel(N);
    for (int j = 0; j < N; j++) {
        inmodel[j] = base[j];
        for (int k = 0; k < 8; k++) inmodel[j] = inmodel[j] && col[(size_t)j * 8 + k] >= 0;
    }
    std::vector<double>  lod((size_t)T * M, 0.0), thr((size_t)T * 2, 0.0);
    std::vector<int32_t> df0(M, 0), nused0(C, 0);
    std::map<std::vector<uint8_t>, std::vector<int>> groups;      // pattern of use -> traits
    for (int t = 0; t < T; t++) {
        std::vector<uint8_t> u(N);
        for (int j = 0; j < N; j++) u[j] = inmodel[j] && y[(size_t)j * T + t] == y[(size_t)j * T + t];
        groups[u].push_back(t);
    }
    for (const auto& g : groups) {
        const std::vector<int>&     tr = g.second;
        const std::vector<uint8_t>& u  = g.first;
        const int                   Tg = (int)tr.size();
        std::vector<double>  yg((size_t)N * Tg), l((size_t)Tg * M), rss((size_t)Tg * C);
        std::vector<int32_t> df(M), nu(C);
        for (int j = 0; j < N; j++)
            for (int t = 0; t < Tg; t++) yg[(size_t)j * Tg + t] = u[j] ? y[(size_t)j * T + tr[t]] : 0.0;
        int rc = cnf2_qtl_scan_hap(ctx, N, rows.data(), col.data(), H, Tg, yg.data(), u.data(), K, K ? cov.data() : nullptr, 0, nullptr,
                                   l.data(), df.data(), nullptr, rss.data(), nu.data(), nullptr, 0);
        if (rc != CNF2_OK) throw EngineError(CNF2_ERR_STATE, std::string("--qtlhap: ") + cnf2_last_error(ctx));
        if (tr[0] == 0) {
            df0    = df;
            nused0 = nu;
        }
        for (int t = 0; t < Tg; t++) std::copy(l.begin() + (size_t)t * M, l.begin() + (size_t)(t + 1) * M, lod.begin() + (size_t)tr[t] * M);
        if (NP > 0) {
            std::vector<int32_t> perm((size_t)NP * N);
            std::vector<double>  res((size_t)N * Tg, 0.0), pm((size_t)NP * Tg * C);
            qtl_permutations(N, NP, opt.qtl_seed, u.data(), nullptr, perm.data());
            qtl_null_residuals(N, Tg, yg.data(), K, cov.data(), u.data(), res.data());
            rc = cnf2_qtl_scan_hap(ctx, N, rows.data(), col.data(), H, Tg, res.data(), u.data(), K, K ? cov.data() : nullptr, NP, perm.data(),
                                   l.data(), df.data(), nullptr, rss.data(), nu.data(), pm.data(), 0);
            if (rc != CNF2_OK) throw EngineError(CNF2_ERR_STATE, std::string("--qtlhap permutations: ") + cnf2_last_error(ctx));
            for (int t = 0; t < Tg; t++) {
                std::vector<double> mx(NP, 0.0);
                for (int p = 0; p < NP; p++)
                    for (int c = 0; c < C; c++) mx[p] = std::max(mx[p], pm[((size_t)p * Tg + t) * C + c]);
                thr[(size_t)tr[t] * 2]     = qtl_threshold(mx, 0.05);
                thr[(size_t)tr[t] * 2 + 1] = qtl_threshold(mx, 0.01);
            }
        }
    }
    FILE* out = fopen(opt.qtlhap.c_str(), "w");
    if (!out) throw EngineError(CNF2_ERR_STATE, "cannot write " + opt.qtlhap);
    for (int c = 0; c < C; c++)
        for (int m = P.chromstarts[c]; m < P.chromstarts[c + 1]; m++) {
            fprintf(out, "%d\t%.5lf\t%d\t%d", c + 1, P.pos[m], (int)nused0[c], (int)df0[m]);
            for (int t = 0; t < T; t++) fprintf(out, "\t%.5lf", lod[(size_t)t * M + m]);
            fprintf(out, "\n");
        }
    if (NP > 0) {
        fprintf(out, "\n");
        for (int t = 0; t < T; t++)
            fprintf(out, "%s\t%.5lf\t%.5lf\n", opt.pheno.columns[opt.qtl_trait_cols[t]].c_str(), thr[(size_t)t * 2], thr[(size_t)t * 2 + 1]);
    }
    if (fclose(out) != 0) throw EngineError(CNF2_ERR_STATE, "cannot write " + opt.qtlhap);
}

// --qtlvc after the last round (single GPU) and after the scans above: one descent sweep, the column map of --qtl-vc-by
// (cnf2h_descent_columns' rule), then per pattern of missing values the variance-component scan (cnf2_qtl_scan_vc: random
// founder-haplotype effects, one variance component per locus) of its traits, and with --qtl-permutations one more on the
// permuted residuals of the null model.  An individual with a parent without two recorded parents is not used.  More than 32
// phased grandparents (64 columns) are refused with the count.  The file has the form of --qtl's: per marker
// "chrom<TAB>pos<TAB>n_used<TAB>rank" of the first trait's pattern -- the individuals used on the chromosome, the rank of the
// marker's design -- and per trait its LOD and h, the locus' share of the variance; after a blank line per trait
// "name<TAB>t5<TAB>t1".
static void qtlvc_scan(const Options& opt, Pedigree& P, cnf2_ctx* ctx)
{
    const int N = (int)P.dous.size(), M = P.n_markers(), C = (int)P.chromstarts.size() - 1;
    const int T = (int)opt.qtl_trait_cols.size(), K = (int)opt.qtl_cov_cols.size(), NP = opt.qtl_permutations;
    std::map<std::string, int> row_of;
    for (size_t r = 0; r < opt.pheno.ids.size(); r++) row_of[opt.pheno.ids[r]] = (int)r;
    std::vector<double>  y((size_t)N * T, NAN), cov((size_t)N * K, 0.0);
    std::vector<uint8_t> base(N, 0);
    for (int j = 0; j < N; j++) {
        const auto it = row_of.find(P.inds[P.dous[j]].name);
        if (it == row_of.end()) continue;
        const std::vector<double>& row = opt.pheno.rows[it->second];
        base[j] = 1;
        for (int k = 0; k < K; k++) {
            cov[(size_t)j * K + k] = row[opt.qtl_cov_cols[k]];
            if (row[opt.qtl_cov_cols[k]] != row[opt.qtl_cov_cols[k]]) base[j] = 0;
        }
        for (int t = 0; t < T; t++) y[(size_t)j * T + t] = row[opt.qtl_trait_cols[t]];
    }
    std::vector<int32_t> par((size_t)P.inds.size() * 2), dous(P.dous.begin(), P.dous.end()), col((size_t)N * 8);
    for (size_t r = 0; r < P.inds.size(); r++) par[2 * r] = P.inds[r].pars[0], par[2 * r + 1] = P.inds[r].pars[1];
    const int by = opt.qtl_vc_by == "haplotype" ? 0 : opt.qtl_vc_by == "founder" ? 1 : 2;
    const int G  = descent_columns(par.data(), N, dous.data(), by, col.data());
    const int H  = std::max(1, by == 0 ? 2 * G : by == 1 ? G : 2);
    if (H > 64)
        throw EngineError(CNF2_ERR_STATE, "--qtlvc: " + std::to_string(G) + " grandparents give " + std::to_string(H) +
                                              " columns, and the scan takes 64: use --qtl-vc-by founder or line");
    std::vector<double> rows((size_t)N * M * 8);
    {
        std::vector<double>  fa((size_t)N * C * 8), ll((size_t)N * C);
        std::vector<int32_t> cnt(C);
        if (cnf2_sweep_descent(ctx, 0, N, fa.data(), ll.data(), rows.data(), cnt.data(), 0) != CNF2_OK)
            throw EngineError(CNF2_ERR_STATE, std::string("--qtlvc: ") + cnf2_last_error(ctx));
    }
    std::vector<uint8_t> inmodel(N);
    for (int j = 0; j < N; j++) {
        inmodel[j] = base[j];
        for (int k = 0; k < 8; k++) inmodel[j] = inmodel[j] && col[(size_t)j * 8 + k] >= 0;
    }
    std::vector<double>  lod((size_t)T * M, 0.0), hh((size_t)T * M, 0.0), thr((size_t)T * 2, 0.0);
    std::vector<int32_t> rank0(M, 0), nused0(C, 0);
    std::map<std::vector<uint8_t>, std::vector<int>> groups;      // pattern of use -> traits
    for (int t = 0; t < T; t++) {
        std::vector<uint8_t> u(N);
        for (int j = 0; j < N; j++) u[j] = inmodel[j] && y[(size_t)j * T + t] == y[(size_t)j * T + t];
        groups[u].push_back(t);
    }
    for (const auto& g : groups) {
        const std::vector<int>&     tr = g.second;
        const std::vector<uint8_t>& u  = g.first;
        const int                   Tg = (int)tr.size();
        std::vector<double>  yg((size_t)N * Tg), l((size_t)Tg * M), h((size_t)Tg * M), s2((size_t)Tg * M), rss((size_t)Tg * C);
        std::vector<int32_t> rk(M), nu(C);
        for (int j = 0; j < N; j++)
            for (int t = 0; t < Tg; t++) yg[(size_t)j * Tg + t] = u[j] ? y[(size_t)j * T + tr[t]] : 0.0;
        int rc = cnf2_qtl_scan_vc(ctx, N, rows.data(), col.data(), H, Tg, yg.data(), u.data(), K, K ? cov.data() : nullptr, 0, nullptr,
                                  l.data(), h.data(), s2.data(), nullptr, nullptr, rk.data(), rss.data(), nu.data(), nullptr, 0);
        if (rc != CNF2_OK) throw EngineError(CNF2_ERR_STATE, std::string("--qtlvc: ") + cnf2_last_error(ctx));
        if (tr[0] == 0) {
            rank0  = rk;
            nused0 = nu;
        }
        for (int t = 0; t < Tg; t++) {
            std::copy(l.begin() + (size_t)t * M, l.begin() + (size_t)(t + 1) * M, lod.begin() + (size_t)tr[t] * M);
            std::copy(h.begin() + (size_t)t * M, h.begin() + (size_t)(t + 1) * M, hh.begin() + (size_t)tr[t] * M);
        }
        if (NP > 0) {
            std::vector<int32_t> perm((size_t)NP * N);
            std::vector<double>  res((size_t)N * Tg, 0.0), pm((size_t)NP * Tg * C);
            qtl_permutations(N, NP, opt.qtl_seed, u.data(), nullptr, perm.data());
            qtl_null_residuals(N, Tg, yg.data(), K, cov.data(), u.data(), res.data());
            rc = cnf2_qtl_scan_vc(ctx, N, rows.data(), col.data(), H, Tg, res.data(), u.data(), K, K ? cov.data() : nullptr, NP, perm.data(),
                                  l.data(), h.data(), s2.data(), nullptr, nullptr, rk.data(), rss.data(), nu.data(), pm.data(), 0);
            if (rc != CNF2_OK) throw EngineError(CNF2_ERR_STATE, std::string("--qtlvc permutations: ") + cnf2_last_error(ctx));
            for (int t = 0; t < Tg; t++) {
                std::vector<double> mx(NP, 0.0);
                for (int p = 0; p < NP; p++)
                    for (int c = 0; c < C; c++) mx[p] = std::max(mx[p], pm[((size_t)p * Tg + t) * C + c]);
                thr[(size_t)tr[t] * 2]     = qtl_threshold(mx, 0.05);
                thr[(size_t)tr[t] * 2 + 1] = qtl_threshold(mx, 0.01);
            }
        }
    }
    FILE* out = fopen(opt.qtlvc.c_str(), "w");
    if (!out) throw EngineError(CNF2_ERR_STATE, "cannot write " + opt.qtlvc);
    for (int c = 0; c < C; c++)
        for (int m = P.chromstarts[c]; m < P.chromstarts[c + 1]; m++) {
            fprintf(out, "%d\t%.5lf\t%d\t%d", c + 1, P.pos[m], (int)nused0[c], (int)rank0[m]);
            for (int t = 0; t < T; t++) fprintf(out, "\t%.5lf\t%.5lf", lod[(size_t)t * M + m], hh[(size_t)t * M + m]);
            fprintf(out, "\n");
        }
    if (NP > 0) {
        fprintf(out, "\n");
        for (int t = 0; t < T; t++)
            fprintf(out, "%s\t%.5lf\t%.5lf\n", opt.pheno.columns[opt.qtl_trait_cols[t]].c_str(), thr[(size_t)t * 2], thr[(size_t)t * 2 + 1]);
    }
    if (fclose(out) != 0) throw EngineError(CNF2_ERR_STATE, "cannot write " + opt.qtlvc);
}

// --qtlimp after the last round (single GPU) and after the other scans: one sampling sweep (cnf2_sweep_sample) of
// --qtl-imp-draws paths per individual with --qtl-imp-seed, then per pattern of missing values the multiple-imputation scan
// (cnf2_qtl_scan_imp) of its traits on those states, and with --qtl-permutations one more on the permuted residuals of the null
// model, whose maxima are taken over the combined profile.  The table, the grouping and the file are --qtl's (qtl_scan above).
static void qtlimp_scan(const Options& opt, Pedigree& P, cnf2_ctx* ctx)
{
    const int N = (int)P.dous.size(), M = P.n_markers(), C = (int)P.chromstarts.size() - 1;
    const int T = (int)opt.qtl_trait_cols.size(), K = (int)opt.qtl_cov_cols.size(), NP = opt.qtl_permutations, D = opt.qtl_imp_draws;
    std::map<std::string, int> row_of;
    for (size_t r = 0; r < opt.pheno.ids.size(); r++) row_of[opt.pheno.ids[r]] = (int)r;
    std::vector<double>  y((size_t)N * T, NAN), cov((size_t)N * K, 0.0);
    std::vector<uint8_t> base(N, 0);
    for (int j = 0; j < N; j++) {
        const auto it = row_of.find(P.inds[P.dous[j]].name);
        if (it == row_of.end()) continue;
        const std::vector<double>& row = opt.pheno.rows[it->second];
        base[j] = 1;
        for (int k = 0; k < K; k++) {
            cov[(size_t)j * K + k] = row[opt.qtl_cov_cols[k]];
            if (row[opt.qtl_cov_cols[k]] != row[opt.qtl_cov_cols[k]]) base[j] = 0;
        }
        for (int t = 0; t < T; t++) y[(size_t)j * T + t] = row[opt.qtl_trait_cols[t]];
    }
    std::vector<uint8_t> st((size_t)N * D * M);
    {
        std::vector<double>  f((size_t)N * C * 8), ll((size_t)N * C);
        std::vector<int32_t> sh((size_t)N * D * C);
        if (cnf2_sweep_sample(ctx, 0, N, D, (uint64_t)opt.qtl_imp_seed, f.data(), ll.data(), st.data(), sh.data(), nullptr, 0) != CNF2_OK)
            throw EngineError(CNF2_ERR_STATE, std::string("--qtlimp: ") + cnf2_last_error(ctx));
    }
    std::vector<double>  lod((size_t)T * M, 0.0), coef((size_t)T * M * 2, NAN), thr((size_t)T * 2, 0.0);
    std::vector<int32_t> rank0(M, 0), nused0(C, 0);
    std::map<std::vector<uint8_t>, std::vector<int>> groups;      // pattern of use -> traits
    for (int t = 0; t < T; t++) {
        std::vector<uint8_t> u(N);
        for (int j = 0; j < N; j++) u[j] = base[j] && y[(size_t)j * T + t] == y[(size_t)j * T + t];
        groups[u].push_back(t);
    }
    const uint32_t flags = opt.qtl_additive ? CNF2_QTL_ADDITIVE : 0;
    for (const auto& g : groups) {
        const std::vector<int>&     tr = g.second;
        const std::vector<uint8_t>& u  = g.first;
        const int                   Tg = (int)tr.size();
        std::vector<double>  yg((size_t)N * Tg), l((size_t)Tg * M), cf((size_t)Tg * M * 2), rss((size_t)Tg * C);
        std::vector<int32_t> rk(M), nu(C);
        for (int j = 0; j < N; j++)
            for (int t = 0; t < Tg; t++) yg[(size_t)j * Tg + t] = u[j] ? y[(size_t)j * T + tr[t]] : 0.0;
        int rc = cnf2_qtl_scan_imp(ctx, N, D, st.data(), Tg, yg.data(), u.data(), K, K ? cov.data() : nullptr, 0, nullptr, l.data(),
                                   cf.data(), rk.data(), rss.data(), nu.data(), nullptr, nullptr, flags);
        if (rc != CNF2_OK) throw EngineError(CNF2_ERR_STATE, std::string("--qtlimp: ") + cnf2_last_error(ctx));
        if (tr[0] == 0) rank0 = rk, nused0 = nu;                   // the file's design columns are the first trait's
        for (int t = 0; t < Tg; t++) {
            std::copy(l.begin() + (size_t)t * M, l.begin() + (size_t)(t + 1) * M, lod.begin() + (size_t)tr[t] * M);
            std::copy(cf.begin() + (size_t)t * M * 2, cf.begin() + (size_t)(t + 1) * M * 2, coef.begin() + (size_t)tr[t] * M * 2);
        }
        if (NP > 0) {
            std::vector<int32_t> perm((size_t)NP * N);
            std::vector<double>  res((size_t)N * Tg, 0.0), pm((size_t)NP * Tg * C);
            qtl_permutations(N, NP, opt.qtl_seed, u.data(), nullptr, perm.data());
            const int n_u = (int)std::count(u.begin(), u.end(), (uint8_t)1);
            if (n_u >= K + 4 && !qtl_null_residuals(N, Tg, yg.data(), K, K ? cov.data() : nullptr, u.data(), res.data()))
                throw EngineError(CNF2_ERR_ARG, "--qtl-permutations: the null design (intercept and covariates) of the individuals used for " +
                                                    opt.pheno.columns[opt.qtl_trait_cols[tr[0]]] + " has no full rank");
            rc = cnf2_qtl_scan_imp(ctx, N, D, st.data(), Tg, res.data(), u.data(), K, K ? cov.data() : nullptr, NP, perm.data(), l.data(),
                                   cf.data(), rk.data(), rss.data(), nu.data(), pm.data(), nullptr, flags);
            if (rc != CNF2_OK) throw EngineError(CNF2_ERR_STATE, std::string("--qtlimp permutations: ") + cnf2_last_error(ctx));
            for (int t = 0; t < Tg; t++) {
                std::vector<double> mx(NP, 0.0);
                for (int p = 0; p < NP; p++)
                    for (int c = 0; c < C; c++) mx[p] = std::max(mx[p], pm[((size_t)p * Tg + t) * C + c]);
                thr[(size_t)tr[t] * 2]     = qtl_threshold(mx, 0.05);
                thr[(size_t)tr[t] * 2 + 1] = qtl_threshold(mx, 0.01);
            }
        }
    }
    FILE* out = fopen(opt.qtlimp.c_str(), "w");
    if (!out) throw EngineError(CNF2_ERR_STATE, "cannot write " + opt.qtlimp);
    auto effect = [&](double v) {
        if (v != v) fprintf(out, "\t-");
        else fprintf(out, "\t%.5lf", v);
    };
    for (int c = 0; c < C; c++)
        for (int m = P.chromstarts[c]; m < P.chromstarts[c + 1]; m++) {
            fprintf(out, "%d\t%.5lf\t%d\t%d", c + 1, P.pos[m], (int)nused0[c], (int)rank0[m]);
            for (int t = 0; t < T; t++) {
                fprintf(out, "\t%.5lf", lod[(size_t)t * M + m]);
                effect(coef[((size_t)t * M + m) * 2]);
                effect(coef[((size_t)t * M + m) * 2 + 1]);
            }
            fprintf(out, "\n");
        }
    if (NP > 0) {
        fprintf(out, "\n");
        for (int t = 0; t < T; t++)
            fprintf(out, "%s\t%.5lf\t%.5lf\n", opt.pheno.columns[opt.qtl_trait_cols[t]].c_str(), thr[(size_t)t * 2], thr[(size_t)t * 2 + 1]);
    }
    if (fclose(out) != 0) throw EngineError(CNF2_ERR_STATE, "cannot write " + opt.qtlimp);
}

// --qtl2 after the last round (single GPU), and after --qtl where both are given: the pair scan (cnf2_qtl_scan2) of every
// --qtl2-every-th marker on the rows a cnf2_sweep_qtl left in the context -- --qtl's, or one of this function's own.  Traits
// are grouped by their pattern of missing values as for --qtl.  The file holds, per trait and chromosome pair with a pair of
// selected loci, the summary of cnf2freq_amd/qtl.py's pair_summary: trait, the two chromosomes, n, the best additive pair
// (markers, positions, lod_add) and, on different chromosomes, the best full pair (markers, positions, lod_full, the
// additive LOD there) and lod_int = best full - best additive ("-" on one chromosome).  With --qtl-permutations K > 0, after a
// blank line, per trait the 5 % and 1 % genome-wide thresholds of lod_add, lod_full and lod_int.
// --qtl2-linked: one pair sweep (cnf2_sweep_pairs) of the selected loci after the origin sweep, and the linked scan
// (cnf2_qtl_scan2_linked) on its rows: a chromosome with itself reports its best full pair like any other chromosome pair, and
// the thresholds of lod_full and lod_int run over all pairs.
static void qtl2_scan(const Options& opt, Pedigree& P, cnf2_ctx* ctx, bool rows_kept)
{
    const int N = (int)P.dous.size(), M = P.n_markers(), C = (int)P.chromstarts.size() - 1;
    const int T = (int)opt.qtl_trait_cols.size(), K = (int)opt.qtl_cov_cols.size(), NP = opt.qtl_permutations;
    const std::vector<int32_t> sel = qtl2_select(P.chromstarts, opt.qtl2_every);
    const int    L  = (int)sel.size();
    const size_t LL = (size_t)L * L;
    std::vector<int> sc(L);
    for (int j = 0, c = 0; j < L; j++) {
        while (sel[j] >= P.chromstarts[c + 1]) c++;
        sc[j] = c;
    }
    std::map<std::string, int> row_of;
    for (size_t r = 0; r < opt.pheno.ids.size(); r++) row_of[opt.pheno.ids[r]] = (int)r;
    std::vector<double>  y((size_t)N * T, NAN), cov((size_t)N * K, 0.0);
    std::vector<uint8_t> base(N, 0);
    for (int j = 0; j < N; j++) {
        const auto it = row_of.find(P.inds[P.dous[j]].name);
        if (it == row_of.end()) continue;
        const std::vector<double>& row = opt.pheno.rows[it->second];
        base[j] = 1;
        for (int k = 0; k < K; k++) {
            cov[(size_t)j * K + k] = row[opt.qtl_cov_cols[k]];
            if (row[opt.qtl_cov_cols[k]] != row[opt.qtl_cov_cols[k]]) base[j] = 0;
        }
        for (int t = 0; t < T; t++) y[(size_t)j * T + t] = row[opt.qtl_trait_cols[t]];
    }
    std::map<std::vector<uint8_t>, std::vector<int>> groups;      // pattern of use -> traits
    for (int t = 0; t < T; t++) {
        std::vector<uint8_t> u(N);
        for (int j = 0; j < N; j++) u[j] = base[j] && y[(size_t)j * T + t] == y[(size_t)j * T + t];
        groups[u].push_back(t);
    }
    const uint32_t flags = (opt.qtl_additive ? CNF2_QTL_ADDITIVE : 0) | CNF2_QTL_ORIGIN_DEVICE;
    std::vector<double>  la((size_t)T * LL), lf((size_t)T * LL), thr((size_t)T * 6, 0.0);
    std::vector<int32_t> nused((size_t)T * C * C, 0);
    std::vector<double>  joint;          // --qtl2-linked: [N][n_pairs][16], swept once
    bool                 linked = false; // ... and the selection holds two loci of one chromosome
    // the scan of one group of traits: the linked call where there are joint rows
    auto scan2 = [&](int Tg, const double* ys, const uint8_t* u, int n_perm, const int32_t* perm, double* a, double* f, int32_t* ra,
                     int32_t* rf, double* rss, int32_t* nu, double* pm) {
        const double* cv = K ? cov.data() : nullptr;
        if (linked)
            return cnf2_qtl_scan2_linked(ctx, N, nullptr, joint.data(), L, sel.data(), Tg, ys, u, K, cv, n_perm, perm, a, f, ra, rf, rss, nu,
                                         pm, flags);
        return cnf2_qtl_scan2(ctx, N, nullptr, L, sel.data(), Tg, ys, u, K, cv, n_perm, perm, a, f, ra, rf, rss, nu, pm, flags);
    };
    for (const auto& g : groups) {
        const std::vector<int>&     tr = g.second;
        const std::vector<uint8_t>& u  = g.first;
        const int                   Tg = (int)tr.size();
        std::vector<double>  yg((size_t)N * Tg), a((size_t)Tg * LL), f((size_t)Tg * LL), rss((size_t)Tg * C * C);
        std::vector<int32_t> ra(LL), rf(LL), nu((size_t)C * C);
        for (int j = 0; j < N; j++)
            for (int t = 0; t < Tg; t++) yg[(size_t)j * Tg + t] = u[j] ? y[(size_t)j * T + tr[t]] : 0.0;
        int rc;
        if (!rows_kept) {          // the sweep, with the rows left in the context; its single-locus scan is not reported
            std::vector<double>  fa((size_t)N * C * 8), ll((size_t)N * C), l1((size_t)Tg * M), c1((size_t)Tg * M * 2), r1((size_t)Tg * C);
            std::vector<int32_t> k1(M), n1(C);
            rc = cnf2_sweep_qtl(ctx, 0, N, fa.data(), ll.data(), Tg, yg.data(), u.data(), K, K ? cov.data() : nullptr, 0, nullptr,
                                l1.data(), c1.data(), k1.data(), r1.data(), n1.data(), nullptr, flags & CNF2_QTL_ADDITIVE);
            if (rc != CNF2_OK) throw EngineError(CNF2_ERR_STATE, std::string("--qtl2: ") + cnf2_last_error(ctx));
            rows_kept = true;
        }
        if (opt.qtl2_linked && joint.empty()) {
            int32_t n_pairs = 0;
            rc = cnf2_linked_pairs(ctx, L, sel.data(), nullptr, &n_pairs);
            if (rc == CNF2_OK && n_pairs > 0) {
                std::vector<double>  fa((size_t)N * C * 8), ll((size_t)N * C), js((size_t)n_pairs * 16);
                std::vector<int32_t> n1(C);
                joint.assign((size_t)N * n_pairs * 16, 0.0);
                rc = cnf2_sweep_pairs(ctx, 0, N, L, sel.data(), fa.data(), ll.data(), joint.data(), js.data(), n1.data(), 0);
                linked = true;
            }
            if (rc != CNF2_OK) throw EngineError(CNF2_ERR_STATE, std::string("--qtl2-linked: ") + cnf2_last_error(ctx));
        }
        rc = scan2(Tg, yg.data(), u.data(), 0, nullptr, a.data(), f.data(), ra.data(), rf.data(), rss.data(), nu.data(), nullptr);
        if (rc != CNF2_OK) throw EngineError(CNF2_ERR_STATE, std::string("--qtl2: ") + cnf2_last_error(ctx));
        for (int t = 0; t < Tg; t++) {
            std::copy(a.begin() + (size_t)t * LL, a.begin() + (size_t)(t + 1) * LL, la.begin() + (size_t)tr[t] * LL);
            std::copy(f.begin() + (size_t)t * LL, f.begin() + (size_t)(t + 1) * LL, lf.begin() + (size_t)tr[t] * LL);
            std::copy(nu.begin(), nu.end(), nused.begin() + (size_t)tr[t] * C * C);
        }
        if (NP > 0) {
            std::vector<int32_t> perm((size_t)NP * N);
            std::vector<double>  res((size_t)N * Tg, 0.0), pm((size_t)NP * Tg * 3);
            qtl_permutations(N, NP, opt.qtl_seed, u.data(), nullptr, perm.data());
            // (as for --qtl: with too few individuals nothing is scanned and the residuals stay 0; with enough of them a null
            // design without full rank is an error)
            const int n_u = (int)std::count(u.begin(), u.end(), (uint8_t)1);
            if (n_u >= K + 10 && !qtl_null_residuals(N, Tg, yg.data(), K, K ? cov.data() : nullptr, u.data(), res.data()))
                throw EngineError(CNF2_ERR_ARG, "--qtl-permutations: the null design (intercept and covariates) of the individuals used for " +
                                                    opt.pheno.columns[opt.qtl_trait_cols[tr[0]]] + " has no full rank");
            rc = scan2(Tg, res.data(), u.data(), NP, perm.data(), a.data(), f.data(), ra.data(), rf.data(), rss.data(), nu.data(), pm.data());
            if (rc != CNF2_OK) throw EngineError(CNF2_ERR_STATE, std::string("--qtl2 permutations: ") + cnf2_last_error(ctx));
            for (int t = 0; t < Tg; t++)
                for (int s = 0; s < 3; s++) {
                    std::vector<double> mx(NP);
                    for (int p = 0; p < NP; p++) mx[p] = pm[((size_t)p * Tg + t) * 3 + s];
                    thr[(size_t)tr[t] * 6 + 2 * s]     = qtl_threshold(mx, 0.05);
                    thr[(size_t)tr[t] * 6 + 2 * s + 1] = qtl_threshold(mx, 0.01);
                }
        }
    }
    FILE* out = fopen(opt.qtl2.c_str(), "w");
    if (!out) throw EngineError(CNF2_ERR_STATE, "cannot write " + opt.qtl2);
    for (int t = 0; t < T; t++)
        for (int c1 = 0; c1 < C; c1++)
            for (int c2 = c1; c2 < C; c2++) {
                int    aj = -1, ak = -1, fj = -1, fk = -1;       // the first pair in (j, k) order wins a tie
                for (int j = 0; j < L; j++)
                    for (int k = j + 1; k < L; k++) {
                        if (sc[j] != c1 || sc[k] != c2) continue;
                        const size_t o = (size_t)t * LL + (size_t)j * L + k;
                        if (aj < 0 || la[o] > la[(size_t)t * LL + (size_t)aj * L + ak]) aj = j, ak = k;
                        if (fj < 0 || lf[o] > lf[(size_t)t * LL + (size_t)fj * L + fk]) fj = j, fk = k;
                    }
                if (aj < 0) continue;
                const double best_add = la[(size_t)t * LL + (size_t)aj * L + ak];
                fprintf(out, "%s\t%d\t%d\t%d\t%d\t%d\t%.5lf\t%.5lf\t%.5lf", opt.pheno.columns[opt.qtl_trait_cols[t]].c_str(), c1 + 1, c2 + 1,
                        (int)nused[((size_t)t * C + c1) * C + c2], (int)sel[aj], (int)sel[ak], P.pos[sel[aj]], P.pos[sel[ak]], best_add);
                if (c1 == c2 && !linked) fprintf(out, "\t-\t-\t-\t-\t-\t-\t-\n");
                else {
                    const size_t o = (size_t)t * LL + (size_t)fj * L + fk;
                    fprintf(out, "\t%d\t%d\t%.5lf\t%.5lf\t%.5lf\t%.5lf\t%.5lf\n", (int)sel[fj], (int)sel[fk], P.pos[sel[fj]], P.pos[sel[fk]], lf[o],
                            la[o], lf[o] - best_add);
                }
            }
    if (NP > 0) {
        fprintf(out, "\n");
        for (int t = 0; t < T; t++) {
            fprintf(out, "%s", opt.pheno.columns[opt.qtl_trait_cols[t]].c_str());
            for (int s = 0; s < 6; s++) fprintf(out, "\t%.5lf", thr[(size_t)t * 6 + s]);
            fprintf(out, "\n");
        }
    }
    if (fclose(out) != 0) throw EngineError(CNF2_ERR_STATE, "cannot write " + opt.qtl2);
}

// --rccl-selftest: the RCCL transport with a world of one on GPU 0 -- the communicator's set-up through the shared region, then
// reduce-scatter, all-gather, the hit-counter sum, a barrier and the host broadcast on the context's exchange buffer, through
// the same entry the engine calls.  (Two ranks need two GPUs: RCCL refuses two ranks on one device.)
static int rccl_selftest()
{
    ShmRegion* R = shm_region_create(1, (size_t)1 << 20);
    cnf2_ctx*  ctx = nullptr;
    if (!R || cnf2_ctx_create(0, &ctx) != CNF2_OK) {
        fprintf(stderr, "rccl selftest: no region / no device: %s\n", cnf2_last_error(nullptr));
        return 3;
    }
    RcclTransport T;
    if (T.init(R, ctx, 0, 1) != 0) return 4;
    const size_t n = 100000;
    void*        buf = nullptr;
    if (cnf2_exchange_buffer(ctx, n * sizeof(double), &buf) != CNF2_OK) return 5;
    std::vector<double> v(n), w(n, 0.0);
    for (size_t i = 0; i < n; i++) v[i] = 0.5 + (double)i * 1e-3;
    int bad = 0;
    bad |= cnf2_exchange_write(ctx, 0, v.data(), n * sizeof(double)) != CNF2_OK;
    bad |= RcclTransport::call(&T, X_SUM_SEGMENTS, buf, n, n) != 0;              // one segment: the sum of one rank's values
    bad |= RcclTransport::call(&T, X_GATHER_SEGMENTS, buf, n * sizeof(double), n * sizeof(double)) != 0;
    bad |= cnf2_exchange_read(ctx, 0, w.data(), n * sizeof(double)) != CNF2_OK;
    for (size_t i = 0; i < n; i++) bad |= w[i] != v[i];
    int32_t h[2] = {7, 11};
    bad |= RcclTransport::call(&T, X_SUM_HITS, h, 2, 2) != 0 || h[0] != 7 || h[1] != 11;
    bad |= RcclTransport::call(&T, X_BARRIER, nullptr, 0, 0) != 0;
    unsigned char hb[300];
    for (int i = 0; i < 300; i++) hb[i] = (unsigned char)(i * 7);
    bad |= RcclTransport::call(&T, X_BCAST_HOST, hb, 300, 0) != 0 || hb[299] != (unsigned char)(299 * 7);
    T.finish();
    cnf2_ctx_destroy(ctx);
    printf("rccl selftest: %s (world 1, %zu doubles through ncclReduceScatter and ncclAllGather in place)\n", bad ? "FAILED" : "ok", n);
    return bad ? 1 : 0;
}

int main(int argc, char** argv)
{
    Options opt;
    if (!parse(argc, argv, opt)) return 2;
    if (opt.rccl_selftest) return rccl_selftest();
    Pedigree P;
    if (!opt.mapfile.empty()) {
        FILE* f = fopen(opt.mapfile.c_str(), "rt");
        fprintf(stderr, "Reading map file %s\n", opt.mapfile.c_str());
        if (!read_alpha_map(f, P)) { fprintf(stderr, "cannot read map\n"); abort(); }
        fclose(f);
    }
    if (!opt.pedfile.empty()) {
        FILE* f = fopen(opt.pedfile.c_str(), "rt");
        fprintf(stderr, "Reading pedigree file %s\n", opt.pedfile.c_str());
        if (!read_alpha_ped(f, P)) { fprintf(stderr, "cannot read pedigree\n"); abort(); }
        fclose(f);
    }
    if (!opt.genfile.empty()) {
        FILE* f = fopen(opt.genfile.c_str(), "rt");
        fprintf(stderr, "Reading genotype file %s\n", opt.genfile.c_str());
        const auto t0 = std::chrono::steady_clock::now();
        if (!read_alpha_gen(f, P)) { fprintf(stderr, "cannot read genotypes\n"); abort(); }
        fclose(f);
        if (getenv("CNF2_TIMING"))
            fprintf(stderr, "  [read] genotype file                     %.3f s\n",
                    std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count());
    }
    // after ALL files are read: the genotype reader is token based, so capping earlier would misalign
    // it (the reference's own notifier runs before the map exists, cnF2freq.cpp:7965-7969)
    if (opt.capmarker > 0) cap_markers(P, opt.capmarker);
    if (!opt.quiet)
        for (auto& l : P.log) printf("%s\n", l.c_str());

    if (opt.parse_only) {
        Tables T;
        build_tables(P, T);
        const int M = P.n_markers();
        printf("markers %d chromstarts", M);
        for (int v : P.chromstarts) printf(" %d", v);
        printf("\nrows %d\n", T.n_rows);
        for (size_t r = 0; r < P.inds.size(); r++) {
            const Individual& I = P.inds[r];
            printf("ind %d %s gen %d empty %d pars %d %d row %d analysed %d :", I.n, I.name.c_str(), I.gen, (int)I.empty,
                   I.pars[0] < 0 ? 0 : P.inds[I.pars[0]].n, I.pars[1] < 0 ? 0 : P.inds[I.pars[1]].n, T.row_of[r],
                   (int)(std::find(T.dous.begin(), T.dous.end(), (int)r) != T.dous.end()));
            for (int m = 0; m < M; m++) printf(" %d%d/%.6g/%.6g", I.allele[m * 2], I.allele[m * 2 + 1], I.sure[m * 2], I.sure[m * 2 + 1]);
            printf("\n");
        }
        return 0;
    }

    if (opt.transport != "" && opt.transport != "rccl" && opt.transport != "shm") {
        fprintf(stderr, "--transport must be rccl or shm\n");
        return 2;
    }
    if (opt.gpus < 1 || opt.gpus > 64) {
        fprintf(stderr, "--gpus must be between 1 and 64\n");
        return 2;
    }
    if (opt.gpus > 1 && (!opt.crossovers.empty() || !opt.remap.empty())) {
        fprintf(stderr, "--crossovers and --remap need a single GPU (--gpus 1): their sums are not reduced across ranks\n");
        return 2;
    }
    if (opt.gpus > 1 && !opt.viterbi.empty()) {
        fprintf(stderr, "--viterbi needs a single GPU (--gpus 1): the ranks' paths are not gathered\n");
        return 2;
    }
    if (opt.gpus > 1 && !opt.sample.empty()) {
        fprintf(stderr, "--sample needs a single GPU (--gpus 1): the ranks' draws are not gathered\n");
        return 2;
    }
    if (opt.gpus > 1 && !opt.place.empty()) {
        fprintf(stderr, "--place needs a single GPU (--gpus 1): the ranks' sums are not reduced\n");
        return 2;
    }
    if (opt.gpus > 1 && !opt.loo.empty()) {
        fprintf(stderr, "--loo needs a single GPU (--gpus 1): the ranks' sums are not reduced\n");
        return 2;
    }
    if (opt.gpus > 1 && !opt.origins.empty()) {
        fprintf(stderr, "--origins needs a single GPU (--gpus 1): the ranks' sums are not reduced\n");
        return 2;
    }
    if (opt.gpus > 1 && !opt.descent.empty()) {
        fprintf(stderr, "--descent needs a single GPU (--gpus 1): the ranks' counts are not reduced\n");
        return 2;
    }
    if (opt.gpus > 1 && !opt.qtl.empty()) {
        fprintf(stderr, "--qtl needs a single GPU (--gpus 1): a regression is not additive over the ranks' blocks\n");
        return 2;
    }
    if (opt.gpus > 1 && !opt.qtl2.empty()) {
        fprintf(stderr, "--qtl2 needs a single GPU (--gpus 1): a regression is not additive over the ranks' blocks\n");
        return 2;
    }
    if (opt.gpus > 1 && !opt.qtlx.empty()) {
        fprintf(stderr, "--qtlx needs a single GPU (--gpus 1): a regression is not additive over the ranks' blocks\n");
        return 2;
    }
    if (opt.gpus > 1 && !opt.qtlem.empty()) {
        fprintf(stderr, "--qtlem needs a single GPU (--gpus 1): a fit is not additive over the ranks' blocks\n");
        return 2;
    }
    if (opt.qtlem.empty() && opt.qtlem_extra_set) {
        fprintf(stderr, "--qtl-em-iterations and --qtl-em-tol need --qtlem FILE\n");
        return 2;
    }
    if (!opt.qtlem.empty() && opt.phenofile.empty()) {
        fprintf(stderr, "--qtlem FILE needs --phenofile FILE\n");
        return 2;
    }
    if (opt.qtlem_iterations < 1 || opt.qtlem_iterations > cnf2::QTLEM_MAX_ITER) {
        fprintf(stderr, "--qtl-em-iterations must be 1 .. %d\n", cnf2::QTLEM_MAX_ITER);
        return 2;
    }
    if (opt.gpus > 1 && !opt.qtlbin.empty()) {
        fprintf(stderr, "--qtlbin needs a single GPU (--gpus 1): a fit is not additive over the ranks' blocks\n");
        return 2;
    }
    if (opt.qtlbin.empty() && opt.qtlbin_extra_set) {
        fprintf(stderr, "--qtl-binary-iterations and --qtl-binary-tol need --qtlbin FILE\n");
        return 2;
    }
    if (!opt.qtlbin.empty() && opt.phenofile.empty()) {
        fprintf(stderr, "--qtlbin FILE needs --phenofile FILE\n");
        return 2;
    }
    if (opt.qtlbin_iterations < 1 || opt.qtlbin_iterations > cnf2::QTLBIN_MAX_ITER) {
        fprintf(stderr, "--qtl-binary-iterations must be 1 .. %d\n", cnf2::QTLBIN_MAX_ITER);
        return 2;
    }
    if (opt.gpus > 1 && !opt.qtlsurv.empty()) {
        fprintf(stderr, "--qtlsurv needs a single GPU (--gpus 1): a fit is not additive over the ranks' blocks\n");
        return 2;
    }
    if (opt.qtlsurv.empty() && opt.qtlsurv_extra_set) {
        fprintf(stderr, "--qtl-surv-time, --qtl-surv-status, --qtl-surv-iterations and --qtl-surv-tol need --qtlsurv FILE\n");
        return 2;
    }
    if (!opt.qtlsurv.empty() && opt.phenofile.empty()) {
        fprintf(stderr, "--qtlsurv FILE needs --phenofile FILE\n");
        return 2;
    }
    if (!opt.qtlsurv.empty() && (opt.qtlsurv_time.empty() || opt.qtlsurv_status.empty())) {
        fprintf(stderr, "--qtlsurv FILE needs --qtl-surv-time NAME and --qtl-surv-status NAME\n");
        return 2;
    }
    if (opt.qtlsurv_iterations < 1 || opt.qtlsurv_iterations > cnf2::QTLSURV_MAX_ITER) {
        fprintf(stderr, "--qtl-surv-iterations must be 1 .. %d\n", cnf2::QTLSURV_MAX_ITER);
        return 2;
    }
    if (opt.gpus > 1 && !opt.qtlvar.empty()) {
        fprintf(stderr, "--qtlvar needs a single GPU (--gpus 1): a fit is not additive over the ranks' blocks\n");
        return 2;
    }
    if (opt.qtlvar.empty() && opt.qtlvar_extra_set) {
        fprintf(stderr, "--qtl-var-covariates, --qtl-var-iterations and --qtl-var-tol need --qtlvar FILE\n");
        return 2;
    }
    if (!opt.qtlvar.empty() && opt.phenofile.empty()) {
        fprintf(stderr, "--qtlvar FILE needs --phenofile FILE\n");
        return 2;
    }
    if (opt.qtlvar_iterations < 1 || opt.qtlvar_iterations > cnf2::QTLVAR_MAX_ITER) {
        fprintf(stderr, "--qtl-var-iterations must be 1 .. %d\n", cnf2::QTLVAR_MAX_ITER);
        return 2;
    }
    if (opt.qtlx.empty() && (opt.qtl_interactive_set || (opt.qtlx_extra_set && opt.qtlem.empty() && opt.qtlbin.empty() && opt.qtlsurv.empty() && opt.qtlvar.empty()))) {
        fprintf(stderr, "--qtl-imprint and --qtl-interactive need --qtlx FILE\n");
        return 2;
    }
    if (!opt.qtlx.empty() && opt.phenofile.empty()) {
        fprintf(stderr, "--qtlx FILE needs --phenofile FILE\n");
        return 2;
    }
    if (opt.gpus > 1 && !opt.qtlcof.empty()) {
        fprintf(stderr, "--qtlcof needs a single GPU (--gpus 1): a regression is not additive over the ranks' blocks\n");
        return 2;
    }
    if (opt.qtlcof.empty() && opt.qtlcof_extra_set) {
        fprintf(stderr, "--qtl-cofactors and --qtl-window need --qtlcof FILE\n");
        return 2;
    }
    if (!opt.qtlcof.empty() && opt.phenofile.empty()) {
        fprintf(stderr, "--qtlcof FILE needs --phenofile FILE\n");
        return 2;
    }
    if (!opt.qtlcof.empty() && opt.qtl_cofactors.empty()) {
        fprintf(stderr, "--qtlcof FILE needs --qtl-cofactors LIST\n");
        return 2;
    }
    if (opt.gpus > 1 && !opt.qtlboot.empty()) {
        fprintf(stderr, "--qtlboot needs a single GPU (--gpus 1): a regression is not additive over the ranks' blocks\n");
        return 2;
    }
    if (opt.qtlboot.empty() && opt.qtlboot_extra_set) {
        fprintf(stderr, "--qtl-boot-chrom and --qtl-boot-replicates need --qtlboot FILE\n");
        return 2;
    }
    if (!opt.qtlboot.empty() && opt.phenofile.empty()) {
        fprintf(stderr, "--qtlboot FILE needs --phenofile FILE\n");
        return 2;
    }
    if (!opt.qtlboot.empty() && (opt.qtl_boot_chrom < 1 || opt.qtl_boot_chrom > (int)P.chromstarts.size() - 1)) {
        fprintf(stderr, "--qtlboot FILE needs --qtl-boot-chrom C with C = 1 .. %d, the chromosomes of the map\n", (int)P.chromstarts.size() - 1);
        return 2;
    }
    if (opt.gpus > 1 && !opt.qtlmv.empty()) {
        fprintf(stderr, "--qtlmv needs a single GPU (--gpus 1): a regression is not additive over the ranks' blocks\n");
        return 2;
    }
    if (opt.qtlmv.empty() && opt.qtl_traits_set) {
        fprintf(stderr, "--qtl-traits needs --qtlmv FILE\n");
        return 2;
    }
    if (!opt.qtlmv.empty() && opt.phenofile.empty()) {
        fprintf(stderr, "--qtlmv FILE needs --phenofile FILE\n");
        return 2;
    }
    if (opt.gpus > 1 && !opt.qtlfam.empty()) {
        fprintf(stderr, "--qtlfam needs a single GPU (--gpus 1): a regression is not additive over the ranks' blocks\n");
        return 2;
    }
    if (opt.qtlfam.empty() && opt.qtlfam_extra_set) {
        fprintf(stderr, "--qtl-fam-side and --qtl-cell need --qtlfam FILE\n");
        return 2;
    }
    if (!opt.qtlfam.empty() && opt.phenofile.empty()) {
        fprintf(stderr, "--qtlfam FILE needs --phenofile FILE\n");
        return 2;
    }
    if (opt.qtl_fam_side != "first" && opt.qtl_fam_side != "second" && opt.qtl_fam_side != "both") {
        fprintf(stderr, "--qtl-fam-side must be first, second or both\n");
        return 2;
    }
    if (opt.qtl_cell != "parent" && opt.qtl_cell != "pair") {
        fprintf(stderr, "--qtl-cell must be parent or pair\n");
        return 2;
    }
    if (opt.gpus > 1 && !opt.qtlhap.empty()) {
        fprintf(stderr, "--qtlhap needs a single GPU (--gpus 1): a regression is not additive over the ranks' blocks\n");
        return 2;
    }
    if (opt.qtlhap.empty() && opt.qtlhap_extra_set) {
        fprintf(stderr, "--qtl-hap-by needs --qtlhap FILE\n");
        return 2;
    }
    if (!opt.qtlhap.empty() && opt.phenofile.empty()) {
        fprintf(stderr, "--qtlhap FILE needs --phenofile FILE\n");
        return 2;
    }
    if (opt.qtl_hap_by != "haplotype" && opt.qtl_hap_by != "founder" && opt.qtl_hap_by != "line") {
        fprintf(stderr, "--qtl-hap-by must be haplotype, founder or line\n");
        return 2;
    }
    if (opt.gpus > 1 && !opt.qtlvc.empty()) {
        fprintf(stderr, "--qtlvc needs a single GPU (--gpus 1): a mixed model is not additive over the ranks' blocks\n");
        return 2;
    }
    if (opt.qtlvc.empty() && opt.qtlvc_extra_set) {
        fprintf(stderr, "--qtl-vc-by needs --qtlvc FILE\n");
        return 2;
    }
    if (!opt.qtlvc.empty() && opt.phenofile.empty()) {
        fprintf(stderr, "--qtlvc FILE needs --phenofile FILE\n");
        return 2;
    }
    if (opt.qtl_vc_by != "haplotype" && opt.qtl_vc_by != "founder" && opt.qtl_vc_by != "line") {
        fprintf(stderr, "--qtl-vc-by must be haplotype, founder or line\n");
        return 2;
    }
    if (opt.gpus > 1 && !opt.qtlimp.empty()) {
        fprintf(stderr, "--qtlimp needs a single GPU (--gpus 1): a regression is not additive over the ranks' blocks\n");
        return 2;
    }
    if (opt.qtlimp.empty() && opt.qtlimp_extra_set) {
        fprintf(stderr, "--qtl-imp-draws and --qtl-imp-seed need --qtlimp FILE\n");
        return 2;
    }
    if (!opt.qtlimp.empty() && opt.phenofile.empty()) {
        fprintf(stderr, "--qtlimp FILE needs --phenofile FILE\n");
        return 2;
    }
    if (opt.qtl_imp_draws < 1 || opt.qtl_imp_draws > 1024) {
        fprintf(stderr, "--qtl-imp-draws must be 1 .. 1024\n");
        return 2;
    }
    if (opt.qtl_boot_replicates < 1 || opt.qtl_boot_replicates > 1000000) {
        fprintf(stderr, "--qtl-boot-replicates must be 1 .. 1000000\n");
        return 2;
    }
    if (opt.qtl_window < 0.0) {
        fprintf(stderr, "--qtl-window must not be negative\n");
        return 2;
    }
    if (opt.qtl.empty() && opt.qtl2.empty() && opt.qtlx.empty() && opt.qtlem.empty() && opt.qtlbin.empty() && opt.qtlcof.empty() && opt.qtlboot.empty() &&
        opt.qtlmv.empty() && opt.qtlsurv.empty() && opt.qtlvar.empty() && opt.qtlimp.empty() && opt.qtlfam.empty() && opt.qtlhap.empty() && opt.qtlvc.empty() && (opt.qtl_extra_set || !opt.phenofile.empty())) {
        fprintf(stderr, "--phenofile, --qtl-covariates, --qtl-permutations, --qtl-seed and --qtl-additive need --qtl FILE or --qtl2 FILE\n");
        return 2;
    }
    if (opt.qtl2.empty() && opt.qtl2_linked) {
        fprintf(stderr, "--qtl2-linked needs --qtl2 FILE\n");
        return 2;
    }
    if (opt.qtl2.empty() && opt.qtl2_every_set) {
        fprintf(stderr, "--qtl2-every needs --qtl2 FILE\n");
        return 2;
    }
    if (!opt.qtl.empty() && opt.phenofile.empty()) {
        fprintf(stderr, "--qtl FILE needs --phenofile FILE\n");
        return 2;
    }
    if (!opt.qtl2.empty() && opt.phenofile.empty()) {
        fprintf(stderr, "--qtl2 FILE needs --phenofile FILE\n");
        return 2;
    }
    if (opt.qtl2_every < 1) {
        fprintf(stderr, "--qtl2-every must be at least 1\n");
        return 2;
    }
    if (!opt.qtl2.empty()) {
        const std::vector<int32_t> sel = qtl2_select(P.chromstarts, opt.qtl2_every);
        if (sel.size() > 4096 || sel.size() < 2) {
            fprintf(stderr, "--qtl2: --qtl2-every S = %d selects %zu loci, and a pair scan takes 2 to 4096: %s S\n", opt.qtl2_every,
                    sel.size(), sel.size() < 2 ? "lower" : "raise");
            return 2;
        }
    }
    if (opt.qtl_permutations < 0) {
        fprintf(stderr, "--qtl-permutations must not be negative\n");
        return 2;
    }
    if ((!opt.qtl.empty() || !opt.qtl2.empty() || !opt.qtlx.empty() || !opt.qtlem.empty() || !opt.qtlbin.empty() || !opt.qtlcof.empty() || !opt.qtlboot.empty() ||
         !opt.qtlmv.empty() || !opt.qtlsurv.empty() || !opt.qtlvar.empty() || !opt.qtlimp.empty() || !opt.qtlfam.empty() || !opt.qtlhap.empty() || !opt.qtlvc.empty()) &&
        !prepare_qtl(opt, P))
        return 2;
    if (!opt.qtlmv.empty() && !prepare_qtlmv(opt)) return 2;
    if (!opt.qtlcof.empty() && !prepare_qtlcof(opt, P)) return 2;
    if (!opt.qtlbin.empty() && !prepare_qtlbin(opt)) return 2;
    if (!opt.qtlsurv.empty() && !prepare_qtlsurv(opt)) return 2;
    if (!opt.qtlvar.empty() && !prepare_qtlvar(opt)) return 2;
    if (!opt.qtlx.empty() && !prepare_qtlx(opt)) return 2;
    if (!opt.qtl2.empty() && opt.qtl_cov_cols.size() > 6) {
        fprintf(stderr, "--qtl2: at most 6 covariates\n");
        return 2;
    }
    if (opt.loo_threshold_set && opt.loo.empty()) {
        fprintf(stderr, "--loo-threshold needs --loo FILE\n");
        return 2;
    }
    if (opt.place.empty() != opt.place_genfile.empty() || opt.place.empty() != (opt.place_markers == 0)) {
        fprintf(stderr, "--place FILE, --place-genfile FILE and --place-markers Q go together\n");
        return 2;
    }
    if (opt.place_markers < 0) {
        fprintf(stderr, "--place-markers must be at least 1\n");
        return 2;
    }
    if ((opt.draws_set || opt.seed_set) && opt.sample.empty()) {
        fprintf(stderr, "--draws and --seed need --sample FILE\n");
        return 2;
    }
    if (opt.draws < 1 || opt.draws > 1024) {
        fprintf(stderr, "--draws must be between 1 and 1024\n");
        return 2;
    }
    if (opt.remap_iterations_set && opt.remap.empty()) {
        fprintf(stderr, "--remap-iterations needs --remap FILE\n");
        return 2;
    }
    if (opt.remap_iterations < 1) {
        fprintf(stderr, "--remap-iterations must be at least 1\n");
        return 2;
    }
    // main() trims dous only after postmarkerdata (cnF2freq.cpp:8083, 8124); the analysed list is fixed at upload here,
    // and postmarkerdata does not read it
    if ((int)P.dous.size() > opt.limit) P.dous.resize(opt.limit);
    if (opt.gpus == 1) return run_rank(opt, P, 0, 1, nullptr);

    // N ranks: the region and the fork come before any HIP call of this process
    ShmRegion* region = shm_region_create(opt.gpus, (size_t)64 << 20);
    if (!region) {
        fprintf(stderr, "cannot map the shared region of %d ranks\n", opt.gpus);
        abort();
    }
    // the ranks share this process's CPUs (affinity mask and cgroup quota): each gets its N-th for its host loops
    set_host_threads(std::max(1, host_threads() / opt.gpus));
    fflush(stdout);
    fflush(stderr);
    static std::vector<pid_t> kids;             // static: the signal handler below ends them
    const pid_t parent = getpid();
    auto stop_ranks = [](int sig) {
        for (pid_t k : kids) kill(k, SIGKILL);
        _exit(128 + sig);
    };
    signal(SIGINT, stop_ranks);
    signal(SIGTERM, stop_ranks);
    for (int r = 0; r < opt.gpus; r++) {
        const pid_t pid = fork();
        if (pid < 0) {
            perror("fork");
            for (pid_t k : kids) kill(k, SIGKILL);
            abort();
        }
        if (pid == 0) {
            // a rank must not outlive the run: if the parent is killed the ranks would wait at a barrier for ever, holding
            // their GPU memory
            prctl(PR_SET_PDEATHSIG, SIGKILL);
            if (getppid() != parent) _exit(5);             // the parent died between fork and prctl
            signal(SIGINT, SIG_DFL);
            signal(SIGTERM, SIG_DFL);
            const int rc = run_rank(opt, P, r, opt.gpus, region);
            fflush(stdout);
            fflush(stderr);
            _exit(rc);
        }
        kids.push_back(pid);
    }
    // a rank that fails would leave the others waiting at a barrier: the first failure ends them all
    int failed = 0;
    for (size_t left = kids.size(); left > 0; left--) {
        int         st = 0;
        const pid_t pid = wait(&st);
        if (pid < 0) break;
        if (!(WIFEXITED(st) && WEXITSTATUS(st) == 0) && !failed) {
            failed = 1;
            fprintf(stderr, "a rank ended abnormally: stopping the others\n");
            for (pid_t k : kids)
                if (k != pid) kill(k, SIGKILL);
        }
    }
    if (failed) {
        // text the ranks had spooled for rank 0 (cnf2_<what>_run<pid>_...): nobody will collect it now
        const std::string tag = "_run" + std::to_string((long)parent) + "_";
        if (DIR* d = opendir(opt.tmppath.c_str())) {
            while (dirent* e = readdir(d)) {
                const std::string name = e->d_name;
                if (name.rfind("cnf2_", 0) == 0 && name.find(tag) != std::string::npos) remove((opt.tmppath + "/" + name).c_str());
            }
            closedir(d);
        }
        abort();                                          // the reference ends every failure this way (cnF2freq.cpp:21-25)
    }
    return 0;
}
