// cnf2_plan.h -- what the sweep entry points of cnf2_capi.hip decide on the host before they launch: the job list, the
// grids and the split of free memory between spill slots and batch buffers.  Pure functions of the window tables, the map
// and a few numbers of the device; plain C++ (no HIP) so that they are unit-tested without a GPU (tests/test_host_plan.py).
#ifndef CNF2_PLAN_H
#define CNF2_PLAN_H

#include <stddef.h>
#include <stdint.h>

#include <algorithm>
#include <vector>

#include "../../include/cnf2hip.h"
#include "cnf2_emission.h"
#include "cnf2_job.h"
#include "cnf2_window.h"

namespace cnf2 {

// ------------------------------------------------------------------------------------------------ job list
// The chromosomes in the order their jobs are listed: longest first (ties in map order).  The waves of a launch take the
// jobs in list order (KernelParams::job_next), so the long jobs start first and a launch ends on the short ones; the jobs of
// one chromosome keep the order of the individuals, so nothing that adds up over individuals sees a difference.
inline std::vector<int> chrom_order(const int32_t* chromstarts, int n_chrom)
{
    std::vector<int> o(n_chrom);
    for (int c = 0; c < n_chrom; c++) o[c] = c;
    std::stable_sort(o.begin(), o.end(), [&](int a, int b) {
        return chromstarts[a + 1] - chromstarts[a] > chromstarts[b + 1] - chromstarts[b];
    });
    return o;
}

inline int max_chrom_len(const int32_t* chromstarts, int n_chrom)
{
    int mx = 0;
    for (int c = 0; c < n_chrom; c++) mx = std::max(mx, (int)(chromstarts[c + 1] - chromstarts[c]));
    return mx;
}

struct JobPlan {
    std::vector<Job>       jobs;         // [0, n_fast): windows without an active tie group (fast kernel); the tied ones after
    size_t                 n_fast = 0;
    std::vector<PackedJob> pjobs;        // CNF2_MERGE_MODES: four windows to a wavefront (fb_packed_kernel)
};

// Job list of the individuals [ind_begin, ind_begin + n): individuals x chromosomes (the loops at cnF2freq.cpp:5283 and
// 5294), windows without an active tie group first (fast kernel), tied windows after (general or tied kernel).  Of `flags`
// CNF2_NO_TIES (no window counts as tied), CNF2_FLUSH_TINY (every window takes the general kernel's route, the second list)
// and CNF2_MERGE_MODES matter: windows whose two parents are homozygous with equal sure everywhere (row_hom) go four to a
// wavefront; groups are formed per chromosome, what does not fill a group of four stays with the ordinary kernel.
inline JobPlan plan_jobs(const Window* windows, const int32_t* chromstarts, int n_chrom, int ind_begin, int n, uint32_t flags,
                         const uint8_t* row_hom)
{
    JobPlan                plan;
    const std::vector<int> order = chrom_order(chromstarts, n_chrom);
    const bool             merge = (flags & CNF2_MERGE_MODES) && !(flags & (CNF2_FULL_SPILL | CNF2_FLUSH_TINY));
    auto tied = [&](const Window& w) { return (w.n_groups > 0 && !(flags & CNF2_NO_TIES)) || (flags & CNF2_FLUSH_TINY); };
    auto mergeable = [&](const Window& w) {
        if (w.n_groups > 0 && !(flags & CNF2_NO_TIES)) return false;
        if (w.shiftignore != 0 || w.shiftend != 8 || (w.flags[0] & SLOT_FOUNDER)) return false;
        for (int k = 1; k <= 4; k += 3) {
            if (!(w.flags[k] & SLOT_PRESENT) || w.row[k] < 0) return false;
            if (!row_hom[w.row[k]]) return false;
        }
        return true;
    };
    // a group shares the producer's instantiation: windows whose grandparents are all present and homozygous everywhere
    // (SLOT_HOM) are grouped apart from the others
    auto homleaf = [](const Window& w) { return slots_homleaf(w.flags); };
    std::vector<uint8_t> packed(merge ? n : 0, 0);
    for (int cls = 0; merge && cls < 2; cls++) {
        std::vector<int> el;
        for (int j = 0; j < n; j++) {
            const Window& w = windows[ind_begin + j];
            if (mergeable(w) && (homleaf(w) ? 1 : 0) == cls) el.push_back(j);
        }
        const size_t full = el.size() / 4 * 4;
        for (size_t k = 0; k < full; k++) packed[el[k]] = 1;
        for (int c : order)
            for (size_t k = 0; k < full; k += 4) {
                PackedJob pj;
                for (int i = 0; i < 4; i++) pj.ind[i] = el[k + i];
                pj.first   = chromstarts[c];
                pj.last    = chromstarts[c + 1] - 1;
                pj.chrom   = c;
                pj.homleaf = cls;
                plan.pjobs.push_back(pj);
            }
    }
    for (int pass = 0; pass < 2; pass++) {
        for (int c : order)
            for (int j = 0; j < n; j++) {
                if (merge && packed[j]) continue;
                if (tied(windows[ind_begin + j]) != (pass == 1)) continue;
                Job jb;
                jb.ind   = j;
                jb.first = chromstarts[c];
                jb.last  = chromstarts[c + 1] - 1;
                jb.chrom = c;
                plan.jobs.push_back(jb);
            }
        if (pass == 0) plan.n_fast = plan.jobs.size();
    }
    return plan;
}

// Groups of four for fb_unipack_kernel among the fast jobs [0, n_fast) of a job list (plan_jobs: chromosome by chromosome in
// chrom_order, the individuals in order within each).  A job can be grouped when its window is uniform (slots_uniform) and has
// both its lines among the call's records (line_keys [n][2], indexed like the jobs' ind; NULL = nobody has).  Per chromosome
// the groupable jobs form fours in list order; what does not fill a four stays where it is, as does every other job.  The
// grouped jobs are moved behind the others of [0, n_fast), group by group (the kernels that sweep single jobs get the front,
// the logarithms are taken of the whole list); *n_single = how many stay in front.  The groups come in list order, so
// chromosome by chromosome in chrom_order.  `windows` is indexed by ind.
inline std::vector<PackedJob> group_uniform_jobs(std::vector<Job>& jobs, size_t n_fast, const Window* windows, const int32_t* line_keys,
                                                 size_t* n_single)
{
    std::vector<PackedJob> groups;
    std::vector<uint8_t>   taken(n_fast, 0);
    auto groupable = [&](const Job& jb) {
        return line_keys && line_keys[2 * (size_t)jb.ind] >= 0 && line_keys[2 * (size_t)jb.ind + 1] >= 0 &&
               slots_uniform(windows[jb.ind].flags);
    };
    for (size_t b = 0; b < n_fast;) {
        size_t e = b;
        while (e < n_fast && jobs[e].chrom == jobs[b].chrom) e++;
        size_t four[4];
        int    k = 0;
        for (size_t j = b; j < e; j++) {
            if (!groupable(jobs[j])) continue;
            four[k++] = j;
            if (k < 4) continue;
            PackedJob pj;
            for (int i = 0; i < 4; i++) {
                pj.ind[i]      = jobs[four[i]].ind;
                taken[four[i]] = 1;
            }
            pj.first   = jobs[b].first;
            pj.last    = jobs[b].last;
            pj.chrom   = jobs[b].chrom;
            pj.homleaf = 1;
            groups.push_back(pj);
            k = 0;
        }
        b = e;
    }
    *n_single = n_fast - 4 * groups.size();
    if (groups.empty()) return groups;
    std::vector<Job> front, back;
    front.reserve(*n_single);
    back.reserve(4 * groups.size());
    for (size_t j = 0; j < n_fast; j++)
        if (!taken[j]) front.push_back(jobs[j]);
    for (const PackedJob& pj : groups)
        for (int i = 0; i < 4; i++) back.push_back(Job{pj.ind[i], pj.first, pj.last, pj.chrom});
    std::copy(front.begin(), front.end(), jobs.begin());
    std::copy(back.begin(), back.end(), jobs.begin() + front.size());
    return groups;
}

// Pairs of those groups for fb_unipack8_kernel: eight windows of a chromosome to a wave.  A four can be paired when every one of
// its windows has all eight shift modes analysed (shiftignore == 0, shiftend == 8); per chromosome such fours pair up in list
// order.  The paired fours move to the front of `groups` -- eight e is groups[2 e] and groups[2 e + 1] -- the others follow in
// the order they had.  All jobs of a chromosome are equally long, and an eight takes longer than a four: with at least as many
// eights as `waves` (the resident waves of the packed grid, 0 = no such rule) only a whole number of rounds of eights is kept
// and the last pairs are handed back as fours, which fill the tail behind them.  Returns the number of eights.
inline size_t pair_uniform_groups(std::vector<PackedJob>& groups, const Window* windows, size_t waves)
{
    auto all_modes = [&](const PackedJob& pj) {
        for (int i = 0; i < 4; i++)
            if (windows[pj.ind[i]].shiftignore != 0 || windows[pj.ind[i]].shiftend != 8) return false;
        return true;
    };
    std::vector<size_t> firsts, seconds;
    for (size_t b = 0; b < groups.size();) {
        size_t e = b;
        while (e < groups.size() && groups[e].chrom == groups[b].chrom) e++;
        size_t open = e;                                   // an eligible four waiting for its partner
        for (size_t g = b; g < e; g++) {
            if (!all_modes(groups[g])) continue;
            if (open == e) open = g;
            else {
                firsts.push_back(open);
                seconds.push_back(g);
                open = e;
            }
        }
        b = e;
    }
    size_t n8 = firsts.size();
    if (waves > 0 && n8 >= waves) n8 = n8 / waves * waves;
    if (n8 == 0) return 0;
    std::vector<uint8_t>   paired(groups.size(), 0);
    std::vector<PackedJob> out;
    out.reserve(groups.size());
    for (size_t k = 0; k < n8; k++) {
        out.push_back(groups[firsts[k]]);
        out.push_back(groups[seconds[k]]);
        paired[firsts[k]] = paired[seconds[k]] = 1;
    }
    for (size_t g = 0; g < groups.size(); g++)
        if (!paired[g]) out.push_back(groups[g]);
    groups.swap(out);
    return n8;
}

// ------------------------------------------------------------------------------------------------ the plan kept across sweeps
// What the job list of a sweep, its groups of four and eight and their device copies depend on.  The windows change only
// with the rows or the pedigree, and the engine and every analysis mode sweep the same windows again and again: a context keeps
// the plan of its last sweep and a call with an equal key takes it as it stands (no list is built, copied or uploaded and
// the stream is not synchronised in front of the kernels).  The grids are NOT part of the plan: they are formed per call from
// the memory that is free then.
struct PlanKey {
    // the windows and the map (counters of their derivations and uploads) and the call's range
    unsigned windows_gen = 0, map_gen = 0;
    int      ind_begin = 0, n = 0;
    // the flags that enter plan_jobs, group_uniform_jobs and pair_uniform_groups or decide whether the call's lines do
    // (PLAN_KEY_FLAGS), and whether the call's mode sweeps uniform windows on their own instantiation at all
    uint32_t flags = 0;
    int      uniform_mode = 0;
    // the lines' state: the call's lines, the cap they were numbered under and what the record buffer had room for
    int      n_lines = 0, lines_cap = 0, lines_fit = 0;
    // the eights are a whole number of rounds of the packed grid's resident waves: blocks of the packed grid, and what it is
    // formed from besides the call's own grid
    int      pack_cap = 0, reserve_blocks = 0, uni_blocks_per_cu = 0;
};
constexpr uint32_t PLAN_KEY_FLAGS = CNF2_MERGE_MODES | CNF2_FULL_SPILL | CNF2_FLUSH_TINY | CNF2_NO_TIES | CNF2_NO_UNIFORM_PACK |
                                    CNF2_NO_UNIFORM_PACK8 | CNF2_NO_LINE_RECORDS | CNF2_ALL_STATES | CNF2_XPOSE;

// the job list and the groups of four of key `a` are those of key `b`: everything but what only the pairing reads
inline bool plan_key_same_jobs(const PlanKey& a, const PlanKey& b)
{
    const uint32_t pairing = CNF2_NO_UNIFORM_PACK8;
    return a.windows_gen == b.windows_gen && a.map_gen == b.map_gen && a.ind_begin == b.ind_begin && a.n == b.n &&
           (a.flags & PLAN_KEY_FLAGS & ~pairing) == (b.flags & PLAN_KEY_FLAGS & ~pairing) && a.uniform_mode == b.uniform_mode &&
           a.n_lines == b.n_lines && a.lines_cap == b.lines_cap && a.lines_fit == b.lines_fit;
}
// ... and the eights too: the whole plan
inline bool plan_key_same(const PlanKey& a, const PlanKey& b)
{
    return plan_key_same_jobs(a, b) && (a.flags & PLAN_KEY_FLAGS) == (b.flags & PLAN_KEY_FLAGS) && a.pack_cap == b.pack_cap &&
           a.reserve_blocks == b.reserve_blocks && a.uni_blocks_per_cu == b.uni_blocks_per_cu;
}

// ------------------------------------------------------------------------------------------------ grids and spill
// Doubles of a wave's spill slot per marker of the longest chromosome: covers every layout (520 or 528 doubles per (pair
// of) marker(s) in the fast kernel, 512 in the general kernel)
constexpr size_t PLAN_SPILL_ROW = 528;
inline size_t spill_stride(int max_len) { return (size_t)max_len * PLAN_SPILL_ROW; }
inline size_t spill_block_bytes(int max_len) { return (size_t)CNF2_WAVES_PER_BLOCK * spill_stride(max_len) * sizeof(double); }

// blocks of a kernel with `per_cu` blocks to a compute unit that are resident at once, less the workgroup slots left free
// for concurrent kernels
inline int resident_blocks(int n_cu, int per_cu, int reserve_blocks) { return std::max(1, n_cu * per_cu - reserve_blocks); }
// one wave per job in flight, capped (at what is resident: the spill stays small)
inline int grid_for(size_t n_jobs, int cap)
{
    const size_t blocks = (n_jobs + CNF2_WAVES_PER_BLOCK - 1) / CNF2_WAVES_PER_BLOCK;
    return (int)std::min(blocks, (size_t)cap);
}

// cnf2_sweep and its modes: the share of free memory (plus what the context already holds of it) the spill slots may take
constexpr double PLAN_SWEEP_SPILL_SHARE = 0.6;

// Grids of the two kernels of a sweep: n_fast jobs of the untied windows (or packed jobs, whichever are more: the packed
// kernel runs before the ordinary fast kernel on the same stream and in the same spill slots) and n_general of the tied
// ones.  One spill slot per resident wave; long chromosomes make slots big: the spill stays within the share by running
// fewer waves, and when both kernels run -- side by side on two streams with disjoint slots -- they share the budget.
// false: not even one block's slots fit.
inline bool plan_sweep_grids(int n_cu, int fast_per_cu, int gen_per_cu, int reserve_blocks, size_t n_fast, size_t n_general,
                             size_t free_bytes, size_t held_bytes, int max_len, int* grid_fast, int* grid_gen)
{
    const size_t budget = (size_t)((double)(free_bytes + held_bytes) * PLAN_SWEEP_SPILL_SHARE);
    const size_t per_blk = spill_block_bytes(max_len);
    const size_t max_blks = budget / per_blk;
    if (max_blks < 1) return false;
    int gf = (int)std::min((size_t)grid_for(n_fast, resident_blocks(n_cu, fast_per_cu, reserve_blocks)), max_blks);
    int gg = (int)std::min((size_t)grid_for(n_general, resident_blocks(n_cu, gen_per_cu, reserve_blocks)), max_blks);
    if (n_fast > 0 && n_general > 0)
        while ((size_t)(gf + gg) * per_blk > budget && gf + gg > 2) {
            if (gf > 1) gf--;
            if (gg > 1 && (size_t)(gf + gg) * per_blk > budget) gg--;
        }
    *grid_fast = gf;
    *grid_gen  = gg;
    return true;
}

// ------------------------------------------------------------------------------------------------ batched consumers
// cnf2_sweep_accumulate and cnf2_sweep_turn_scan: the spill takes at most a quarter of what is free, the batch buffer half of
// the rest; a batch holds at most PLAN_BATCH_MAX_JOBS jobs
constexpr size_t PLAN_BATCH_SPILL_PART = 4;
constexpr size_t PLAN_BATCH_ROWS_PART  = 2;
constexpr size_t PLAN_BATCH_MAX_JOBS   = 1000000;

// A batch of the batched consumers is swept by the resident waves in rounds (a wave takes the next job when it has finished
// one): 6.1 rounds take the time of 7.  When the jobs do not fit one batch, a batch is a whole number of rounds.
inline size_t whole_rounds(size_t batch, size_t n_jobs, int grid_cap)
{
    const size_t waves = (size_t)grid_cap * CNF2_WAVES_PER_BLOCK;
    if (batch >= n_jobs || batch < waves) return batch;
    return batch / waves * waves;
}

enum BatchFit { BATCH_FITS = 0, BATCH_NO_SPILL, BATCH_NO_PART, BATCH_NO_ROWS };   // what memory did not suffice for
struct BatchPlan {
    BatchFit fit = BATCH_FITS;
    int      grid_cap = 0;     // blocks of a sweep launch (one spill slot per wave)
    size_t   batch = 0;        // jobs per batch
};

// free_bytes: what the device reports free; held_bytes: the spill and the batch buffer the context already holds (they are
// reused or replaced).  row_doubles: doubles of the batch buffer per job and marker (512 for the accumulate weights,
// CNF2_TURN_ROW for the turn scan).  part_need / part_held: doubles of the per-individual rows of CNF2_DETERMINISTIC (0 without)
// and what the context holds of them; they are taken out of what is free BEFORE the batch buffer is sized, so that the batch
// buffer cannot leave them without memory.  batch_jobs: the caller's cap on a batch (0 = none).
inline BatchPlan plan_batches(int n_cu, int per_cu, int reserve_blocks, size_t free_bytes, size_t held_bytes, int max_len,
                              size_t row_doubles, size_t n_jobs, int batch_jobs, size_t part_need, size_t part_held)
{
    BatchPlan    plan;
    size_t       free_b = free_bytes + held_bytes;
    const size_t per_blk = spill_block_bytes(max_len);
    plan.grid_cap = resident_blocks(n_cu, per_cu, reserve_blocks);
    const size_t spill_max = free_b / PLAN_BATCH_SPILL_PART;
    if ((size_t)plan.grid_cap * per_blk > spill_max) plan.grid_cap = (int)(spill_max / per_blk);
    if (plan.grid_cap < 1) {
        plan.fit = BATCH_NO_SPILL;
        return plan;
    }
    if (part_need) {
        const size_t need = part_need * sizeof(double), have = part_held * sizeof(double);
        if (need > free_b / 2 + have) {
            plan.fit = BATCH_NO_PART;
            return plan;
        }
        free_b -= need > have ? need - have : 0;
    }
    const size_t per_job = (size_t)max_len * row_doubles;
    plan.batch = (free_b - (size_t)plan.grid_cap * per_blk) / PLAN_BATCH_ROWS_PART / (per_job * sizeof(double));
    if (plan.batch < 1) {
        plan.fit = BATCH_NO_ROWS;
        return plan;
    }
    plan.batch = std::min(std::min(plan.batch, n_jobs), PLAN_BATCH_MAX_JOBS);
    plan.batch = whole_rounds(plan.batch, n_jobs, plan.grid_cap);
    if (batch_jobs > 0 && plan.batch > (size_t)batch_jobs) plan.batch = (size_t)batch_jobs;
    return plan;
}

} // namespace cnf2
#endif
