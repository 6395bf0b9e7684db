// cnf2_qtl_host.h -- the host side of `cnF2freq --qtl` (and cnf2h_qtl_permutations of include/cnf2host.h): the phenotype
// table, the permutations and null-model residuals of a permutation test by the rules of cnf2freq_amd/qtl.py, and the
// thresholds.  The scan itself is cnf2_qtl_scan / cnf2_sweep_qtl of include/cnf2hip.h; nothing here regresses on markers.
#ifndef CNF2_QTL_HOST_H
#define CNF2_QTL_HOST_H

#include <math.h>
#include <stdint.h>

#include <algorithm>
#include <fstream>
#include <map>
#include <numeric>
#include <sstream>
#include <string>
#include <vector>

#include "../cnf2_qtl.h"

namespace cnf2host {

// value number idx of stream seed: synth.splitmix64 of the Python package
inline uint64_t qtl_splitmix64(uint64_t seed, uint64_t idx)
{
    uint64_t z = seed + (idx + 1) * 0x9E3779B97F4A7C15ull;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

// perm[P][n] by the rule of qtl.permutations: within every stratum the used individuals, ascending, are ordered by the key
// splitmix64(seed, p n + i) with a stable sort; unused individuals map to themselves.  use / strata may be null.
inline void qtl_permutations(int n, int P, uint64_t seed, const uint8_t* use, const int32_t* strata, int32_t* perm)
{
    std::map<int32_t, std::vector<int32_t>> groups;
    for (int i = 0; i < n; i++)
        if (!use || use[i]) groups[strata ? strata[i] : 0].push_back(i);
    std::vector<uint64_t> key(n);
    for (int p = 0; p < P; p++) {
        int32_t* row = perm + (size_t)p * n;
        for (int i = 0; i < n; i++) {
            row[i] = i;
            key[i] = qtl_splitmix64(seed, (uint64_t)p * (uint64_t)n + (uint64_t)i);
        }
        for (const auto& g : groups) {
            std::vector<int32_t> order(g.second);
            std::stable_sort(order.begin(), order.end(), [&](int32_t a, int32_t b) { return key[a] < key[b]; });
            for (size_t j = 0; j < order.size(); j++) row[g.second[j]] = order[j];
        }
    }
}

// count[B][n] by the rule of qtl.bootstrap_counts: within every stratum the k used individuals, ascending, are idx[0..k); draw
// j of replicate b -- one per used individual j -- picks idx[floor(u k)] of j's stratum with u = (splitmix64(seed, b n + j)
// >> 11) 2^-53.  Every row sums to the used individuals of each stratum.  use / strata may be null.
inline void qtl_bootstrap_counts(int n, int B, uint64_t seed, const uint8_t* use, const int32_t* strata, int32_t* count)
{
    std::map<int32_t, std::vector<int32_t>> groups;
    for (int i = 0; i < n; i++)
        if (!use || use[i]) groups[strata ? strata[i] : 0].push_back(i);
    std::fill(count, count + (size_t)B * n, 0);
    for (int b = 0; b < B; b++) {
        int32_t* row = count + (size_t)b * n;
        for (const auto& g : groups) {
            const size_t k = g.second.size();
            for (int32_t j : g.second) {
                const double u = (double)(qtl_splitmix64(seed, (uint64_t)b * (uint64_t)n + (uint64_t)j) >> 11) * 0x1p-53;
                row[g.second[std::min(k - 1, (size_t)floor(u * (double)k))]]++;
            }
        }
    }
}

// res[n][T]: the residuals of every phenotype column on [1, cov] over the used individuals, 0 for the others
// (qtl.null_residuals).  false when the null design has no Cholesky factor.  The normal equations are those of the columns
// minus their means over the used individuals (qtl_column_mean, as in the scans): the residuals do not depend on offsets.
inline bool qtl_null_residuals(int n, int T, const double* pheno, int K, const double* cov, const uint8_t* use, double* res)
{
    using namespace cnf2;
    const int nx = K + 1;
    double    zmean[QTL_NX] = {0.0};
    for (int k = 1; k < nx; k++) zmean[k] = qtl_column_mean(cov + (k - 1), n, K, use);
    auto      x  = [&](int i, int k) { return k == 0 ? 1.0 : cov[(size_t)i * K + (k - 1)] - zmean[k]; };
    double    S[QTL_NX * QTL_NX] = {0.0};
    for (int i = 0; i < n; i++)
        if (use[i])
            for (int j = 0; j < nx; j++)
                for (int k = 0; k <= j; k++) S[j * QTL_NX + k] += x(i, j) * x(i, k);
    std::fill(res, res + (size_t)n * T, 0.0);
    if (!qtl_cholesky(S, nx)) return false;
    for (int t = 0; t < T; t++) {
        const double ymean     = qtl_column_mean(pheno + t, n, T, use);
        double       b[QTL_NX] = {0.0};
        for (int i = 0; i < n; i++)
            if (use[i])
                for (int k = 0; k < nx; k++) b[k] += x(i, k) * (pheno[(size_t)i * T + t] - ymean);
        qtl_chol_solve(S, nx, b);
        for (int i = 0; i < n; i++)
            if (use[i]) {
                double fit = 0.0;
                for (int k = 0; k < nx; k++) fit += x(i, k) * b[k];
                res[(size_t)i * T + t] = (pheno[(size_t)i * T + t] - ymean) - fit;
            }
    }
    return true;
}

// grp[n] / cell[n] of the analysed records dous[n] for the within-family scan (cnf2_qtl_scan_fam; qtl.families): the parent on
// the side (par[.][side]) and the pair of parents, both numbered from 0 in ascending order of the records; -1 where the
// parent on the side is missing or has no recorded parents.  par[n_rec][2], -1 = none.  Returns the parents counted.
inline int qtl_families(const int32_t* par, int n, const int32_t* dous, int side, int32_t* grp, int32_t* cell)
{
    std::vector<int32_t>                     parents;
    std::vector<std::pair<int32_t, int32_t>> pairs;
    for (int i = 0; i < n; i++) {
        const int32_t p = par[2 * dous[i] + side];
        grp[i]          = (p >= 0 && (par[2 * p] >= 0 || par[2 * p + 1] >= 0)) ? p : -1;
        if (grp[i] >= 0) {
            parents.push_back(p);
            pairs.push_back({par[2 * dous[i]], par[2 * dous[i] + 1]});
        }
    }
    std::sort(parents.begin(), parents.end());
    parents.erase(std::unique(parents.begin(), parents.end()), parents.end());
    std::sort(pairs.begin(), pairs.end());
    pairs.erase(std::unique(pairs.begin(), pairs.end()), pairs.end());
    for (int i = 0; i < n; i++) {
        cell[i] = -1;
        if (grp[i] < 0) continue;
        const std::pair<int32_t, int32_t> pr = {par[2 * dous[i]], par[2 * dous[i] + 1]};
        grp[i]  = (int32_t)(std::lower_bound(parents.begin(), parents.end(), grp[i]) - parents.begin());
        cell[i] = (int32_t)(std::lower_bound(pairs.begin(), pairs.end(), pr) - pairs.begin());
    }
    return (int)parents.size();
}

// col[n][8] of the analysed records dous[n] for the founder-haplotype scan (cnf2_qtl_scan_hap; origins.descent_columns): cell
// 4 s + 2 w + b of a descent row belongs to grandparent par[par[dous[i]][s]][w], strand b.  The distinct grandparents are
// numbered g from 0 in ascending order of the records.  by 0 "haplotype": column 2 g + b; 1 "founder": column g; 2 "line":
// column w.  A side whose parent is missing or has no two recorded parents gets -1 in its four cells.  Returns the
// grandparents counted.
inline int descent_columns(const int32_t* par, int n, const int32_t* dous, int by, int32_t* col)
{
    std::vector<int32_t> grand;
    auto gp = [&](int i, int s, int w) -> int32_t {
        const int32_t p = par[2 * dous[i] + s];
        if (p < 0 || par[2 * p] < 0 || par[2 * p + 1] < 0) return -1;
        return par[2 * p + w];
    };
    for (int i = 0; i < n; i++)
        for (int s = 0; s < 2; s++)
            for (int w = 0; w < 2; w++)
                if (gp(i, s, w) >= 0) grand.push_back(gp(i, s, w));
    std::sort(grand.begin(), grand.end());
    grand.erase(std::unique(grand.begin(), grand.end()), grand.end());
    for (int i = 0; i < n; i++)
        for (int s = 0; s < 2; s++)
            for (int w = 0; w < 2; w++) {
                const int32_t r = gp(i, s, w);
                const int32_t g = r < 0 ? -1 : (int32_t)(std::lower_bound(grand.begin(), grand.end(), r) - grand.begin());
                for (int b = 0; b < 2; b++)
                    col[8 * i + 4 * s + 2 * w + b] = r < 0 ? -1 : by == 0 ? 2 * g + b : by == 1 ? g : w;
            }
    return (int)grand.size();
}

// res[n][T]: the residuals of every phenotype column on a mean per cell[n] and cov over the used individuals, 0 for the
// others (qtl.cell_residuals): every column minus its mean over the used members of the cell, then qtl_null_residuals, whose
// intercept finds nothing left.  false when the centred covariates have no Cholesky factor.
inline bool qtl_cell_residuals(int n, int T, const double* pheno, int K, const double* cov, const uint8_t* use, const int32_t* cell,
                               double* res)
{
    std::vector<double>                  y(pheno, pheno + (size_t)n * T), z(cov, cov + (size_t)n * K);
    std::map<int32_t, std::vector<int>> members;
    for (int i = 0; i < n; i++)
        if (use[i]) members[cell[i]].push_back(i);
    auto centre = [&](std::vector<double>& v, int w) {
        for (const auto& m : members)
            for (int k = 0; k < w; k++) {
                double mean = 0.0;
                for (int pass = 0; pass < 2; pass++) {
                    double s = 0.0;
                    for (int i : m.second) s += v[(size_t)i * w + k] - mean;
                    mean += s / (double)m.second.size();
                }
                for (int i : m.second) v[(size_t)i * w + k] -= mean;
            }
    };
    centre(y, T);
    centre(z, K);
    return qtl_null_residuals(n, T, y.data(), K, z.data(), use, res);
}

// the (1 - alpha) threshold of P maxima (sorted in place): the order statistic number ceil((1 - alpha) P), as qtl.thresholds
inline double qtl_threshold(std::vector<double>& maxima, double alpha)
{
    std::sort(maxima.begin(), maxima.end());
    const int P = (int)maxima.size();
    const int k = std::min(P - 1, std::max(0, (int)ceil((1.0 - alpha) * P) - 1));
    return maxima[k];
}

// A whitespace table: a header "id name...", then one line per individual; "NA" or "-" is missing (NaN)
struct PhenoTable {
    std::vector<std::string>         columns;   // without the id column
    std::vector<std::string>         ids;
    std::vector<std::vector<double>> rows;      // [ids][columns]
};

inline bool read_pheno_table(const std::string& path, PhenoTable& T, std::string* err)
{
    std::ifstream in(path);
    if (!in) {
        *err = "cannot read " + path;
        return false;
    }
    std::string line, tok;
    int         lineno = 0;
    while (std::getline(in, line)) {
        lineno++;
        std::istringstream       ss(line);
        std::vector<std::string> f;
        while (ss >> tok) f.push_back(tok);
        if (f.empty()) continue;
        if (T.columns.empty() && T.ids.empty()) {
            if (f.size() < 2) {
                *err = path + ": the header needs an id column and at least one name";
                return false;
            }
            T.columns.assign(f.begin() + 1, f.end());
            continue;
        }
        if (f.size() != T.columns.size() + 1) {
            *err = path + ": line " + std::to_string(lineno) + " has " + std::to_string(f.size()) + " fields, the header " +
                   std::to_string(T.columns.size() + 1);
            return false;
        }
        std::vector<double> v;
        for (size_t k = 1; k < f.size(); k++) {
            if (f[k] == "NA" || f[k] == "-") {
                v.push_back(NAN);
                continue;
            }
            char*        end = nullptr;
            const double x = strtod(f[k].c_str(), &end);
            if (*end != 0 || !std::isfinite(x)) {
                *err = path + ": line " + std::to_string(lineno) + ": \"" + f[k] + "\" is not a number, NA or -";
                return false;
            }
            v.push_back(x);
        }
        T.ids.push_back(f[0]);
        T.rows.push_back(v);
    }
    if (T.columns.empty()) {
        *err = path + ": no header";
        return false;
    }
    return true;
}

} // namespace cnf2host
#endif
