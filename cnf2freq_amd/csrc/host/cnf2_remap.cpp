// cnf2_remap.cpp -- see cnf2_remap.h.
#include "cnf2_remap.h"

#include <math.h>
#include <stdio.h>

#include "cnf2_readers.h"

namespace cnf2host {

namespace {
// d of a recombination fraction r under rate g (< 0): r = 0.5 (1 - exp(g d))
double dist_of(double r, double g) { return log1p(-2.0 * r) / g; }

// derivative (and second derivative) in d of  sum over the two meiosis types of S log r + (n - S) log(1 - r)
void derivs(double d, const double Sg[2], const double ng[2], const double g[2], double* f1, double* f2)
{
    *f1 = 0.0;
    *f2 = 0.0;
    for (int k = 0; k < 2; k++) {
        if (ng[k] <= 0.0) continue;
        const double ex = exp(g[k] * d);
        const double r  = 0.5 * (1.0 - ex);
        const double r1 = -0.5 * g[k] * ex;             // dr/dd > 0
        const double r2 = -0.5 * g[k] * g[k] * ex;      // d2r/dd2 < 0
        const double a  = Sg[k] / r - (ng[k] - Sg[k]) / (1.0 - r);
        const double b  = -Sg[k] / (r * r) - (ng[k] - Sg[k]) / ((1.0 - r) * (1.0 - r));
        *f1 += a * r1;
        *f2 += b * r1 * r1 + a * r2;
    }
}
}  // namespace

double mstep_interval(const double S[6], double C, const double genrec[3])
{
    // TYPEGENS = {1,0,0,1,0,0}: bits 0 and 3 recombine at genrec[1], the other four at genrec[0]
    const double Sg[2] = {S[1] + S[2] + S[4] + S[5], S[0] + S[3]};
    const double ng[2] = {4.0 * C, 2.0 * C};
    const double g[2]  = {genrec[0], genrec[1]};
    if (genrec[0] == genrec[1]) {
        double r = (Sg[0] + Sg[1]) / (6.0 * C);
        r        = r < REMAP_RMIN ? REMAP_RMIN : r > REMAP_RMAX ? REMAP_RMAX : r;
        return dist_of(r, g[0]);
    }
    // bracket: the lengths at which the faster-recombining type reaches REMAP_RMIN / REMAP_RMAX
    const double gmax = fabs(g[0]) > fabs(g[1]) ? g[0] : g[1], gmin = fabs(g[0]) > fabs(g[1]) ? g[1] : g[0];
    double lo = dist_of(REMAP_RMIN, gmax), hi = dist_of(REMAP_RMAX, gmin);
    double f1, f2;
    derivs(lo, Sg, ng, g, &f1, &f2);
    if (f1 <= 0.0) return lo;
    derivs(hi, Sg, ng, g, &f1, &f2);
    if (f1 >= 0.0) return hi;
    // start from the pooled closed form, then Newton steps kept inside the bracket (bisection where a step leaves it)
    double r0 = (Sg[0] + Sg[1]) / (6.0 * C);
    r0        = r0 < REMAP_RMIN ? REMAP_RMIN : r0 > REMAP_RMAX ? REMAP_RMAX : r0;
    const double gw = (4.0 * g[0] + 2.0 * g[1]) / 6.0;
    double d = dist_of(r0, gw);
    if (!(d > lo && d < hi)) d = 0.5 * (lo + hi);
    for (int it = 0; it < 200; it++) {
        derivs(d, Sg, ng, g, &f1, &f2);
        if (f1 > 0.0) lo = d;
        else hi = d;
        double dn = (f2 < 0.0) ? d - f1 / f2 : 0.5 * (lo + hi);
        if (!(dn > lo && dn < hi)) dn = 0.5 * (lo + hi);
        if (fabs(dn - d) <= 1e-13 * (fabs(d) + 1e-300) || hi - lo <= 1e-15 * hi) return dn;
        d = dn;
    }
    return d;
}

void map_mstep(const double* pos, int n_markers, const int32_t* chromstarts, int n_chrom, const double* genrec,
               const double* xo_sum, const int32_t* n_contrib, double* new_pos)
{
    const double gdef[3] = {-0.02, -0.02, -0.02};
    if (!genrec) genrec = gdef;
    for (int c = 0; c < n_chrom; c++) {
        const int first = chromstarts[c], last = chromstarts[c + 1] - 1;
        if (first > last || last >= n_markers) continue;
        new_pos[first] = pos[first];
        for (int m = first; m < last; m++) {
            const double dist = pos[m + 1] - pos[m];
            double       d    = dist;
            if (dist > 0.0 && n_contrib[c] > 0) d = mstep_interval(xo_sum + (size_t)m * 6, (double)n_contrib[c], genrec);
            new_pos[m + 1] = new_pos[m] + d;
        }
    }
}

bool write_map_checked(const char* path, const double* pos, int n_markers, const int32_t* chromstarts, int n_chrom,
                       std::string* err)
{
    FILE* f = fopen(path, "w");
    if (!f) {
        *err = std::string("cannot write ") + path;
        return false;
    }
    for (int m = 0; m < n_markers; m++) fprintf(f, "%.17g\n", pos[m]);
    if (fclose(f) != 0) {
        *err = std::string("cannot write ") + path;
        return false;
    }
    Pedigree P;
    FILE*    in = fopen(path, "r");
    const bool ok = read_alpha_map(in, P);
    if (in) fclose(in);
    if (!ok || (int)P.pos.size() != n_markers || (int)P.chromstarts.size() != n_chrom + 1) {
        *err = std::string(path) + ": the written map does not read back with the same chromosomes";
        return false;
    }
    for (int c = 0; c <= n_chrom; c++)
        if (P.chromstarts[c] != chromstarts[c]) {
            *err = std::string(path) + ": the written map does not read back with the same chromosomes";
            return false;
        }
    for (int m = 0; m < n_markers; m++)
        if (P.pos[m] != pos[m]) {
            *err = std::string(path) + ": the written map does not read back to the same positions";
            return false;
        }
    return true;
}

}  // namespace cnf2host
