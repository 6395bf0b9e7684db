// cnf2_remap.h -- the M-step of the marker map from summed crossover posteriors (cnf2_sweep_crossovers), shared by the
// executable's --remap and by libcnf2host.so (cnf2h_map_mstep, include/cnf2host.h).
#ifndef CNF2_REMAP_H
#define CNF2_REMAP_H

#include <stdint.h>

#include <string>

namespace cnf2host {

// r-hat is kept in [REMAP_RMIN, REMAP_RMAX]: an interval never closes to a zero length (which would freeze it: a gap with
// dist <= 0 performs no transition and is left alone) and never opens to r = 0.5 (d = infinity)
constexpr double REMAP_RMIN = 1e-9;
constexpr double REMAP_RMAX = 0.499;

// Per interval m -> m+1 with pos[m+1] - pos[m] > 0: the d > 0 that maximises
//     sum_t  S_t log r_t(d) + (C - S_t) log(1 - r_t(d)),   r_t(d) = 0.5 (1 - exp(genrec[TYPEGENS[t]] d)),
// S_t = xo_sum[m][t], C = n_contrib[chromosome of m].  genrec[0] == genrec[1]: closed form r = sum S / 6C; otherwise a
// safeguarded Newton iteration on the derivative (bisection inside the bracket of the clamp).  Intervals with dist <= 0
// or C == 0 keep their length.  new_pos starts every chromosome at its old first position and adds the lengths.
void map_mstep(const double* pos, int n_markers, const int32_t* chromstarts, int n_chrom, const double* genrec,
               const double* xo_sum, const int32_t* n_contrib, double* new_pos);

// writes the map in the format read_alpha_map parses (one position per line, "%.17g": exact) and reads it back: returns
// false (with the reason in *err) if the file cannot be written or does not give the same positions and chromstarts -- a
// chromosome whose new last position is not above the next chromosome's first one would merge with it
bool write_map_checked(const char* path, const double* pos, int n_markers, const int32_t* chromstarts, int n_chrom,
                       std::string* err);

// interval length maximising the expected complete-data log-likelihood of one interval (see map_mstep)
double mstep_interval(const double S[6], double C, const double genrec[3]);

}  // namespace cnf2host
#endif
