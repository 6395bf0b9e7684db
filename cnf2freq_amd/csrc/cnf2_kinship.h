// cnf2_kinship.h -- what the kernels of cnf2_kinship_kernels.hip read and write (cnf2_kinship_sums, include/cnf2hip.h), and
// the split of the marker range, which host and device code share.
//
// sum[i][j] = sum over the markers m of a chromosome range of a_i(m) a_j(m), a_i(m) = origin[i][m][3] - origin[i][m][0]:
// the realised line-origin similarity as raw sums.  The kinship K = (1 + sum / markers) / 2 is the caller's, so that
// leaving a chromosome out is a subtraction of sums.
#ifndef CNF2_KINSHIP_H
#define CNF2_KINSHIP_H

#include <stddef.h>
#include <stdint.h>

namespace cnf2 {

constexpr int KIN_TILE   = 128;      // individuals per side of a block's output tile (four waves, 64 x 64 each)
constexpr int KIN_KC     = 16;       // markers per LDS panel
constexpr int KIN_CHUNK  = 256;      // markers per partial sum where the marker range is split
constexpr int KIN_ROUND  = 32;       // chunks whose partial sums are held together at most (and under 256 MB)
constexpr int KIN_SPLIT_TILES = 128; // the range is split where the lower triangle has fewer block tiles than this

// How a call sums: with fewer than KIN_SPLIT_TILES block tiles (n <= 1920) and more than KIN_CHUNK markers every chunk
// of KIN_CHUNK markers is summed on its own from zero and the chunks' sums are added in ascending order; else every
// output tile sums the whole range in one pass.  A function of n and the marker count alone: the bits do not depend on
// the machine or on how many chunks are in flight together.
inline bool kin_is_split(int n, int n_mark)
{
    const long nt = (n + KIN_TILE - 1) / KIN_TILE;
    return nt * (nt + 1) / 2 < KIN_SPLIT_TILES && n_mark > KIN_CHUNK;
}

#if defined(__HIPCC__)
struct KinParams {
    int           n, M;          // individuals, markers of the map (the stride of origin)
    int           m_lo, n_mark;  // the range's first marker and its markers
    int           n_pad, m_pad;  // the image's sides: n up to KIN_TILE, n_mark up to KIN_KC
    const double* origin;        // [n][M][4]
    double*       image;         // [m_pad][n_pad]: a, marker-major, zero past n and past n_mark
    int           k_lo, k_len;   // the image rows block z = 0 sums (block z: k_lo + z k_len ..), a multiple of KIN_KC
    double*       out;           // [gridDim.z][n][n]
    int           parts, first;  // kin_finish_kernel: partial sums to add; first != 0: onto zero, not onto sum
    double*       sum;           // [n][n]
};
void launch_kin_pack(const KinParams& q, hipStream_t stream);
void launch_kin_syrk(const KinParams& q, int chunks, hipStream_t stream);
void launch_kin_finish(const KinParams& q, hipStream_t stream);
#endif

} // namespace cnf2
#endif
