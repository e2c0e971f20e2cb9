// mvn_density.hpp -- what k_mvn_rows (mvn_kernels.hpp) and k_gmm_rows (gmm_kernels.hpp) share: the shape of a rows
// kernel and the arithmetic of one gaussian log-density of a lane's observation.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

namespace bhmm {
namespace mvn {

constexpr int ROWS_THREADS = 256; // steps per workgroup of k_mvn_rows
constexpr int ROWS_NB = 16;       // states whose l pass through LDS at a time (ROWS_NB * ROWS_THREADS doubles)
constexpr int X_PIECE = 3968;     // doubles of a tile's observations staged at a time: X_PIECE * 33 / 32 <= ROWS_NB * ROWS_THREADS
static_assert(X_PIECE + X_PIECE / 32 <= ROWS_NB * ROWS_THREADS, "the skewed piece must fit s_l");
// doubles of one state's whitening table
__host__ __device__ inline size_t factor_size(int D, bool diag) { return diag ? (size_t)D : (size_t)D * (D + 1) / 2; }

// NaN stays; a NaN l makes m NaN
__device__ inline double nan_max(double m, double l) { return m != m ? m : ((l > m || l != l) ? l : m); }

// l = -|W (x - mu)|^2 / 2 + c of the lane's observation x for one table entry (k_mvn_rows, k_gmm_rows): the mean is
// subtracted first, the difference whitened row by row of the packed triangle (DIAG: D reciprocals), every product
// an explicit fma.  mui, Wi and c are uniform over the wavefront.
template <int DMAX, bool DIAG>
__device__ __forceinline__ double log_density(const double (&x)[DMAX], int D, const double *__restrict__ mui,
                                              const double *__restrict__ Wi, double c)
{
    double d[DMAX];
#pragma unroll
    for (int a = 0; a < DMAX; ++a)
        d[a] = a < D ? x[a] - mui[a] : 0.0;
    double q = 0.0;
#pragma unroll
    for (int a = 0; a < DMAX; ++a) {
        if (a < D) { // (uniform)
            double z;
            if constexpr (DIAG) {
                z = Wi[a] * d[a];
            } else {
                const double *Wa = Wi + a * (a + 1) / 2;
                z = 0.0;
#pragma unroll
                for (int b = 0; b <= a; ++b)
                    z = fma(Wa[b], d[b], z);
            }
            q = fma(z, z, q);
        }
    }
    return fma(-0.5, q, c);
}

} // namespace mvn
} // namespace bhmm
