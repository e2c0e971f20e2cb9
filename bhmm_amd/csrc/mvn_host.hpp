// mvn_host.hpp -- what mvn_api.hip defines and gmm_api.hip also calls: the checks of shapes and parameters, the
// launcher of the moment kernels for any column count, the device temporaries of a level-1 call.
#pragma once
#include <hip/hip_runtime.h>

#include <string>
#include <vector>

#include "host_internal.hpp"

namespace bhmm {

// n table entries (states, or components of all states), D dimensions, the covariance type; BHMM_ERR_INVALID
int mvn_shape_ok(const char *who, int n, int D, int cov_type);
// [mu | W | c] of n entries, validated, in tab[0 .. n * (D + factor size + 1)); BHMM_ERR_INVALID / BHMM_ERR_SIGMA
int mvn_make_table(const char *who, int n, int D, int cov_type, const double *means, const double *covs,
                   std::vector<double> &tab);
// k_mvn_moments + k_mvn_moments_finish over the observations of c->mvn with weights gamma_dev [total][ncols] (device)
// about means [ncols * D] (host) into out [ncols * moment stride] (host); device time in c->mvn.moments_ms.
// Synchronous.
int mvn_run_moments(bhmm_ctx *c, const double *gamma_dev, int ncols, const double *means, int cov_type, double *out);
// k_mvn_path_moments + k_mvn_moments_finish over the observations of c->mvn with the hard labels at path_dev (device;
// int32, or path_u8: one byte per step) in [0, nlabels): the states of a hidden path, or its components s_t M + c_t.
// About means [nlabels * D] (host) or, means == NULL, means_dev (device) into out [nlabels * moment stride] (host);
// device time in c->mvn.path_moments_ms.  BHMM_ERR_INVALID (who: the caller's name) for a label out of range, nothing
// is delivered then.  Synchronous.
int mvn_run_path_moments(bhmm_ctx *c, const char *who, const void *path_dev, int path_u8, int nlabels,
                         const double *means, const double *means_dev, int cov_type, double *out);

// k_mvn_shift on the stream: c->mvn.shift[k] = sum of c->mvn.m over trajectory k
hipError_t mvn_launch_shift(bhmm_ctx *c);

struct MvnTmp { // device allocations of one level-1 call
    std::vector<void *> ptrs;
    ~MvnTmp()
    {
        for (void *p : ptrs)
            (void)hipFree(p);
    }
    int alloc(double **out, size_t count)
    {
        void *p = nullptr;
        const hipError_t e = hipMalloc(&p, count * sizeof(double));
        if (e != hipSuccess) {
            (void)hipGetLastError();
            set_error("hipMalloc of " + std::to_string(count * sizeof(double)) + " bytes failed");
            return BHMM_ERR_NO_MEM;
        }
        ptrs.push_back(p);
        *out = static_cast<double *>(p);
        return BHMM_OK;
    }
};

} // namespace bhmm
