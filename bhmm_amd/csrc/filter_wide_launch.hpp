// filter_wide_launch.hpp -- what filter_api.hip sees of filter_wide.hip: the 72 instantiations of k_filter_wide
// (filter_wide_kernels.hpp) and the forgetting probe of the 9..64-state family compile in a unit of their own.
#pragma once
#include <stdint.h>

#include "ctx.hpp"
#include "score_wide_kernels.hpp" // ScoreWideModel, Segs

namespace bhmm {

struct FilterWideArgs {
    const ScoreWideModel *dm; // the model's table entry on the device
    int W;                    // warm-up in steps
    Segs sg;                  // the filter plan
    void *rows, *logc;        // double / float (f32) or nullptr
    const double *V;          // device copy of the projection, or nullptr
    int Q;
    bool f32;
    double *aentry, *aexit;   // [nseg][n]
    uint8_t *dead;            // [nseg]
};

// one launch of k_filter_wide on c->stream; np: lanes per segment (16, 32, 64)
int filter_wide_launch(bhmm_ctx *c, int np, const FilterWideArgs &a);

// k_wide_probe<np, kind>, forward chains only (the first P / (64 / np) workgroups); curve: 2 * Wmax words, zeroed
int filter_wide_probe_launch(bhmm_ctx *c, int np, const WideModel &m, const int64_t *d_starts, int P, int Wmax,
                             unsigned int *d_curve);

} // namespace bhmm
