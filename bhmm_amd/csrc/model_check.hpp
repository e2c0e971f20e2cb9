// model_check.hpp -- validation of caller-supplied models shared by the units that take a model at face
// value (bhmm_score, score_api.hip; bhmm_posterior_decode, post_api.hip): stochastic rows, finite entries,
// positive sigmas.  Host code only.
#pragma once
#include <math.h>

#include <cmath>
#include <string>

#include "host_common.hpp"
#include "host_internal.hpp"

namespace bhmm {

constexpr double MODEL_STOCH_TOL = 1e-8; // rows of A, pi and B must sum to 1 within this

// who: the entry point named in the message ("bhmm_score")
inline int check_prob_rows(const char *who, const double *p, int rows, int cols, int s, const char *what)
{
    for (int r = 0; r < rows; ++r) {
        double sum = 0.0;
        for (int j = 0; j < cols; ++j) {
            const double v = p[(size_t)r * cols + j];
            if (!std::isfinite(v) || v < 0.0)
                return invalid_arg(std::string(who) + ": model " + std::to_string(s) + ": " + what +
                                   " has a negative or non-finite entry");
            sum += v;
        }
        if (!(fabs(sum - 1.0) <= MODEL_STOCH_TOL))
            return invalid_arg(std::string(who) + ": model " + std::to_string(s) + ": " + what +
                               (rows > 1 ? " row " + std::to_string(r) : std::string()) + " sums to " +
                               std::to_string(sum) + ", not 1");
    }
    return BHMM_OK;
}

// S stacked models in the conventions of bhmm_score
inline int check_models(const bhmm_ctx *c, const char *who, int S, const double *A, const double *pi,
                        const double *par0, const double *par1)
{
    const int n = c->n;
    int rc;
    for (int s = 0; s < S; ++s) {
        if ((rc = check_prob_rows(who, A + (size_t)s * n * n, n, n, s, "A")) ||
            (rc = check_prob_rows(who, pi + (size_t)s * n, 1, n, s, "pi")))
            return rc;
        if (c->kind == EMIT_GAUSS) {
            for (int i = 0; i < n; ++i) {
                const double mu = par0[(size_t)s * n + i], sg = par1[(size_t)s * n + i];
                if (!std::isfinite(mu) || !std::isfinite(sg) || !(sg > 0.0) ||
                    !std::isfinite(1.0 / (sqrt(2.0 * M_PI) * sg)))
                    return invalid_arg(std::string(who) + ": model " + std::to_string(s) +
                                       ": means must be finite and sigmas positive and finite");
            }
        } else if (c->kind == EMIT_DISC) {
            if ((rc = check_prob_rows(who, par0 + (size_t)s * n * c->M, n, c->M, s, "B")))
                return rc;
        }
    }
    return BHMM_OK;
}

} // namespace bhmm
