// pair_launch.hpp -- what the units of bhmm_posterior_transitions share: one verified pass of k_pair_sweep
// (pair_kernels.hpp) for N = 1 .. 8 states, and the launch of k_pair_tile.  The pass is instantiated in
// pair_sweep_n.hip, once per N (one translation unit each, like score_tile_nt.hip: the sixteen kernels of one N take
// minutes to compile), and only declared for pair_api.hip.  Buffers, options and counters of the call are the
// context's (ctx.hpp: pair, opt.pair_*, last.pair_*).
#pragma once
#include <vector>

#include "fused_host.hpp"
#include "host_common.hpp"
#include "host_internal.hpp"
#include "launch.hpp"
#include "pair_kernels.hpp"

namespace bhmm {

struct PairOut {      // where the rows go on the device, and what they are
    void *dev;        // [total][Qp] of double / float
    const double *W;  // device copy of the pair weights, [n][n][PAIR_QMAX] padded with zeros, or nullptr
    int Q;            // its columns (0: the jump form)
    int Qp;           // values per row
    bool f32;
};

// the sweep over every range of chunk groups at warm-up W and the check; *v: failed with boundaries out of tolerance
template <int N, int KIND>
int pair_pass(bhmm_ctx *c, const Model<N> *dm, int W, const PairOut &o, plan::Verdict *v);

// ---- k_pair_tile, the matrix-core row kernel of the generic path (pair_tile.hip) ----
constexpr int PAIR_TILE_MAX_N = 128; // eight column tiles of 16 states
// matrices of a call with Q weight columns: A, then one per column, or the one of the jump form
inline int pair_tile_matrices(int Q) { return 1 + (Q > 0 ? Q : 1); }
// Bop: [A | M_1 | ...] for n states in the operand order of k_pair_tile, padded with zeros to 16 * ceil(n / 16);
// Wpad: [n][n][PAIR_QMAX] (unused where Q == 0)
void pair_tile_operands(const double *A, const double *Wpad, int n, int Q, std::vector<double> &Bop);
// k_pair_tile over c->pair.filt / gam with the matrices in c->pair.Bop, rows to o.dev; n <= 128
int pair_tile_rows(bhmm_ctx *c, const PairOut &o);

#define PAIR_PASS_DECL(X, NV)                                                                                      \
    X template int pair_pass<NV, EMIT_GAUSS>(bhmm_ctx *, const Model<NV> *, int, const PairOut &, plan::Verdict *); \
    X template int pair_pass<NV, EMIT_DISC>(bhmm_ctx *, const Model<NV> *, int, const PairOut &, plan::Verdict *);

} // namespace bhmm
