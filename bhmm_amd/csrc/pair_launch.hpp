// pair_launch.hpp -- one verified pass of k_pair_sweep (pair_kernels.hpp) for N = 1 .. 8 states.  The template is
// instantiated in pair_sweep_n.hip, once per N (one translation unit each, like score_tile_nt.hip: the sixteen
// kernels of one N take minutes to compile), and only declared for pair_api.hip.
#pragma once
#include <vector>

#include "fused_host.hpp"
#include "host_common.hpp"
#include "host_internal.hpp"
#include "launch.hpp"
#include "pair_kernels.hpp"

namespace bhmm {

// The buffers of bhmm_posterior_transitions -- model, B^T, alpha-row workspace of one range of chunk groups, boundary
// vectors of both directions, failure counter, probe curve, the pair weights W [n][n][PAIR_QMAX] (padded), the result
// staged on the device when the caller's buffer is on the host (out), and for the generic path the filtered rows
// (filt) and posterior rows (gam) of every step, [total][n] doubles each, and a device copy of the transition matrix
// (A) -- with its options and the counters of its last call.  One per context, kept by pair_api.hip beside the
// context (not in ctx.hpp: no other unit reads or writes any of it, and none is compiled differently for it);
// released by bhmm_pair_release.  device / stream: the context it was made for -- a state found under the address
// of a context with another device or stream belongs to a context that is gone, and is discarded.  W_host / A_host:
// what W and A on the device hold (an unchanged matrix is not uploaded again).  Bop / Bop_host: the matrices
// [A | M_1 | ...] of k_pair_tile in its operand order (pair_tile_kernels.hpp), kept under the same rule -- they are
// formed on the host at every call that takes that kernel and uploaded only where they differ from the kept copy, so
// a change of A, W, Q or of the form (jump / projected) rebuilds them and nothing else does.
struct PairState {
    int device = -1;
    hipStream_t stream = nullptr;
    std::vector<double> W_host, A_host, Bop_host;
    DevBuf<char> model, probe, out;
    DevBuf<double> Bt, ws, aentry, aexit, bassumed, bout, W, filt, gam, A, Bop;
    DevBuf<uint8_t> dead;
    DevBuf<unsigned int> fails;
    int opt_W = 0;         // option pair_W: warm-up fixed by the caller (0: measured)
    int opt_ws_mb = 8192;  // option pair_ws_mb: budget of the alpha-row workspace in MiB (0: unbounded)
    bool opt_fused = true; // option pair_fused: 0 never takes the fused path
    int fallbacks = 0;     // read-only pair_fallbacks: calls whose boundaries did not verify at the first warm-up
    int path = 0;          // read-only pair_path: first pass of the last call, 1 fused, 0 generic
    int opt_rows = -1;     // option pair_rows: row kernel of the generic path, 0 k_pair_rows, 1 k_pair_tile up to 128
                           // states, -1 by class (tile_takes, pair_api.hip)
    int rows_kernel = 0;   // read-only pair_rows_kernel: row kernel of the last generic pass (0 / 1 as above)
};

struct PairOut {      // where the rows go on the device, and what they are
    void *dev;        // [total][Qp] of double / float
    const double *W;  // device copy of the pair weights, [n][n][PAIR_QMAX] padded with zeros, or nullptr
    int Q;            // its columns (0: the jump form)
    int Qp;           // values per row
    bool f32;
};

// the sweep over every range of chunk groups at warm-up W and the check; *v: failed with boundaries out of tolerance
template <int N, int KIND>
int pair_pass(bhmm_ctx *c, PairState &b, const Model<N> *dm, int W, const double *dBt, const PairOut &o,
              plan::Verdict *v);

// ---- k_pair_tile, the matrix-core row kernel of the generic path (pair_tile.hip) ----
constexpr int PAIR_TILE_MAX_N = 128; // eight column tiles of 16 states
// matrices of a call with Q weight columns: A, then one per column, or the one of the jump form
inline int pair_tile_matrices(int Q) { return 1 + (Q > 0 ? Q : 1); }
// Bop: [A | M_1 | ...] for n states in the operand order of k_pair_tile, padded with zeros to 16 * ceil(n / 16);
// Wpad: [n][n][PAIR_QMAX] (unused where Q == 0)
void pair_tile_operands(const double *A, const double *Wpad, int n, int Q, std::vector<double> &Bop);
// k_pair_tile over b.filt / b.gam with the matrices in b.Bop, rows to o.dev; n <= 128
int pair_tile_rows(bhmm_ctx *c, PairState &b, const PairOut &o);

#define PAIR_PASS_DECL(X, NV)                                                                                     \
    X template int pair_pass<NV, EMIT_GAUSS>(bhmm_ctx *, PairState &, const Model<NV> *, int, const double *,     \
                                             const PairOut &, plan::Verdict *);                                   \
    X template int pair_pass<NV, EMIT_DISC>(bhmm_ctx *, PairState &, const Model<NV> *, int, const double *,      \
                                            const PairOut &, plan::Verdict *);

} // namespace bhmm
