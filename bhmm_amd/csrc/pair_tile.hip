// pair_tile.hip -- k_pair_tile (pair_tile_kernels.hpp): its sixteen instantiations (1 .. 8 column tiles, double /
// float), the matrices [A | M_1 | ...] in the kernel's operand order, and the launch over the rows that the generic
// path of bhmm_posterior_transitions (pair_api.hip) has left in c->pair.filt / gam.  DESIGN.md section 21.
#include <algorithm>

#include "pair_launch.hpp"
#include "pair_tile_kernels.hpp"

namespace bhmm {
namespace {

template <int NT, typename OT>
int rows_as(bhmm_ctx *c, const PairOut &o, int nm)
{
    const int64_t tiles = (c->total + 15) / 16; // one per wavefront
    const dim3 grid((unsigned)((tiles + PAIR_TILE_WAVES - 1) / PAIR_TILE_WAVES)), block(64 * PAIR_TILE_WAVES);
    const auto &b = c->pair;
    BHMM_HIP(launch(k_pair_tile<NT, OT>, grid, block, 0, c->stream, b.filt.p, b.gam.p, b.Bop.p, nm, c->n, c->total,
                    c->K, c->d_offsets.p, static_cast<OT *>(o.dev)));
    return BHMM_OK;
}

template <int NT>
int rows_nt(bhmm_ctx *c, const PairOut &o, int nm)
{
    return o.f32 ? rows_as<NT, float>(c, o, nm) : rows_as<NT, double>(c, o, nm);
}

} // namespace

void pair_tile_operands(const double *A, const double *Wpad, int n, int Q, std::vector<double> &Bop)
{
    const int NT = (n + 15) / 16, KK = 4 * NT, nm = pair_tile_matrices(Q);
    Bop.assign((size_t)nm * NT * KK * 64, 0.0);
    for (int m = 0; m < nm; ++m)
        for (int i = 0; i < n; ++i)
            for (int j = 0; j < n; ++j) {
                const double a = A[(size_t)i * n + j];
                double v = a; // m == 0: A itself
                if (m > 0)
                    v = Q == 0 ? (i == j ? 0.0 : a) : a * Wpad[((size_t)i * n + j) * PAIR_QMAX + (m - 1)];
                // element (k = i, column j): fragment kk = i / 4 of column tile j / 16, lane 16 (i % 4) + j % 16
                Bop[(((size_t)m * NT + j / 16) * KK + i / 4) * 64 + 16 * (i % 4) + j % 16] = v;
            }
}

int pair_tile_rows(bhmm_ctx *c, const PairOut &o)
{
    const int nm = pair_tile_matrices(o.Q);
    switch ((c->n + 15) / 16) {
    case 1: return rows_nt<1>(c, o, nm);
    case 2: return rows_nt<2>(c, o, nm);
    case 3: return rows_nt<3>(c, o, nm);
    case 4: return rows_nt<4>(c, o, nm);
    case 5: return rows_nt<5>(c, o, nm);
    case 6: return rows_nt<6>(c, o, nm);
    case 7: return rows_nt<7>(c, o, nm);
    case 8: return rows_nt<8>(c, o, nm);
    }
    return invalid_arg("pair_tile_rows: more than 128 states");
}

} // namespace bhmm
