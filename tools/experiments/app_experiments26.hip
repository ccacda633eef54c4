// Round 6: the uniform Jacobi kernel with the row form in edge waves too (Sweep.hpp: row form, edge waves; units whose
// columns all lie inside the grid test rows only, and nothing in the batches that lie inside the grid with all their
// rows) against the same kernel with the per-cell path in edge waves (row_form_edges = false: the code of round 5).
// x_ju6_edges / x_ju6_cells; tools/kernel_resources.sh on this file for the steady loops,
// AB_ONLY=x_ju6_edges,x_ju6_cells tools/ab_staged.py uniform for the times.  -> profiles/r06_edge_rows.txt
#include "app_registry.hpp"
#include "apps/jacobi.hpp"

using namespace stencil::apps;
template <typename B, int V> struct Variant : public B {
    using Block = typename B::Block;
    Variant() = default;
    Variant(B const &f) : B(f) {}
    static Variant from_params(Block const &b) { return Variant(B::from_params(b)); }
};
using JU = Jacobi5Uniform<false, false>;
namespace stencil {
namespace hip {
template <typename B, bool SOA> struct SweepTuning<Variant<B, 0>, SOA> : SweepTuning<B, SOA> {
    static constexpr bool narrow_form = false;
};
template <typename B, bool SOA> struct SweepTuning<Variant<B, 1>, SOA> : SweepTuning<B, SOA> {
    static constexpr bool narrow_form = false;
    static constexpr bool row_form_edges = false;
};
} // namespace hip
} // namespace stencil
using V0 = Variant<JU, 0>;
using V1 = Variant<JU, 1>;
STSTHIP_REGISTER_APP("x_ju6_edges", V0, false);
STSTHIP_REGISTER_APP("x_ju6_cells", V1, false);
