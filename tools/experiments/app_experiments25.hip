// Round 5: the uniform Jacobi kernel with the packed row form (forms/Jacobi5Uniform.hpp: row_at_level, a lane's cells in
// the order c0 c2 c1 c3, v_pk_add_f32 / v_pk_mul_f32) against the same kernel on the per-cell path (row_form = false:
// the code of round 4).  x_ju5_rows / x_ju5_cells; tools/kernel_resources.sh on this file for the steady loops,
// AB_ONLY=x_ju5_rows,x_ju5_cells tools/ab_staged.py uniform for the times.  -> profiles/r05_packed_rows.txt
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
    static constexpr bool row_form = false;
};
} // namespace hip
} // namespace stencil
using V0 = Variant<JU, 0>;
using V1 = Variant<JU, 1>;
STSTHIP_REGISTER_APP("x_ju5_rows", V0, false);
STSTHIP_REGISTER_APP("x_ju5_cells", V1, false);
