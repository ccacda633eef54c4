// Declared linear five-point functors: the trait a transition function's author specialises, and the device-side
// probe that checks the declaration before stencil::hip::StencilUpdate routes the function to a faster, bit-identical
// form of its sweep (forms/Jacobi5Uniform.hpp: 5 instead of 9 floating-point operations per cell), whose kernels
// libststhip.so holds precompiled -- without contraction, whatever the application's own build does.
//
// Declared and verified, never guessed.  Sampling cannot prove that a function is linear -- a clamp where no sample
// falls would go unnoticed -- so nothing is rerouted on the strength of samples alone: the author asserts the form by
// specialising LinearCross5<F>, and the probe only catches a declaration that does not hold in THIS build of F (a
// different expression, other coefficients, or the same source contracted into fused multiply-adds).
//
// The probe compares F with the declared expression inside F's own translation unit, so what that build does to both
// alike it cannot see that way: a build that flushes fp32 subnormals to zero (-fgpu-flush-denormals-to-zero: its
// kernels run with the flushing denormal mode) flushes F and the declared expression alike, while the library's
// kernels keep subnormals.  The table's last entry is therefore a sentinel whose results the host knows: a product of
// two normal numbers that is exactly a subnormal, and a subnormal plus +0.  A build that returns zero for either is
// not routed.
#pragma once
#include "../Stencil.hpp"
#include "internal/Runtime.hpp"

#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <type_traits>
#include <vector>

namespace stencil {
namespace hip {

// The declaration.  The primary template is empty: a function declares nothing.  A specialisation provides
//     static void coefficients(F const &f, float (&c)[5]);        // order: N, W, S, E, C
// and thereby asserts that F::operator()(s) is, for EVERY stencil s, exactly
//     c[0]*s[-1][0] + c[1]*s[0][-1] + c[2]*s[1][0] + c[3]*s[0][1] + c[4]*s[0][0]
// evaluated from left to right in float, every operation rounded on its own, and that it reads nothing else of the
// stencil (no id, iteration, grid_range).  `coefficients` may be a member template where F is only forward-declared
// at the point of the specialisation (examples/reference_linear_forms.hpp).
template <typename F> struct LinearCross5 {};

// Which form of the sweep a call of StencilUpdate ran.
enum class SweepForm { general, jacobi5_uniform };

inline const char *to_string(SweepForm form) { return form == SweepForm::jacobi5_uniform ? "jacobi5_uniform" : "general"; }

namespace internal {

template <typename F>
concept DeclaresLinearCross5 = requires(F const &f, float (&c)[5]) { LinearCross5<F>::coefficients(f, c); };

// STSTHIP_LINEAR_FORM (0: never route, everything else: route where allowed) and STSTHIP_TRACE_FORM (set and not 0:
// one line per call on stderr), read once per process.  They live here and not in ststhip_options: the route is a
// matter of the template layer, the C ABI knows nothing of it.
struct FormKnobs {
    bool route, trace;
};
inline FormKnobs const &form_knobs() {
    static const FormKnobs knobs = [] {
        const char *route = std::getenv("STSTHIP_LINEAR_FORM");
        const char *trace = std::getenv("STSTHIP_TRACE_FORM");
        return FormKnobs{!(route && std::strcmp(route, "0") == 0), trace && *trace && std::strcmp(trace, "0") != 0};
    }();
    return knobs;
}

inline void trace_form(SweepForm form, const char *why_general) {
    if (!form_knobs().trace)
        return;
    if (form == SweepForm::general)
        std::fprintf(stderr, "[ststhip] sweep form: general (%s)\n", why_general ? why_general : "no reason recorded");
    else
        std::fprintf(stderr, "[ststhip] sweep form: %s\n", to_string(form));
}

// One stencil of the probe's table: the five cells a cross reads (the corners are filled with values a linear cross
// must ignore), the centre's position, the grid's extent and the generation.
struct LinearFormSample {
    float n, w, s, e, c;
    float corner[4];
    std::uint32_t row, col, rows, cols;
    std::uint64_t iteration;
};
// What the device made of one sample, as bits.
struct LinearFormResult {
    std::uint32_t function;   // F::operator()
    std::uint32_t declared;   // the declared expression, every operation rounded on its own
};
struct LinearFormCoefficients {
    float c[5];
};

constexpr int linear_form_random_samples = 4096;
constexpr int linear_form_samples = 1 + 5 + linear_form_random_samples + 1; // the last one is the sentinel
constexpr std::uint64_t linear_form_seed = 0x5715C11A5EEDull;

// The fixed table: the zero stencil, the five unit impulses (N, W, S, E, C), then seeded random stencils of both
// signs and magnitudes from 2^-20 to 2^20 at varying positions and generations; last the subnormal sentinel:
// n * w = 2^-100 * 2^-30 is exactly the subnormal 2^-130, s + e = 2^-140 + 0 is s.
inline std::vector<LinearFormSample> const &linear_form_table() {
    static const std::vector<LinearFormSample> table = [] {
        std::vector<LinearFormSample> t(linear_form_samples);
        std::uint64_t state = linear_form_seed;
        auto next = [&state] { // splitmix64
            std::uint64_t z = (state += 0x9E3779B97F4A7C15ull);
            z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
            z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
            return z ^ (z >> 31);
        };
        auto value = [&next] {
            const std::uint64_t r = next();
            const std::uint32_t exponent = 127u - 20u + std::uint32_t((r >> 32) % 40u); // 2^-20 .. 2^19 times [1, 2)
            const std::uint32_t bits = (std::uint32_t(r >> 63) << 31) | (exponent << 23) | (std::uint32_t(r) & 0x7FFFFFu);
            float v;
            std::memcpy(&v, &bits, sizeof v);
            return v;
        };
        for (int i = 0; i < linear_form_samples; i++) {
            LinearFormSample &s = t[i];
            s = LinearFormSample{};
            s.rows = s.cols = 8;
            s.row = s.col = 3;
            if (i >= 1 && i <= 5) {
                float *cell[5] = {&s.n, &s.w, &s.s, &s.e, &s.c};
                *cell[i - 1] = 1.0f;
            } else if (i == linear_form_samples - 1) {
                s.n = 0x1p-100f, s.w = 0x1p-30f, s.s = 0x1p-140f, s.e = 0.0f;
            } else if (i > 5) {
                s.n = value(), s.w = value(), s.s = value(), s.e = value(), s.c = value();
                for (float &corner : s.corner)
                    corner = value();
                s.rows = 1u + std::uint32_t(next() % (1u << 20));
                s.cols = 1u + std::uint32_t(next() % (1u << 20));
                s.row = std::uint32_t(next() % s.rows);
                s.col = std::uint32_t(next() % s.cols);
                s.iteration = next() % (1ull << 40);
            }
        }
        return t;
    }();
    return table;
}

// A value the compiler has to have in a register as it is: a product that went through here cannot become part of a
// fused multiply-add, whatever -ffp-contract says (=fast disregards `#pragma clang fp contract(off)`).
STST_DEVICE inline float rounded_here(float v) {
#if defined(__HIP_DEVICE_COMPILE__)
    asm volatile("" : "+v"(v));
#endif
    return v;
}

STST_DEVICE inline std::uint32_t bits_of(float v) { return __builtin_bit_cast(std::uint32_t, v); }

// Evaluates F on the table, and beside each value the declared expression with every product and sum rounded on its
// own.
template <typename F>
__global__ void linear_form_probe_kernel(const F f, const LinearFormCoefficients coef, const LinearFormSample *samples,
                                         int n_samples, LinearFormResult *results) {
#pragma clang fp contract(off)
    const int i = int(blockIdx.x * blockDim.x + threadIdx.x);
    if (i >= n_samples)
        return;
    const LinearFormSample s = samples[i];
    if (i == n_samples - 1) { // the sentinel: the operands come from memory, so this build's kernels do the arithmetic
        results[i] = LinearFormResult{bits_of(rounded_here(s.n * s.w)), bits_of(rounded_here(s.s + s.e))};
        return;
    }
    using StencilImpl = Stencil<float, 1, typename F::TimeDependentValue>;
    StencilImpl st(sycl::id<2>(s.row, s.col), sycl::range<2>(s.rows, s.cols), std::size_t(s.iteration), 0,
                   typename F::TimeDependentValue{});
    st[sycl::id<2>(0, 0)] = s.corner[0], st[sycl::id<2>(0, 1)] = s.n, st[sycl::id<2>(0, 2)] = s.corner[1];
    st[sycl::id<2>(1, 0)] = s.w, st[sycl::id<2>(1, 1)] = s.c, st[sycl::id<2>(1, 2)] = s.e;
    st[sycl::id<2>(2, 0)] = s.corner[2], st[sycl::id<2>(2, 1)] = s.s, st[sycl::id<2>(2, 2)] = s.corner[3];
    LinearFormResult r;
    r.function = bits_of(f(st));
    auto cross = [&](float c0, float c1, float c2, float c3, float c4) {
        float sum = rounded_here(c0 * s.n);
        sum = rounded_here(sum + rounded_here(c1 * s.w));
        sum = rounded_here(sum + rounded_here(c2 * s.s));
        sum = rounded_here(sum + rounded_here(c3 * s.e));
        return rounded_here(sum + rounded_here(c4 * s.c));
    };
    r.declared = bits_of(cross(coef.c[0], coef.c[1], coef.c[2], coef.c[3], coef.c[4]));
    results[i] = r;
}

// What the probe found for one (transition function, build).
struct LinearFormVerdict {
    bool verified = false; // F is the declared expression on every sample, the impulses return the coefficients, and
                           // this build keeps fp32 subnormals as the library's kernels do
    float coef[5] = {};
    const char *reason = "the linear form has not been probed"; // why not verified
};

// Runs the probe on the current device and waits for it.  Anything that keeps it from running means "general".
template <typename F> LinearFormVerdict probe_linear_form(F const &f) {
    LinearFormVerdict verdict;
    LinearFormCoefficients coef;
    LinearCross5<F>::coefficients(f, coef.c);
    std::memcpy(verdict.coef, coef.c, sizeof verdict.coef);
    void *samples = nullptr, *results = nullptr;
    std::vector<LinearFormResult> host(linear_form_samples);
    bool ran = false;
    try {
        ststhip_stream stream = default_stream();
        std::vector<LinearFormSample> const &table = linear_form_table();
        samples = device_alloc(table.size() * sizeof(LinearFormSample));
        results = device_alloc(host.size() * sizeof(LinearFormResult));
        check(ststhip_memcpy_h2d(samples, table.data(), table.size() * sizeof(LinearFormSample), stream), "probe upload");
        check(ststhip_memset(results, 0, host.size() * sizeof(LinearFormResult), stream), "probe memset");
        const LinearFormSample *table_on_device = static_cast<const LinearFormSample *>(samples);
        LinearFormResult *results_on_device = static_cast<LinearFormResult *>(results);
        int n_samples = linear_form_samples;
        void *kernel_args[] = {const_cast<F *>(&f), &coef, &table_on_device, &n_samples, &results_on_device};
        check(ststhip_launch(reinterpret_cast<const void *>(&linear_form_probe_kernel<F>),
                             unsigned((linear_form_samples + 255) / 256), 1, 1, 256, 1, 1, kernel_args, 0, stream),
              "linear form probe");
        check(ststhip_memcpy_d2h(host.data(), results, host.size() * sizeof(LinearFormResult), stream), "probe download");
        check(ststhip_stream_synchronize(stream), "probe synchronize");
        ran = true;
    } catch (...) {
    }
    if (samples)
        ststhip_free(samples);
    if (results)
        ststhip_free(results);
    if (!ran) {
        verdict.reason = "the linear form probe could not run";
        return verdict;
    }
    LinearFormResult const &sentinel = host[linear_form_samples - 1];
    const bool keeps_subnormals = sentinel.function == 0x00080000u /* 2^-130 */ && sentinel.declared == 0x00000200u /* 2^-140 */;
    bool same = true;
    for (int i = 0; i < linear_form_samples - 1; i++)
        same = same && host[i].function == host[i].declared;
    bool impulses = true;
    for (int k = 0; k < 5; k++) {
        std::uint32_t declared;
        std::memcpy(&declared, &coef.c[k], sizeof declared);
        impulses = impulses && host[1 + k].function == declared;
    }
    verdict.verified = keeps_subnormals && same && impulses;
    if (!keeps_subnormals)
        verdict.reason = "this build flushes fp32 subnormals";
    else if (!same)
        verdict.reason = "the probe found the function to differ from its declared linear form in this build";
    else if (!impulses)
        verdict.reason = "the function's unit impulses do not return the declared coefficients";
    else
        verdict.reason = nullptr;
    return verdict;
}

// Five bit-equal, positive, finite coefficients?
inline bool uniform_positive(const float (&c)[5]) {
    for (int k = 1; k < 5; k++)
        if (std::memcmp(&c[k], &c[0], sizeof(float)) != 0)
            return false;
    return c[0] > 0.0f && std::isfinite(c[0]);
}

// The verdict StencilUpdate keeps, with the bytes of transition_function and halo_value it was taken for.
template <typename F> struct LinearFormCache {
    LinearFormVerdict verdict;
    bool valid = false;
    unsigned char function_bytes[sizeof(F)];
    unsigned char halo_bytes[sizeof(typename F::Cell)];

    bool holds(F const &f, typename F::Cell const &halo) const {
        return valid && std::memcmp(function_bytes, &f, sizeof(F)) == 0 &&
               std::memcmp(halo_bytes, &halo, sizeof halo_bytes) == 0;
    }
    void take(F const &f, typename F::Cell const &halo) {
        verdict = probe_linear_form(f);
        std::memcpy(function_bytes, &f, sizeof(F));
        std::memcpy(halo_bytes, &halo, sizeof halo_bytes);
        valid = true;
    }
};
struct NoLinearFormCache {};

} // namespace internal
} // namespace hip
} // namespace stencil
