// ststhip_grid_relax (include/ststhip.h): red-black relaxation of a grid IN PLACE.  A half-sweep updates the cells of one
// colour of a rectangle with the five-point operator of ststhip_grid_stencil's CROSS5,
// u = w_n * N + w_w * W + w_c * C + w_e * E + w_s * S (+ rhs_coef * rhs); the four neighbours of a cell have the other
// colour, so a half-sweep reads nothing that it writes.  Gauss-Seidel and SOR smoothers without a second grid.
//
// The host-side validation, the walk of a rectangle and the launch limits are those of stencil.hip, repeated here the
// way stencil.hip repeats those of algebra.hip.  Two kernels, templated on the element type and has_rhs, one launch
// (plus at most two for the columns that fill no unit) per half-sweep and entry:
//
//   relax_rows_kernel    where u and rhs are dense within a row (planes).  The scheme of stencil_rows_kernel: a lane
//                        owns a unit of 16, 8 or 4 bytes (the widest that u and rhs allow relative to each other in
//                        every row, so the row distances count), a workgroup walks down a chunk of relax_chunk_rows
//                        rows with the last three rows of u in registers; the neighbours across units come from the
//                        adjacent lanes by DPP wave shifts, the two elements beyond a wave's span by one extra load in
//                        its first and last lane.  It computes the unit's active elements and stores the WHOLE unit:
//                        the inactive elements go back with the bytes just loaded.  Nobody changes an inactive cell
//                        during a half-sweep, and no unit reaches outside the rectangle, so that store changes nothing
//                        but the active cells.  Every value a lane uses besides its own cell is an inactive cell's:
//                        rows held in registers, or read by a neighbouring chunk while this one stores, are never stale.
//   relax_cells_kernel   members of cells and anything else: a lane owns one ACTIVE cell (lane k of a row segment takes
//                        column first_active(row) + 2k, so no lane idles on the other colour) and loads its own
//                        element, its four neighbours and the right-hand side itself.  The walk of stencil_cells_kernel.
//                        It also computes the columns in front of and behind the units of the dense kernel.
//
// No LDS, no atomics, no scratch.  The results are defined operation by operation (ststhip.h): this file is built with
// -ffp-contract=off like the rest of the library, nothing below may be rewritten into a fused multiply-add, and a tap
// with weight zero is multiplied like every other (0 * inf is NaN).
#include "ststhip.h"

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdlib>
#include <string>

namespace ststhip_detail {
int fail(int status, const char *message); // runtime.hip
}

namespace {

using u64 = unsigned long long;
using i64 = long long;

constexpr unsigned relax_threads = 256;
constexpr unsigned relax_wave = 64;
// Rows a workgroup of the dense kernel walks down with three rows of u in registers: 2 / 32 more rows read.
constexpr unsigned relax_chunk_rows = 32;
// Active cells a lane of the general kernel takes: all loaded before the first is stored.
constexpr unsigned relax_lane_cells = 4;
// A row segment of the general kernel, in COLUMNS (even): relax_lane_cells active cells per lane.
constexpr unsigned relax_segment_cells = 8 * relax_threads;
// The general kernel: at most this many workgroups per launch (or one per segment of a row), as the stencil.
constexpr unsigned relax_block_cap = 2048;
// gridDim.y of the dense kernel; a workgroup takes chunks blockIdx.y, + gridDim.y, ...
constexpr unsigned relax_chunk_blocks = 65535;
static_assert(relax_segment_cells == 2 * relax_lane_cells * relax_threads);

// V elements moved as one access.
template <typename T, int V> struct alignas(sizeof(T) * V) Pack {
    T v[V];
};

// u, rhs: the first element of the rectangle (dense kernel: of its row; the units begin `head` elements on).
template <typename T> struct RelaxJob {
    unsigned char *u;
    const unsigned char *rhs;
    u64 u_row_bytes, rhs_row_bytes; // bytes between two rows
    unsigned u_step, rhs_step;      // bytes between two elements of a row
    unsigned n_rows, n_cols;
    // Where the view of u ends, relative to the rectangle: row 0 has no row above it in the view (top_edge), row
    // bottom_at - 1 none below; the same for columns.
    unsigned top_edge, left_edge, bottom_at, right_at;
    // Cell (r, c) of the rectangle is active in this half-sweep where (r + c + phase) is even.
    unsigned phase;
    unsigned head, n_units; // dense kernel: elements in front of the first unit, units per row
    T w[5], rhs_coef, halo; // n, w, c, e, s
};

// CROSS5 of stencil.hip: acc = w_n * N, then acc = acc + w_k * s_k in the order W, C, E, S; every product and every sum
// rounded once.
template <typename T> __device__ inline T apply_cross(const T (&w)[5], T n, T west, T c, T e, T s) {
    T acc = w[0] * n;
    acc = acc + w[1] * west;
    acc = acc + w[2] * c;
    acc = acc + w[3] * e;
    acc = acc + w[4] * s;
    return acc;
}

// ------------------------------------------------------------------ general: one active element per lane
template <typename T, bool RHS> __global__ void __launch_bounds__(relax_threads) relax_cells_kernel(RelaxJob<T> j) {
    const unsigned seg_begin = blockIdx.x * relax_segment_cells; // even, < n_cols
    const unsigned rest = j.n_cols - seg_begin;
    const unsigned len = rest < relax_segment_cells ? rest : relax_segment_cells;
    const int step = int(j.u_step);
    for (unsigned r = blockIdx.y; r < j.n_rows; r += gridDim.y) {
        const unsigned first = (r + j.phase) & 1u; // the row's first active column (seg_begin is even)
        // the rows above and below; one outside the view is never read
        const bool north_ok = !(r == 0 && j.top_edge != 0), south_ok = r + 1 != j.bottom_at;
        unsigned char *mid = j.u + (u64(r) * j.u_row_bytes + u64(seg_begin) * j.u_step);
        const unsigned char *north = north_ok ? mid - j.u_row_bytes : mid, *south = south_ok ? mid + j.u_row_bytes : mid;
        const unsigned char *f = nullptr;
        if constexpr (RHS)
            f = j.rhs + (u64(r) * j.rhs_row_bytes + u64(seg_begin) * j.rhs_step);
        // all of the lane's cells are computed before the first is stored: the loads of one cell need not wait for the
        // store of another, which the compiler cannot tell apart from them
        T out[relax_lane_cells];
#pragma unroll
        for (unsigned k = 0; k < relax_lane_cells; k++) {
            const unsigned c = first + 2u * (threadIdx.x + k * relax_threads);
            out[k] = T();
            if (c < len) {
                const unsigned g = seg_begin + c; // the column within the rectangle
                const bool west_ok = !(g == 0 && j.left_edge != 0), east_ok = g + 1 != j.right_at;
                const int at = int(c * j.u_step); // (c + 1) * step stays below 2^31
                T n = j.halo, w = j.halo, e = j.halo, s = j.halo;
                if (north_ok)
                    n = *reinterpret_cast<const T *>(north + at);
                if (west_ok)
                    w = *reinterpret_cast<const T *>(mid + (at - step));
                const T own = *reinterpret_cast<const T *>(mid + at);
                if (east_ok)
                    e = *reinterpret_cast<const T *>(mid + (at + step));
                if (south_ok)
                    s = *reinterpret_cast<const T *>(south + at);
                T acc = apply_cross<T>(j.w, n, w, own, e, s);
                if constexpr (RHS)
                    acc = acc + j.rhs_coef * *reinterpret_cast<const T *>(f + c * j.rhs_step);
                out[k] = acc;
            }
        }
#pragma unroll
        for (unsigned k = 0; k < relax_lane_cells; k++) {
            const unsigned c = first + 2u * (threadIdx.x + k * relax_threads);
            if (c < len)
                *reinterpret_cast<T *>(mid + c * j.u_step) = out[k];
        }
    }
}

// ------------------------------------------------------------------ dense rows: three rows of u in registers
// Value held by the neighbouring lane, moved with DPP wave shifts over the 32-bit words of T (hip/internal/Sweep.hpp).
template <int DppCtrl, typename T> __device__ inline T lane_shift(T value) {
    constexpr int n_words = int(sizeof(T) / 4);
    struct Words {
        int w[n_words];
    } words;
    __builtin_memcpy(&words, &value, sizeof(T));
#pragma unroll
    for (int i = 0; i < n_words; i++)
        words.w[i] = __builtin_amdgcn_update_dpp(0, words.w[i], DppCtrl, 0xf, 0xf, true);
    T shifted;
    __builtin_memcpy(&shifted, &words, sizeof(T));
    return shifted;
}
template <typename T> __device__ inline T from_west_lane(T v) { return lane_shift<0x138>(v); } // wave_shr:1
template <typename T> __device__ inline T from_east_lane(T v) { return lane_shift<0x130>(v); } // wave_shl:1

// What a lane has requested of one row of u: its unit and, in the first and last lane of a wave's span, the element in
// front of and behind the span.  `edge` is that element of a first or of a last lane -- one load instruction serves both
// ends of the span --, `east` the second one of a lane that is both (a span of one unit).
template <typename T, int V> struct RawRow {
    Pack<T, V> unit;
    T edge, east;
};

template <typename T, int V, bool RHS> __global__ void __launch_bounds__(relax_threads) relax_rows_kernel(RelaxJob<T> j) {
    using P = Pack<T, V>;
    const unsigned unit = blockIdx.x * relax_threads + threadIdx.x;
    if (unit >= j.n_units)
        return; // (a lane behind the last unit: nobody reads its registers, the last unit's lane loads its neighbour)
    const unsigned lane = threadIdx.x % relax_wave;
    const unsigned c0 = j.head + unit * unsigned(V); // the unit's first column within the rectangle
    const bool west_end = lane == 0, east_end = lane == relax_wave - 1 || unit + 1 == j.n_units;
    // the element beyond the span is a cell of the view (false only in a wave at the view's edge)
    const bool west_ok = c0 != 0 || j.left_edge == 0, east_ok = c0 + unsigned(V) != j.right_at;
    const unsigned at = c0 * unsigned(sizeof(T)); // < 2^31
    const bool edge_ok = (west_end || east_end) && (west_end ? west_ok : east_ok);
    const int edge_at = west_end ? -int(sizeof(T)) : int(sizeof(P));
    const bool both_ok = west_end && east_end && east_ok;

    // row: -1 .. n_rows, relative to the rectangle
    auto request = [&](int row) {
        RawRow<T, V> raw;
        raw.edge = raw.east = j.halo;
        const bool row_ok = row < 0 ? j.top_edge == 0 : unsigned(row) != j.bottom_at; // uniform
        if (row_ok) {
            const unsigned char *p = j.u + (i64(row) * i64(j.u_row_bytes) + at);
            raw.unit = *reinterpret_cast<const P *>(p);
            if (edge_ok)
                raw.edge = *reinterpret_cast<const T *>(p + edge_at);
            if (both_ok)
                raw.east = *reinterpret_cast<const T *>(p + sizeof(P));
        } else {
#pragma unroll
            for (int e = 0; e < V; e++)
                raw.unit.v[e] = j.halo;
        }
        return raw;
    };
    auto request_rhs = [&](unsigned row) {
        P own{};
        if constexpr (RHS)
            own = *reinterpret_cast<const P *>(j.rhs + (u64(row) * j.rhs_row_bytes + at));
        return own;
    };

    const unsigned n_chunks = (j.n_rows + relax_chunk_rows - 1) / relax_chunk_rows;
    for (unsigned chunk = blockIdx.y; chunk < n_chunks; chunk += gridDim.y) {
        const unsigned begin = chunk * relax_chunk_rows;
        const unsigned rest = j.n_rows - begin;
        const unsigned end = begin + (rest < relax_chunk_rows ? rest : relax_chunk_rows);
        // The rows begin - 1 and end are the neighbouring chunks' (or lie outside the rectangle): read, never stored.
        P above = request(int(begin) - 1).unit;
        RawRow<T, V> here = request(int(begin));
        // rows begin + 1 and begin + 2, this row's and the next right-hand side: on their way
        RawRow<T, V> coming = request(int(begin) + 1);
        RawRow<T, V> after = begin + 2 <= end ? request(int(begin) + 2) : coming;
        P own = request_rhs(begin);
        P own_next = begin + 1 < end ? request_rhs(begin + 1) : own;
        for (unsigned r = begin; r < end; r++) {
            // the third row from here and the right-hand side after next, before this row's arithmetic
            const RawRow<T, V> later = r + 3 <= end ? request(int(r) + 3) : after;
            const P own_later = r + 2 < end ? request_rhs(r + 2) : own_next;
            // this row with its left and right neighbour: v[0], v[1 .. V], v[V + 1]
            T v[V + 2];
            const T west = from_west_lane(here.unit.v[V - 1]), east = from_east_lane(here.unit.v[0]);
            v[0] = west_end ? here.edge : west;
#pragma unroll
            for (int e = 0; e < V; e++)
                v[1 + e] = here.unit.v[e];
            v[V + 1] = east_end ? (west_end ? here.east : here.edge) : east;
            const unsigned odd = (r + c0 + j.phase) & 1u; // element e is active where e + odd is even
            P out;
#pragma unroll
            for (int e = 0; e < V; e++) {
                T acc = apply_cross<T>(j.w, above.v[e], v[e], v[e + 1], v[e + 2], coming.unit.v[e]);
                if constexpr (RHS)
                    acc = acc + j.rhs_coef * own.v[e];
                out.v[e] = ((unsigned(e) + odd) & 1u) == 0 ? acc : here.unit.v[e];
            }
            *reinterpret_cast<P *>(j.u + (u64(r) * j.u_row_bytes + at)) = out;
            above = here.unit;
            here = coming;
            coming = after;
            after = later;
            own = own_next;
            own_next = own_later;
        }
    }
}

// ------------------------------------------------------------------ host side
static int invalid(const char *what) {
    const std::string msg = std::string("grid relax: ") + what;
    return ststhip_detail::fail(STSTHIP_ERR_INVALID, msg.c_str());
}

static int hip_failed(hipError_t err, const char *what) {
    const std::string msg = std::string(what) + ": " + hipGetErrorString(err);
    return ststhip_detail::fail(STSTHIP_ERR_HIP, msg.c_str());
}

// What does not depend on the rectangle.  0 = fine.
static int check_view(ststhip_grid_view const &v, unsigned elem_size) {
    if (v.stride == 0)
        return invalid("stride 0");
    if (v.pitch < v.width)
        return invalid("pitch < width");
    if (reinterpret_cast<std::uintptr_t>(v.base) % elem_size != 0 || v.stride % elem_size != 0)
        return invalid("a base or stride that is no multiple of the element's size");
    // every byte offset formed, (r * pitch + c) * stride with r < height and c < width <= pitch, fits in 63 bits
    u64 row_bytes = 0, grid_bytes = 0;
    if (__builtin_mul_overflow(u64(v.pitch), u64(v.stride), &row_bytes) ||
        __builtin_mul_overflow(row_bytes, u64(v.height) + 1, &grid_bytes) || v.height + 1 == 0 || grid_bytes >> 63 != 0)
        return invalid("extents, pitch and stride describe more than 2^63 bytes");
    return 0;
}

// The cells first .. first + n - 1 lie inside [0, extent).  n >= 1.
static bool inside(u64 first, u64 n, u64 extent) { return first < extent && n - 1 <= extent - 1 - first; }

// A row of n_cols elements in a view: n_cols * stride bytes, below 2^31.
static bool row_fits(u64 n_cols, u64 stride) {
    u64 bytes = 0;
    return !__builtin_mul_overflow(n_cols, stride, &bytes) && bytes >> 31 == 0;
}

// A rectangle of a view as bytes: its first element and the distance from there to the byte behind its last element.
struct Span {
    std::uintptr_t first;
    u64 bytes;
};
static Span span_of(ststhip_grid_view const &v, u64 row, u64 col, u64 n_rows, u64 n_cols, unsigned elem_size) {
    // (all products are bounded by the view's byte size, which check_view has found to fit)
    return Span{reinterpret_cast<std::uintptr_t>(v.base) + (row * v.pitch + col) * v.stride,
                ((n_rows - 1) * v.pitch + (n_cols - 1)) * v.stride + elem_size};
}
static bool intersect(Span a, Span b) { return a.first < b.first + b.bytes && b.first < a.first + a.bytes; }

// Another member of the same cells, by the regions' rule.
static bool other_member(ststhip_grid_view const &a, Span sa, ststhip_grid_view const &b, Span sb, unsigned elem) {
    const u64 apart = sa.first > sb.first ? sa.first - sb.first : sb.first - sa.first;
    return a.stride == b.stride && a.pitch == b.pitch && apart >= elem && apart + elem <= a.stride;
}

static int resolve_stream(ststhip_stream &stream) {
    if (int rc = ststhip_init(-1))
        return rc;
    if (!stream)
        if (int rc = ststhip_default_stream(&stream))
            return rc;
    return STSTHIP_OK;
}

// One entry, validated.  `empty`: nothing to compute.
static int check_relax(ststhip_grid_relax_desc const &d, bool &empty) {
    if (d.type != STSTHIP_F32 && d.type != STSTHIP_F64)
        return invalid("unknown element type");
    if (d.first_colour > 1)
        return invalid("first_colour is neither 0 nor 1");
    if (d.parity > 1)
        return invalid("parity is neither 0 nor 1");
    if (d.n_half_sweeps < 1 || d.n_half_sweeps > 1024)
        return invalid("need 1..1024 half-sweeps");
    if (d.reserved != 0)
        return invalid("reserved is not 0");
    const bool has_rhs = d.has_rhs != 0;
    for (int k = 0; k < 5; k++)
        if (!std::isfinite(d.weight[k]))
            return invalid("a weight that is not finite");
    if (has_rhs && !std::isfinite(d.rhs_coef))
        return invalid("an rhs_coef that is not finite");
    const unsigned elem = d.type == STSTHIP_F64 ? 8u : 4u;
    if (d.n_rows >> 31 != 0 || d.n_cols >> 31 != 0)
        return invalid("n_rows or n_cols of 2^31 or more");
    if (int rc = check_view(d.u, elem))
        return rc;
    if (has_rhs)
        if (int rc = check_view(d.rhs, elem))
            return rc;
    empty = d.n_rows == 0 || d.n_cols == 0;
    if (empty)
        return 0;
    if (!d.u.base || (has_rhs && !d.rhs.base))
        return invalid("null base with a non-empty rectangle");
    if (!inside(d.u_row, d.n_rows, d.u.height) || !inside(d.u_col, d.n_cols, d.u.width))
        return invalid("the rectangle does not lie inside the view of u");
    if (has_rhs && (!inside(d.rhs_row, d.n_rows, d.rhs.height) || !inside(d.rhs_col, d.n_cols, d.rhs.width)))
        return invalid("the right-hand side's rectangle does not lie inside its view");
    if (!row_fits(d.n_cols, d.u.stride) || (has_rhs && !row_fits(d.n_cols, d.rhs.stride)))
        return invalid("a row of the rectangle spans 2^31 bytes or more");
    if (has_rhs) {
        // what the entry reads or writes of u: the rectangle and its neighbours inside the view
        u64 read_row = d.u_row, read_col = d.u_col, read_rows = d.n_rows, read_cols = d.n_cols;
        if (read_row > 0)
            read_row--, read_rows++;
        if (read_col > 0)
            read_col--, read_cols++;
        if (read_row + read_rows < d.u.height)
            read_rows++;
        if (read_col + read_cols < d.u.width)
            read_cols++;
        const Span f = span_of(d.rhs, d.rhs_row, d.rhs_col, d.n_rows, d.n_cols, elem);
        if (intersect(f, span_of(d.u, read_row, read_col, read_rows, read_cols, elem)) &&
            !other_member(d.u, span_of(d.u, d.u_row, d.u_col, d.n_rows, d.n_cols, elem), d.rhs, f, elem))
            return invalid("the right-hand side overlaps what the relaxation reads or writes (only another member of "
                           "the same cells may share memory with u; u itself is no right-hand side)");
    }
    return 0;
}

// Workgroups of a launch of the general kernel over n_rows rows of n_segments segments.
static dim3 plan_blocks(u64 n_segments, u64 n_rows) {
    const u64 down = std::max<u64>(1, std::min<u64>(n_rows, relax_block_cap / std::max<u64>(1, n_segments)));
    return dim3(unsigned(n_segments), unsigned(down), 1);
}

// The general kernel on the columns first .. first + n_cols - 1 of the rectangle of job `whole`.
template <typename T, bool RHS> static void launch_cells(RelaxJob<T> whole, unsigned first, unsigned n_cols, hipStream_t s) {
    RelaxJob<T> j = whole;
    j.u += u64(first) * j.u_step;
    if (RHS)
        j.rhs += u64(first) * j.rhs_step;
    j.n_cols = n_cols;
    j.left_edge = first == 0 ? whole.left_edge : 0;
    j.right_at = whole.right_at - first; // (right_at >= the whole rectangle's n_cols > first)
    j.phase = (whole.phase + first) & 1u;
    const dim3 grid = plan_blocks((u64(n_cols) + relax_segment_cells - 1) / relax_segment_cells, j.n_rows);
    hipLaunchKernelGGL((relax_cells_kernel<T, RHS>), grid, dim3(relax_threads), 0, s, j);
}

template <typename T, int V, bool RHS> static void launch_rows(RelaxJob<T> const &j, hipStream_t s) {
    const u64 n_chunks = (u64(j.n_rows) + relax_chunk_rows - 1) / relax_chunk_rows;
    const dim3 grid(unsigned((u64(j.n_units) + relax_threads - 1) / relax_threads),
                    unsigned(std::min<u64>(n_chunks, relax_chunk_blocks)), 1);
    hipLaunchKernelGGL((relax_rows_kernel<T, V, RHS>), grid, dim3(relax_threads), 0, s, j);
}

// STSTHIP_RELAX_GENERAL (any value): planes take the general kernel too -- the A/B partner of the dense kernel
// (tools/bench_grid_relax.py) and a second implementation for the tests.  Read at every call.
static bool general_only() { return std::getenv("STSTHIP_RELAX_GENERAL") != nullptr; }

// One half-sweep of one entry: the cells of the rectangle where (r + c + j.phase) is even.
template <typename T, bool RHS> static void launch_half_sweep(RelaxJob<T> j, bool dense, unsigned unit_bytes, hipStream_t s) {
    if (!dense) {
        launch_cells<T, RHS>(j, 0, j.n_cols, s);
        return;
    }
    const unsigned per_unit = unit_bytes / unsigned(sizeof(T));
    const unsigned tail_begin = j.head + j.n_units * per_unit;
    if (j.n_units > 0) {
        if (per_unit == 1)
            launch_rows<T, 1, RHS>(j, s);
        else if (per_unit == 2)
            launch_rows<T, 2, RHS>(j, s);
        else if constexpr (sizeof(T) == 4)
            launch_rows<T, 4, RHS>(j, s);
    }
    // the columns that fill no unit: fewer than a unit's on either side
    if (j.head > 0)
        launch_cells<T, RHS>(j, 0, j.head, s);
    if (tail_begin < j.n_cols)
        launch_cells<T, RHS>(j, tail_begin, j.n_cols - tail_begin, s);
}

template <typename T, bool RHS> static hipError_t launch_relax(ststhip_grid_relax_desc const &d, hipStream_t s) {
    RelaxJob<T> j{};
    j.u = reinterpret_cast<unsigned char *>(span_of(d.u, d.u_row, d.u_col, 1, 1, sizeof(T)).first);
    j.u_row_bytes = d.u.pitch * d.u.stride;
    // (a single column is dense; its neighbours are one stride away all the same)
    j.u_step = unsigned(d.u.stride);
    if (RHS) {
        j.rhs = reinterpret_cast<const unsigned char *>(span_of(d.rhs, d.rhs_row, d.rhs_col, 1, 1, sizeof(T)).first);
        j.rhs_row_bytes = d.rhs.pitch * d.rhs.stride;
        j.rhs_step = unsigned(d.rhs.stride);
    }
    j.n_rows = unsigned(d.n_rows);
    j.n_cols = unsigned(d.n_cols);
    j.top_edge = d.u_row == 0;
    j.left_edge = d.u_col == 0;
    j.bottom_at = unsigned(std::min<u64>(d.u.height - d.u_row, 0xffffffffu)); // (n_rows < 2^31 never gets there)
    j.right_at = unsigned(std::min<u64>(d.u.width - d.u_col, 0xffffffffu));
    for (int k = 0; k < 5; k++)
        j.w[k] = T(d.weight[k]); // double to the element's type, once
    j.rhs_coef = T(d.rhs_coef);
    j.halo = T(d.halo);

    const bool dense = j.u_step == sizeof(T) && (!RHS || j.rhs_step == sizeof(T)) && !general_only();
    unsigned unit_bytes = unsigned(sizeof(T));
    if (dense) {
        // the widest unit both sides allow in every row: the lowest set bit of their distance and of the row distances
        // (u's wherever the view has a second row: the rows above and below the rectangle are read as units too); 16
        // at the most, sizeof(T) at the least
        const auto low = [](const void *p) { return unsigned(reinterpret_cast<std::uintptr_t>(p)); };
        unsigned apart = 16u;
        if (RHS)
            apart |= low(j.u) - low(j.rhs);
        if (d.u.height > 1)
            apart |= unsigned(j.u_row_bytes);
        if (RHS && j.n_rows > 1)
            apart |= unsigned(j.rhs_row_bytes);
        unit_bytes = apart & (0u - apart);
        const unsigned per_unit = unit_bytes / unsigned(sizeof(T));
        j.head = std::min(((0u - low(j.u)) & (unit_bytes - 1u)) / unsigned(sizeof(T)), j.n_cols);
        j.n_units = (j.n_cols - j.head) / per_unit;
    }
    // the colour of the rectangle's cell (0, 0) in the view's coordinates
    const unsigned corner = unsigned((d.u_row + d.u_col + d.parity) & 1u);
    for (unsigned k = 0; k < d.n_half_sweeps; k++) {
        // cell (r, c) is active where (r + c + corner) & 1 == (first_colour + k) & 1
        j.phase = (corner + d.first_colour + k) & 1u;
        launch_half_sweep<T, RHS>(j, dense, unit_bytes, s);
        if (const hipError_t err = hipGetLastError(); err != hipSuccess)
            return err;
    }
    return hipSuccess;
}

template <typename T> static hipError_t launch_relax(ststhip_grid_relax_desc const &d, hipStream_t s) {
    return d.has_rhs != 0 ? launch_relax<T, true>(d, s) : launch_relax<T, false>(d, s);
}

} // namespace

extern "C" {

int ststhip_grid_relax(int n, const ststhip_grid_relax_desc *relaxations, ststhip_stream stream) {
    if (n < 1 || n > 8)
        return invalid("need 1..8 entries");
    if (!relaxations)
        return invalid("null argument");
    bool empty[8], any = false;
    for (int i = 0; i < n; i++) {
        if (int rc = check_relax(relaxations[i], empty[i]))
            return rc;
        any = any || !empty[i];
    }
    if (!any)
        return STSTHIP_OK;
    if (int rc = resolve_stream(stream))
        return rc;
    for (int i = 0; i < n; i++) {
        if (empty[i])
            continue;
        hipStream_t s = static_cast<hipStream_t>(stream);
        const hipError_t err = relaxations[i].type == STSTHIP_F64 ? launch_relax<double>(relaxations[i], s)
                                                                  : launch_relax<float>(relaxations[i], s);
        if (err != hipSuccess)
            return hip_failed(err, "ststhip_grid_relax");
    }
    return STSTHIP_OK;
}

} // extern "C"
