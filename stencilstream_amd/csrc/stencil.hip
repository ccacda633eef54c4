// ststhip_grid_stencil (include/ststhip.h): a 3 x 3 (BOX9) or five-point (CROSS5) linear operator applied to a grid
// once, with an optional right-hand side: dst = sum_k w_k * src(i + a_k, j + b_k) (+ rhs_coef * rhs).  A residual
// r = f - A u, a relaxation with a source term.
//
// The host-side validation, the walk of a rectangle and the launch limits are those of algebra.hip, repeated here the
// way algebra.hip repeats those of regions.hip.  Two kernels, templated on the element type, the shape and has_rhs:
//
//   stencil_rows_kernel    BOX9 where every side is dense within a row (planes); a CROSS5 was not faster than the
//                          general kernel there (profiles/grid_stencil.txt) and has no instantiation.  The sweep's
//                          idea for one generation: a wave owns a run of 64 units of consecutive columns, a lane one
//                          unit (16 bytes down to one element: the
//                          widest that dst, src and rhs allow relative to each other for ALL rows of the rectangle, so
//                          the row distances count too), and walks down a chunk of stencil_chunk_rows rows with the last
//                          three source rows of its columns in registers.  A source element is loaded once per chunk
//                          (plus two warm-up rows), the left and right neighbours of a lane's unit come from the
//                          adjacent lanes by DPP wave shifts, the two elements beyond the wave's span by one extra load
//                          in its first and last lane (one instruction for both).  Rows outside the view become the
//                          halo once per row (uniform over the workgroup), columns only in the lanes at the view's
//                          edge.  Two source rows and two right-hand sides are on their way during a row's arithmetic.
//   stencil_cells_kernel   members of cells and anything else: one element per lane, its five or nine neighbours
//                          loaded by the lane itself; the caches carry the reuse.  The walk of combine_strided_kernel.
//                          It also computes the columns in front of and behind the units of the dense kernel.
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

constexpr unsigned stencil_threads = 256;
constexpr unsigned stencil_wave = 64;
// Rows a workgroup of the dense kernel walks down with three source rows in registers: 2 / 32 more rows read.
constexpr unsigned stencil_chunk_rows = 32;
// A row segment of the general kernel: four elements per lane.
constexpr unsigned stencil_segment_cells = 4 * stencil_threads;
// The general kernel: at most this many workgroups per launch (or one per segment of a row), as the algebra.
constexpr unsigned stencil_block_cap = 2048;
// gridDim.y of the dense kernel; a workgroup takes chunks blockIdx.y, + gridDim.y, ...
constexpr unsigned stencil_chunk_blocks = 65535;

// V elements moved as one access.
template <typename T, int V> struct alignas(sizeof(T) * V) Pack {
    T v[V];
};

// dst, src, rhs: the first element of the rectangle (dense kernel: of its row; the units begin `head` elements on).
template <typename T> struct StencilJob {
    unsigned char *dst;
    const unsigned char *src, *rhs;
    u64 dst_row_bytes, src_row_bytes, rhs_row_bytes; // bytes between two rows
    unsigned dst_step, src_step, rhs_step;           // bytes between two elements of a row
    unsigned n_rows, n_cols;
    // Where the source view ends, relative to the rectangle: row 0 has no row above it in the view (top_edge), row
    // bottom_at - 1 none below; the same for columns.
    unsigned top_edge, left_edge, bottom_at, right_at;
    unsigned head, n_units; // dense kernel: elements in front of the first unit, units per row
    T w[9], rhs_coef, halo;
};

// The taps in row-major order: acc = w_first * s_first, then acc = acc + w_k * s_k; every product and every sum rounded
// once.  s[3 * (a + 1) + (b + 1)] is the neighbour (a, b); CROSS5 neither reads nor multiplies the corners.
template <typename T, unsigned SHAPE> __device__ inline T apply_taps(const T (&w)[9], const T (&s)[9]) {
    if constexpr (SHAPE == STSTHIP_STENCIL_BOX9) {
        T acc = w[0] * s[0];
#pragma unroll
        for (int k = 1; k < 9; k++)
            acc = acc + w[k] * s[k];
        return acc;
    } else {
        T acc = w[1] * s[1];
        acc = acc + w[3] * s[3];
        acc = acc + w[4] * s[4];
        acc = acc + w[5] * s[5];
        acc = acc + w[7] * s[7];
        return acc;
    }
}

// ------------------------------------------------------------------ general: one element per lane
template <typename T, unsigned SHAPE, bool RHS>
__global__ void __launch_bounds__(stencil_threads) stencil_cells_kernel(StencilJob<T> j) {
    const unsigned seg_begin = blockIdx.x * stencil_segment_cells; // < n_cols
    const unsigned rest = j.n_cols - seg_begin;
    const unsigned len = rest < stencil_segment_cells ? rest : stencil_segment_cells;
    for (unsigned r = blockIdx.y; r < j.n_rows; r += gridDim.y) {
        // the three source rows; one outside the view is never read
        const bool row_ok[3] = {!(r == 0 && j.top_edge != 0), true, r + 1 != j.bottom_at};
        const unsigned char *mid = j.src + (u64(r) * j.src_row_bytes + u64(seg_begin) * j.src_step);
        const unsigned char *row[3] = {row_ok[0] ? mid - j.src_row_bytes : mid, mid, row_ok[2] ? mid + j.src_row_bytes : mid};
        unsigned char *d = j.dst + (u64(r) * j.dst_row_bytes + u64(seg_begin) * j.dst_step);
        const unsigned char *f = nullptr;
        if constexpr (RHS)
            f = j.rhs + (u64(r) * j.rhs_row_bytes + u64(seg_begin) * j.rhs_step);
        for (unsigned c = threadIdx.x; c < len; c += stencil_threads) {
            const unsigned g = seg_begin + c; // the column within the rectangle
            const bool col_ok[3] = {!(g == 0 && j.left_edge != 0), true, g + 1 != j.right_at};
            const int at = int(c * j.src_step), step = int(j.src_step); // (c + 1) * step stays below 2^31
            T s[9];
#pragma unroll
            for (int p = 0; p < 3; p++) {
#pragma unroll
                for (int q = 0; q < 3; q++) {
                    if (SHAPE == STSTHIP_STENCIL_CROSS5 && p != 1 && q != 1)
                        continue;
                    s[3 * p + q] = j.halo;
                    if (row_ok[p] && col_ok[q])
                        s[3 * p + q] = *reinterpret_cast<const T *>(row[p] + (at + (q - 1) * step));
                }
            }
            T own = T();
            if constexpr (RHS)
                own = *reinterpret_cast<const T *>(f + c * j.rhs_step);
            T acc = apply_taps<T, SHAPE>(j.w, s);
            if constexpr (RHS)
                acc = acc + j.rhs_coef * own;
            *reinterpret_cast<T *>(d + c * j.dst_step) = acc;
        }
    }
}

// ------------------------------------------------------------------ dense rows: three source rows in registers
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

// What a lane has requested of one source row: its unit and, in the first and last lane of a wave's span, the element
// in front of and behind the span.
// `edge` is that element of a first or of a last lane -- one load instruction serves both ends of the span --, `east`
// the second one of a lane that is both (a span of one unit).
template <typename T, int V> struct RawRow {
    Pack<T, V> unit;
    T edge, east;
};
// A lane's unit with its left and right neighbour: v[0], v[1 .. V], v[V + 1].
template <typename T, int V> struct Row {
    T v[V + 2];
};

template <typename T, int V, unsigned SHAPE, bool RHS>
__global__ void __launch_bounds__(stencil_threads) stencil_rows_kernel(StencilJob<T> j) {
    using P = Pack<T, V>;
    const unsigned unit = blockIdx.x * stencil_threads + threadIdx.x;
    if (unit >= j.n_units)
        return; // (a lane behind the last unit: nobody reads its registers, the last unit's lane loads its neighbour)
    const unsigned lane = threadIdx.x % stencil_wave;
    const unsigned c0 = j.head + unit * unsigned(V); // the unit's first column within the rectangle
    const bool west_end = lane == 0, east_end = lane == stencil_wave - 1 || unit + 1 == j.n_units;
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
            const unsigned char *p = j.src + (i64(row) * i64(j.src_row_bytes) + at);
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
    auto finish = [&](RawRow<T, V> const &raw) {
        Row<T, V> row;
        const T west = from_west_lane(raw.unit.v[V - 1]), east = from_east_lane(raw.unit.v[0]);
        row.v[0] = west_end ? raw.edge : west;
#pragma unroll
        for (int e = 0; e < V; e++)
            row.v[1 + e] = raw.unit.v[e];
        row.v[V + 1] = east_end ? (west_end ? raw.east : raw.edge) : east;
        return row;
    };
    auto request_rhs = [&](unsigned row) {
        P own{};
        if constexpr (RHS)
            own = *reinterpret_cast<const P *>(j.rhs + (u64(row) * j.rhs_row_bytes + at));
        return own;
    };

    const unsigned n_chunks = (j.n_rows + stencil_chunk_rows - 1) / stencil_chunk_rows;
    for (unsigned chunk = blockIdx.y; chunk < n_chunks; chunk += gridDim.y) {
        const unsigned begin = chunk * stencil_chunk_rows;
        const unsigned rest = j.n_rows - begin;
        const unsigned end = begin + (rest < stencil_chunk_rows ? rest : stencil_chunk_rows);
        Row<T, V> above = finish(request(int(begin) - 1));
        Row<T, V> here = finish(request(int(begin)));
        // rows begin + 1 and begin + 2, this row's and the next right-hand side: on their way
        RawRow<T, V> coming = request(int(begin) + 1);
        RawRow<T, V> after = begin + 2 <= end ? request(int(begin) + 2) : coming;
        P own = request_rhs(begin);
        P own_next = begin + 1 < end ? request_rhs(begin + 1) : own;
        for (unsigned r = begin; r < end; r++) {
            // the third row from here and the right-hand side after next, before this row's arithmetic
            const RawRow<T, V> later = r + 3 <= end ? request(int(r) + 3) : after;
            const P own_later = r + 2 < end ? request_rhs(r + 2) : own_next;
            const Row<T, V> below = finish(coming);
            P out;
#pragma unroll
            for (int e = 0; e < V; e++) {
                const T s[9] = {above.v[e], above.v[e + 1], above.v[e + 2], here.v[e],  here.v[e + 1],
                                here.v[e + 2], below.v[e],    below.v[e + 1], below.v[e + 2]};
                T acc = apply_taps<T, SHAPE>(j.w, s);
                if constexpr (RHS)
                    acc = acc + j.rhs_coef * own.v[e];
                out.v[e] = acc;
            }
            *reinterpret_cast<P *>(j.dst + (u64(r) * j.dst_row_bytes + at)) = out;
            above = here;
            here = below;
            coming = after;
            after = later;
            own = own_next;
            own_next = own_later;
        }
    }
}

// ------------------------------------------------------------------ host side
static int invalid(const char *what) {
    const std::string msg = std::string("grid stencil: ") + what;
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
static int check_stencil(ststhip_grid_stencil_desc const &d, bool &empty) {
    if (d.type != STSTHIP_F32 && d.type != STSTHIP_F64)
        return invalid("unknown element type");
    if (d.shape != STSTHIP_STENCIL_CROSS5 && d.shape != STSTHIP_STENCIL_BOX9)
        return invalid("unknown shape");
    if (d.reserved != 0)
        return invalid("reserved is not 0");
    const bool has_rhs = d.has_rhs != 0;
    for (int k = 0; k < 9; k++) {
        if (!std::isfinite(d.weight[k]))
            return invalid("a weight that is not finite");
        if (d.shape == STSTHIP_STENCIL_CROSS5 && k % 2 == 0 && k != 4 && d.weight[k] != 0.0)
            return invalid("a corner weight of a CROSS5 stencil that is not zero");
    }
    if (has_rhs && !std::isfinite(d.rhs_coef))
        return invalid("an rhs_coef that is not finite");
    const unsigned elem = d.type == STSTHIP_F64 ? 8u : 4u;
    if (d.n_rows >> 31 != 0 || d.n_cols >> 31 != 0)
        return invalid("n_rows or n_cols of 2^31 or more");
    if (int rc = check_view(d.dst, elem))
        return rc;
    if (int rc = check_view(d.src, elem))
        return rc;
    if (has_rhs)
        if (int rc = check_view(d.rhs, elem))
            return rc;
    empty = d.n_rows == 0 || d.n_cols == 0;
    if (empty)
        return 0;
    if (!d.dst.base || !d.src.base || (has_rhs && !d.rhs.base))
        return invalid("null base with a non-empty rectangle");
    if (!inside(d.dst_row, d.n_rows, d.dst.height) || !inside(d.dst_col, d.n_cols, d.dst.width))
        return invalid("the destination rectangle does not lie inside its view");
    if (!inside(d.src_row, d.n_rows, d.src.height) || !inside(d.src_col, d.n_cols, d.src.width))
        return invalid("the source rectangle does not lie inside its view");
    if (has_rhs && (!inside(d.rhs_row, d.n_rows, d.rhs.height) || !inside(d.rhs_col, d.n_cols, d.rhs.width)))
        return invalid("the right-hand side's rectangle does not lie inside its view");
    if (!row_fits(d.n_cols, d.dst.stride) || !row_fits(d.n_cols, d.src.stride) || (has_rhs && !row_fits(d.n_cols, d.rhs.stride)))
        return invalid("a row of the rectangle spans 2^31 bytes or more");
    const Span to = span_of(d.dst, d.dst_row, d.dst_col, d.n_rows, d.n_cols, elem);
    // what the stencil reads: the rectangle and its neighbours inside the view
    u64 read_row = d.src_row, read_col = d.src_col, read_rows = d.n_rows, read_cols = d.n_cols;
    if (read_row > 0)
        read_row--, read_rows++;
    if (read_col > 0)
        read_col--, read_cols++;
    if (read_row + read_rows < d.src.height)
        read_rows++;
    if (read_col + read_cols < d.src.width)
        read_cols++;
    if (intersect(to, span_of(d.src, read_row, read_col, read_rows, read_cols, elem)) &&
        !other_member(d.dst, to, d.src, span_of(d.src, d.src_row, d.src_col, d.n_rows, d.n_cols, elem), elem))
        return invalid("what the stencil reads overlaps the destination (only another member of the destination's cells "
                       "may share memory with it; a stencil in place is a race)");
    if (has_rhs) {
        const Span f = span_of(d.rhs, d.rhs_row, d.rhs_col, d.n_rows, d.n_cols, elem);
        const bool in_place = d.rhs.stride == d.dst.stride && d.rhs.pitch == d.dst.pitch && f.first == to.first;
        if (intersect(to, f) && !in_place && !other_member(d.dst, to, d.rhs, f, elem))
            return invalid("the right-hand side overlaps the destination (only the destination itself, or another "
                           "member of the same cells, may share memory with it)");
    }
    return 0;
}

// Workgroups of a launch of the general kernel over n_rows rows of n_segments segments.
static dim3 plan_blocks(u64 n_segments, u64 n_rows) {
    const u64 down = std::max<u64>(1, std::min<u64>(n_rows, stencil_block_cap / std::max<u64>(1, n_segments)));
    return dim3(unsigned(n_segments), unsigned(down), 1);
}

// The general kernel on the columns first .. first + n_cols - 1 of the rectangle of job `whole`.
template <typename T, unsigned SHAPE, bool RHS> static void launch_cells(StencilJob<T> whole, unsigned first, unsigned n_cols, hipStream_t s) {
    StencilJob<T> j = whole;
    j.dst += u64(first) * j.dst_step;
    j.src += u64(first) * j.src_step;
    if (RHS)
        j.rhs += u64(first) * j.rhs_step;
    j.n_cols = n_cols;
    j.left_edge = first == 0 ? whole.left_edge : 0;
    j.right_at = whole.right_at - first; // (right_at >= the whole rectangle's n_cols > first)
    const dim3 grid = plan_blocks((u64(n_cols) + stencil_segment_cells - 1) / stencil_segment_cells, j.n_rows);
    hipLaunchKernelGGL((stencil_cells_kernel<T, SHAPE, RHS>), grid, dim3(stencil_threads), 0, s, j);
}

template <typename T, int V, unsigned SHAPE, bool RHS> static void launch_rows(StencilJob<T> const &j, hipStream_t s) {
    const u64 n_chunks = (u64(j.n_rows) + stencil_chunk_rows - 1) / stencil_chunk_rows;
    const dim3 grid(unsigned((u64(j.n_units) + stencil_threads - 1) / stencil_threads),
                    unsigned(std::min<u64>(n_chunks, stencil_chunk_blocks)), 1);
    hipLaunchKernelGGL((stencil_rows_kernel<T, V, SHAPE, RHS>), grid, dim3(stencil_threads), 0, s, j);
}

// STSTHIP_STENCIL_GENERAL (any value): planes take the general kernel too -- the A/B partner of the dense kernel
// (tools/bench_stencil.py) and a second implementation for the tests.  Read at every call.
static bool general_only() { return std::getenv("STSTHIP_STENCIL_GENERAL") != nullptr; }

template <typename T, unsigned SHAPE, bool RHS> static hipError_t launch_stencil(ststhip_grid_stencil_desc const &d, hipStream_t s) {
    StencilJob<T> j{};
    j.dst = reinterpret_cast<unsigned char *>(span_of(d.dst, d.dst_row, d.dst_col, 1, 1, sizeof(T)).first);
    j.src = reinterpret_cast<const unsigned char *>(span_of(d.src, d.src_row, d.src_col, 1, 1, sizeof(T)).first);
    j.dst_row_bytes = d.dst.pitch * d.dst.stride;
    j.src_row_bytes = d.src.pitch * d.src.stride;
    // (a single column is dense; its neighbours are one stride away all the same)
    j.dst_step = unsigned(d.dst.stride);
    j.src_step = unsigned(d.src.stride);
    if (RHS) {
        j.rhs = reinterpret_cast<const unsigned char *>(span_of(d.rhs, d.rhs_row, d.rhs_col, 1, 1, sizeof(T)).first);
        j.rhs_row_bytes = d.rhs.pitch * d.rhs.stride;
        j.rhs_step = unsigned(d.rhs.stride);
    }
    j.n_rows = unsigned(d.n_rows);
    j.n_cols = unsigned(d.n_cols);
    j.top_edge = d.src_row == 0;
    j.left_edge = d.src_col == 0;
    j.bottom_at = unsigned(std::min<u64>(d.src.height - d.src_row, 0xffffffffu)); // (n_rows < 2^31 never gets there)
    j.right_at = unsigned(std::min<u64>(d.src.width - d.src_col, 0xffffffffu));
    for (int k = 0; k < 9; k++)
        j.w[k] = T(d.weight[k]); // double to the element's type, once
    j.rhs_coef = T(d.rhs_coef);
    j.halo = T(d.halo);

    const bool dense = j.dst_step == sizeof(T) && j.src_step == sizeof(T) && (!RHS || j.rhs_step == sizeof(T));
    // A cross takes the general kernel on planes too: with five loads per element the caches carry the reuse as well
    // as the registers do, and the dense kernel was not the faster of the two (profiles/grid_stencil.txt, the A/B), so
    // it is instantiated for BOX9 only.
    constexpr bool has_dense = SHAPE == STSTHIP_STENCIL_BOX9;
    if (!has_dense || !dense || general_only()) {
        launch_cells<T, SHAPE, RHS>(j, 0, j.n_cols, s);
        return hipGetLastError();
    }
    // the widest unit all sides allow in every row: the lowest set bit of their distances and, where there is more
    // than one row, of the row distances; 16 at the most, sizeof(T) at the least
    const auto low = [](const void *p) { return unsigned(reinterpret_cast<std::uintptr_t>(p)); };
    unsigned apart = 16u | (low(j.dst) - low(j.src));
    if (RHS)
        apart |= low(j.dst) - low(j.rhs);
    if (j.n_rows > 1)
        apart |= unsigned(j.dst_row_bytes) | unsigned(j.src_row_bytes) | (RHS ? unsigned(j.rhs_row_bytes) : 0u);
    const unsigned width = apart & (0u - apart);
    const unsigned per_unit = width / unsigned(sizeof(T));
    j.head = std::min(((0u - low(j.dst)) & (width - 1u)) / unsigned(sizeof(T)), j.n_cols);
    j.n_units = (j.n_cols - j.head) / per_unit;
    const unsigned tail_begin = j.head + j.n_units * per_unit;
    if constexpr (has_dense) {
        if (j.n_units > 0) {
            if (per_unit == 1)
                launch_rows<T, 1, SHAPE, RHS>(j, s);
            else if (per_unit == 2)
                launch_rows<T, 2, SHAPE, RHS>(j, s);
            else if constexpr (sizeof(T) == 4)
                launch_rows<T, 4, SHAPE, RHS>(j, s);
        }
    }
    // the columns that fill no unit: fewer than a unit's on either side
    if (j.head > 0)
        launch_cells<T, SHAPE, RHS>(j, 0, j.head, s);
    if (tail_begin < j.n_cols)
        launch_cells<T, SHAPE, RHS>(j, tail_begin, j.n_cols - tail_begin, s);
    return hipGetLastError();
}

template <typename T> static hipError_t launch_stencil(ststhip_grid_stencil_desc const &d, hipStream_t s) {
    const bool box = d.shape == STSTHIP_STENCIL_BOX9;
    if (d.has_rhs != 0)
        return box ? launch_stencil<T, STSTHIP_STENCIL_BOX9, true>(d, s) : launch_stencil<T, STSTHIP_STENCIL_CROSS5, true>(d, s);
    return box ? launch_stencil<T, STSTHIP_STENCIL_BOX9, false>(d, s) : launch_stencil<T, STSTHIP_STENCIL_CROSS5, false>(d, s);
}

} // namespace

extern "C" {

int ststhip_grid_stencil(int n, const ststhip_grid_stencil_desc *stencils, ststhip_stream stream) {
    if (n < 1 || n > 8)
        return invalid("need 1..8 entries");
    if (!stencils)
        return invalid("null argument");
    bool empty[8], any = false;
    for (int i = 0; i < n; i++) {
        if (int rc = check_stencil(stencils[i], empty[i]))
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
        const hipError_t err = stencils[i].type == STSTHIP_F64 ? launch_stencil<double>(stencils[i], s)
                                                               : launch_stencil<float>(stencils[i], s);
        if (err != hipSuccess)
            return hip_failed(err, "ststhip_grid_stencil");
    }
    return STSTHIP_OK;
}

} // extern "C"
