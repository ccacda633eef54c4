// ststhip_grid_diffusion (include/ststhip.h): the five-point finite-volume operator whose weights are face coefficients
// stored in two grids (kx: east faces, ky: south faces), A u = sigma u + scale * sum over faces of k (u_c - u_nb), in
// three modes: apply (with an optional right-hand side), one damped Jacobi step, and the diagonal solve
// z = rhs_coef * f / diag(A).
//
// The host-side validation, the walk of a rectangle and the launch limits are those of stencil.hip, repeated here the way
// stencil.hip repeats those of algebra.hip.  Two kernels, the general one templated on the element type, the mode and
// has_rhs, the dense one on the element type and the unit:
//
//   diffusion_rows_kernel   APPLY without a right-hand side where every view is dense within a row (planes).  With a
//                           right-hand side, for JACOBI and for SOLVE_DIAG it was not reliably faster than the general
//                           kernel there (profiles/grid_diffusion.txt: ahead in one session, behind in the other; behind
//                           for SOLVE_DIAG) and has no instantiation.  The scheme of stencil_rows_kernel: a wave owns a
//                           run of 64 units of consecutive columns, a lane one unit (16 bytes down to one element: the
//                           widest that dst, u, kx and ky allow relative to each other for ALL rows of the
//                           rectangle), and walks down a chunk of diffusion_chunk_rows rows with the last three rows
//                           of u and the last two rows of ky of its columns in registers: kn of a row is ks of the row
//                           above.  w, e and kw across units come from the adjacent lanes by DPP wave shifts, the
//                           elements beyond the wave's span (u on both sides, kx on the west) by one extra load in its
//                           first and last lane.  The next row of every input is requested before a row's arithmetic.
//   diffusion_cells_kernel  members of cells, JACOBI, SOLVE_DIAG (which compiles the loads of u out) and anything else:
//                           one element per lane, its neighbours and faces loaded by the lane itself; the caches carry
//                           the reuse.  The walk of stencil_cells_kernel.  It also computes the columns in front of and
//                           behind the units of the dense kernel.
//
// No LDS, no atomics, no scratch.  The results are defined operation by operation (ststhip.h): this file is built with
// -ffp-contract=off like the rest of the library, so no product is fused with a sum; `/` is the correctly rounded
// quotient (v_div_scale / v_rcp / v_div_fmas / v_div_fixup, which holds the only fused multiply-adds of this file's
// code), and a face or scalar that is zero is multiplied like every other (0 * inf is NaN).
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

constexpr unsigned diffusion_threads = 256;
constexpr unsigned diffusion_wave = 64;
// Rows a workgroup of the dense kernel walks down: 2 / 32 more rows of u and 1 / 32 more rows of ky read.
constexpr unsigned diffusion_chunk_rows = 32;
// A row segment of the general kernel: four elements per lane.
constexpr unsigned diffusion_segment_cells = 4 * diffusion_threads;
// At most this many workgroups per launch (or one per segment, or per 256 units, of a row).
constexpr unsigned diffusion_block_cap = 2048;

// V elements moved as one access.
template <typename T, int V> struct alignas(sizeof(T) * V) Pack {
    T v[V];
};

// dst, u, kx, ky, rhs: the first element of the rectangle (dense kernel: the units begin `head` elements on).
template <typename T> struct DiffusionJob {
    unsigned char *dst;
    const unsigned char *u, *kx, *ky, *rhs;
    u64 dst_row_bytes, u_row_bytes, kx_row_bytes, ky_row_bytes, rhs_row_bytes; // bytes between two rows
    unsigned dst_step, u_step, kx_step, ky_step, rhs_step;                     // bytes between two elements of a row
    unsigned n_rows, n_cols;
    // Where u's view ends, relative to the rectangle: row 0 has no row above it in the view (top_edge), row
    // bottom_at - 1 none below; the same for columns.
    unsigned top_edge, left_edge, bottom_at, right_at;
    // Column 0 has no column to its west in kx's view; row 0 no row above it in ky's view.
    unsigned kx_left_edge, ky_top_edge;
    unsigned head, n_units; // dense kernel: elements in front of the first unit, units per row
    T sigma, scale, omega, rhs_coef, halo, k_halo;
};

// One element, in the order ststhip.h states; every operation rounded once.
template <typename T, unsigned MODE, bool RHS>
__device__ inline T diffuse_cell(DiffusionJob<T> const &j, T c, T n, T w, T e, T s, T kn, T kw, T ke, T ks, T f) {
    T acc = T();
    if constexpr (MODE != STSTHIP_DIFFUSION_SOLVE_DIAG) {
        acc = kn * (c - n);
        acc = acc + kw * (c - w);
        acc = acc + ke * (c - e);
        acc = acc + ks * (c - s);
    }
    T d = T();
    if constexpr (MODE != STSTHIP_DIFFUSION_APPLY) {
        d = kn + kw;
        d = d + ke;
        d = d + ks;
        d = j.scale * d;
        d = j.sigma + d;
    }
    if constexpr (MODE == STSTHIP_DIFFUSION_APPLY) {
        T y = j.sigma * c;
        y = y + j.scale * acc;
        if constexpr (RHS)
            y = y + j.rhs_coef * f;
        return y;
    } else if constexpr (MODE == STSTHIP_DIFFUSION_JACOBI) {
        T t = j.sigma * c;
        t = t + j.scale * acc;
        T r = j.rhs_coef * f;
        r = r - t;
        return c + j.omega * (r / d);
    } else {
        return (j.rhs_coef * f) / d;
    }
}

// ------------------------------------------------------------------ general: one element per lane
template <typename T, unsigned MODE, bool RHS>
__global__ void __launch_bounds__(diffusion_threads) diffusion_cells_kernel(DiffusionJob<T> j) {
    constexpr bool READS_U = MODE != STSTHIP_DIFFUSION_SOLVE_DIAG;
    const unsigned seg_begin = blockIdx.x * diffusion_segment_cells; // < n_cols
    const unsigned rest = j.n_cols - seg_begin;
    const unsigned len = rest < diffusion_segment_cells ? rest : diffusion_segment_cells;
    for (unsigned r = blockIdx.y; r < j.n_rows; r += gridDim.y) {
        // a row outside its view is never read
        const bool north_ok = !(r == 0 && j.top_edge != 0), south_ok = r + 1 != j.bottom_at;
        const bool kn_ok = !(r == 0 && j.ky_top_edge != 0);
        const unsigned char *mid = nullptr;
        if constexpr (READS_U)
            mid = j.u + (u64(r) * j.u_row_bytes + u64(seg_begin) * j.u_step);
        const unsigned char *east = j.kx + (u64(r) * j.kx_row_bytes + u64(seg_begin) * j.kx_step);
        const unsigned char *south = j.ky + (u64(r) * j.ky_row_bytes + u64(seg_begin) * j.ky_step);
        const unsigned char *north = kn_ok ? south - j.ky_row_bytes : south;
        unsigned char *d = j.dst + (u64(r) * j.dst_row_bytes + u64(seg_begin) * j.dst_step);
        const unsigned char *f = nullptr;
        if constexpr (RHS)
            f = j.rhs + (u64(r) * j.rhs_row_bytes + u64(seg_begin) * j.rhs_step);
        for (unsigned c = threadIdx.x; c < len; c += diffusion_threads) {
            const unsigned g = seg_begin + c; // the column within the rectangle
            T centre = T(), n = j.halo, w = j.halo, e = j.halo, s = j.halo;
            if constexpr (READS_U) {
                const int at = int(c * j.u_step), step = int(j.u_step); // (c + 1) * step stays below 2^31
                centre = *reinterpret_cast<const T *>(mid + at);
                if (north_ok)
                    n = *reinterpret_cast<const T *>(mid - j.u_row_bytes + at);
                if (!(g == 0 && j.left_edge != 0))
                    w = *reinterpret_cast<const T *>(mid + (at - step));
                if (g + 1 != j.right_at)
                    e = *reinterpret_cast<const T *>(mid + (at + step));
                if (south_ok)
                    s = *reinterpret_cast<const T *>(mid + j.u_row_bytes + at);
            }
            const int k_at = int(c * j.kx_step);
            const T ke = *reinterpret_cast<const T *>(east + k_at);
            T kw = j.k_halo;
            if (!(g == 0 && j.kx_left_edge != 0))
                kw = *reinterpret_cast<const T *>(east + (k_at - int(j.kx_step)));
            const T ks = *reinterpret_cast<const T *>(south + c * j.ky_step);
            T kn = j.k_halo;
            if (kn_ok)
                kn = *reinterpret_cast<const T *>(north + c * j.ky_step);
            T own = T();
            if constexpr (RHS)
                own = *reinterpret_cast<const T *>(f + c * j.rhs_step);
            *reinterpret_cast<T *>(d + c * j.dst_step) = diffuse_cell<T, MODE, RHS>(j, centre, n, w, e, s, kn, kw, ke, ks, own);
        }
    }
}

// ------------------------------------------------------------------ dense rows: rows of u and ky in registers
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
// A lane's unit of u with its left and right neighbour: v[0], v[1 .. V], v[V + 1].
template <typename T, int V> struct Row {
    T v[V + 2];
};
// A lane's unit of kx and, in the first lane of a wave's span, the east face of the cell in front of the span.
template <typename T, int V> struct FaceRow {
    Pack<T, V> unit;
    T west;
};

template <typename T, int V> __global__ void __launch_bounds__(diffusion_threads) diffusion_rows_kernel(DiffusionJob<T> j) {
    using P = Pack<T, V>;
    const unsigned unit = blockIdx.x * diffusion_threads + threadIdx.x;
    if (unit >= j.n_units)
        return; // (a lane behind the last unit: nobody reads its registers, the last unit's lane loads its neighbour)
    const unsigned lane = threadIdx.x % diffusion_wave;
    const unsigned c0 = j.head + unit * unsigned(V); // the unit's first column within the rectangle
    const bool west_end = lane == 0, east_end = lane == diffusion_wave - 1 || unit + 1 == j.n_units;
    // the element beyond the span is a cell of u's view (false only in a wave at the view's edge)
    const bool west_ok = c0 != 0 || j.left_edge == 0, east_ok = c0 + unsigned(V) != j.right_at;
    const unsigned at = c0 * unsigned(sizeof(T)); // < 2^31
    const bool edge_ok = (west_end || east_end) && (west_end ? west_ok : east_ok);
    const int edge_at = west_end ? -int(sizeof(T)) : int(sizeof(P));
    const bool both_ok = west_end && east_end && east_ok;
    // ... and of kx's view
    const bool face_ok = west_end && (c0 != 0 || j.kx_left_edge == 0);

    // row: -1 .. n_rows, relative to the rectangle; `edges`: the row will be a centre row
    auto request = [&](int row, bool edges) {
        RawRow<T, V> raw;
        raw.edge = raw.east = j.halo;
        const bool row_ok = row < 0 ? j.top_edge == 0 : unsigned(row) != j.bottom_at; // uniform
        if (row_ok) {
            const unsigned char *p = j.u + (i64(row) * i64(j.u_row_bytes) + at);
            raw.unit = *reinterpret_cast<const P *>(p);
            if (edges && edge_ok)
                raw.edge = *reinterpret_cast<const T *>(p + edge_at);
            if (edges && both_ok)
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
    auto request_kx = [&](unsigned row) {
        FaceRow<T, V> raw;
        raw.west = j.k_halo;
        const unsigned char *p = j.kx + (u64(row) * j.kx_row_bytes + at);
        raw.unit = *reinterpret_cast<const P *>(p);
        if (face_ok)
            raw.west = *reinterpret_cast<const T *>(p - sizeof(T));
        return raw;
    };
    // row: -1 .. n_rows - 1
    auto request_ky = [&](int row) {
        P k;
        if (row >= 0 || j.ky_top_edge == 0) { // uniform
            k = *reinterpret_cast<const P *>(j.ky + (i64(row) * i64(j.ky_row_bytes) + at));
        } else {
#pragma unroll
            for (int e = 0; e < V; e++)
                k.v[e] = j.k_halo;
        }
        return k;
    };

    const unsigned n_chunks = (j.n_rows + diffusion_chunk_rows - 1) / diffusion_chunk_rows;
    for (unsigned chunk = blockIdx.y; chunk < n_chunks; chunk += gridDim.y) {
        const unsigned begin = chunk * diffusion_chunk_rows;
        const unsigned rest = j.n_rows - begin;
        const unsigned end = begin + (rest < diffusion_chunk_rows ? rest : diffusion_chunk_rows);
        P above = request(int(begin) - 1, false).unit;
        Row<T, V> here = finish(request(int(begin), true));
        RawRow<T, V> coming = request(int(begin) + 1, true);
        P north = request_ky(int(begin) - 1);
        P south = request_ky(int(begin));
        FaceRow<T, V> east = request_kx(begin);
        for (unsigned r = begin; r < end; r++) {
            // the next row of every input, before this row's arithmetic
            const bool more = r + 1 < end;
            const RawRow<T, V> later = more ? request(int(r) + 2, true) : coming;
            const P south_next = more ? request_ky(int(r) + 1) : south;
            const FaceRow<T, V> east_next = more ? request_kx(r + 1) : east;
            const T face_west = from_west_lane(east.unit.v[V - 1]);
            const T kw0 = west_end ? east.west : face_west;
            P out;
#pragma unroll
            for (int e = 0; e < V; e++) {
                const T kw = e == 0 ? kw0 : east.unit.v[e == 0 ? 0 : e - 1];
                out.v[e] = diffuse_cell<T, STSTHIP_DIFFUSION_APPLY, false>(j, here.v[e + 1], above.v[e], here.v[e], here.v[e + 2],
                                                                           coming.unit.v[e], north.v[e], kw, east.unit.v[e],
                                                                           south.v[e], T());
            }
            *reinterpret_cast<P *>(j.dst + (u64(r) * j.dst_row_bytes + at)) = out;
#pragma unroll
            for (int e = 0; e < V; e++)
                above.v[e] = here.v[e + 1];
            if (more)
                here = finish(coming);
            coming = later;
            north = south;
            south = south_next;
            east = east_next;
        }
    }
}

// ------------------------------------------------------------------ host side
static int invalid(const char *what) {
    const std::string msg = std::string("grid diffusion: ") + what;
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

// One side that is only read: where its rectangle begins and how far what is read of it goes beyond the rectangle.
struct ReadSide {
    ststhip_grid_view const *view;
    u64 row, col;
    bool north, west, south, east; // a cell more on that side, where the view goes on
    const char *outside, *overlap;
};

// One entry, validated.  `empty`: nothing to compute.
static int check_diffusion(ststhip_grid_diffusion_desc const &d, bool &empty) {
    if (d.type != STSTHIP_F32 && d.type != STSTHIP_F64)
        return invalid("unknown element type");
    if (d.mode != STSTHIP_DIFFUSION_APPLY && d.mode != STSTHIP_DIFFUSION_JACOBI && d.mode != STSTHIP_DIFFUSION_SOLVE_DIAG)
        return invalid("unknown mode");
    if (d.reserved != 0)
        return invalid("reserved is not 0");
    const bool has_rhs = d.has_rhs != 0, reads_u = d.mode != STSTHIP_DIFFUSION_SOLVE_DIAG;
    if (!has_rhs && d.mode != STSTHIP_DIFFUSION_APPLY)
        return invalid("a Jacobi step or a diagonal solve without a right-hand side");
    if (!std::isfinite(d.sigma) || !std::isfinite(d.scale))
        return invalid("a sigma or scale that is not finite");
    if (has_rhs && !std::isfinite(d.rhs_coef))
        return invalid("an rhs_coef that is not finite");
    if (d.mode == STSTHIP_DIFFUSION_JACOBI && !std::isfinite(d.omega))
        return invalid("an omega that is not finite");
    const unsigned elem = d.type == STSTHIP_F64 ? 8u : 4u;
    if (d.n_rows >> 31 != 0 || d.n_cols >> 31 != 0)
        return invalid("n_rows or n_cols of 2^31 or more");
    const ReadSide sides[4] = {
        {&d.u, d.u_row, d.u_col, true, true, true, true, "the rectangle of u does not lie inside its view",
         "what is read of u overlaps the destination (only another member of the destination's cells may share memory "
         "with it; an operator in place is a race)"},
        {&d.kx, d.kx_row, d.kx_col, false, true, false, false, "the rectangle of kx does not lie inside its view",
         "what is read of kx overlaps the destination (only another member of the destination's cells may share memory "
         "with it)"},
        {&d.ky, d.ky_row, d.ky_col, true, false, false, false, "the rectangle of ky does not lie inside its view",
         "what is read of ky overlaps the destination (only another member of the destination's cells may share memory "
         "with it)"},
        {&d.rhs, d.rhs_row, d.rhs_col, false, false, false, false,
         "the right-hand side's rectangle does not lie inside its view",
         "the right-hand side overlaps the destination (only the destination itself, or another member of the same "
         "cells, may share memory with it)"}};
    const bool used[4] = {reads_u, true, true, has_rhs};
    if (int rc = check_view(d.dst, elem))
        return rc;
    for (int k = 0; k < 4; k++)
        if (used[k])
            if (int rc = check_view(*sides[k].view, elem))
                return rc;
    empty = d.n_rows == 0 || d.n_cols == 0;
    if (empty)
        return 0;
    if (!d.dst.base)
        return invalid("null base with a non-empty rectangle");
    for (int k = 0; k < 4; k++)
        if (used[k] && !sides[k].view->base)
            return invalid("null base with a non-empty rectangle");
    if (!inside(d.dst_row, d.n_rows, d.dst.height) || !inside(d.dst_col, d.n_cols, d.dst.width))
        return invalid("the destination rectangle does not lie inside its view");
    for (int k = 0; k < 4; k++)
        if (used[k] && (!inside(sides[k].row, d.n_rows, sides[k].view->height) ||
                        !inside(sides[k].col, d.n_cols, sides[k].view->width)))
            return invalid(sides[k].outside);
    if (!row_fits(d.n_cols, d.dst.stride))
        return invalid("a row of the rectangle spans 2^31 bytes or more");
    for (int k = 0; k < 4; k++)
        if (used[k] && !row_fits(d.n_cols, sides[k].view->stride))
            return invalid("a row of the rectangle spans 2^31 bytes or more");
    const Span to = span_of(d.dst, d.dst_row, d.dst_col, d.n_rows, d.n_cols, elem);
    for (int k = 0; k < 4; k++) {
        if (!used[k])
            continue;
        ReadSide const &s = sides[k];
        ststhip_grid_view const &v = *s.view;
        // what is read: the rectangle and its neighbours inside the view
        u64 read_row = s.row, read_col = s.col, read_rows = d.n_rows, read_cols = d.n_cols;
        if (s.north && read_row > 0)
            read_row--, read_rows++;
        if (s.west && read_col > 0)
            read_col--, read_cols++;
        if (s.south && read_row + read_rows < v.height)
            read_rows++;
        if (s.east && read_col + read_cols < v.width)
            read_cols++;
        if (!intersect(to, span_of(v, read_row, read_col, read_rows, read_cols, elem)))
            continue;
        const Span own = span_of(v, s.row, s.col, d.n_rows, d.n_cols, elem);
        const bool in_place = k == 3 && v.stride == d.dst.stride && v.pitch == d.dst.pitch && own.first == to.first;
        if (!in_place && !other_member(d.dst, to, v, own, elem))
            return invalid(s.overlap);
    }
    return 0;
}

// Workgroups of a launch of the general kernel over n_rows rows of n_segments segments.
static dim3 plan_blocks(u64 n_segments, u64 n_rows) {
    const u64 down = std::max<u64>(1, std::min<u64>(n_rows, diffusion_block_cap / std::max<u64>(1, n_segments)));
    return dim3(unsigned(n_segments), unsigned(down), 1);
}

// The general kernel on the columns first .. first + n_cols - 1 of the rectangle of job `whole`.
template <typename T, unsigned MODE, bool RHS>
static void launch_cells(DiffusionJob<T> whole, unsigned first, unsigned n_cols, hipStream_t s) {
    DiffusionJob<T> j = whole;
    j.dst += u64(first) * j.dst_step;
    if (MODE != STSTHIP_DIFFUSION_SOLVE_DIAG)
        j.u += u64(first) * j.u_step;
    j.kx += u64(first) * j.kx_step;
    j.ky += u64(first) * j.ky_step;
    if (RHS)
        j.rhs += u64(first) * j.rhs_step;
    j.n_cols = n_cols;
    j.left_edge = first == 0 ? whole.left_edge : 0;
    j.kx_left_edge = first == 0 ? whole.kx_left_edge : 0;
    j.right_at = whole.right_at - first; // (right_at >= the whole rectangle's n_cols > first)
    const dim3 grid = plan_blocks((u64(n_cols) + diffusion_segment_cells - 1) / diffusion_segment_cells, j.n_rows);
    hipLaunchKernelGGL((diffusion_cells_kernel<T, MODE, RHS>), grid, dim3(diffusion_threads), 0, s, j);
}

template <typename T, int V> static void launch_rows(DiffusionJob<T> const &j, hipStream_t s) {
    const u64 n_chunks = (u64(j.n_rows) + diffusion_chunk_rows - 1) / diffusion_chunk_rows;
    const u64 across = (u64(j.n_units) + diffusion_threads - 1) / diffusion_threads;
    const dim3 grid(unsigned(across), unsigned(std::max<u64>(1, std::min<u64>(n_chunks, diffusion_block_cap / across))), 1);
    hipLaunchKernelGGL((diffusion_rows_kernel<T, V>), grid, dim3(diffusion_threads), 0, s, j);
}

// STSTHIP_DIFFUSION_GENERAL (any value): planes take the general kernel too -- the A/B partner of the dense kernel
// (tools/bench_grid_diffusion.py) and a second implementation for the tests.  Read at every call.
static bool general_only() { return std::getenv("STSTHIP_DIFFUSION_GENERAL") != nullptr; }

template <typename T, unsigned MODE, bool RHS>
static hipError_t launch_diffusion(ststhip_grid_diffusion_desc const &d, hipStream_t s) {
    constexpr bool READS_U = MODE != STSTHIP_DIFFUSION_SOLVE_DIAG;
    const auto first_of = [](ststhip_grid_view const &v, u64 row, u64 col) {
        return reinterpret_cast<unsigned char *>(span_of(v, row, col, 1, 1, sizeof(T)).first);
    };
    DiffusionJob<T> j{};
    j.dst = first_of(d.dst, d.dst_row, d.dst_col);
    j.dst_row_bytes = d.dst.pitch * d.dst.stride;
    j.dst_step = unsigned(d.dst.stride); // (a single column is dense; its neighbours are one stride away all the same)
    j.n_rows = unsigned(d.n_rows);
    j.n_cols = unsigned(d.n_cols);
    if (READS_U) {
        j.u = first_of(d.u, d.u_row, d.u_col);
        j.u_row_bytes = d.u.pitch * d.u.stride;
        j.u_step = unsigned(d.u.stride);
        j.top_edge = d.u_row == 0;
        j.left_edge = d.u_col == 0;
        j.bottom_at = unsigned(std::min<u64>(d.u.height - d.u_row, 0xffffffffu)); // (n_rows < 2^31 never gets there)
        j.right_at = unsigned(std::min<u64>(d.u.width - d.u_col, 0xffffffffu));
    }
    j.kx = first_of(d.kx, d.kx_row, d.kx_col);
    j.kx_row_bytes = d.kx.pitch * d.kx.stride;
    j.kx_step = unsigned(d.kx.stride);
    j.kx_left_edge = d.kx_col == 0;
    j.ky = first_of(d.ky, d.ky_row, d.ky_col);
    j.ky_row_bytes = d.ky.pitch * d.ky.stride;
    j.ky_step = unsigned(d.ky.stride);
    j.ky_top_edge = d.ky_row == 0;
    if (RHS) {
        j.rhs = first_of(d.rhs, d.rhs_row, d.rhs_col);
        j.rhs_row_bytes = d.rhs.pitch * d.rhs.stride;
        j.rhs_step = unsigned(d.rhs.stride);
    }
    // double to the element's type, once
    j.sigma = T(d.sigma);
    j.scale = T(d.scale);
    j.omega = T(d.omega);
    j.rhs_coef = T(d.rhs_coef);
    j.halo = T(d.halo);
    j.k_halo = T(d.k_halo);

    const bool dense = j.dst_step == sizeof(T) && (!READS_U || j.u_step == sizeof(T)) && j.kx_step == sizeof(T) &&
                       j.ky_step == sizeof(T) && (!RHS || j.rhs_step == sizeof(T));
    // Everything but an APPLY without a right-hand side takes the general kernel on planes too.  The dense kernel lost
    // to it for SOLVE_DIAG, which reads no neighbour of u, and with a fourth input (APPLY with a right-hand side,
    // JACOBI) it was ahead by 5 % in one session and behind by 2 to 3 % in the other (profiles/grid_diffusion.txt, the
    // A/B), so it is instantiated for the one case it won twice.
    constexpr bool has_dense = MODE == STSTHIP_DIFFUSION_APPLY && !RHS;
    if (!has_dense || !dense || general_only()) {
        launch_cells<T, MODE, RHS>(j, 0, j.n_cols, s);
        return hipGetLastError();
    }
    // the widest unit all sides allow in every row: the lowest set bit of their distances and, where there is more
    // than one row, of the row distances; 16 at the most, sizeof(T) at the least.  The rows of u above and below the
    // rectangle and the row of ky above it are read as units too, so their row distances count wherever such a row
    // lies inside the view.
    const auto low = [](const void *p) { return unsigned(reinterpret_cast<std::uintptr_t>(p)); };
    unsigned apart = 16u | (low(j.dst) - low(j.kx)) | (low(j.dst) - low(j.ky)) | (low(j.dst) - low(j.u));
    if (j.n_rows > 1)
        apart |= unsigned(j.dst_row_bytes) | unsigned(j.kx_row_bytes);
    if (j.n_rows > 1 || j.top_edge == 0 || j.bottom_at != j.n_rows)
        apart |= unsigned(j.u_row_bytes);
    if (j.n_rows > 1 || j.ky_top_edge == 0)
        apart |= unsigned(j.ky_row_bytes);
    const unsigned width = apart & (0u - apart);
    const unsigned per_unit = width / unsigned(sizeof(T));
    j.head = std::min(((0u - low(j.dst)) & (width - 1u)) / unsigned(sizeof(T)), j.n_cols);
    j.n_units = (j.n_cols - j.head) / per_unit;
    const unsigned tail_begin = j.head + j.n_units * per_unit;
    if constexpr (has_dense) {
        if (j.n_units > 0) {
            if (per_unit == 1)
                launch_rows<T, 1>(j, s);
            else if (per_unit == 2)
                launch_rows<T, 2>(j, s);
            else if constexpr (sizeof(T) == 4)
                launch_rows<T, 4>(j, s);
        }
    }
    // the columns that fill no unit: fewer than a unit's on either side
    if (j.head > 0)
        launch_cells<T, MODE, RHS>(j, 0, j.head, s);
    if (tail_begin < j.n_cols)
        launch_cells<T, MODE, RHS>(j, tail_begin, j.n_cols - tail_begin, s);
    return hipGetLastError();
}

template <typename T> static hipError_t launch_diffusion(ststhip_grid_diffusion_desc const &d, hipStream_t s) {
    if (d.mode == STSTHIP_DIFFUSION_JACOBI)
        return launch_diffusion<T, STSTHIP_DIFFUSION_JACOBI, true>(d, s);
    if (d.mode == STSTHIP_DIFFUSION_SOLVE_DIAG)
        return launch_diffusion<T, STSTHIP_DIFFUSION_SOLVE_DIAG, true>(d, s);
    return d.has_rhs != 0 ? launch_diffusion<T, STSTHIP_DIFFUSION_APPLY, true>(d, s)
                          : launch_diffusion<T, STSTHIP_DIFFUSION_APPLY, false>(d, s);
}

} // namespace

extern "C" {

int ststhip_grid_diffusion(int n, const ststhip_grid_diffusion_desc *entries, ststhip_stream stream) {
    if (n < 1 || n > 8)
        return invalid("need 1..8 entries");
    if (!entries)
        return invalid("null argument");
    bool empty[8], any = false;
    for (int i = 0; i < n; i++) {
        if (int rc = check_diffusion(entries[i], empty[i]))
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
        const hipError_t err = entries[i].type == STSTHIP_F64 ? launch_diffusion<double>(entries[i], s)
                                                              : launch_diffusion<float>(entries[i], s);
        if (err != hipSuccess)
            return hip_failed(err, "ststhip_grid_diffusion");
    }
    return STSTHIP_OK;
}

} // extern "C"
