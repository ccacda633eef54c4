// ststhip_grid_combine / ststhip_grid_resample (include/ststhip.h): linear combinations of a few grids and the 2:1
// transfer between a fine and a coarse grid, computed where the cells are.
//
// The kernels walk a rectangle the way regions.hip and norms.hip do: a workgroup owns row segments -- segment
// blockIdx.x of rows blockIdx.y, + gridDim.y, ... of the rectangle --, consecutive lanes take consecutive elements of
// one row, the address arithmetic per row is wave-uniform (64-bit) and a lane adds a 32-bit offset (the validation
// keeps a row's byte extent below 2^31).  No atomics, no LDS, no scratch; the number of workgroups follows from the
// rectangle alone, capped by a constant.
//
//   combine_rows_kernel     every side dense within a row: per row the widest access that the destination and all
//                           terms allow relative to each other (16 bytes down to one element), the unaligned head and
//                           tail peeled off as single elements; all loads of a lane's elements before the arithmetic.
//   combine_strided_kernel  members of cells: one element per lane, four per lane and segment.
//   restrict_kernel         a lane produces coarse elements from two source rows; on dense, aligned f32 rows one
//                           16-byte load per row gives two results and one 8-byte store.
//   prolong_kernel          a lane owns a coarse cell, reads its 3 x 3 neighbourhood (the halo where the view ends)
//                           and writes the 2 x 2 fine cells; the caches carry the reuse between neighbouring lanes.
//
// The results are defined operation by operation (ststhip.h): this file is built with -ffp-contract=off like the rest
// of the library, and nothing below may be rewritten into a fused multiply-add.
#include "ststhip.h"

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <string>

namespace ststhip_detail {
int fail(int status, const char *message); // runtime.hip
}

namespace {

using u64 = unsigned long long;

constexpr unsigned algebra_threads = 256;
// A row segment of the dense combine: four 16-byte accesses per lane and side.
constexpr unsigned algebra_segment_bytes = 4 * 16 * algebra_threads;
// A row segment of the other kernels: four elements (restrict, prolong: coarse cells) per lane.
constexpr unsigned algebra_segment_cells = 4 * algebra_threads;
// At most this many workgroups per launch (or one per segment of a row, if a row alone has more), as the regions.
constexpr unsigned algebra_block_cap = 2048;
constexpr int max_terms = 4;

inline __device__ unsigned low_bits(const void *p) { return unsigned(reinterpret_cast<std::uintptr_t>(p)); }

// V elements moved as one access.
template <typename T, int V> struct alignas(sizeof(T) * V) Pack {
    T v[V];
};

// dst, src[t]: the first element of the rectangle.
template <typename T, int NT> struct CombineJob {
    unsigned char *dst;
    const unsigned char *src[NT];
    u64 dst_row_bytes, src_row_bytes[NT]; // bytes between two rows
    unsigned dst_step, src_step[NT];      // strided: bytes between two elements of a row
    unsigned n_rows, row_len;             // row_len: elements of a row of the rectangle
    T coef[NT];
};

// acc = c0 * x0, then acc = acc + ck * xk: every product and every sum rounded once, left to right.
template <typename T, int NT> __device__ inline T combine_one(const T (&coef)[NT], const T (&x)[NT]) {
    T acc = coef[0] * x[0];
#pragma unroll
    for (int t = 1; t < NT; t++)
        acc = acc + coef[t] * x[t];
    return acc;
}

// n units of V elements, every side aligned to a unit, by the whole workgroup: the loads of a lane's two units of
// every term are requested before the first product.
template <typename T, int NT, int V>
__device__ inline void combine_units(unsigned char *d, const unsigned char *const *s, const T (&coef)[NT], unsigned n) {
    using P = Pack<T, V>;
    for (unsigned base = 0; base < n; base += 2 * algebra_threads) {
        P x[2][NT];
#pragma unroll
        for (unsigned k = 0; k < 2; k++) {
            const unsigned i = base + threadIdx.x + k * algebra_threads;
            if (i < n) {
#pragma unroll
                for (int t = 0; t < NT; t++)
                    x[k][t] = reinterpret_cast<const P *>(s[t])[i];
            }
        }
#pragma unroll
        for (unsigned k = 0; k < 2; k++) {
            const unsigned i = base + threadIdx.x + k * algebra_threads;
            if (i < n) {
                P out;
#pragma unroll
                for (int e = 0; e < V; e++) {
                    T xs[NT];
#pragma unroll
                    for (int t = 0; t < NT; t++)
                        xs[t] = x[k][t].v[e];
                    out.v[e] = combine_one<T, NT>(coef, xs);
                }
                reinterpret_cast<P *>(d)[i] = out;
            }
        }
    }
}

template <typename T, int NT> __global__ void __launch_bounds__(algebra_threads) combine_rows_kernel(CombineJob<T, NT> j) {
    constexpr unsigned segment = algebra_segment_bytes / unsigned(sizeof(T)); // elements
    const unsigned seg_begin = blockIdx.x * segment;                          // < row_len
    const unsigned rest = j.row_len - seg_begin;
    const unsigned len = rest < segment ? rest : segment;
    for (unsigned r = blockIdx.y; r < j.n_rows; r += gridDim.y) {
        unsigned char *d = j.dst + (u64(r) * j.dst_row_bytes + u64(seg_begin) * sizeof(T));
        const unsigned char *s[NT];
        // the widest access all sides allow: the lowest set bit of their distances, 16 at the most (every address is
        // a multiple of sizeof(T), so it is sizeof(T) at the least)
        unsigned apart = 16u;
#pragma unroll
        for (int t = 0; t < NT; t++) {
            s[t] = j.src[t] + (u64(r) * j.src_row_bytes[t] + u64(seg_begin) * sizeof(T));
            apart |= low_bits(d) - low_bits(s[t]);
        }
        const unsigned w = apart & (0u - apart);
        const unsigned per_unit = w / unsigned(sizeof(T));
        unsigned head = ((0u - low_bits(d)) & (w - 1u)) / unsigned(sizeof(T)); // elements in front of the first unit
        head = head < len ? head : len;
        const unsigned n_units = (len - head) / per_unit;
        const unsigned tail_begin = head + n_units * per_unit;
        const unsigned n_edge = head + (len - tail_begin); // < 8
        const unsigned char *body[NT];
#pragma unroll
        for (int t = 0; t < NT; t++)
            body[t] = s[t] + head * sizeof(T);
        if (per_unit == 1)
            combine_units<T, NT, 1>(d + head * sizeof(T), body, j.coef, n_units);
        else if (per_unit == 2)
            combine_units<T, NT, 2>(d + head * sizeof(T), body, j.coef, n_units);
        else if constexpr (sizeof(T) == 4)
            combine_units<T, NT, 4>(d + head * sizeof(T), body, j.coef, n_units);
        if (per_unit > 1 && threadIdx.x < n_edge) {
            const unsigned e = threadIdx.x < head ? threadIdx.x : tail_begin + (threadIdx.x - head);
            T xs[NT];
#pragma unroll
            for (int t = 0; t < NT; t++)
                xs[t] = reinterpret_cast<const T *>(s[t])[e];
            reinterpret_cast<T *>(d)[e] = combine_one<T, NT>(j.coef, xs);
        }
    }
}

template <typename T, int NT> __global__ void __launch_bounds__(algebra_threads) combine_strided_kernel(CombineJob<T, NT> j) {
    const unsigned seg_begin = blockIdx.x * algebra_segment_cells; // < row_len
    const unsigned rest = j.row_len - seg_begin;
    const unsigned len = rest < algebra_segment_cells ? rest : algebra_segment_cells;
    for (unsigned r = blockIdx.y; r < j.n_rows; r += gridDim.y) {
        unsigned char *d = j.dst + (u64(r) * j.dst_row_bytes + u64(seg_begin) * j.dst_step);
        const unsigned char *s[NT];
#pragma unroll
        for (int t = 0; t < NT; t++)
            s[t] = j.src[t] + (u64(r) * j.src_row_bytes[t] + u64(seg_begin) * j.src_step[t]);
        T x[4][NT];
#pragma unroll
        for (unsigned k = 0; k < 4; k++) {
            const unsigned c = threadIdx.x + k * algebra_threads;
            if (c < len) {
#pragma unroll
                for (int t = 0; t < NT; t++)
                    x[k][t] = *reinterpret_cast<const T *>(s[t] + c * j.src_step[t]);
            }
        }
#pragma unroll
        for (unsigned k = 0; k < 4; k++) {
            const unsigned c = threadIdx.x + k * algebra_threads;
            if (c < len)
                *reinterpret_cast<T *>(d + c * j.dst_step) = combine_one<T, NT>(j.coef, x[k]);
        }
    }
}

// dst: the first coarse element, src: the first fine element of the rectangle.
template <typename T> struct ResampleJob {
    unsigned char *dst;
    const unsigned char *src;
    u64 dst_row_bytes, src_row_bytes; // bytes between two rows of the destination's / the source's view
    unsigned dst_step, src_step;      // bytes between two elements of a row
    unsigned n_rows, n_cols;          // coarse cells
    // prolong: where the source view ends, relative to the rectangle.  Coarse row 0 has no row above it in the view
    // (top_edge), coarse row bottom_at - 1 none below; the same for columns.
    unsigned top_edge, left_edge, bottom_at, right_at;
    T halo;
};

// ((s(2i,2j) + s(2i,2j+1)) + (s(2i+1,2j) + s(2i+1,2j+1))) * 0.25
template <typename T> __device__ inline T mean_of(T a, T b, T c, T d) { return ((a + b) + (c + d)) * T(0.25); }

template <typename T> __global__ void __launch_bounds__(algebra_threads) restrict_kernel(ResampleJob<T> j) {
    const unsigned seg_begin = blockIdx.x * algebra_segment_cells; // < n_cols
    const unsigned rest = j.n_cols - seg_begin;
    const unsigned len = rest < algebra_segment_cells ? rest : algebra_segment_cells;
    for (unsigned r = blockIdx.y; r < j.n_rows; r += gridDim.y) {
        unsigned char *d = j.dst + (u64(r) * j.dst_row_bytes + u64(seg_begin) * j.dst_step);
        const unsigned char *s0 = j.src + (u64(2 * r) * j.src_row_bytes + u64(2 * seg_begin) * j.src_step);
        const unsigned char *s1 = s0 + j.src_row_bytes;
        unsigned done = 0;
        if constexpr (sizeof(T) == 4) {
            // dense rows whose first elements sit on 16 (source) and 8 (destination) bytes: four source elements of
            // either row per lane
            if (j.dst_step == 4 && j.src_step == 4 && ((low_bits(s0) | low_bits(s1)) & 15u) == 0 && (low_bits(d) & 7u) == 0) {
                const unsigned n_pairs = len / 2;
                for (unsigned p = threadIdx.x; p < n_pairs; p += algebra_threads) {
                    const Pack<T, 4> a = reinterpret_cast<const Pack<T, 4> *>(s0)[p];
                    const Pack<T, 4> b = reinterpret_cast<const Pack<T, 4> *>(s1)[p];
                    Pack<T, 2> out;
                    out.v[0] = mean_of(a.v[0], a.v[1], b.v[0], b.v[1]);
                    out.v[1] = mean_of(a.v[2], a.v[3], b.v[2], b.v[3]);
                    reinterpret_cast<Pack<T, 2> *>(d)[p] = out;
                }
                done = 2 * n_pairs; // (an odd row leaves its last element to the loop below)
            }
        }
        T x[4][4];
#pragma unroll
        for (unsigned k = 0; k < 4; k++) {
            const unsigned c = done + threadIdx.x + k * algebra_threads;
            if (c < len) {
                const unsigned at = 2 * c * j.src_step;
                x[k][0] = *reinterpret_cast<const T *>(s0 + at);
                x[k][1] = *reinterpret_cast<const T *>(s0 + at + j.src_step);
                x[k][2] = *reinterpret_cast<const T *>(s1 + at);
                x[k][3] = *reinterpret_cast<const T *>(s1 + at + j.src_step);
            }
        }
#pragma unroll
        for (unsigned k = 0; k < 4; k++) {
            const unsigned c = done + threadIdx.x + k * algebra_threads;
            if (c < len)
                *reinterpret_cast<T *>(d + c * j.dst_step) = mean_of(x[k][0], x[k][1], x[k][2], x[k][3]);
        }
    }
}

template <typename T> __global__ void __launch_bounds__(algebra_threads) prolong_kernel(ResampleJob<T> j) {
    const unsigned seg_begin = blockIdx.x * algebra_segment_cells; // < n_cols
    const unsigned rest = j.n_cols - seg_begin;
    const unsigned len = rest < algebra_segment_cells ? rest : algebra_segment_cells;
    const T near = T(0.75), far = T(0.25);
    for (unsigned r = blockIdx.y; r < j.n_rows; r += gridDim.y) {
        // the three source rows; one outside the view is never read
        const bool row_ok[3] = {!(r == 0 && j.top_edge != 0), true, r + 1 != j.bottom_at};
        const unsigned char *mid = j.src + (u64(r) * j.src_row_bytes + u64(seg_begin) * j.src_step);
        const unsigned char *row[3] = {row_ok[0] ? mid - j.src_row_bytes : mid, mid, row_ok[2] ? mid + j.src_row_bytes : mid};
        unsigned char *d0 = j.dst + (u64(2 * r) * j.dst_row_bytes + u64(2 * seg_begin) * j.dst_step);
        unsigned char *d1 = d0 + j.dst_row_bytes;
        // dense fine rows whose first elements sit on two elements: a lane's two cells of a row as one store
        const bool paired = j.dst_step == sizeof(T) && ((low_bits(d0) | low_bits(d1)) & unsigned(2 * sizeof(T) - 1)) == 0;
        for (unsigned c = threadIdx.x; c < len; c += algebra_threads) {
            const unsigned g = seg_begin + c; // the column within the rectangle
            const bool col_ok[3] = {!(g == 0 && j.left_edge != 0), true, g + 1 != j.right_at};
            const int at = int(c * j.src_step), step = int(j.src_step); // (c + 1) * step stays below 2^31
            T v[3][3];
#pragma unroll
            for (int p = 0; p < 3; p++) {
#pragma unroll
                for (int q = 0; q < 3; q++) {
                    v[p][q] = j.halo;
                    if (row_ok[p] && col_ok[q])
                        v[p][q] = *reinterpret_cast<const T *>(row[p] + (at + (q - 1) * step));
                }
            }
            // h(r) = 0.75 * c(r, j) + 0.25 * c(r, j_far) for j_far = j - 1 and j + 1
            T h[3][2];
#pragma unroll
            for (int p = 0; p < 3; p++) {
                const T centre = near * v[p][1];
                h[p][0] = centre + far * v[p][0];
                h[p][1] = centre + far * v[p][2];
            }
            // v = 0.75 * h(i) + 0.25 * h(i_far) for i_far = i - 1 and i + 1
            Pack<T, 2> up, down;
#pragma unroll
            for (int b = 0; b < 2; b++) {
                const T centre = near * h[1][b];
                up.v[b] = centre + far * h[0][b];
                down.v[b] = centre + far * h[2][b];
            }
            if (paired) {
                reinterpret_cast<Pack<T, 2> *>(d0)[c] = up;
                reinterpret_cast<Pack<T, 2> *>(d1)[c] = down;
            } else {
                const unsigned to = 2 * c * j.dst_step;
                *reinterpret_cast<T *>(d0 + to) = up.v[0];
                *reinterpret_cast<T *>(d0 + to + j.dst_step) = up.v[1];
                *reinterpret_cast<T *>(d1 + to) = down.v[0];
                *reinterpret_cast<T *>(d1 + to + j.dst_step) = down.v[1];
            }
        }
    }
}

// ------------------------------------------------------------------ host side
static int invalid(const char *what) {
    const std::string msg = std::string("grid algebra: ") + what;
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

// Workgroups of a launch over n_rows rows of n_segments segments.
static dim3 plan_blocks(u64 n_segments, u64 n_rows) {
    const u64 down = std::max<u64>(1, std::min<u64>(n_rows, algebra_block_cap / std::max<u64>(1, n_segments)));
    return dim3(unsigned(n_segments), unsigned(down), 1);
}

static int resolve_stream(ststhip_stream &stream) {
    if (int rc = ststhip_init(-1))
        return rc;
    if (!stream)
        if (int rc = ststhip_default_stream(&stream))
            return rc;
    return STSTHIP_OK;
}

static unsigned elem_size_of(unsigned type) { return type == STSTHIP_F64 ? 8u : 4u; }

// One combine entry, validated.  `empty`: nothing to compute.
static int check_combine(ststhip_grid_combine_desc const &c, bool &empty) {
    if (c.type != STSTHIP_F32 && c.type != STSTHIP_F64)
        return invalid("unknown element type");
    if (c.n_terms < 1 || c.n_terms > unsigned(max_terms))
        return invalid("need 1..4 terms");
    const unsigned elem = elem_size_of(c.type);
    if (c.n_rows >> 31 != 0 || c.n_cols >> 31 != 0)
        return invalid("n_rows or n_cols of 2^31 or more");
    if (int rc = check_view(c.dst, elem))
        return rc;
    for (unsigned t = 0; t < c.n_terms; t++)
        if (int rc = check_view(c.term[t].src, elem))
            return rc;
    empty = c.n_rows == 0 || c.n_cols == 0;
    if (empty)
        return 0;
    if (!c.dst.base)
        return invalid("null base with a non-empty rectangle");
    if (!inside(c.dst_row, c.n_rows, c.dst.height) || !inside(c.dst_col, c.n_cols, c.dst.width))
        return invalid("the destination rectangle does not lie inside its view");
    if (!row_fits(c.n_cols, c.dst.stride))
        return invalid("a row of the rectangle spans 2^31 bytes or more");
    const Span d = span_of(c.dst, c.dst_row, c.dst_col, c.n_rows, c.n_cols, elem);
    for (unsigned t = 0; t < c.n_terms; t++) {
        ststhip_grid_view const &v = c.term[t].src;
        if (!v.base)
            return invalid("null base with a non-empty rectangle");
        if (!inside(c.term[t].row, c.n_rows, v.height) || !inside(c.term[t].col, c.n_cols, v.width))
            return invalid("a term's rectangle does not lie inside its view");
        if (!row_fits(c.n_cols, v.stride))
            return invalid("a row of the rectangle spans 2^31 bytes or more");
        const Span s = span_of(v, c.term[t].row, c.term[t].col, c.n_rows, c.n_cols, elem);
        if (intersect(d, s)) {
            const bool same_cells = v.stride == c.dst.stride && v.pitch == c.dst.pitch;
            const u64 apart = d.first > s.first ? d.first - s.first : s.first - d.first;
            const bool in_place = same_cells && apart == 0;
            const bool members = same_cells && apart >= elem && apart + elem <= v.stride;
            if (!in_place && !members)
                return invalid("a term overlaps the destination (only the destination itself, or another member of "
                               "the same cells, may share memory with it)");
        }
    }
    return 0;
}

template <typename T, int NT> static hipError_t launch_combine(ststhip_grid_combine_desc const &c, hipStream_t s) {
    CombineJob<T, NT> j{};
    j.dst = reinterpret_cast<unsigned char *>(span_of(c.dst, c.dst_row, c.dst_col, 1, 1, sizeof(T)).first);
    j.dst_row_bytes = c.n_rows == 1 ? 0 : c.dst.pitch * c.dst.stride;
    j.dst_step = c.n_cols == 1 ? unsigned(sizeof(T)) : unsigned(c.dst.stride); // (a single column is dense)
    j.n_rows = unsigned(c.n_rows);
    j.row_len = unsigned(c.n_cols);
    bool dense = j.dst_step == sizeof(T);
    for (int t = 0; t < NT; t++) {
        ststhip_grid_view const &v = c.term[t].src;
        j.src[t] = reinterpret_cast<const unsigned char *>(span_of(v, c.term[t].row, c.term[t].col, 1, 1, sizeof(T)).first);
        j.src_row_bytes[t] = c.n_rows == 1 ? 0 : v.pitch * v.stride;
        j.src_step[t] = c.n_cols == 1 ? unsigned(sizeof(T)) : unsigned(v.stride);
        j.coef[t] = T(c.term[t].coef); // double to the element's type, once
        dense = dense && j.src_step[t] == sizeof(T);
    }
    if (dense) {
        const u64 segment = algebra_segment_bytes / sizeof(T);
        const dim3 grid = plan_blocks((u64(j.row_len) + segment - 1) / segment, j.n_rows);
        hipLaunchKernelGGL((combine_rows_kernel<T, NT>), grid, dim3(algebra_threads), 0, s, j);
    } else {
        const dim3 grid = plan_blocks((u64(j.row_len) + algebra_segment_cells - 1) / algebra_segment_cells, j.n_rows);
        hipLaunchKernelGGL((combine_strided_kernel<T, NT>), grid, dim3(algebra_threads), 0, s, j);
    }
    return hipGetLastError();
}

template <typename T> static hipError_t launch_combine(ststhip_grid_combine_desc const &c, hipStream_t s) {
    switch (c.n_terms) {
    case 1: return launch_combine<T, 1>(c, s);
    case 2: return launch_combine<T, 2>(c, s);
    case 3: return launch_combine<T, 3>(c, s);
    default: return launch_combine<T, 4>(c, s);
    }
}

// One resample entry, validated.
static int check_resample(ststhip_grid_resample_desc const &r, bool &empty) {
    if (r.type != STSTHIP_F32 && r.type != STSTHIP_F64)
        return invalid("unknown element type");
    if (r.mode != STSTHIP_RESTRICT_MEAN && r.mode != STSTHIP_PROLONG_BILINEAR)
        return invalid("unknown mode");
    const unsigned elem = elem_size_of(r.type);
    if (r.n_rows >> 30 != 0 || r.n_cols >> 30 != 0)
        return invalid("n_rows or n_cols of the fine side of 2^31 or more");
    if (int rc = check_view(r.dst, elem))
        return rc;
    if (int rc = check_view(r.src, elem))
        return rc;
    empty = r.n_rows == 0 || r.n_cols == 0;
    if (empty)
        return 0;
    if (!r.dst.base || !r.src.base)
        return invalid("null base with a non-empty rectangle");
    const bool prolong = r.mode == STSTHIP_PROLONG_BILINEAR;
    const u64 dst_rows = prolong ? 2 * r.n_rows : r.n_rows, dst_cols = prolong ? 2 * r.n_cols : r.n_cols;
    const u64 src_rows = prolong ? r.n_rows : 2 * r.n_rows, src_cols = prolong ? r.n_cols : 2 * r.n_cols;
    if (!inside(r.dst_row, dst_rows, r.dst.height) || !inside(r.dst_col, dst_cols, r.dst.width))
        return invalid("the destination rectangle does not lie inside its view");
    if (!inside(r.src_row, src_rows, r.src.height) || !inside(r.src_col, src_cols, r.src.width))
        return invalid("the source rectangle does not lie inside its view");
    if (!row_fits(dst_cols, r.dst.stride) || !row_fits(src_cols, r.src.stride))
        return invalid("a row of the rectangle spans 2^31 bytes or more");
    // what a prolongation reads: the rectangle and its neighbours inside the view
    u64 read_row = r.src_row, read_col = r.src_col, read_rows = src_rows, read_cols = src_cols;
    if (prolong) {
        if (read_row > 0)
            read_row--, read_rows++;
        if (read_col > 0)
            read_col--, read_cols++;
        if (read_row + read_rows < r.src.height)
            read_rows++;
        if (read_col + read_cols < r.src.width)
            read_cols++;
    }
    if (intersect(span_of(r.dst, r.dst_row, r.dst_col, dst_rows, dst_cols, elem),
                  span_of(r.src, read_row, read_col, read_rows, read_cols, elem)))
        return invalid("source and destination overlap");
    return 0;
}

template <typename T> static hipError_t launch_resample(ststhip_grid_resample_desc const &r, hipStream_t s) {
    ResampleJob<T> j{};
    j.dst = reinterpret_cast<unsigned char *>(span_of(r.dst, r.dst_row, r.dst_col, 1, 1, sizeof(T)).first);
    j.src = reinterpret_cast<const unsigned char *>(span_of(r.src, r.src_row, r.src_col, 1, 1, sizeof(T)).first);
    j.dst_row_bytes = r.dst.pitch * r.dst.stride;
    j.src_row_bytes = r.src.pitch * r.src.stride;
    j.dst_step = unsigned(r.dst.stride);
    j.src_step = unsigned(r.src.stride);
    j.n_rows = unsigned(r.n_rows);
    j.n_cols = unsigned(r.n_cols);
    const dim3 grid = plan_blocks((u64(j.n_cols) + algebra_segment_cells - 1) / algebra_segment_cells, j.n_rows);
    if (r.mode == STSTHIP_RESTRICT_MEAN) {
        hipLaunchKernelGGL(restrict_kernel<T>, grid, dim3(algebra_threads), 0, s, j);
    } else {
        j.top_edge = r.src_row == 0;
        j.left_edge = r.src_col == 0;
        j.bottom_at = unsigned(std::min<u64>(r.src.height - r.src_row, 0xffffffffu)); // (n_rows < 2^30 never gets there)
        j.right_at = unsigned(std::min<u64>(r.src.width - r.src_col, 0xffffffffu));
        j.halo = T(r.halo);
        hipLaunchKernelGGL(prolong_kernel<T>, grid, dim3(algebra_threads), 0, s, j);
    }
    return hipGetLastError();
}

} // namespace

extern "C" {

int ststhip_grid_combine(int n, const ststhip_grid_combine_desc *combines, ststhip_stream stream) {
    if (n < 1 || n > 8)
        return invalid("need 1..8 entries");
    if (!combines)
        return invalid("null argument");
    bool empty[8], any = false;
    for (int i = 0; i < n; i++) {
        if (int rc = check_combine(combines[i], empty[i]))
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
        const hipError_t err = combines[i].type == STSTHIP_F64 ? launch_combine<double>(combines[i], s)
                                                               : launch_combine<float>(combines[i], s);
        if (err != hipSuccess)
            return hip_failed(err, "ststhip_grid_combine");
    }
    return STSTHIP_OK;
}

int ststhip_grid_resample(int n, const ststhip_grid_resample_desc *resamples, ststhip_stream stream) {
    if (n < 1 || n > 8)
        return invalid("need 1..8 entries");
    if (!resamples)
        return invalid("null argument");
    bool empty[8], any = false;
    for (int i = 0; i < n; i++) {
        if (int rc = check_resample(resamples[i], empty[i]))
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
        const hipError_t err = resamples[i].type == STSTHIP_F64 ? launch_resample<double>(resamples[i], s)
                                                                : launch_resample<float>(resamples[i], s);
        if (err != hipSuccess)
            return hip_failed(err, "ststhip_grid_resample");
    }
    return STSTHIP_OK;
}

} // extern "C"
