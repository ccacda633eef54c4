// ststhip_grid_norms / ststhip_grid_distance (include/ststhip.h): count, non-finite count, max |v|, sum v, sum |v| and
// sum v*v of up to 8 fields of a grid, or of the difference of two grids, in one read of the cells.
//
// Reproducible by construction: no floating-point atomics.  A lane accumulates in double over the cells it owns, the 64
// lanes of a wave combine with an xor butterfly (both partners of a step add the same two numbers, so every lane ends
// with the same bits), the four waves of a workgroup combine through LDS in wave order, every workgroup stores one
// partial per field and quantity, and norms_final_kernel adds the partials in index order.  Which cells a workgroup
// owns, and how many workgroups there are, follows from the rectangle and the layout alone (plan_blocks): never from
// the device's CU count or an occupancy query.
//
// A workgroup owns row segments: segment blockIdx.x of rows row_begin + blockIdx.y, + gridDim.y, ...  All address
// arithmetic per row is wave-uniform; a lane adds a 32-bit column offset.  No division per cell.
#include "ststhip.h"

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <string>

namespace ststhip_detail {
int fail(int status, const char *message); // runtime.hip
}

namespace {

using u64 = unsigned long long;

constexpr unsigned norm_threads = 256;
constexpr unsigned norm_waves = norm_threads / 64;
// A row segment of a contiguous field (stride = element size) is 8 KiB: 512 16-byte vectors, two per lane and row.
constexpr unsigned norm_segment_bytes = 8192;
// A row segment of strided fields is 1024 cells: four cells per lane and row, one element per lane and load.
constexpr unsigned norm_segment_cells = 1024;
// At most this many workgroups per launch (or one per segment of a row, if a row alone has more segments): 8 per CU of
// a 256-CU chip, the usual size of a memory-bound grid; it is a constant, not a query, so that the partials are the
// same on every device.
constexpr unsigned norm_block_cap = 2048;
// max |v|, sum v, sum |v|, sum v*v, number of non-finite v
constexpr unsigned norm_quantities = 5;

struct Acc {
    double max_abs, sum, sum_abs, sum_sq;
    unsigned nonfinite;
};

__device__ inline Acc acc_zero() { return Acc{-HUGE_VAL, 0.0, 0.0, 0.0, 0u}; }

// One cell.  `inside` = the cell belongs to the rectangle (and was loaded); a cell that does not changes nothing:
// x + 0.0 == x for every sum that started at +0.0.
__device__ inline void take(Acc &a, double v, bool inside) {
    const double av = fabs(v);
    const bool finite = av < HUGE_VAL; // false for NaN and for +-infinity
    const bool use = inside && finite;
    a.nonfinite += (inside && !finite) ? 1u : 0u;
    const double w = use ? v : 0.0;
    a.max_abs = (use && av > a.max_abs) ? av : a.max_abs;
    a.sum += w;
    a.sum_abs += use ? av : 0.0;
    a.sum_sq += w * w;
}

// Combine the lanes' accumulators of NF fields and store the workgroup's partials: field k, quantity q of workgroup `block`
// goes to partial[(k * norm_quantities + q) * n_blocks + block].  The count travels as the bits of a 64-bit integer.
template <int NF> __device__ inline void store_partials(Acc (&acc)[NF], u64 *partial, unsigned n_blocks, unsigned block) {
    __shared__ double lds_value[norm_waves][NF][4];
    __shared__ u64 lds_count[norm_waves][NF];
    const unsigned wave = threadIdx.x >> 6;
#pragma unroll
    for (int k = 0; k < NF; k++) {
        double mx = acc[k].max_abs, s = acc[k].sum, sa = acc[k].sum_abs, sq = acc[k].sum_sq;
        u64 n = acc[k].nonfinite;
#pragma unroll
        for (int delta = 32; delta >= 1; delta >>= 1) {
            const double other = __shfl_xor(mx, delta, 64);
            mx = other > mx ? other : mx;
            s += __shfl_xor(s, delta, 64);
            sa += __shfl_xor(sa, delta, 64);
            sq += __shfl_xor(sq, delta, 64);
            n += __shfl_xor(n, delta, 64);
        }
        if ((threadIdx.x & 63u) == 0) {
            lds_value[wave][k][0] = mx;
            lds_value[wave][k][1] = s;
            lds_value[wave][k][2] = sa;
            lds_value[wave][k][3] = sq;
            lds_count[wave][k] = n;
        }
    }
    __syncthreads();
    if (threadIdx.x < unsigned(NF)) {
        const unsigned k = threadIdx.x;
        double mx = lds_value[0][k][0], s = lds_value[0][k][1], sa = lds_value[0][k][2], sq = lds_value[0][k][3];
        u64 n = lds_count[0][k];
        for (unsigned w = 1; w < norm_waves; w++) {
            mx = lds_value[w][k][0] > mx ? lds_value[w][k][0] : mx;
            s += lds_value[w][k][1];
            sa += lds_value[w][k][2];
            sq += lds_value[w][k][3];
            n += lds_count[w][k];
        }
        u64 *out = partial + u64(k) * norm_quantities * n_blocks + block;
        out[0 * u64(n_blocks)] = u64(__double_as_longlong(mx));
        out[1 * u64(n_blocks)] = u64(__double_as_longlong(s));
        out[2 * u64(n_blocks)] = u64(__double_as_longlong(sa));
        out[3 * u64(n_blocks)] = u64(__double_as_longlong(sq));
        out[4 * u64(n_blocks)] = n;
    }
}

// ------------------------------------------------------------------ one contiguous field: 16-byte loads
// Per row the segment is split where the addresses say: a head of up to VEC - 1 elements in front of the first 16-byte
// boundary, whole vectors, a tail.  Head and tail go through one scalar load per lane; so does the whole segment where the
// two grids of a distance sit differently relative to a 16-byte boundary.
template <typename T, bool DIST>
__global__ void __launch_bounds__(norm_threads)
    norms_rows_kernel(const T *a, const T *b, u64 pitch, u64 row_begin, u64 row_end, u64 col_begin, u64 col_end,
                      u64 *partial) {
    constexpr unsigned VEC = 16 / sizeof(T);
    constexpr unsigned SEG = norm_segment_bytes / sizeof(T);
    typedef T Vec __attribute__((ext_vector_type(VEC)));

    const u64 seg_begin = col_begin + u64(blockIdx.x) * SEG;
    const u64 rest = col_end - seg_begin;
    const unsigned len = rest < SEG ? unsigned(rest) : SEG;
    const unsigned lane = threadIdx.x;
    Acc acc[1] = {acc_zero()};

    for (u64 r = row_begin + blockIdx.y; r < row_end; r += gridDim.y) {
        const T *pa = a + (r * pitch + seg_begin);
        const T *pb = DIST ? b + (r * pitch + seg_begin) : pa;
        unsigned head = unsigned(((16u - unsigned(reinterpret_cast<std::uintptr_t>(pa) & 15u)) & 15u) / sizeof(T));
        if (DIST && ((reinterpret_cast<std::uintptr_t>(pa) ^ reinterpret_cast<std::uintptr_t>(pb)) & 15u) != 0)
            head = len;
        head = head < len ? head : len;
        const unsigned n_vec = (len - head) / VEC; // <= SEG / VEC = 2 * norm_threads
        const unsigned tail_begin = head + n_vec * VEC;
        const unsigned n_edge = head + (len - tail_begin);

        // both vectors of the lane are requested before the first is used
        const unsigned i0 = lane, i1 = lane + norm_threads;
        const bool in0 = i0 < n_vec, in1 = i1 < n_vec;
        Vec a0 = Vec(0), a1 = Vec(0), b0 = Vec(0), b1 = Vec(0);
        if (in0)
            a0 = *reinterpret_cast<const Vec *>(pa + head + i0 * VEC);
        if (in1)
            a1 = *reinterpret_cast<const Vec *>(pa + head + i1 * VEC);
        if (DIST) {
            if (in0)
                b0 = *reinterpret_cast<const Vec *>(pb + head + i0 * VEC);
            if (in1)
                b1 = *reinterpret_cast<const Vec *>(pb + head + i1 * VEC);
        }
#pragma unroll
        for (unsigned j = 0; j < VEC; j++)
            take(acc[0], DIST ? double(a0[j]) - double(b0[j]) : double(a0[j]), in0);
#pragma unroll
        for (unsigned j = 0; j < VEC; j++)
            take(acc[0], DIST ? double(a1[j]) - double(b1[j]) : double(a1[j]), in1);

        for (unsigned i = lane; i < n_edge; i += norm_threads) {
            const unsigned e = i < head ? i : tail_begin + (i - head);
            take(acc[0], DIST ? double(pa[e]) - double(pb[e]) : double(pa[e]), true);
        }
    }
    store_partials<1>(acc, partial, gridDim.x * gridDim.y, blockIdx.y * gridDim.x + blockIdx.x);
}

// ------------------------------------------------------------------ strided fields: one element per lane and load
// All strided fields of a call in one launch over the rectangle that contains their rectangles: the members of one AoS
// cell are read while the cell's cache lines are there.  That is what the grouping is for, and it holds where the fields
// share their cells (the callers in this tree: members of one grid).  Fields of unrelated grids or with disjoint
// rectangles are still reduced correctly -- every field has its own inside test -- but a lane then looks at every field
// over the whole hull and nothing is shared; such fields are better given calls of their own.
struct StridedTable {
    const unsigned char *a[8];
    const unsigned char *b[8];
    u64 stride[8];    // bytes between cells of a row
    u64 row_bytes[8]; // bytes between rows
    u64 row_begin[8], row_end[8], col_begin[8], col_end[8];
    unsigned type[8];
};

template <int NF, bool DIST>
__global__ void __launch_bounds__(norm_threads)
    norms_strided_kernel(StridedTable t, u64 row_begin, u64 row_end, u64 col_begin, u64 col_end, u64 *partial) {
    constexpr unsigned per_lane = norm_segment_cells / norm_threads;
    // loads of a lane in flight: the fields of `cells_at_once` cells; more fields, fewer cells (registers)
    constexpr unsigned cells_at_once = NF <= 2 ? 4 : NF <= 4 ? 2 : 1;
    const u64 seg_begin = col_begin + u64(blockIdx.x) * norm_segment_cells;
    Acc acc[NF];
#pragma unroll
    for (int k = 0; k < NF; k++)
        acc[k] = acc_zero();

    for (u64 r = row_begin + blockIdx.y; r < row_end; r += gridDim.y) {
#pragma unroll cells_at_once
        for (unsigned j = 0; j < per_lane; j++) {
            const unsigned dc = threadIdx.x + j * norm_threads; // < norm_segment_cells
            const u64 c = seg_begin + dc;
#pragma unroll
            for (int k = 0; k < NF; k++) {
                const bool inside = r >= t.row_begin[k] && r < t.row_end[k] && c >= t.col_begin[k] && c < t.col_end[k];
                double v = 0.0;
                if (inside) {
                    const u64 at = r * t.row_bytes[k] + seg_begin * t.stride[k] + u64(dc) * t.stride[k];
                    if (t.type[k] == STSTHIP_F64) {
                        v = *reinterpret_cast<const double *>(t.a[k] + at);
                        if (DIST)
                            v -= *reinterpret_cast<const double *>(t.b[k] + at);
                    } else {
                        v = double(*reinterpret_cast<const float *>(t.a[k] + at));
                        if (DIST)
                            v -= double(*reinterpret_cast<const float *>(t.b[k] + at));
                    }
                }
                take(acc[k], v, inside);
            }
        }
    }
    store_partials<NF>(acc, partial, gridDim.x * gridDim.y, blockIdx.y * gridDim.x + blockIdx.x);
}

// ------------------------------------------------------------------ partials -> results, in index order
struct FinalTable {
    u64 offset[8];        // of the field's partials, in 8-byte words
    unsigned n_blocks[8]; // 0: the field's rectangle is empty
};

// One workgroup of five waves per field: wave q owns quantity q.  Its 64 lanes stage a run of the quantity's partials in
// LDS with one coalesced load each, then lane 0 folds the run in index order: a maximum, a sum or an integer sum,
// chosen once per wave, so no wave takes more than one path.
constexpr unsigned final_run = 256;
__global__ void __launch_bounds__(norm_quantities * 64) norms_final_kernel(const u64 *partial, FinalTable t, u64 *out) {
    __shared__ u64 staged[norm_quantities][final_run];
    const unsigned f = blockIdx.x, n_blocks = t.n_blocks[f];
    const unsigned q = threadIdx.x >> 6, lane = threadIdx.x & 63u;
    const u64 *p = partial + t.offset[f] + u64(q) * n_blocks;
    double folded = q == 0 ? -HUGE_VAL : 0.0;
    u64 count = 0;
    for (unsigned begin = 0; begin < n_blocks; begin += final_run) {
        const unsigned n = n_blocks - begin < final_run ? n_blocks - begin : final_run;
        for (unsigned i = lane; i < n; i += 64)
            staged[q][i] = p[begin + i];
        __syncthreads();
        if (lane == 0) {
            switch (q) {
            case 0:
                for (unsigned i = 0; i < n; i++) {
                    const double d = __longlong_as_double((long long)staged[0][i]);
                    folded = d > folded ? d : folded;
                }
                break;
            case 4:
                for (unsigned i = 0; i < n; i++)
                    count += staged[4][i];
                break;
            default:
                for (unsigned i = 0; i < n; i++)
                    folded += __longlong_as_double((long long)staged[q][i]);
            }
        }
        __syncthreads();
    }
    if (lane == 0)
        out[f * norm_quantities + q] = q == 4 ? count : u64(__double_as_longlong(folded));
}

// ------------------------------------------------------------------ host side
struct Rect {
    u64 row_begin, row_end, col_begin, col_end;
    bool empty() const { return row_end <= row_begin || col_end <= col_begin; }
};

// Workgroups of a launch over `rect` with row segments of `segment` cells: grid.x segments of a row, grid.y of them
// side by side down the rows.  A function of the rectangle only.
static dim3 plan_blocks(Rect const &rect, unsigned segment) {
    const u64 n_segments = (rect.col_end - rect.col_begin + segment - 1) / segment;
    const u64 n_rows = rect.row_end - rect.row_begin;
    const u64 down = std::max<u64>(1, std::min<u64>(n_rows, norm_block_cap / std::max<u64>(1, n_segments)));
    return dim3(unsigned(n_segments), unsigned(down), 1);
}

static int hip_failed(hipError_t err, const char *what) {
    const std::string msg = std::string(what) + ": " + hipGetErrorString(err);
    return ststhip_detail::fail(STSTHIP_ERR_HIP, msg.c_str());
}

template <bool DIST>
static void launch_rows(ststhip_norm_field const &f, const void *other, Rect const &rect, dim3 grid, u64 *partial,
                        hipStream_t s) {
    if (f.type == STSTHIP_F64)
        hipLaunchKernelGGL((norms_rows_kernel<double, DIST>), grid, dim3(norm_threads), 0, s,
                           static_cast<const double *>(f.base), static_cast<const double *>(other), u64(f.pitch),
                           rect.row_begin, rect.row_end, rect.col_begin, rect.col_end, partial);
    else
        hipLaunchKernelGGL((norms_rows_kernel<float, DIST>), grid, dim3(norm_threads), 0, s,
                           static_cast<const float *>(f.base), static_cast<const float *>(other), u64(f.pitch),
                           rect.row_begin, rect.row_end, rect.col_begin, rect.col_end, partial);
}

template <int NF, bool DIST>
static void launch_strided_n(StridedTable const &t, Rect const &rect, dim3 grid, u64 *partial, hipStream_t s) {
    hipLaunchKernelGGL((norms_strided_kernel<NF, DIST>), grid, dim3(norm_threads), 0, s, t, rect.row_begin,
                       rect.row_end, rect.col_begin, rect.col_end, partial);
}

template <bool DIST>
static void launch_strided(int n, StridedTable const &t, Rect const &rect, dim3 grid, u64 *partial, hipStream_t s) {
    switch (n) {
    case 1: return launch_strided_n<1, DIST>(t, rect, grid, partial, s);
    case 2: return launch_strided_n<2, DIST>(t, rect, grid, partial, s);
    case 3: return launch_strided_n<3, DIST>(t, rect, grid, partial, s);
    case 4: return launch_strided_n<4, DIST>(t, rect, grid, partial, s);
    case 5: return launch_strided_n<5, DIST>(t, rect, grid, partial, s);
    case 6: return launch_strided_n<6, DIST>(t, rect, grid, partial, s);
    case 7: return launch_strided_n<7, DIST>(t, rect, grid, partial, s);
    default: return launch_strided_n<8, DIST>(t, rect, grid, partial, s);
    }
}

static int grid_norms(int n_fields, const ststhip_norm_field *fields, const void *const *other, bool distance,
                      ststhip_norm_result *result, ststhip_stream stream) {
    using ststhip_detail::fail;
    // ---- validation: nothing below this block is reached with a bad argument, nothing in it touches the device
    if (n_fields < 1 || n_fields > 8)
        return fail(STSTHIP_ERR_INVALID, "grid norms: need 1..8 fields");
    if (!fields || !result || (distance && !other))
        return fail(STSTHIP_ERR_INVALID, "grid norms: null argument");
    Rect rect[8];
    bool any = false;
    for (int i = 0; i < n_fields; i++) {
        ststhip_norm_field const &f = fields[i];
        if (f.type != STSTHIP_F32 && f.type != STSTHIP_F64)
            return fail(STSTHIP_ERR_INVALID, "grid norms: unknown field type (STSTHIP_F32 or STSTHIP_F64)");
        const u64 size = f.type == STSTHIP_F64 ? 8 : 4;
        if (f.stride == 0)
            return fail(STSTHIP_ERR_INVALID, "grid norms: stride 0");
        if (f.stride % size != 0 || reinterpret_cast<std::uintptr_t>(f.base) % size != 0 ||
            (distance && reinterpret_cast<std::uintptr_t>(other[i]) % size != 0))
            return fail(STSTHIP_ERR_INVALID, "grid norms: base or stride not aligned to the element");
        if (f.pitch < f.width)
            return fail(STSTHIP_ERR_INVALID, "grid norms: pitch < width");
        // every byte offset the kernels form, (r * pitch + c) * stride with r < height and c < width <= pitch, fits in 63 bits,
        // and a row has fewer row segments than a launch has room for in x
        u64 row_bytes = 0, grid_bytes = 0;
        if (__builtin_mul_overflow(u64(f.pitch), u64(f.stride), &row_bytes) ||
            __builtin_mul_overflow(row_bytes, u64(f.height) + 1, &grid_bytes) || grid_bytes >> 63 != 0 ||
            f.width / norm_segment_cells >= 0x7fffffffull)
            return fail(STSTHIP_ERR_INVALID, "grid norms: extents, pitch and stride describe more than 2^63 bytes");
        rect[i].row_begin = std::min<u64>(f.row_begin, f.height);
        rect[i].row_end = std::max<u64>(rect[i].row_begin, std::min<u64>(f.row_end, f.height));
        rect[i].col_begin = std::min<u64>(f.col_begin, f.width);
        rect[i].col_end = std::max<u64>(rect[i].col_begin, std::min<u64>(f.col_end, f.width));
        if (!rect[i].empty() && (!f.base || (distance && !other[i])))
            return fail(STSTHIP_ERR_INVALID, "grid norms: null grid with a non-empty rectangle");
        any = any || !rect[i].empty();
    }
    for (int i = 0; i < n_fields; i++) {
        const u64 n_cells = rect[i].empty() ? 0 : (rect[i].row_end - rect[i].row_begin) * (rect[i].col_end - rect[i].col_begin);
        result[i] = ststhip_norm_result{n_cells, 0, -HUGE_VAL, 0.0, 0.0, 0.0};
    }
    if (!any)
        return STSTHIP_OK;
    if (int rc = ststhip_init(-1))
        return rc;
    if (!stream)
        if (int rc = ststhip_default_stream(&stream))
            return rc;
    hipStream_t s = static_cast<hipStream_t>(stream);

    // ---- plan: one launch per contiguous field, one for all strided fields together
    FinalTable final_table{};
    dim3 grid_of[8];
    StridedTable strided{};
    int strided_field[8], n_strided = 0;
    Rect hull{~0ull, 0, ~0ull, 0};
    u64 words = 0;
    for (int i = 0; i < n_fields; i++) {
        if (rect[i].empty())
            continue;
        ststhip_norm_field const &f = fields[i];
        const u64 size = f.type == STSTHIP_F64 ? 8 : 4;
        if (f.stride == size) {
            grid_of[i] = plan_blocks(rect[i], unsigned(norm_segment_bytes / size));
            final_table.offset[i] = words;
            final_table.n_blocks[i] = grid_of[i].x * grid_of[i].y;
            words += u64(norm_quantities) * final_table.n_blocks[i];
            continue;
        }
        const int k = n_strided++;
        strided_field[k] = i;
        strided.a[k] = static_cast<const unsigned char *>(f.base);
        strided.b[k] = distance ? static_cast<const unsigned char *>(other[i]) : nullptr;
        strided.stride[k] = f.stride;
        strided.row_bytes[k] = f.pitch * f.stride;
        strided.row_begin[k] = rect[i].row_begin;
        strided.row_end[k] = rect[i].row_end;
        strided.col_begin[k] = rect[i].col_begin;
        strided.col_end[k] = rect[i].col_end;
        strided.type[k] = f.type;
        hull.row_begin = std::min(hull.row_begin, rect[i].row_begin);
        hull.row_end = std::max(hull.row_end, rect[i].row_end);
        hull.col_begin = std::min(hull.col_begin, rect[i].col_begin);
        hull.col_end = std::max(hull.col_end, rect[i].col_end);
    }
    dim3 strided_grid(0, 0, 1);
    u64 strided_words = 0;
    if (n_strided > 0) {
        strided_grid = plan_blocks(hull, norm_segment_cells);
        strided_words = words;
        for (int k = 0; k < n_strided; k++) { // the launch's partials: field k of the launch after field k - 1
            final_table.offset[strided_field[k]] = words;
            final_table.n_blocks[strided_field[k]] = strided_grid.x * strided_grid.y;
            words += u64(norm_quantities) * strided_grid.x * strided_grid.y;
        }
    }
    const u64 out_words = u64(n_fields) * norm_quantities;

    // ---- run: partials in stream-ordered scratch, only the copy of the results to the host synchronises
    void *scratch = nullptr;
    if (int rc = ststhip_malloc_async(&scratch, (words + out_words) * sizeof(u64), stream))
        return rc;
    u64 *partial = static_cast<u64 *>(scratch);
    u64 *out = partial + words;
    hipError_t err = hipSuccess;
    for (int i = 0; i < n_fields && err == hipSuccess; i++) {
        const u64 size = fields[i].type == STSTHIP_F64 ? 8 : 4;
        if (rect[i].empty() || fields[i].stride != size)
            continue;
        if (distance)
            launch_rows<true>(fields[i], other[i], rect[i], grid_of[i], partial + final_table.offset[i], s);
        else
            launch_rows<false>(fields[i], nullptr, rect[i], grid_of[i], partial + final_table.offset[i], s);
        err = hipGetLastError();
    }
    if (n_strided > 0 && err == hipSuccess) {
        if (distance)
            launch_strided<true>(n_strided, strided, hull, strided_grid, partial + strided_words, s);
        else
            launch_strided<false>(n_strided, strided, hull, strided_grid, partial + strided_words, s);
        err = hipGetLastError();
    }
    u64 host[8 * norm_quantities] = {0};
    if (err == hipSuccess) {
        hipLaunchKernelGGL(norms_final_kernel, dim3(unsigned(n_fields)), dim3(norm_quantities * 64), 0, s, partial, final_table, out);
        err = hipGetLastError();
    }
    if (err == hipSuccess)
        err = hipMemcpyAsync(host, out, out_words * sizeof(u64), hipMemcpyDeviceToHost, s);
    if (err == hipSuccess)
        err = hipStreamSynchronize(s);
    const int rc = err == hipSuccess ? STSTHIP_OK : hip_failed(err, distance ? "ststhip_grid_distance" : "ststhip_grid_norms");
    ststhip_free_async(scratch, stream);
    if (rc != STSTHIP_OK)
        return rc;
    for (int i = 0; i < n_fields; i++) {
        if (rect[i].empty())
            continue;
        const u64 *h = host + i * norm_quantities;
        std::memcpy(&result[i].max_abs, &h[0], sizeof(double));
        std::memcpy(&result[i].sum, &h[1], sizeof(double));
        std::memcpy(&result[i].sum_abs, &h[2], sizeof(double));
        std::memcpy(&result[i].sum_sq, &h[3], sizeof(double));
        result[i].n_nonfinite = h[4];
    }
    return STSTHIP_OK;
}

} // namespace

extern "C" {

int ststhip_grid_norms(int n_fields, const ststhip_norm_field *fields, ststhip_norm_result *result,
                       ststhip_stream stream) {
    return grid_norms(n_fields, fields, nullptr, false, result, stream);
}

int ststhip_grid_distance(int n_fields, const ststhip_norm_field *fields, const void *const *other_base,
                          ststhip_norm_result *result, ststhip_stream stream) {
    return grid_norms(n_fields, fields, other_base, true, result, stream);
}

} // extern "C"
